"""Centered clipping without a GPU: the numpy restatement of the contract (include/byzagg.h) that
tests/test_gpu_centered_clip.py holds the kernels to, its own properties, and the public surface (names and signatures at
every layer, not a `defend` key).

The restatement: q = rowsq(G, v) in fp64 on the difference, d = sqrt(q), the scale 1 / tau / d / 0 (a row at a non-finite
distance is excluded: skipped, never multiplied, still counted in the divisor), the update the sequential fp64 loop over
the rows on the difference, v rounded to fp32 once per iteration."""
import inspect
import os
import re

import numpy as np

from tests.test_geometric_median import attacked, restated_rowsq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -------------------------------------------------------------------------------------------------
def restated_scales(q, tau):
    """(scales, clipped, excluded) from the squared distances."""
    with np.errstate(invalid='ignore', divide='ignore'):
        d = np.sqrt(q)
        finite = np.isfinite(d)
        over = finite & (d > tau)
        s = np.where(over, tau / np.where(over, d, 1.0), np.where(finite, 1.0, 0.0))
    return s, int(over.sum()), int((~finite).sum())


def restated_clip_update(g, v, s):
    """fl32(v + S / n): S added in row order in fp64 on the difference, rows of scale 0 skipped (not multiplied)."""
    g = np.asarray(g, dtype=np.float32)
    vd = np.asarray(v, dtype=np.float32).astype(np.float64)
    acc = np.zeros(g.shape[1], dtype=np.float64)
    for i in range(g.shape[0]):
        si = float(s[i])
        if si != 0.0:
            acc = acc + si * (g[i].astype(np.float64) - vd)
    return (vd + acc / float(g.shape[0])).astype(np.float32)


def restated_centered_clip(g, tau=10.0, iters=3, start=None):
    """(out, info); info also lists every iteration's centre ('centres', v_0 first) and its smallest relative gap
    |d_i - tau| / tau over the rows at a finite distance ('gaps'; inf where tau is infinite or no row is finite) and its
    clipped-row count ('clipped_history')."""
    g = np.asarray(g, dtype=np.float32)
    n, d = g.shape
    v = np.zeros(d, dtype=np.float32) if start is None else np.array(start, dtype=np.float32).reshape(d)
    info = {'clipped_rows': 0, 'excluded_rows': 0, 'scales': np.ones(n), 'centres': [v], 'gaps': [], 'clipped_history': []}
    for _ in range(int(iters)):
        q = restated_rowsq(g, v)
        s, clipped, excluded = restated_scales(q, tau)
        dist = np.sqrt(q[np.isfinite(q)])
        info['gaps'].append(float(np.abs(dist - tau).min() / tau) if np.isfinite(tau) and dist.size else np.inf)
        v = restated_clip_update(g, v, s)
        info.update(clipped_rows=clipped, excluded_rows=excluded, scales=s)
        info['centres'].append(v)
        info['clipped_history'].append(clipped)
    return v, info


def median_tau(g):
    """The midpoint of the two middle sorted row norms (n >= 2), 0.4 of the row's norm (n = 1)."""
    norms = np.sort(np.sqrt((np.asarray(g, dtype=np.float64) ** 2).sum(axis=1)))
    n = len(norms)
    return 0.4 * float(norms[0]) if n == 1 else 0.5 * float(norms[n // 2 - 1] + norms[n // 2])


# ---- the restatement's own properties -------------------------------------------------------------------------------
def test_infinite_tau_and_one_iteration_is_the_fp64_mean_rounded_once():
    g = attacked(37, 300, seed=1)
    out, info = restated_centered_clip(g, tau=np.inf, iters=1)
    acc = np.zeros(300, dtype=np.float64)
    for row in g:
        acc = acc + row.astype(np.float64)
    assert np.array_equal(out, (acc / 37.0).astype(np.float32))
    assert np.allclose(out, g.astype(np.float64).mean(axis=0), rtol=2.0 ** -23, atol=1e-12)
    assert info['clipped_rows'] == 0 and info['excluded_rows'] == 0 and np.array_equal(info['scales'], np.ones(37))


def test_no_iteration_returns_the_start():
    g = attacked(12, 40, seed=2)
    start = np.random.default_rng(2).standard_normal(40).astype(np.float32)
    out, info = restated_centered_clip(g, iters=0, start=start)
    assert np.array_equal(out, start) and info['clipped_rows'] == 0
    out, _ = restated_centered_clip(g, iters=0)
    assert np.array_equal(out, np.zeros(40, dtype=np.float32))


def test_no_step_is_longer_than_tau():
    g = attacked(60, 200, seed=3, shift=5.0)
    for tau in (0.5, 3.0, 40.0):
        _, info = restated_centered_clip(g, tau=tau, iters=5)
        for a, b in zip(info['centres'][:-1], info['centres'][1:]):
            step = np.linalg.norm(b.astype(np.float64) - a.astype(np.float64))
            assert step <= tau * (1.0 + 1e-6), (tau, step)


def test_from_zero_one_iteration_is_the_norm_clipped_mean():
    g = attacked(45, 120, seed=4)
    tau = median_tau(g)
    out, info = restated_centered_clip(g, tau=tau, iters=1)
    x = g.astype(np.float64)
    norms = np.sqrt((x ** 2).sum(axis=1))
    want = (x * np.minimum(1.0, tau / norms)[:, None]).mean(axis=0)
    assert np.allclose(out, want, rtol=1e-6, atol=1e-7)
    assert 0 < info['clipped_rows'] < 45


def test_a_non_finite_row_adds_nothing_and_still_counts():
    g = attacked(20, 50, seed=5)
    g[3, 10] = np.nan
    g[8, 10] = np.inf
    g[11, 10] = -np.inf
    out, info = restated_centered_clip(g, tau=median_tau(np.delete(g, [3, 8, 11], axis=0)))
    assert info['excluded_rows'] == 3 and np.isfinite(out).all()
    assert info['scales'][[3, 8, 11]].tolist() == [0.0, 0.0, 0.0]
    # the divisor stays n: one iteration from zero moves 17/20 of what the clean rows alone would
    clean = np.delete(g, [3, 8, 11], axis=0)
    one, _ = restated_centered_clip(g, tau=np.inf, iters=1)
    ref, _ = restated_centered_clip(clean, tau=np.inf, iters=1)
    assert np.allclose(one, ref.astype(np.float64) * 17.0 / 20.0, rtol=1e-6, atol=1e-7)
    bad = np.full((4, 5), np.inf, dtype=np.float32)
    start = np.arange(5, dtype=np.float32)
    out, info = restated_centered_clip(bad, start=start)
    assert np.array_equal(out, start) and info['excluded_rows'] == 4


def test_clipping_resists_the_drift_that_moves_the_mean():
    n, d = 200, 64
    g = attacked(n, d, seed=6, shift=1e3)
    f = int(n * 0.24)
    honest = g[f:].astype(np.float64).mean(axis=0)
    out, _ = restated_centered_clip(g, tau=median_tau(g[f:]), iters=3)
    assert np.linalg.norm(out - honest) <= 3 * median_tau(g[f:])          # three steps of at most tau * f / n each ...
    assert np.linalg.norm(np.mean(g, axis=0) - honest) >= 0.2 * 1e3 * np.sqrt(d)      # ... where the mean moves by 240 a column


# ---- the surface ----------------------------------------------------------------------------------------------------
def test_the_new_names_and_their_signatures():
    from attacking_federate_learning_amd import _native, defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.centered_clip)) == \
        '(users_grads, users_count, corrupted_count, tau=10.0, iters=3, start=None)'
    assert str(inspect.signature(Engine.centered_clip)) == '(self, g, tau=10.0, iters=3, start=None, return_info=False)'
    assert str(inspect.signature(Engine.clip_update)) == '(self, g, v, scales)'
    assert str(inspect.signature(ShardedAggregator.centered_clip)) == \
        '(self, g_local, tau=10.0, iters=3, start=None, gather=False, return_info=False, total_columns=None)'
    assert str(inspect.signature(DeviceServer.defend_centered_clip)) == '(self, tau=10.0, iters=3)'
    assert callable(HipKernels.clip_update)
    assert "this package's choices" in ' '.join(Engine.centered_clip.__doc__.split())
    new = ('byz_clip_update_dev', 'byz_centered_clip_dev', 'byz_centered_clip_info', 'byz_centered_clip_host',
           'byz_centered_clip_sharded_dev')
    header = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    for name in new:
        assert name in _native.EXPORTED_SYMBOLS, name
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
    assert 'typedef struct byz_cclip_params' in header
    assert re.search(r'#define BYZ_CCLIP_MAX_ITER 65536\b', header)
    assert [f[0] for f in _native.CclipParams._fields_] == ['tau', 'iters']
    assert len(_native._PROTOTYPES['byz_clip_update_dev']) == 9
    assert len(_native._PROTOTYPES['byz_centered_clip_dev']) == 10
    assert len(_native._PROTOTYPES['byz_centered_clip_info']) == 3
    assert len(_native._PROTOTYPES['byz_centered_clip_host']) == 8
    assert len(_native._PROTOTYPES['byz_centered_clip_sharded_dev']) == 12
    assert re.search(r'#define BYZ_ABI_VERSION 1\b', header)


def test_centered_clip_is_not_a_defend_key():
    from attacking_federate_learning_amd import defences
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert 'centered_clip' not in defences.defend
    assert not any('clip' in k.lower() for k in defences.defend)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_cc', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.centered_clip) and 'centered_clip' not in mod.defend
