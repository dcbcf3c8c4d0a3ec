"""FLTrust without a GPU: the numpy restatement of the contract (include/byzagg.h) that
tests/test_gpu_fltrust.py holds the kernels to, its own properties, and the public surface (names and signatures at every
layer, not a `defend` key).

The restatement: p_i = x_i . r, q_i = |x_i|^2 and q0 = |r|^2 as fp64 sums, c_i = p_i / (sqrt(q_i) * sqrt(q0)), the trust score
its ReLU (0 for a row whose p or q is not finite, 0 everywhere under a zero or non-finite root), the weight
ts_i * (sqrt(q0) / sqrt(q_i)), T = sum ts_i, and the sum the sequential fp64 loop over the rows of restated_wmean, divided
by T; no trusted row is the zero vector."""
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 777), (2, 4096), (7, 1023), (9, 1025), (33, 2051), (100, 5000), (1000, 2048), (4097, 300), (20000, 64), (16, 1)]


# ---- the inputs ------------------------------------------------------------------------------------------------------
def trusted(n, d, seed, mal_prop=0.24):
    """Honest rows a_i * s + noise round a common direction s, the first mal_prop * n rows round -2 s, and a root gradient
    s + noise: both ReLU branches are taken wherever n >= 7, and no cosine lies within 0.03 of zero (0.0370 is
    the smallest at SHAPES with seed = n + d, at 20000 x 64)."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(d).astype(np.float32)
    a = (0.5 + rng.permutation(n) / n).astype(np.float32)
    g = a[:, None] * s[None, :] + rng.standard_normal((n, d)).astype(np.float32)
    f = int(n * mal_prop)
    if f:
        g[:f] = (-2.0 * s)[None, :] + 0.5 * rng.standard_normal((f, d)).astype(np.float32)
    r = (s + 0.5 * rng.standard_normal(d)).astype(np.float32)
    return g.astype(np.float32), r


# ---- the restatement -------------------------------------------------------------------------------------------------
def restated_dots(g, r):
    """(p, q, q0): fp64 sums."""
    x = np.asarray(g, dtype=np.float32).astype(np.float64)
    rd = np.asarray(r, dtype=np.float32).astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        return (x * rd[None, :]).sum(axis=1), (x * x).sum(axis=1), float((rd * rd).sum())


def restated_trust(p, q, q0):
    """(ts, w, T, info) from the sums, in the header's order of operations; info also carries the cosines c ('cosines', NaN
    where a row is not usable)."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    q0 = np.float64(q0)
    root_ok = bool(np.isfinite(q0) and q0 > 0)
    finite = np.isfinite(p) & np.isfinite(q)
    usable = finite & (q > 0)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        root_norm = np.sqrt(q0)
        norm = np.sqrt(np.where(usable, q, 1.0))
        c = p / (norm * root_norm)
        ts = np.where(usable & (c > 0), c, 0.0) if root_ok else np.zeros_like(p)
        w = np.where(ts != 0, ts * (root_norm / norm), 0.0)
    info = {'trusted_rows': int((ts > 0).sum()), 'excluded_rows': int((~finite).sum()), 'root_ok': root_ok,
            'cosines': np.where(usable, c, np.nan)}
    return ts, w, float(ts.sum()), info


def restated_scaled_sum(g, w, total):
    """fl32(S / T) where T > 0, zeros otherwise: S added in row order in fp64, rows of weight 0 skipped (not multiplied):
    restated_wmean's loop (tests/test_geometric_median.py) with the divisor given."""
    g = np.asarray(g, dtype=np.float32)
    acc = np.zeros(g.shape[1], dtype=np.float64)
    for i in range(g.shape[0]):
        wi = float(w[i])
        if wi != 0.0:
            acc = acc + wi * g[i].astype(np.float64)
    if not total > 0.0:
        return np.zeros(g.shape[1], dtype=np.float32)
    return (acc / float(total)).astype(np.float32)


def restated_fltrust(g, r):
    """(out, info); info: trusted_rows, excluded_rows, root_ok, trust_sum, trust, weights, cosines."""
    p, q, q0 = restated_dots(g, r)
    ts, w, total, info = restated_trust(p, q, q0)
    info.update(trust_sum=total, trust=ts, weights=w)
    return restated_scaled_sum(g, w, total), info


def norm64(v):
    return float(np.sqrt((np.asarray(v, dtype=np.float64) ** 2).sum()))


# ---- the generator keeps its promises --------------------------------------------------------------------------------
def test_the_generator_takes_both_branches_and_keeps_every_cosine_away_from_zero():
    for n, d in SHAPES:
        g, r = trusted(n, d, seed=n + d)
        _, info = restated_fltrust(g, r)
        c = info['cosines']
        assert np.isfinite(c).all() and np.abs(c).min() >= 0.03, (n, d, np.abs(c).min())
        if n >= 7:
            assert 0 < info['trusted_rows'] < n, (n, d)
        assert info['excluded_rows'] == 0 and info['root_ok']


# ---- the restatement's own properties -------------------------------------------------------------------------------
def test_the_result_is_no_longer_than_the_root():
    # a non-negative combination, weights summing to 1, of rows each rescaled to the root's norm
    for n, d, seed in [(37, 300, 1), (200, 64, 2), (9, 1025, 3)]:
        g, r = trusted(n, d, seed)
        out, info = restated_fltrust(g, r)
        assert info['trusted_rows'] > 0
        assert norm64(out) <= norm64(r) * (1.0 + 1e-6)
        assert (info['trust'] >= 0).all() and (info['weights'] >= 0).all()


def test_rows_equal_to_minus_the_root_get_no_trust():
    g, r = trusted(20, 50, seed=4)
    g[[3, 11]] = -r
    out, info = restated_fltrust(g, r)
    assert info['trust'][[3, 11]].tolist() == [0.0, 0.0] and info['weights'][[3, 11]].tolist() == [0.0, 0.0]
    assert np.allclose(info['cosines'][[3, 11]], -1.0, rtol=0, atol=1e-12)
    assert np.array_equal(out, restated_fltrust(np.delete(g, [3, 11], axis=0), r)[0])


def test_a_non_finite_row_is_excluded_and_the_result_stays_finite():
    g, r = trusted(20, 50, seed=5)
    g[3, 10] = np.nan
    g[8, 10] = np.inf
    g[11, 10] = -np.inf
    out, info = restated_fltrust(g, r)
    assert info['excluded_rows'] == 3 and np.isfinite(out).all()
    assert info['trust'][[3, 8, 11]].tolist() == [0.0, 0.0, 0.0]
    assert np.array_equal(out, restated_fltrust(np.delete(g, [3, 8, 11], axis=0), r)[0])
    bad = np.full((4, 5), np.inf, dtype=np.float32)
    bad[::2] = np.nan
    out, info = restated_fltrust(bad, np.arange(1, 6, dtype=np.float32))
    assert np.array_equal(out, np.zeros(5, dtype=np.float32)) and info['excluded_rows'] == 4 and info['trusted_rows'] == 0


def test_nothing_but_negative_cosines_is_the_zero_step():
    g, r = trusted(30, 80, seed=6, mal_prop=0.0)
    g = (-np.abs(g)).astype(np.float32)              # an all-negative matrix against an all-positive root
    r = np.abs(r).astype(np.float32)
    out, info = restated_fltrust(g, r)
    assert info['trusted_rows'] == 0 and info['trust_sum'] == 0.0 and info['root_ok']
    assert np.array_equal(out, np.zeros(80, dtype=np.float32))
    assert (info['cosines'] < 0).all()


def test_a_zero_root_and_a_nan_root_are_the_zero_step():
    g, r = trusted(12, 40, seed=7)
    broken = r.copy()
    broken[5] = np.nan
    for root in (np.zeros(40, dtype=np.float32), broken):
        out, info = restated_fltrust(g, root)
        assert not info['root_ok'] and info['trusted_rows'] == 0
        assert np.array_equal(out, np.zeros(40, dtype=np.float32)) and not np.isnan(out).any()


def test_copies_of_the_root_return_the_root():
    _, r = trusted(5, 300, seed=8)
    g = np.repeat(r[None, :], 11, axis=0)
    out, info = restated_fltrust(g, r)
    assert info['trusted_rows'] == 11 and np.allclose(info['trust'], 1.0, rtol=0, atol=1e-15)
    assert np.allclose(out, r, rtol=2.0 ** -23, atol=0.0)


def test_a_sign_flipped_majority_moves_the_mean_and_not_the_result():
    n, d = 50, 200
    g, r = trusted(n, d, seed=9, mal_prop=0.0)
    f = int(n * 0.6)
    g[:f] = -g[:f]                                      # 60 % of the rows point the other way
    out, info = restated_fltrust(g, r)
    mean = g.astype(np.float64).mean(axis=0)
    rd = r.astype(np.float64)
    assert float(mean @ rd) < 0.0 < float(out.astype(np.float64) @ rd)
    # within the honest rows' cone: the flipped rows carry no weight, the result is what the honest rows alone give
    assert (info['weights'][:f] == 0).all() and (info['weights'][f:] > 0).all()
    assert np.array_equal(out, restated_fltrust(g[f:], r)[0])


def test_the_sum_skips_zero_weights_and_a_zero_divisor_gives_zeros():
    rng = np.random.default_rng(10)
    g = rng.standard_normal((9, 17)).astype(np.float32)
    w = rng.random(9)
    w[[2, 5]] = 0.0
    g[5] = np.inf
    out = restated_scaled_sum(g, w, w.sum())
    assert np.isfinite(out).all()
    assert np.allclose(out, (w[:, None] * np.where(np.isfinite(g), g, 0)).sum(axis=0) / w.sum(), rtol=1e-6, atol=1e-7)
    assert np.array_equal(restated_scaled_sum(g, w, 0.0), np.zeros(17, dtype=np.float32))


# ---- the surface ----------------------------------------------------------------------------------------------------
def test_the_new_names_and_their_signatures():
    from attacking_federate_learning_amd import _native, defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.fltrust)) == \
        '(users_grads, users_count, corrupted_count, root_grad, return_info=False)'
    assert str(inspect.signature(Engine.fltrust)) == '(self, g, root, return_info=False)'
    assert str(inspect.signature(Engine.row_dots)) == '(self, g, r)'
    assert str(inspect.signature(Engine.scaled_rows_sum)) == '(self, g, weights, divisor)'
    assert str(inspect.signature(Engine.fltrust_info)) == '(self)'
    assert str(inspect.signature(ShardedAggregator.fltrust)) == '(self, g_local, root_local, gather=False, return_info=False)'
    assert str(inspect.signature(DeviceServer.defend_fltrust)) == '(self, root_grad)'
    assert 'clients.per_client_gradients' in DeviceServer.defend_fltrust.__doc__
    assert callable(HipKernels.row_dots) and callable(HipKernels.scaled_rows_sum)
    counts = {'byz_row_dots_dev': 9, 'byz_scaled_rows_sum_dev': 9, 'byz_fltrust_dev': 10, 'byz_fltrust_info': 5,
              'byz_fltrust_host': 8, 'byz_fltrust_sharded_dev': 12}
    header = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    for name, count in counts.items():
        assert name in _native.EXPORTED_SYMBOLS, name
        assert len(_native._PROTOTYPES[name]) == count, name
        proto = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, header)
        assert proto, name
        assert len(proto.group(1).split(',')) == count, name          # the header and the binding agree on the arguments
    assert re.search(r'#define BYZ_ABI_VERSION 1\b', header)


def test_fltrust_is_not_a_defend_key():
    from attacking_federate_learning_amd import defences
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert not any('trust' in k.lower() for k in defences.defend)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_flt', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.fltrust) and 'fltrust' not in mod.defend
