"""The geometric median without a GPU: the numpy restatement of the contract (include/byzagg.h) that
tests/test_gpu_geometric_median.py holds the kernels to, its convergence where the median is known, and the public
surface (names and signatures at every layer, not a `defend` key).

The restatement: wmean is the sequential fp64 loop over the rows (a row of weight 0 skipped), rowsq the fp64 sum of the
squared differences, z rounded to fp32 between iterations, the finiteness fallback when no_defense's mean is not finite."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -------------------------------------------------------------------------------------------------
def restated_wmean(g, w):
    """fl32(S / W): S and W added in row order in fp64, rows of weight 0 skipped (not multiplied)."""
    g = np.asarray(g, dtype=np.float32)
    acc = np.zeros(g.shape[1], dtype=np.float64)
    total = 0.0
    for i in range(g.shape[0]):
        wi = float(w[i])
        if wi != 0.0:
            acc = acc + wi * g[i].astype(np.float64)
            total = total + wi
    with np.errstate(divide='ignore', invalid='ignore'):
        return (acc / total).astype(np.float32)


def restated_rowsq(g, z):
    diff = np.asarray(g, dtype=np.float32).astype(np.float64) - np.asarray(z, dtype=np.float32).astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        return (diff * diff).sum(axis=1)


def restated_geometric_median(g, nu=1e-6, max_iter=10, ftol=1e-6):
    """(out, info); info also lists the stop ratio |F - F_new| / F_new of every iteration ('ratios')."""
    g = np.asarray(g, dtype=np.float32)
    n = g.shape[0]
    with np.errstate(over='ignore', invalid='ignore'):
        mean0 = np.mean(g, axis=0)
    if np.isfinite(mean0).all():
        active = np.ones(n, dtype=bool)
        z = mean0
    else:
        active = np.isfinite(restated_rowsq(g, np.zeros(g.shape[1], dtype=np.float32)))
        z = restated_wmean(g, active.astype(np.float64))
    info = {'iterations': 0, 'objective': 0.0, 'excluded_rows': int((~active).sum()), 'ratios': []}
    if not active.any():
        info['weights'] = np.zeros(n)
        return np.full(g.shape[1], np.nan, dtype=np.float32), info
    d = np.sqrt(restated_rowsq(g, z))
    F = float(d[active].sum())
    beta = None
    for k in range(1, int(max_iter) + 1):
        beta = np.where(active, 1.0 / np.maximum(nu, np.where(active, d, 1.0)), 0.0)
        z = restated_wmean(g, beta)
        d = np.sqrt(restated_rowsq(g, z))
        F_new = float(d[active].sum())
        info['ratios'].append(abs(F - F_new) / F_new if F_new > 0 else np.inf)
        stop = abs(F - F_new) <= ftol * F_new
        F = F_new
        info['iterations'] = k
        if stop:
            break
    info['objective'] = F
    info['weights'] = beta / beta.sum() if beta is not None else active / active.sum()
    return z, info


def weiszfeld_fp64(g, iters=5000, nu=1e-12):
    """A long plain fp64 Weiszfeld run: the yardstick of the general case."""
    x = np.asarray(g, dtype=np.float64)
    z = x.mean(axis=0)
    for _ in range(iters):
        d = np.maximum(np.sqrt(((x - z) ** 2).sum(axis=1)), nu)
        z = (x / d[:, None]).sum(axis=0) / (1.0 / d).sum()
    return z


def optimality_residual(g, z):
    """|sum_i (z - x_i) / d_i|: the gradient of the objective, zero at the median (away from the data points)."""
    x = np.asarray(g, dtype=np.float64)
    diff = np.asarray(z, dtype=np.float64) - x
    d = np.sqrt((diff ** 2).sum(axis=1))
    return float(np.linalg.norm((diff / d[:, None]).sum(axis=0)))


def attacked(n, d, seed, mal_prop=0.24, shift=0.0):
    """Honest rows of different scales; the first mal_prop * n rows one drifted vector (moved by `shift` in every
    coordinate on top of the attack's mean - 1.5 std)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d)).astype(np.float32)
    g *= (1.0 + 0.5 * rng.permutation(n) / n).astype(np.float32)[:, None]
    f = int(n * mal_prop)
    if f:
        head = g[:f]
        g[:f] = (head.mean(axis=0) - 1.5 * head.std(axis=0) + np.float32(shift)).astype(np.float32)
    return g


# ---- the restatement's own properties -------------------------------------------------------------------------------
def test_wmean_skips_zero_weights_and_is_the_sequential_loop():
    rng = np.random.default_rng(0)
    g = rng.standard_normal((9, 17)).astype(np.float32)
    g[4] = np.inf
    w = rng.random(9)
    w[4] = 0.0
    out = restated_wmean(g, w)
    assert np.isfinite(out).all()
    keep = w != 0
    want = (w[keep, None] * g[keep].astype(np.float64)).sum(axis=0) / w[keep].sum()
    assert np.allclose(out, want, rtol=1e-6)
    assert np.isnan(restated_wmean(g, np.zeros(9))).all()


def test_max_iter_zero_is_numpys_mean():
    g = attacked(37, 300, seed=1)
    out, info = restated_geometric_median(g, max_iter=0)
    assert np.array_equal(out, np.mean(g, axis=0))
    assert info['iterations'] == 0 and info['excluded_rows'] == 0
    assert np.allclose(info['weights'], 1.0 / 37)


def test_collinear_points_with_odd_count_find_the_one_dimensional_median():
    rng = np.random.default_rng(2)
    t = np.sort(rng.standard_normal(11)) * 3.0
    u = rng.standard_normal(8)
    u /= np.linalg.norm(u)
    c = rng.standard_normal(8)
    g = (c[None, :] + t[:, None] * u[None, :]).astype(np.float32)
    out, info = restated_geometric_median(g, max_iter=400, ftol=0.0)
    want = g[5].astype(np.float64)                      # the middle point: the median of a line
    spread = float(t[-1] - t[0])
    assert np.linalg.norm(out - want) <= 2e-3 * spread, np.linalg.norm(out - want)


def test_a_symmetric_configuration_has_its_centre_as_median():
    rng = np.random.default_rng(3)
    centre = rng.standard_normal(6).astype(np.float32)
    half = rng.standard_normal((5, 6)).astype(np.float32)
    g = np.concatenate([centre + half, centre - half, centre + 2 * half[:2], centre - 2 * half[:2]]).astype(np.float32)
    out, _ = restated_geometric_median(g, max_iter=300, ftol=0.0)
    assert np.allclose(out, centre, atol=1e-5)


@pytest.mark.parametrize('n,d,seed', [(15, 4, 4), (40, 30, 5), (101, 12, 6)])
def test_the_general_case_meets_a_long_fp64_weiszfeld_run(n, d, seed):
    g = attacked(n, d, seed=seed)
    g[int(n * 0.24):] += np.random.default_rng(seed).standard_normal((n - int(n * 0.24), d)).astype(np.float32)
    out, info = restated_geometric_median(g, max_iter=300, ftol=0.0)
    want = weiszfeld_fp64(g)
    scale = float(np.abs(g).max())
    assert np.linalg.norm(out - want) <= 1e-4 * scale * np.sqrt(d)
    # the optimality residual of a unit-vector sum (at most n): small at the fp32 point
    assert optimality_residual(g, out) <= 1e-2 * n, optimality_residual(g, out)
    assert optimality_residual(g, want) <= 1e-6 * n


def test_non_finite_rows_are_left_out():
    g = attacked(20, 50, seed=7)
    g[3, 10] = np.nan
    g[8, 10] = np.inf
    g[11, 10] = -np.inf
    out, info = restated_geometric_median(g)
    assert info['excluded_rows'] == 3
    assert np.isfinite(out).all()
    assert info['weights'][[3, 8, 11]].tolist() == [0.0, 0.0, 0.0]
    clean = np.delete(g, [3, 8, 11], axis=0)
    want, _ = restated_geometric_median(clean)
    assert np.allclose(out, want, rtol=1e-5, atol=1e-6)
    out, info = restated_geometric_median(np.full((4, 5), np.inf, dtype=np.float32))
    assert np.isnan(out).all() and info['iterations'] == 0 and info['excluded_rows'] == 4


def test_one_row_stops_at_the_first_iteration():
    g = attacked(1, 64, seed=8)
    out, info = restated_geometric_median(g, ftol=0.0, max_iter=50)
    assert info['iterations'] == 1 and info['objective'] == 0.0
    assert np.array_equal(out, g[0])


def test_the_median_resists_the_drift_that_moves_the_mean():
    n, d = 200, 64
    g = attacked(n, d, seed=9, shift=1e3)
    f = int(n * 0.24)
    out, _ = restated_geometric_median(g, max_iter=100)
    honest, _ = restated_geometric_median(g[f:], max_iter=100)
    spread = float(np.sqrt(((g[f:] - g[f:].mean(axis=0)) ** 2).sum(axis=1)).mean())
    assert np.linalg.norm(out - honest) <= 2.0 * spread
    assert np.linalg.norm(np.mean(g, axis=0) - g[f:].mean(axis=0)) >= 0.2 * 1e3 * np.sqrt(d)


# ---- the surface ----------------------------------------------------------------------------------------------------
def test_the_new_names_and_their_signatures():
    from attacking_federate_learning_amd import _native, defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.geometric_median)) == \
        '(users_grads, users_count, corrupted_count, nu=1e-06, max_iter=10, ftol=1e-06)'
    assert str(inspect.signature(Engine.geometric_median)) == \
        '(self, g, nu=1e-06, max_iter=10, ftol=1e-06, return_info=False)'
    assert str(inspect.signature(Engine.weighted_mean)) == '(self, g, weights, validate=True)'
    assert str(inspect.signature(Engine.row_sqdist)) == '(self, g, z)'
    assert str(inspect.signature(ShardedAggregator.geometric_median)) == \
        '(self, g_local, nu=1e-06, max_iter=10, ftol=1e-06, gather=False, return_info=False, total_columns=None)'
    assert callable(HipKernels.row_sqdist) and callable(HipKernels.weighted_mean)
    new = ('byz_row_sqdist_dev', 'byz_weighted_mean_dev', 'byz_geometric_median_dev', 'byz_geometric_median_info',
           'byz_geometric_median_host', 'byz_geometric_median_sharded_dev')
    header = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    for name in new:
        assert name in _native.EXPORTED_SYMBOLS, name
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
    assert 'typedef struct byz_geomed_params' in header
    # the update budget is capped (every update's launches are enqueued whatever the stop); the GPU tests use the value
    assert re.search(r'#define BYZ_GEOMED_MAX_ITER 65536\b', header)
    assert [f[0] for f in _native.GeomedParams._fields_] == ['nu', 'max_iter', 'ftol']
    assert len(_native._PROTOTYPES['byz_geometric_median_dev']) == 9
    assert len(_native._PROTOTYPES['byz_geometric_median_sharded_dev']) == 11
    # the ABI version stays (tests/test_abi_and_surface.py pins it)
    assert re.search(r'#define BYZ_ABI_VERSION 1\b', header)


def test_geometric_median_is_not_a_defend_key():
    from attacking_federate_learning_amd import defences
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert not any('median' in k.lower() or 'geo' in k.lower() for k in defences.defend)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_gm', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.geometric_median) and 'geometric_median' not in mod.defend
