"""Multi-Metrics (Huang et al., ICCV 2023) without a GPU: the numpy restatement of the rule -- Manhattan matrix, features, scores,
selection, aggregate -- which IS the specification (include/byzagg.h), the closed-form 3 x 3 inverse against
np.linalg.inv, the Manhattan matrix against scipy's cityblock distances, the degenerate cases, ties, broken rows, the planted
property, and the surface -- header, ctypes table, build list, signatures, the refusals that need no device.
tests/test_gpu_multi_metrics.py imports the restatement."""
import inspect
import os
import re

import numpy as np
import pytest

from tests.test_flame import restated_cosine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'attacking_federate_learning_amd', 'csrc')

NEW_SYMBOLS = ('byz_manhattan_distances_dev', 'byz_manhattan_sums_dev', 'byz_manhattan_from_sums_dev', 'byz_multi_metrics_features_dev',
               'byz_multi_metrics_select_dev', 'byz_multi_metrics_dev', 'byz_multi_metrics_info', 'byz_multi_metrics_host',
               'byz_multi_metrics_sharded_dev')
MIN_DET = 1e-12


# ---- the restatement ------------------------------------------------------------------------------------------------------
def restated_manhattan(g, block=16, exact=False):
    """m_ij = sum_c |g_ic - g_jc| in fp64, rounded once to float32; the diagonal and every pair whose sum, or whose rounded
    value, is not finite are +inf (a NaN or an infinity in either row, or overflow).  A zero row is an ordinary row.
    exact=True: the fp64 sums before the rounding, +inf in the same places."""
    g = np.asarray(g, dtype=np.float64)
    n = g.shape[0]
    m = np.empty((n, n), dtype=np.float64)
    with np.errstate(all='ignore'):
        for r0 in range(0, n, block):
            m[r0:r0 + block] = np.abs(g[r0:r0 + block, None, :] - g[None, :, :]).sum(axis=2)
        out = m.astype(np.float32)
    broken = ~np.isfinite(m) | ~np.isfinite(out)
    out[broken] = np.inf
    np.fill_diagonal(out, np.inf)
    if exact:
        m[broken] = np.inf
        np.fill_diagonal(m, np.inf)
        return m
    return out


def restated_euclidean(g):
    """The Euclidean distances in fp64 rounded to float32, diagonal +inf: what pairwise_distances holds within its 1e-5."""
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(all='ignore'):
        e = np.sqrt(np.maximum(0.0, ((g[:, None, :] - g[None, :, :]) ** 2).sum(axis=2))).astype(np.float32)
    np.fill_diagonal(e, np.inf)
    return e


def usable_rows(g):
    """cosine_distances' notion: the Gram diagonal is finite and > 0."""
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(all='ignore'):
        diag = (g * g).sum(axis=1)
    return np.isfinite(diag) & (diag > 0)


def usable_from_cosine(cos):
    """What byz_multi_metrics_features_dev can know: row i of the cosine matrix has a finite off-diagonal entry."""
    c = np.array(cos, dtype=np.float64)
    np.fill_diagonal(c, np.inf)
    return np.isfinite(c).any(axis=1)


def restated_features(man, euc, cos, usable=None):
    """x_i = (sum m_ij, sum e_ij, sum c_ij) over the usable j != i: the float32 entries added in ascending j in fp64; rows outside
    U get (inf, inf, inf)."""
    usable = usable_from_cosine(cos) if usable is None else np.asarray(usable, dtype=bool)
    n = len(usable)
    x = np.full((n, 3), np.inf, dtype=np.float64)
    for i in np.flatnonzero(usable):
        others = usable.copy()
        others[i] = False
        for k, mat in enumerate((man, euc, cos)):
            with np.errstate(all='ignore'):
                x[i, k] = np.asarray(mat[i], dtype=np.float64)[others].sum()
    return x


def closed_form_inverse(r):
    """adj R / det R of a symmetric 3 x 3 matrix -> (inverse, det): the library's order of operations."""
    r00, r01, r02, r11, r12, r22 = r[0, 0], r[0, 1], r[0, 2], r[1, 1], r[1, 2], r[2, 2]
    a00, a01, a02 = r11 * r22 - r12 * r12, r02 * r12 - r01 * r22, r01 * r12 - r02 * r11
    a11, a12, a22 = r00 * r22 - r02 * r02, r01 * r02 - r00 * r12, r00 * r11 - r01 * r01
    det = r00 * a00 + r01 * a01 + r02 * a02
    with np.errstate(all='ignore'):
        inv = np.array([[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]) / det
    return inv, det


def restated_scores(x):
    """(scores, info): U = the rows with three finite features; s = the sample standard deviations (ddof = 1), taken about the
    first usable row so that a constant feature's is exactly 0; z = x / s; R = cov(z); score = z^T R^-1 z, uncentred.
    Degenerate (u < 4, an s that is zero or not finite, det R <= 1e-12): score = x[:, 0].  Rows outside U: +inf."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    ok = np.isfinite(x).all(axis=1)
    u = int(ok.sum())
    scores = np.full(n, np.inf)
    info = {'usable': u, 'degenerate': 1, 'det': 0.0}
    if u == 0:
        return scores, info
    xu = x[ok]
    degenerate = u < 4
    if not degenerate:
        with np.errstate(all='ignore'):
            y = xu - xu[0]
            y = y - y.mean(axis=0)
            cov = y.T @ y / (u - 1)
            s = np.sqrt(np.diagonal(cov))
        degenerate = bool((~(s > 0) | ~np.isfinite(s)).any())
    if not degenerate:
        r = cov / np.outer(s, s)
        inv, det = closed_form_inverse(r)
        degenerate = not (det > MIN_DET) or not np.isfinite(det)
        info['det'] = float(det) if np.isfinite(det) else 0.0
    if degenerate:
        scores[ok] = xu[:, 0]
    else:
        z = xu / s
        scores[ok] = np.einsum('ik,kl,il->i', z, inv, z)
        info['degenerate'] = 0
    return scores, info


def restated_select(x, keep):
    """(flags, scores, info): the min(u, keep) rows of U smallest by (score ascending, row ascending; a NaN last)."""
    scores, info = restated_scores(x)
    ok = np.isfinite(np.asarray(x, dtype=np.float64)).all(axis=1)
    rows = np.flatnonzero(ok)
    key = np.where(np.isnan(scores[rows]), np.inf, scores[rows])
    nan_last = np.isnan(scores[rows]).astype(np.int64)
    order = rows[np.lexsort((rows, key, nan_last))]
    kept = min(info['usable'], int(keep))
    flags = np.zeros(len(scores), dtype=np.int32)
    flags[order[:kept]] = 1
    info['kept'] = kept
    return flags, scores, info


def boundary_gap(scores, flags):
    """The relative gap between the largest chosen and the smallest rejected usable score (inf when there is no boundary)."""
    chosen = scores[flags != 0]
    rest = scores[(flags == 0) & np.isfinite(scores)]
    if len(chosen) == 0 or len(rest) == 0:
        return np.inf
    return (rest.min() - chosen.max()) / max(abs(rest.min()), abs(chosen.max()), 1e-300)


def restated_aggregate(g, flags):
    chosen = np.flatnonzero(flags)
    g = np.asarray(g, dtype=np.float32)
    return np.mean(g[chosen], axis=0) if len(chosen) else np.zeros(g.shape[1], dtype=np.float32)


def restated_multi_metrics(g, p=0.3):
    """The whole rule on the CPU -> (vector, flags, scores, info)."""
    g = np.asarray(g, dtype=np.float32)
    keep = int(p * g.shape[0])
    man, euc, cos = restated_manhattan(g), restated_euclidean(g), restated_cosine(g).astype(np.float32)
    x = restated_features(man, euc, cos, usable_rows(g))
    flags, scores, info = restated_select(x, keep)
    return restated_aggregate(g, flags), flags, scores, info


def planted(n, d, f, seed):
    """Honest rows mu + 0.5 N(0, 1); the last f rows alternately scaled x 3, negated, or shifted by +8 on d / 20 coordinates."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal(d)
    g = mu + 0.5 * rng.standard_normal((n, d))
    for k, i in enumerate(range(n - f, n)):
        if k % 3 == 0:
            g[i] *= 3.0
        elif k % 3 == 1:
            g[i] = -g[i]
        else:
            g[i, rng.choice(d, d // 20, replace=False)] += 8.0
    return g.astype(np.float32)


PLANTED_SHAPES = ((33, 1000, 8), (65, 4099, 16), (130, 513, 30))


# ---- the restatement against independent code ---------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(6))
def test_closed_form_inverse_against_numpy(seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((40, 3)) @ rng.standard_normal((3, 3))
    r = np.corrcoef(z.T)
    cond = np.linalg.cond(r)
    assert cond < 1e6
    inv, det = closed_form_inverse(r)
    want = np.linalg.inv(r)
    assert np.abs(inv - want).max() <= 1e-12 * cond * np.abs(want).max()
    assert abs(det - np.linalg.det(r)) <= 1e-12 * cond * abs(det)


@pytest.mark.parametrize('n,d', ((2, 1), (3, 7), (33, 257), (65, 1000)))
def test_manhattan_restatement_against_scipy(n, d):
    from scipy.spatial.distance import cdist
    g = np.random.default_rng(n * 1000 + d).standard_normal((n, d)).astype(np.float32)
    want = cdist(g.astype(np.float64), g.astype(np.float64), 'cityblock')
    got = restated_manhattan(g)
    off = ~np.eye(n, dtype=bool)
    assert np.array_equal(got[off], want.astype(np.float32)[off])
    assert np.isinf(np.diagonal(got)).all() and np.array_equal(got, got.T)


def test_manhattan_restatement_on_broken_rows():
    g = np.random.default_rng(5).standard_normal((7, 40)).astype(np.float32)
    g[1, 3] = np.nan
    g[2, 5] = np.inf
    g[3] = 3e38
    g[4] = -3e38
    g[5] = 0.0
    m = restated_manhattan(g)
    for i in (1, 2):
        assert np.isinf(m[i]).all() and np.isinf(m[:, i]).all()
    assert np.isinf(m[3, 4]) and np.isinf(m[3, 0])          # 40 x 3e38 overflows float32
    assert np.isfinite(m[5, 0]) and np.isfinite(m[0, 6])    # a zero row is an ordinary row


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def test_scores_are_the_mahalanobis_norm_of_the_paper():
    x = np.random.default_rng(3).standard_normal((50, 3)) * [100.0, 3.0, 0.01] + [900.0, 40.0, 0.3]
    scores, info = restated_scores(x)
    assert info['degenerate'] == 0 and info['usable'] == 50
    sigma = np.cov(x.T)                                     # the paper's own form: x^T Sigma^-1 x, the same number
    want = np.einsum('ik,kl,il->i', x, np.linalg.inv(sigma), x)
    assert np.abs(scores - want).max() <= 1e-9 * np.abs(want).max()


def test_degenerate_fewer_than_four_usable_rows():
    x = np.full((6, 3), np.inf)
    x[[1, 3, 4]] = [[5.0, 1.0, 0.1], [2.0, 9.0, 0.9], [3.0, 0.5, 0.5]]
    flags, scores, info = restated_select(x, 2)
    assert info == {'usable': 3, 'degenerate': 1, 'det': 0.0, 'kept': 2}
    assert np.array_equal(np.flatnonzero(flags), [3, 4]) and np.array_equal(scores[[1, 3, 4]], [5.0, 2.0, 3.0])
    assert np.isinf(scores[[0, 2, 5]]).all()


def test_degenerate_constant_feature_and_identical_rows():
    rng = np.random.default_rng(8)
    x = rng.standard_normal((12, 3)) + 10.0
    x[:, 1] = 0.1                                           # 0.1 * k is not exact: the deviation must still be exactly 0
    flags, scores, info = restated_select(x, 4)
    assert info['degenerate'] == 1 and np.array_equal(scores, x[:, 0])
    assert np.array_equal(np.flatnonzero(flags), np.sort(np.argsort(x[:, 0], kind='stable')[:4]))
    g = np.tile(rng.standard_normal(64).astype(np.float32), (10, 1))
    vec, flags, scores, info = restated_multi_metrics(g, 0.3)
    assert info['degenerate'] == 1 and not np.isnan(scores).any()
    assert np.array_equal(np.flatnonzero(flags), [0, 1, 2])              # every score ties: the lower rows
    assert np.array_equal(vec, np.mean(g[:3], axis=0))


def test_degenerate_singular_correlation():
    rng = np.random.default_rng(9)
    a = rng.standard_normal(20)
    x = np.stack([a, 2.0 * a + 1.0, rng.standard_normal(20)], axis=1)    # two features perfectly correlated: det R = 0
    _, scores, info = restated_select(x, 5)
    assert info['degenerate'] == 1 and info['det'] <= MIN_DET and np.array_equal(scores, x[:, 0])


def test_ties_go_to_the_lower_row_and_nan_is_last():
    x = np.random.default_rng(10).standard_normal((9, 3)) + 5.0
    x[6] = x[2]
    x[7] = x[2]
    flags, scores, _ = restated_select(x, 9)
    assert scores[6] == scores[2] == scores[7]
    order = np.lexsort((np.arange(9), scores))
    pos = {int(r): k for k, r in enumerate(order)}
    assert pos[2] < pos[6] < pos[7]
    for keep in range(1, 9):
        f, _, _ = restated_select(x, keep)
        assert np.array_equal(np.flatnonzero(f), np.sort(order[:keep]))


def test_a_broken_row_is_never_chosen():
    g = planted(20, 300, 4, seed=2)
    g[0] = 0.0
    g[5, 17] = np.nan
    g[9, 3] = -np.inf
    vec, flags, scores, info = restated_multi_metrics(g, 1.0)
    assert info['usable'] == 17 and info['kept'] == 17
    assert not flags[[0, 5, 9]].any() and flags.sum() == 17
    assert np.isinf(scores[[0, 5, 9]]).all() and np.isfinite(vec).all()
    zeros, flags, _, info = restated_multi_metrics(np.zeros((6, 10), dtype=np.float32), 0.5)
    assert info['usable'] == 0 and info['kept'] == 0 and not flags.any() and np.array_equal(zeros, np.zeros(10, dtype=np.float32))


@pytest.mark.parametrize('n,d,f', PLANTED_SHAPES)
@pytest.mark.parametrize('seed', range(6))
def test_planted_attackers_are_not_chosen(n, d, f, seed):
    """No planted attacker is among the int(0.3 n) chosen, and every honest score is below every attacker's.  The figures of
    this restatement with mu ~ N(0, 1) over the 18 cases: honest scores at most 4.3, attacker scores at least 21.4, cond(R)
    between 44 and 74, the relative score gap at the keep boundary between 1.9e-5 and 2.8e-3 (recorded, not asserted: they
    move with mu, which the rule's description leaves open)."""
    g = planted(n, d, f, seed)
    vec, flags, scores, info = restated_multi_metrics(g, 0.3)
    assert info['degenerate'] == 0 and info['kept'] == int(0.3 * n)
    assert not flags[n - f:].any()
    assert scores[:n - f].max() < scores[n - f:].min()      # every honest client scores below every attacker
    assert np.array_equal(vec, np.mean(g[np.flatnonzero(flags)], axis=0))


# ---- the surface ------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_new_entry_points_and_keeps_the_abi_version():
    from attacking_federate_learning_amd import _native
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    assert '#define BYZ_ABI_VERSION 1\n' in text
    assert 'BYZ_K_MISC = 8, BYZ_K_PLANE_SPLIT = 9, BYZ_K_COUNT = 10' in text          # the timing enum did not change
    assert re.search(r'#define BYZ_MANHATTAN_CHAIN %d\b' % _native.MANHATTAN_CHAIN, text)
    assert (_native.MANHATTAN_CHAIN + 2) * 2.0 ** -24 <= 1e-5                         # the project's distance tolerance
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    for name in ('byz_multi_metrics_dev', 'byz_multi_metrics_select_dev'):
        assert not re.search(r'\bdouble\s+\w+\s*[,)]', re.search(r'int\s+%s\s*\((.*?)\)' % name, code, flags=re.S).group(1))
    kernel = open(os.path.join(CSRC, 'manhattan.hip')).read()
    assert '(kChain + 2) * 2^-24' in kernel and 'kChain = BYZ_MANHATTAN_CHAIN' in kernel


def test_the_ctypes_table_lists_them():
    import ctypes
    from attacking_federate_learning_amd import _native
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS, name
    i64, i32, vp, f64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double
    P = ctypes.POINTER
    assert _native._PROTOTYPES['byz_manhattan_distances_dev'] == [vp, vp, i64, i64, i64, vp, vp]
    assert _native._PROTOTYPES['byz_manhattan_sums_dev'] == [vp, vp, i64, i64, i64, vp, vp]
    assert _native._PROTOTYPES['byz_manhattan_from_sums_dev'] == [vp, vp, i64, vp, vp]
    assert _native._PROTOTYPES['byz_multi_metrics_features_dev'] == [vp, vp, vp, vp, i64, vp, vp]
    assert _native._PROTOTYPES['byz_multi_metrics_select_dev'] == [vp, vp, i64, i64, vp, vp, vp]
    assert _native._PROTOTYPES['byz_multi_metrics_dev'] == [vp, vp, i64, i64, i64, i64, vp, vp, vp]
    assert _native._PROTOTYPES['byz_multi_metrics_info'] == [vp, P(i64), P(i64), P(i32), P(f64)]
    assert _native._PROTOTYPES['byz_multi_metrics_host'] == [vp, vp, i64, i64, i64, vp, vp]
    assert _native._PROTOTYPES['byz_multi_metrics_sharded_dev'] == [vp, vp, i64, i64, i64, i64, vp, vp, vp, vp, vp]


def test_the_sources_are_on_the_build_list():
    from attacking_federate_learning_amd import build_native
    for src in ('manhattan.hip', 'multi_metrics.hip'):
        assert src in build_native.SOURCES
        assert '-ffp-contract=off' in build_native.EXTRA_FLAGS[src]
        assert os.path.exists(os.path.join(CSRC, src))


def test_python_surface():
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.multi_metrics)) == '(users_grads, users_count, corrupted_count, p=0.3, return_info=False)'
    assert str(inspect.signature(defences.manhattan_distances)) == '(users_grads)'
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    for fn in (defences.multi_metrics, defences.manhattan_distances):
        assert fn not in defences.defend.values()
    assert not hasattr(defences.DefenseTypes, 'MultiMetrics')
    assert str(inspect.signature(Engine.manhattan_distances)) == '(self, g)'
    assert str(inspect.signature(Engine.multi_metrics_features)) == '(self, man, euc, cos)'
    assert list(inspect.signature(Engine.multi_metrics_select).parameters)[:5] == ['self', 'features', 'keep', 'on_device', 'return_scores']
    assert inspect.signature(Engine.multi_metrics_select).parameters['on_device'].default is False
    assert inspect.signature(Engine.multi_metrics_select).parameters['return_scores'].default is False
    assert str(inspect.signature(Engine.multi_metrics)) == '(self, g, p=0.3, return_info=False)'
    assert str(inspect.signature(Engine.multi_metrics_info)) == '(self)'
    assert str(inspect.signature(DeviceServer.defend_multi_metrics)) == '(self, p=0.3)'
    assert list(inspect.signature(ShardedAggregator.multi_metrics).parameters)[:5] == [
        'self', 'g_local', 'users_count', 'corrupted_count', 'p']
    assert callable(HipKernels.manhattan_sums) and callable(HipKernels.manhattan_from_sums) and callable(HipKernels.multi_metrics_select)


def test_the_refusals_that_need_no_gpu():
    from attacking_federate_learning_amd.engine import Engine
    assert Engine._multi_metrics_keep(33, p=0.3) == 9
    assert Engine._multi_metrics_keep(10, p=1.0) == 10
    assert Engine._multi_metrics_keep(16384, p=0.3) == 4915
    assert Engine._multi_metrics_keep(20, keep=20) == 20
    for n, p in ((3, 0.3), (10, 1.01), (10, 0.0), (10, -0.5), (10, float('nan')), (10, float('inf'))):
        with pytest.raises(ValueError):
            Engine._multi_metrics_keep(n, p=p)
    for n, keep in ((10, 0), (10, 11), (10, -1)):
        with pytest.raises(ValueError):
            Engine._multi_metrics_keep(n, keep=keep)
    with pytest.raises(NotImplementedError):
        Engine._multi_metrics_keep(16385, p=0.3)
    with pytest.raises(NotImplementedError):
        Engine._multi_metrics_keep(16385, keep=5)
    # a dict (the reference's form of the distances) is refused before anything touches a device
    eng = object.__new__(Engine)
    with pytest.raises(ValueError):
        Engine.multi_metrics_features(eng, {0: {1: 1.0}}, {0: {1: 1.0}}, {0: {1: 1.0}})


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    from attacking_federate_learning_amd import defences
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_multi_metrics', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.multi_metrics is defences.multi_metrics and mod.manhattan_distances is defences.manhattan_distances
    assert 'multi_metrics' not in mod.defend


def test_the_documents_name_the_new_entry_points():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert name in integration, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '3.4n' in design and '(K + 2) * 2^-24' in design and 'VGPR' in design
    papers = open(os.path.join(ROOT, 'PAPERS.md')).read()
    assert 'Multi-metrics adaptively identifies backdoors' in papers and 'Huang' in papers
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'defences.multi_metrics' in readme and 'defences.manhattan_distances' in readme
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'multi_metrics_timing.md'))
