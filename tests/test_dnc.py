"""DnC, the spectral defence (Shejwalkar and Houmansadr, NDSS 2021, Algorithm 2), without a GPU: the numpy restatement of the
contract (include/byzagg.h) that tests/test_gpu_dnc.py holds the kernels to, the restatement against
np.linalg.svd on attacked matrices, the contract's corner cases, the sampling helper and the public surface.

The restatement is the header's N-space form, operation by operation: the sampled columns centred in fp64 over the active
rows, M = C C^T, a power iteration on M from the row of largest norm, s_i = y_i^2 / lambda, the rows ranked by (s_i, i)."""
import inspect
import os
import re

import numpy as np
import pytest

from tests.test_geometric_median import attacked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -------------------------------------------------------------------------------------------------
def restated_scores(g, columns, power_iters=32):
    """(scores, info): one iteration's fp64 scores, +inf for an inactive row; info has 'active', 'i0', 'zero'."""
    g = np.asarray(g, dtype=np.float32)
    n = g.shape[0]
    x = g[:, np.asarray(columns, dtype=np.int64)]
    active = np.isfinite(x).all(axis=1)
    scores = np.full(n, np.inf, dtype=np.float64)
    info = {'active': active, 'i0': -1, 'zero': True}
    if not active.any():
        return scores, info
    xa = x[active].astype(np.float64)
    total = np.zeros(xa.shape[1], dtype=np.float64)
    for row in xa:                                   # ascending over the active rows
        total = total + row
    c = xa - total / float(xa.shape[0])
    m = c @ c.T
    diag = np.diag(m)
    i0 = int(np.argmax(diag))                        # the first maximum: the lowest index on a tie
    u = np.zeros(len(diag), dtype=np.float64)
    u[i0] = 1.0
    zero = diag[i0] == 0.0
    for _ in range(int(power_iters)):
        y = m @ u
        norm = float(np.sqrt(y @ y))
        if norm == 0.0:
            zero = True
            break
        u = y / norm
    y = m @ u
    lam = float(u @ y)
    if lam == 0.0:
        zero = True
    scores[active] = 0.0 if zero else (y * y) / lam
    info.update(i0=int(np.flatnonzero(active)[i0]), zero=bool(zero))
    return scores, info


def ranked(scores):
    """Row indices by (s_i, i) ascending."""
    return np.lexsort((np.arange(len(scores)), scores))


def gap_at_cut(scores, remove_count):
    """(score of the lowest removed row - score of the highest kept row) / the largest finite score; inf when nothing is
    removed, or when the cut falls between a finite and an infinite score."""
    if remove_count == 0:
        return np.inf
    s = np.sort(scores)
    n_keep = len(s) - remove_count
    finite = s[np.isfinite(s)]
    top = float(finite.max()) if finite.size and finite.max() > 0 else 1.0
    if not np.isfinite(s[n_keep]) and np.isfinite(s[n_keep - 1]):
        return np.inf
    if not np.isfinite(s[n_keep - 1]):
        return 0.0
    return float(s[n_keep] - s[n_keep - 1]) / top


def restated_dnc(g, remove_count, columns, power_iters=32):
    """(out, good, per-iteration scores): columns is one list per iteration."""
    g = np.asarray(g, dtype=np.float32)
    n = g.shape[0]
    columns = np.asarray(columns, dtype=np.int64)
    columns = columns.reshape(1, -1) if columns.ndim == 1 else columns
    kept = np.ones(n, dtype=bool)
    all_scores = []
    for cols in columns:
        s, _ = restated_scores(g, cols, power_iters)
        all_scores.append(s)
        keep_t = np.zeros(n, dtype=bool)
        keep_t[ranked(s)[:n - remove_count]] = True
        kept &= keep_t
    good = np.flatnonzero(kept).astype(np.int32)
    if good.size == 0:
        return np.full(g.shape[1], np.nan, dtype=np.float32), good, all_scores
    with np.errstate(over='ignore', invalid='ignore'):
        return np.mean(g[good], axis=0), good, all_scores


def sampled(d, b, seed):
    return np.sort(np.random.default_rng(seed).choice(d, b, replace=False))


ATTACKED_SHAPES = [(100, 5000, 1000, 1), (1000, 4000, 1000, 2), (1000, 4000, 500, 3), (50, 3000, 3000, 5),
                   (400, 20000, 2000, 6)]


# ---- the restatement against numpy's SVD ----------------------------------------------------------------------------
@pytest.mark.parametrize('n,d,b,seed', ATTACKED_SHAPES)
def test_the_restatement_meets_numpys_svd_and_removes_the_attackers(n, d, b, seed):
    g = attacked(n, d, seed, mal_prop=0.24)
    f = int(n * 0.24)
    cols = sampled(d, b, seed + 100)
    s, info = restated_scores(g, cols, power_iters=32)
    c = g[:, cols].astype(np.float64)
    c = c - c.mean(axis=0)
    v = np.linalg.svd(c, full_matrices=False)[2][0]
    proj = (c @ v) ** 2
    assert np.abs(s - proj).max() <= 1e-9 * proj.max(), np.abs(s - proj).max() / proj.max()
    assert gap_at_cut(s, f) >= 0.8, gap_at_cut(s, f)
    out, good, _ = restated_dnc(g, f, cols)
    assert good.tolist() == list(range(f, n))                      # the removed set is exactly the attackers
    assert np.array_equal(out, np.mean(g[f:], axis=0))


# ---- the contract's corners -----------------------------------------------------------------------------------------
def test_power_iters_zero_scores_from_one_column_of_m():
    g = attacked(60, 700, seed=7)
    cols = sampled(700, 200, 8)
    s, info = restated_scores(g, cols, power_iters=0)
    c = g[:, cols].astype(np.float64)
    c = c - c.mean(axis=0)
    m = c @ c.T
    i0 = int(np.argmax(np.diag(m)))
    assert info['i0'] == i0
    assert np.allclose(s, m[:, i0] ** 2 / m[i0, i0], rtol=1e-12, atol=0.0)
    assert np.isfinite(s).all() and s[i0] == pytest.approx(m[i0, i0], rel=1e-12)


def test_an_all_equal_matrix_scores_zero_and_keeps_the_lowest_indices():
    g = np.full((9, 40), 2.5, dtype=np.float32)
    s, info = restated_scores(g, np.arange(40))
    assert info['zero'] and np.array_equal(s, np.zeros(9))
    out, good, _ = restated_dnc(g, 3, np.arange(40))
    assert good.tolist() == [0, 1, 2, 3, 4, 5] and np.array_equal(out, g[0])


def test_non_finite_sampled_values_make_a_row_inactive_and_first_to_go():
    g = attacked(40, 300, seed=9)
    cols = sampled(300, 100, 10)
    g[[17, 30], cols[5]] = [np.nan, np.inf]
    g[33, cols[7]] = -np.inf
    s, info = restated_scores(g, cols)
    assert np.isinf(s[[17, 30, 33]]).all() and np.isfinite(np.delete(s, [17, 30, 33])).all()
    assert int((~info['active']).sum()) == 3
    _, good, _ = restated_dnc(g, 3, cols)
    assert sorted(set(range(40)) - set(good.tolist())) == [17, 30, 33]
    # more inactive rows than are removed: the lowest-indexed of them stay, as the ranking says
    _, good, _ = restated_dnc(g, 2, cols)
    assert sorted(set(range(40)) - set(good.tolist())) == [30, 33]
    # no active row at all: every score +inf, the lowest indices kept
    bad = np.full((5, 8), np.nan, dtype=np.float32)
    s, _ = restated_scores(bad, np.arange(8))
    assert np.isinf(s).all()
    assert restated_dnc(bad, 2, np.arange(8))[1].tolist() == [0, 1, 2]


def test_non_finite_values_in_unsampled_columns_change_nothing_of_the_selection():
    g = attacked(50, 400, seed=11)
    f = 12
    cols = sampled(400, 150, 12)
    other = np.setdiff1d(np.arange(400), cols)
    _, want, _ = restated_dnc(g, f, cols)
    h = g.copy()
    h[20, other[3]] = np.nan
    h[45, other[9]] = np.inf
    s0, _ = restated_scores(g, cols)
    s1, _ = restated_scores(h, cols)
    assert np.array_equal(s0, s1)
    out, good, _ = restated_dnc(h, f, cols)
    assert np.array_equal(good, want)
    assert np.isnan(out[other[3]]) and np.isinf(out[other[9]])        # (they do reach the mean of the kept rows)


def test_remove_count_zero_is_numpys_mean():
    g = attacked(37, 300, seed=13)
    out, good, _ = restated_dnc(g, 0, sampled(300, 64, 14))
    assert good.tolist() == list(range(37)) and np.array_equal(out, np.mean(g, axis=0))


def test_the_intersection_over_several_iterations():
    g = np.random.default_rng(15).standard_normal((30, 500)).astype(np.float32)
    lists = np.stack([sampled(500, 60, 16 + t) for t in range(3)])
    _, good, scores = restated_dnc(g, 5, lists)
    keeps = [set(ranked(s)[:25].tolist()) for s in scores]
    assert good.tolist() == sorted(keeps[0] & keeps[1] & keeps[2])
    assert 15 <= len(good) < 25                                       # pure noise: the iterations disagree
    _, good2, _ = restated_dnc(g, 5, lists[:2])
    assert good2.tolist() == sorted(keeps[0] & keeps[1])


def test_an_empty_intersection_gives_nan_and_a_count_of_zero():
    # two rows, one removed per iteration; the two samples are built to rank them in opposite orders
    g = np.zeros((2, 4), dtype=np.float32)
    g[0] = [3.0, 0.0, 1.0, 0.0]
    g[1] = [-3.0, 0.0, -1.0, 0.0]
    # both rows score alike on either sample (two centred rows are mirror images): the index breaks the tie, row 1 goes
    out, good, _ = restated_dnc(g, 1, [[0, 1], [2, 3]])
    assert good.tolist() == [0]
    # three rows, two removed per iteration, different survivors
    g = np.zeros((3, 4), dtype=np.float32)
    g[0, 0], g[1, 0], g[2, 0] = 0.0, 5.0, -5.1          # sample {0, 1}: row 0 is nearest the mean -> survives
    g[0, 2], g[1, 2], g[2, 2] = 7.0, 0.1, -7.0          # sample {2, 3}: row 1 is nearest the mean -> survives
    out, good, scores = restated_dnc(g, 2, [[0, 1], [2, 3]])
    assert ranked(scores[0])[0] == 0 and ranked(scores[1])[0] == 1
    assert good.size == 0 and np.isnan(out).all() and out.shape == (4,)


def test_the_sampling_helper():
    from attacking_federate_learning_amd.engine import dnc_columns
    a = dnc_columns(5000, 300, 3, seed=4)
    assert a.shape == (3, 300) and a.dtype == np.int64
    assert np.array_equal(a, dnc_columns(5000, 300, 3, seed=4))
    assert not np.array_equal(a, dnc_columns(5000, 300, 3, seed=5))
    assert (np.diff(a, axis=1) > 0).all() and a.min() >= 0 and a.max() < 5000       # sorted and distinct
    assert not np.array_equal(a[0], a[1])
    rng = np.random.default_rng(4)
    for row in a:                                                                   # the documented draw
        assert np.array_equal(row, np.sort(rng.choice(5000, 300, replace=False)))
    for sub in (40, 41, 10000):
        assert np.array_equal(dnc_columns(40, sub, 2, seed=1), np.stack([np.arange(40)] * 2))
    with pytest.raises(ValueError):
        dnc_columns(40, 0)


# ---- the surface ----------------------------------------------------------------------------------------------------
def test_the_new_names_and_their_signatures():
    from attacking_federate_learning_amd import _native, defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.dnc)) == \
        ('(users_grads, users_count, corrupted_count, niters=1, filter_frac=1.0, sub_dim=10000, power_iters=32, seed=0, '
         'columns=None, return_index=False)')
    assert str(inspect.signature(Engine.dnc)) == \
        '(self, g, remove_count, columns, power_iters=32, return_selection=False, validate_columns=True)'
    assert str(inspect.signature(Engine.dnc_scores)) == '(self, g, columns, power_iters=32, validate_columns=True)'
    assert str(inspect.signature(Engine.dnc_select)) == '(self, g, remove_count, columns, power_iters=32, validate_columns=True)'
    assert str(inspect.signature(ShardedAggregator.dnc)) == \
        ('(self, g_local, users_count, corrupted_count, niters=1, filter_frac=1.0, sub_dim=10000, power_iters=32, seed=0, '
         'columns=None, gather=False, return_index=False, total_columns=None)')
    assert callable(HipKernels.dnc) and callable(HipKernels.dnc_scores) and callable(HipKernels.dnc_select)
    assert callable(defences.dnc_columns)
    new = ('byz_dnc_scores_dev', 'byz_dnc_select_dev', 'byz_dnc_dev', 'byz_dnc_info', 'byz_dnc_host', 'byz_dnc_sharded_dev')
    header = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    for name in new:
        assert name in _native.EXPORTED_SYMBOLS, name
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
    assert 'typedef struct byz_dnc_params' in header
    assert [f[0] for f in _native.DncParams._fields_] == ['n_iters', 'sub_dim', 'power_iters', 'remove_count']
    assert re.search(r'#define BYZ_DNC_MAX_SAMPLED 268435456\b', header)
    assert re.search(r'#define BYZ_DNC_MAX_PRODUCTS 65536\b', header)
    assert len(_native._PROTOTYPES['byz_dnc_dev']) == 10 and len(_native._PROTOTYPES['byz_dnc_sharded_dev']) == 13
    assert re.search(r'#define BYZ_ABI_VERSION 1\b', header)
    # the kernel-timing ids keep their numbers
    assert re.search(r'BYZ_K_MISC = 8, BYZ_K_PLANE_SPLIT = 9, BYZ_K_COUNT = 10', header)
    from attacking_federate_learning_amd import build_native
    assert 'dnc.hip' in build_native.SOURCES and '-ffp-contract=off' in build_native.EXTRA_FLAGS['dnc.hip']


def test_remove_count_follows_filter_frac():
    """defences.dnc removes min(n - 1, int(filter_frac * corrupted_count)) rows per iteration: checked through a stand-in
    engine, since nothing here has a GPU."""
    from attacking_federate_learning_amd import defences
    seen = {}

    class Stub:
        def dnc(self, g, remove_count, columns, power_iters=32):
            seen.update(remove=remove_count, columns=np.asarray(columns), power_iters=power_iters)
            return 'out'

        def dnc_select(self, g, remove_count, columns, power_iters=32):
            seen.update(remove=remove_count)
            return 'good'
    real = defences.get_engine
    defences.get_engine = lambda: Stub()
    try:
        g = np.zeros((10, 50), dtype=np.float32)
        assert defences.dnc(g, 10, 4, niters=2, filter_frac=1.5, sub_dim=20, seed=3) == 'out'
        assert seen['remove'] == 6 and seen['columns'].shape == (2, 20) and seen['power_iters'] == 32
        assert np.array_equal(seen['columns'], defences.dnc_columns(50, 20, 2, 3))
        assert defences.dnc(g, 10, 40, return_index=True) == 'good' and seen['remove'] == 9
        assert defences.dnc(g, 10, 3, filter_frac=0.5) == 'out' and seen['remove'] == 1
        assert seen['columns'].shape == (1, 50)                       # sub_dim >= D: every column
    finally:
        defences.get_engine = real


def test_dnc_is_not_a_defend_key():
    from attacking_federate_learning_amd import defences
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert not any('dnc' in k.lower() for k in defences.defend)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_dnc', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.dnc) and callable(mod.dnc_columns) and 'dnc' not in mod.defend
