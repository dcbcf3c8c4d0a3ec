"""Multi-Krum without a GPU: the public surface (names and signatures at every layer, not a `defend` key) and the numpy
restatement of the contract (include/byzagg.h) that tests/test_gpu_multi_krum.py holds the kernels to.

The restatement: every row's Krum score is oracle.faithful.krum_scores' (defences.py:33-34: the sequential fp32 sum of the
first users_count - corrupted_count ascending distances); rows are ranked by (NaN?, score, visit position 1, 0, 2, ...) with
np.lexsort and the first m taken.  For m = 1 it must be the reference's own krum(..., return_index=True)."""
import inspect
import os
import re

import numpy as np
import pytest

from oracle import faithful

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -------------------------------------------------------------------------------------------------
def visit_positions(n):
    """Position of every row in the reference's dict order 1, 0, 2, 3, ..."""
    vp = np.arange(n, dtype=np.int64)
    if n >= 2:
        vp[0], vp[1] = 1, 0
    return vp


def restated_scores(dist, users_count, corrupted_count):
    """Every row's Krum score as fp32, vectorised over the rows: sorted distances to the other rows, then the first
    python_prefix_len(n - 1, users_count - corrupted_count) of them added left to right in fp32 from 0."""
    dist = np.asarray(dist, dtype=np.float32)
    n = dist.shape[0]
    keep = faithful.python_prefix_len(n - 1, int(users_count) - int(corrupted_count))
    others = dist[~np.eye(n, dtype=bool)].reshape(n, n - 1)
    ordered = np.sort(others, axis=1)
    acc = np.zeros(n, dtype=np.float32)
    for k in range(keep):
        acc = acc + ordered[:, k]
    return acc


def restated_ranking(scores, m):
    """The first m rows by (NaN?, score, visit position): every NaN last, -0.0 == +0.0, a tie by visit position."""
    scores = np.asarray(scores, dtype=np.float32)
    nan = np.isnan(scores)
    order = np.lexsort((visit_positions(len(scores)), np.where(nan, np.float32(0.0), scores), nan))
    return order[:m].astype(np.int32)


def restated_multi_krum(g, users_count, corrupted_count, m=None):
    """(aggregate, selection) on the numpy oracle's distances."""
    m = int(users_count) - int(corrupted_count) if m is None else int(m)
    sel = restated_ranking(restated_scores(faithful.distance_matrix(g), users_count, corrupted_count), m)
    return np.mean(g[np.sort(sel)], axis=0), sel


def attacked(n, d, f, seed, tie01=False):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d)).astype(np.float32)
    g *= (1.0 + 0.5 * rng.permutation(n) / n).astype(np.float32)[:, None]
    if f:
        head = g[:f]
        g[:f] = (head.mean(axis=0) - 1.5 * head.std(axis=0)).astype(np.float32)
    if tie01:
        g[1] = g[0]
    return g


CASES = [(12, 40, 2, False), (23, 157, 5, False), (30, 64, 7, True), (17, 33, 0, True), (40, 20, 9, False), (9, 5, 2, True)]


# ---- the surface ----------------------------------------------------------------------------------------------------
def test_the_new_names_and_their_signatures():
    from attacking_federate_learning_amd import _native, defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.multi_krum)) == \
        '(users_grads, users_count, corrupted_count, m=None, distances=None, return_index=False)'
    assert str(inspect.signature(Engine.multi_krum)) == \
        '(self, g, users_count, corrupted_count, m=None, distances=None, return_selection=False)'
    assert str(inspect.signature(Engine.multi_krum_select)) == \
        '(self, distances, users_count, corrupted_count, m=None, on_device=False)'
    assert str(inspect.signature(Engine.mean_rows)) == '(self, g, row_index, validate_index=True)'
    assert 'multi_krum' in vars(ShardedAggregator) and 'multi_krum_clients' in vars(ShardedAggregator)
    assert str(inspect.signature(ShardedAggregator.multi_krum_clients)) == \
        '(self, rows_local, rows_per_rank, users_count, corrupted_count, m=None, return_selection=False)'
    assert callable(HipKernels.multi_krum_select) and callable(HipKernels.mean_rows)
    new = ('byz_mean_rows_dev', 'byz_multi_krum_select_dev', 'byz_multi_krum_dev', 'byz_multi_krum_sharded_dev',
           'byz_multi_krum_host')
    header = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    for name in new:
        assert name in _native.EXPORTED_SYMBOLS, name
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
    # the C argument lists (tests/test_abi_and_surface.py checks every prototype's kinds against the header)
    assert len(_native._PROTOTYPES['byz_multi_krum_dev']) == 12
    assert len(_native._PROTOTYPES['byz_multi_krum_sharded_dev']) == 14


def test_multi_krum_is_not_a_defend_key():
    from attacking_federate_learning_amd import defences
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert not any('multi' in k.lower() for k in defences.defend)
    assert not any('multi' in a.lower() for a in vars(defences.DefenseTypes))


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_mk', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.multi_krum) and 'multi_krum' not in mod.defend


# ---- the restatement's own properties -------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d,f,tie01', CASES)
def test_restated_scores_are_the_oracles(n, d, f, tie01):
    g = attacked(n, d, f, seed=n * d, tie01=tie01)
    dist = faithful.distance_matrix(g)
    want = faithful.krum_scores(dist, faithful.visit_order(n), n, f)
    got = restated_scores(dist, n, f)
    assert np.array_equal(got, np.asarray([np.float32(want[u]) for u in range(n)], dtype=np.float32))


@pytest.mark.parametrize('n,d,f,tie01', CASES)
def test_m_one_is_the_oracles_krum_and_m_all_is_no_defense(n, d, f, tie01):
    g = attacked(n, d, f, seed=n + d, tie01=tie01)
    out, sel = restated_multi_krum(g, n, f, m=1)
    assert sel.tolist() == [faithful.krum(g, n, f, return_index=True)]
    assert np.array_equal(out, g[sel[0]])
    out, sel = restated_multi_krum(g, n, f, m=n)
    assert sorted(sel.tolist()) == list(range(n))
    assert np.array_equal(out, faithful.no_defense(g, n, f))
    if tie01:
        # rows 0 and 1 are one vector: they tie, and row 1 (visited first) ranks ahead of row 0
        sel = restated_multi_krum(g, n, f, m=n)[1].tolist()
        assert sel.index(1) + 1 == sel.index(0)


def test_ranking_of_special_scores():
    s = np.asarray([3.0, np.nan, -0.0, 0.0, np.inf, 1e20, -np.nan, 2.0], dtype=np.float32)
    # +0.0 and -0.0 tie (visit order: row 3 after row 2), NaNs last in visit order whatever the sign, inf and 1e20 by value
    assert restated_ranking(s, 8).tolist() == [2, 3, 7, 0, 5, 4, 1, 6]


@pytest.mark.reference
@pytest.mark.parametrize('n,d,f,tie01', CASES)
def test_m_one_reproduces_the_unmodified_reference(reference_modules, n, d, f, tie01):
    ref = reference_modules['defences']
    g = attacked(n, d, f, seed=7 * n + d, tie01=tie01)
    want = ref.krum(g.copy(), n, f, return_index=True)
    assert want >= 0
    _, sel = restated_multi_krum(g, n, f, m=1)
    assert sel.tolist() == [want]
