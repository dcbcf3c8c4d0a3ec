"""FABA (Xia, Chen, Yu and Ma, IJCAI 2019) without a GPU: the numpy restatement of the selection that include/byzagg.h states
operation for operation (tests/test_gpu_faba.py holds the device to it, flags and order as integers), the restatement against
a direct FABA (the fp64 mean of the kept rows, the squared distances to it, the argmax), the properties of the rule, and the
Python surface with the refusals that need no GPU."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('byz_faba_select_dev', 'byz_faba_dev', 'byz_faba_info', 'byz_faba_host')


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def usable(c):
    """finite and >= 0 (-0.0 is)"""
    c = np.asarray(c)
    return np.isfinite(c) & (c >= 0)


def terms(c, power):
    e = np.asarray(c, dtype=np.float32).astype(np.float64)
    return e * e if power == 2 else e


def restated_initial(dist, power=2):
    """(s, bad): row i's fp64 sum of the usable off-diagonal entries' terms in the header's order -- 64 chains over the columns
    l, l + 64, ... ascending, folded 32, 16, 8, 4, 2, 1 -- and the count of those that are not usable.  An entry that is
    skipped adds +0.0 here, which changes no bit: the chains start at +0.0 and never fall below it."""
    c = np.asarray(dist, dtype=np.float32)
    n = c.shape[0]
    off = ~np.eye(n, dtype=bool)
    ok = usable(c) & off
    bad = (off & ~ok).sum(axis=1).astype(np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        t = np.where(ok, terms(c, power), 0.0)
    t = np.pad(t, ((0, 0), (0, -n % 64))).reshape(n, -1, 64)
    chains = np.zeros((n, 64), dtype=np.float64)
    for k in range(t.shape[1]):
        chains = chains + t[:, k, :]
    h = 32
    while h >= 1:
        chains = chains[:, :h] + chains[:, h:2 * h]
        h //= 2
    return chains[:, 0].copy(), bad


def restated_faba_select(dist, r, power=2, return_info=False):
    """(kept (n) bool, order: the removed rows in removal order): the key (bad descending, s descending by value, row
    ascending), one fp64 subtraction or one decrement a row and step from row q of the matrix, r steps and on while a kept
    row's bad count is positive; a matrix without any usable entry judges nobody."""
    c = np.asarray(dist, dtype=np.float32)
    n = c.shape[0]
    s, bad = restated_initial(c, power)
    judged = bool((bad < n - 1).any())
    kept = np.ones(n, dtype=bool)
    rows = np.arange(n)
    order, last = [], 0.0
    for step in range(n):
        idx = np.flatnonzero(kept)
        cand = idx[bad[idx] == bad[idx].max()]
        q = int(cand[s[cand] == s[cand].max()][0])
        if step >= r and bad[q] == 0 and judged:
            break
        kept[q] = False
        order.append(q)
        last = float(s[q])
        ok = usable(c[q])
        others = rows != q
        with np.errstate(invalid='ignore', over='ignore'):
            s = np.where(others & ok, s - terms(c[q], power), s)
        bad = bad - (others & ~ok)
    order = np.asarray(order, dtype=np.int64)
    if not return_info:
        return kept, order
    info = {'removed': len(order), 'kept': int(kept.sum()), 'forced': max(len(order) - int(r), 0), 'last_score': last,
            'divisor': float(kept.sum())}
    return kept, order, info


def direct_faba(g, r):
    """FABA as the paper writes it, in fp64: (order, the smallest relative gap between the two largest scores of a step)."""
    g = np.asarray(g, dtype=np.float64)
    kept = np.ones(g.shape[0], dtype=bool)
    order, gap = [], np.inf
    for _ in range(r):
        idx = np.flatnonzero(kept)
        score = ((g[idx] - g[idx].mean(axis=0)) ** 2).sum(axis=1)
        top = np.sort(score)[-2:]
        gap = min(gap, (top[1] - top[0]) / top[1])
        q = int(idx[np.argmax(score)])
        kept[q] = False
        order.append(q)
    return np.asarray(order, dtype=np.int64), gap


def euclidean_f32(g):
    """the pairwise distances in fp64 on the differences, rounded once to fp32, the diagonal +inf: a `Distances` matrix"""
    g = np.asarray(g, dtype=np.float64)
    d = np.stack([np.sqrt(((g - row) ** 2).sum(axis=1)) for row in g]).astype(np.float32)
    d = np.maximum(d, d.T)                      # symmetric as bits
    np.fill_diagonal(d, np.inf)
    return d


def shifted_case(n, d, seed):
    """N(0, 1) rows, the first n // 5 shifted by 0.5 N(0, 1) (one shift vector: a cluster beside the crowd)"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d))
    g[:n // 5] += 0.5 * rng.standard_normal(d)
    return g.astype(np.float32)


def random_symmetric(n, seed, lo=0.5, hi=1.5):
    """a dense symmetric fp32 matrix of distinct-looking entries, the diagonal +inf: what the large shapes upload directly"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(lo, hi, size=(n, n)).astype(np.float32)
    a = np.triu(a, 1)
    a = a + a.T
    np.fill_diagonal(a, np.inf)
    return a


# ---- the restatement is FABA ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(6))
def test_the_restatement_is_the_direct_rule(seed):
    n, d, r = 65, 2000, 31
    g = shifted_case(n, d, seed)
    want, gap = direct_faba(g, r)
    print('seed %d: smallest relative gap between the top two direct scores %.3e' % (seed, gap))
    assert gap >= 1e-5
    kept, order = restated_faba_select(euclidean_f32(g), r, power=2)
    assert order.tolist() == want.tolist()
    assert kept.sum() == n - r and not kept[order].any()


def test_the_identity_behind_it():
    """|g_i - mean(S)|^2 = (1/m) sum_j |g_i - g_j|^2 - (1/(2 m^2)) sum_jk |g_j - g_k|^2 on a random set"""
    rng = np.random.default_rng(5)
    g = rng.standard_normal((17, 40))
    d2 = ((g[:, None, :] - g[None, :, :]) ** 2).sum(axis=2)
    m = g.shape[0]
    lhs = ((g - g.mean(axis=0)) ** 2).sum(axis=1)
    rhs = d2.sum(axis=1) / m - d2.sum() / (2.0 * m * m)
    assert np.abs(lhs - rhs).max() <= 1e-12 * lhs.max()


# ---- the properties of the rule -----------------------------------------------------------------------------------------------
def test_r_zero_keeps_every_row():
    kept, order = restated_faba_select(random_symmetric(40, 1), 0)
    assert kept.all() and order.size == 0


def test_the_full_peeling_keeps_one_row():
    kept, order, info = restated_faba_select(random_symmetric(40, 2), 39, return_info=True)
    assert kept.sum() == 1 and sorted(order.tolist() + np.flatnonzero(kept).tolist()) == list(range(40))
    assert info == {'removed': 39, 'kept': 1, 'forced': 0, 'last_score': info['last_score'], 'divisor': 1.0}


@pytest.mark.parametrize('power', [1, 2])
def test_duplicates_go_lowest_row_first(power):
    rng = np.random.default_rng(3)
    g = rng.standard_normal((20, 50)).astype(np.float32)
    g[[3, 8, 11, 15]] = 4.0 * rng.standard_normal(50).astype(np.float32)      # one far block of identical rows
    kept, order = restated_faba_select(euclidean_f32(g), 4, power=power)
    assert order.tolist() == [3, 8, 11, 15]


def test_broken_rows_go_first_and_count_towards_r():
    c = random_symmetric(30, 4)
    for b in (7, 2, 19):
        c[b, :] = np.nan
        c[:, b] = np.nan
    np.fill_diagonal(c, np.inf)
    kept, order, info = restated_faba_select(c, 5, return_info=True)
    assert order[:3].tolist() == [2, 7, 19] and order.size == 5 and info['forced'] == 0
    # more broken rows than r: every one of them still goes, and nobody else
    kept, order, info = restated_faba_select(c, 1, return_info=True)
    assert order.tolist() == [2, 7, 19] and info == {'removed': 3, 'kept': 27, 'forced': 2, 'last_score': 0.0, 'divisor': 27.0}
    kept, order = restated_faba_select(c, 0)
    assert order.tolist() == [2, 7, 19]


@pytest.mark.parametrize('value', [np.inf, np.nan, -1.0])
def test_one_unusable_pair_costs_one_of_its_two_rows(value):
    c = random_symmetric(25, 6)
    c[4, 17] = c[17, 4] = value
    kept, order = restated_faba_select(c, 0)
    assert order.size == 1 and order[0] in (4, 17) and kept.sum() == 24
    s, bad = restated_initial(c)
    assert order[0] == (4 if s[4] >= s[17] else 17)          # the one with the larger sum; equal sums: the lower row


def test_negative_zero_is_a_usable_zero():
    c = random_symmetric(12, 7)
    c[2, 5] = c[5, 2] = -0.0
    s, bad = restated_initial(c, power=1)
    assert bad.sum() == 0 and not np.signbit(s).any()
    kept, order = restated_faba_select(c, 0, power=1)
    assert kept.all()


def test_an_all_nan_matrix_keeps_nobody():
    for n in (2, 9):
        c = np.full((n, n), np.nan, dtype=np.float32)
        kept, order, info = restated_faba_select(c, 0, return_info=True)
        assert not kept.any() and order.tolist() == list(range(n))
        assert info == {'removed': n, 'kept': 0, 'forced': n, 'last_score': 0.0, 'divisor': 0.0}


def test_the_initial_sums_are_the_stated_chains():
    """against a scalar walk of the header's sentence on a small matrix, both powers"""
    c = random_symmetric(131, 8)
    c[5, 9] = c[9, 5] = np.nan
    for power in (1, 2):
        s, bad = restated_initial(c, power)
        for i in (0, 5, 64, 130):
            chain = [0.0] * 64
            for j in range(131):
                if j != i and np.isfinite(c[i, j]) and c[i, j] >= 0:
                    e = float(c[i, j])
                    chain[j % 64] = chain[j % 64] + (e * e if power == 2 else e)
            for h in (32, 16, 8, 4, 2, 1):
                for lane in range(h):
                    chain[lane] = chain[lane] + chain[lane + h]
            assert chain[0] == s[i] and bad[i] == (1 if i in (5, 9) else 0)


# ---- the surface ------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_new_entry_points_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    assert '#define BYZ_ABI_VERSION 1\n' in text
    assert 'BYZ_K_MISC = 8, BYZ_K_PLANE_SPLIT = 9, BYZ_K_COUNT = 10' in text          # the timing enum did not change
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    assert '64 chains' in text and 'bad descending, s descending by value, row ascending' in text


def test_the_ctypes_table_lists_them():
    import ctypes
    from attacking_federate_learning_amd import _native
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS, name
    i64, vp, f64, i = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    P = ctypes.POINTER
    assert _native._PROTOTYPES['byz_faba_select_dev'] == [vp, vp, i64, i64, i, vp, vp, vp]
    assert _native._PROTOTYPES['byz_faba_dev'] == [vp, vp, i64, i64, i64, i64, vp, vp, vp, vp, vp]
    assert _native._PROTOTYPES['byz_faba_info'] == [vp, P(i64), P(i64), P(i64), P(f64), P(f64)]
    assert _native._PROTOTYPES['byz_faba_host'] == [vp, vp, i64, i64, i64, vp, vp, vp, vp]


def test_the_source_is_on_the_build_list():
    from attacking_federate_learning_amd import build_native
    assert 'faba.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['faba.hip']


def test_the_report_joins_the_typed_block():
    text = open(os.path.join(ROOT, 'attacking_federate_learning_amd', 'csrc', 'device_scalars.hpp')).read()
    assert re.search(r'struct FabaReport \{', text) and re.search(r'FabaReport faba;', text)
    assert 'sizeof(FabaReport)' in text and 'BYZ_AT(faba.last_score)' in text and 'BYZ_AT(faba.kept_f64)' in text
    assert re.search(r'kReportFaba, kReportCount', text)


def test_python_surface():
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.faba)) == '(users_grads, users_count, corrupted_count, distances=None, return_info=False)'
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert defences.faba not in defences.defend.values()
    doc = defences.faba.__doc__
    assert 'drift attack' in doc and 'FAR from the crowd' in doc and 'users_count >= 2*corrupted_count + 1' in doc
    assert str(inspect.signature(Engine.faba_select)) == (
        '(self, distances, remove_count, power=2, on_device=False, like=None, return_order=False)')
    assert str(inspect.signature(Engine.faba)) == '(self, g, users_count, corrupted_count, distances=None, return_info=False)'
    assert str(inspect.signature(Engine.faba_info)) == '(self)'
    assert str(inspect.signature(DeviceServer.defend_faba)) == '(self)'
    assert callable(ShardedAggregator.faba) and callable(HipKernels.faba_select)


def test_the_assertion_needs_no_gpu():
    from attacking_federate_learning_amd import defences
    g = np.zeros((6, 4), dtype=np.float32)
    with pytest.raises(AssertionError):
        defences.faba(g, 6, 3)


def test_the_refusals_that_need_no_gpu():
    from attacking_federate_learning_amd.engine import Engine
    assert Engine._faba_args(2, 0) == (0, 2)
    assert Engine._faba_args(2, 1, 1) == (1, 1)
    assert Engine._faba_args(16384, 16383, 2) == (16383, 2)
    for n, r, power in ((1, 0, 2), (10, -1, 2), (10, 10, 2), (10, 3, 0), (10, 3, 3), (10, 3, 2.5)):
        with pytest.raises(ValueError):
            Engine._faba_args(n, r, power)
    with pytest.raises(NotImplementedError):
        Engine._faba_args(16385, 3, 2)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    from attacking_federate_learning_amd import defences
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_faba', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.faba is defences.faba and 'faba' not in mod.defend


def test_the_documents_name_the_new_entry_points():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert name in integration, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '3.4q' in design and 'byz_faba_select_dev' in design
    papers = open(os.path.join(ROOT, 'PAPERS.md')).read()
    assert 'FABA' in papers and 'IJCAI 2019' in papers
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'defences.faba' in readme and 'faba.hip' in readme
    assert 'faba_timing.md' in open(os.path.join(ROOT, 'profiles', 'INDEX.md')).read()
