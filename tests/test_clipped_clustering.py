"""ClippedClustering and the agglomerative linkage under it, on the CPU: the rule of include/byzagg.h restated in
numpy, held to scipy and scikit-learn, and the surface of the new entry points.

The restatement IS the contract the device is compared with bit for bit (tests/test_gpu_clipped_clustering.py): the merge order
(distance, lower slot, higher slot), the Lance-Williams update in fp64 in the stated order of operations, the cut numbered by
lowest row, the larger cluster with ties to the lowest usable row.  scipy merges in nearest-neighbour-chain order, so its
roundings differ: sorted heights are compared within 1e-12 relative, and the two-way partition only on inputs whose last two
restated heights differ by more than 1e-9 relative -- an input that violates that gap FAILS, it is not skipped."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ('byz_linkage_dev', 'byz_linkage_info', 'byz_linkage_cut_dev', 'byz_clipped_clustering_select_dev',
               'byz_clipped_clustering_dev', 'byz_clipped_clustering_info', 'byz_clipped_clustering_host',
               'byz_clipped_clustering_sharded_dev')
METHODS = ('average', 'complete', 'single')


# ---- the restatement ------------------------------------------------------------------------------------------------------
def restated_working_copy(dist, fill=2.0):
    """(W, usable): the fp64 working copy, entry (i, j) read from the lower triangle; usable = a finite off-diagonal entry."""
    d = np.asarray(dist, dtype=np.float32)
    n = d.shape[0]
    sym = np.where(np.tri(n, n, -1, dtype=bool), d, d.T)      # (i, j) and (j, i) both from the entry below the diagonal
    off = ~np.eye(n, dtype=bool)
    usable = (np.isfinite(sym) & off).any(axis=1)
    w = sym.astype(np.float64)
    w[~np.isfinite(w) | (w < 0)] = float(fill)
    w = np.where(w == 0.0, 0.0, w)                  # -0.0 counts as +0.0
    np.fill_diagonal(w, 0.0)
    return w, usable


def restated_linkage(dist, method='average', fill=2.0):
    """(pair (u - 1, 2), height (u - 1), size (u - 1), usable (n)) of include/byzagg.h's rule."""
    w, usable = restated_working_copy(dist, fill)
    n = w.shape[0]
    active = usable.copy()
    sizes = np.ones(n, dtype=np.float64)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    u = int(usable.sum())
    pair, height, size = np.zeros((max(u - 1, 0), 2), np.int32), np.zeros(max(u - 1, 0)), np.zeros(max(u - 1, 0), np.int32)
    for t in range(u - 1):
        cand = np.where(upper & active[:, None] & active[None, :], w, np.inf)
        flat = int(np.argmin(cand))                 # the first minimum in row-major order: (distance, a, b) with a < b
        a, b = divmod(flat, n)
        assert active[a] and active[b] and a < b
        pair[t], height[t], size[t] = (a, b), w[a, b], int(sizes[a] + sizes[b])
        k = active.copy()
        k[[a, b]] = False
        if method == 'average':
            new = (sizes[a] * w[a, k] + sizes[b] * w[b, k]) / (sizes[a] + sizes[b])
        elif method == 'complete':
            new = np.maximum(w[a, k], w[b, k])
        else:
            new = np.minimum(w[a, k], w[b, k])
        w[a, k] = new
        w[k, a] = new
        active[b] = False
        sizes[a] += sizes[b]
    return pair, height, size, usable


def restated_cut(pair, usable, n_clusters):
    """(labels, sizes): the first u - c merges replayed; clusters numbered by their lowest row, -1 for a row that is not usable."""
    n = usable.size
    root = np.arange(n)
    for a, b in pair[:max(int(usable.sum()) - n_clusters, 0)]:
        root[root == b] = a
    labels = np.full(n, -1, dtype=np.int32)
    lowest = sorted(set(root[usable]))              # a cluster's slot is its lowest row
    for number, r in enumerate(lowest):
        labels[usable & (root == r)] = number
    sizes = np.zeros(n_clusters, dtype=np.int32)
    for number in range(min(len(lowest), n_clusters)):
        sizes[number] = int((labels == number).sum())
    return labels, sizes


def restated_select(dist, method='average', fill=2.0):
    """The admitted mask: the larger of two clusters, the lowest usable row's cluster on a tie."""
    pair, _, _, usable = restated_linkage(dist, method, fill)
    labels, sizes = restated_cut(pair, usable, 2)
    return labels == (1 if sizes[1] > sizes[0] else 0)


def restated_clip_scales(g, clip=None):
    """(s, clip): s_i = 1, clip / d_i or 0 (a row that is not finite), clip=None: the median of the finite norms."""
    d = np.sqrt((np.asarray(g, dtype=np.float64) ** 2).sum(axis=1))
    finite = np.isfinite(d)
    if clip is None:
        clip = float(np.median(d[finite])) if finite.any() else 0.0
    with np.errstate(all='ignore'):
        s = np.where(finite, np.where(d <= clip, 1.0, clip / d), 0.0)
    return s, clip


def restated_clipped_clustering(g, clip=None, method='average', fill=2.0, dist=None):
    """(vector in fp64, admitted mask, clip) of the whole rule; dist=None: the fp64 cosine matrix rounded to float32."""
    from tests.test_flame import restated_cosine
    g = np.asarray(g, dtype=np.float32)
    if dist is None:
        dist = restated_cosine(g).astype(np.float32)
    admitted = restated_select(dist, method, fill)
    s, clip = restated_clip_scales(g, clip)
    count = int(admitted.sum())
    if count == 0:
        return np.zeros(g.shape[1]), admitted, clip
    rows = np.where(np.isfinite(g[admitted].astype(np.float64)).all(axis=1, keepdims=True), g[admitted].astype(np.float64), 0.0)
    return (s[admitted][:, None] * rows).sum(axis=0) / count, admitted, clip


def to_scipy(pair, height, size, usable):
    """scipy's linkage matrix over the usable rows from the rule's merges (Engine.linkage's relabelling)."""
    u = int(usable.sum())
    ident = np.full(usable.size, -1, dtype=np.int64)
    ident[usable] = np.arange(u)
    z = np.zeros((max(u - 1, 0), 4))
    for t in range(z.shape[0]):
        a, b = pair[t]
        z[t] = (min(ident[a], ident[b]), max(ident[a], ident[b]), height[t], size[t])
        ident[a] = u + t
    return z


def same_partition(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return np.array_equal(x[:, None] == x[None, :], y[:, None] == y[None, :])


# ---- the cases ------------------------------------------------------------------------------------------------------------
def cosine_case(kind, n, d, seed):
    """float32 cosine matrices (diagonal +inf): 'cloud' one Gaussian cloud round a mean, 'minority' a quarter of the rows pointing
    the other way, 'twins' with blocks of duplicate rows."""
    from tests.test_flame import restated_cosine
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal(d)
    g = mu + rng.standard_normal((n, d))
    if kind == 'minority':
        g[:n // 4] = -4.0 * mu + 0.1 * rng.standard_normal((n // 4, d))
    if kind == 'twins':
        g[1::3] = g[0::3][:len(g[1::3])]
    return g.astype(np.float32), restated_cosine(g.astype(np.float32)).astype(np.float32)


def planted(n, d, seed):
    """Section 1's planted cases: a quarter of the rows, the first ones, set to -4 mu + 0.1 noise."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal(d)
    g = (mu + rng.standard_normal((n, d))).astype(np.float32)
    f = n // 4
    g[:f] = (-4.0 * mu + 0.1 * rng.standard_normal((f, d))).astype(np.float32)
    return g, f


CASES = [(kind, n, 40 + 3 * n, 1000 * i + n) for i, kind in enumerate(('cloud', 'minority', 'twins')) for n in (3, 4, 7, 16, 33, 69)]


@pytest.mark.parametrize('method', METHODS)
def test_the_restatement_is_scipy_and_sklearn(method):
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    from sklearn.cluster import AgglomerativeClustering
    worst = 0.0
    for kind, n, d, seed in CASES:
        _, c = cosine_case(kind, n, d, seed)
        pair, height, size, usable = restated_linkage(c, method)
        assert usable.all() and len(height) == n - 1 and size[-1] == n
        assert (np.diff(height) >= -1e-15).all()                       # the three linkages are monotone
        w, _ = restated_working_copy(c)
        z = linkage(squareform(w, checks=False), method=method)
        rel = np.abs(np.sort(height) - z[:, 2]) / np.maximum(z[:, 2], 1e-300)
        rel = rel[z[:, 2] > 0]
        worst = max(worst, float(rel.max()) if rel.size else 0.0)
        assert (rel <= 1e-12).all(), (kind, n, float(rel.max()))
        assert np.array_equal(np.sort(height)[z[:, 2] == 0], z[:, 2][z[:, 2] == 0])
        if n < 3:
            continue
        gap = (height[-1] - height[-2]) / height[-1]
        assert gap > 1e-9, ('the case must separate its last two merges', kind, n, gap)      # a condition on the input: no skip
        labels, sizes = restated_cut(pair, usable, 2)
        assert same_partition(labels, fcluster(z, 2, 'maxclust')), (kind, n)
        assert same_partition(labels, fcluster(to_scipy(pair, height, size, usable), 2, 'maxclust')), (kind, n)
        sk = AgglomerativeClustering(n_clusters=2, metric='precomputed', linkage=method).fit(w)
        assert same_partition(labels, sk.labels_), (kind, n)
        assert sizes.sum() == n and labels.min() == 0 and labels[0] == 0
    assert worst <= 1e-12


def test_the_planted_minority_is_rejected_exactly():
    from sklearn.cluster import AgglomerativeClustering
    for n in (9, 65, 130):
        for d in (33, 257, 1025):
            g, f = planted(n, d, seed=7 * n + d)
            out, admitted, clip = restated_clipped_clustering(g)
            assert np.array_equal(np.flatnonzero(admitted), np.arange(f, n)), (n, d)
            from tests.test_flame import restated_cosine
            c = restated_cosine(g).astype(np.float32)
            _, height, _, _ = restated_linkage(c)
            assert (height[-1] - height[-2]) / height[-1] > 0.5, (n, d)
            w, _ = restated_working_copy(c)
            sk = AgglomerativeClustering(n_clusters=2, metric='precomputed', linkage='average').fit(w).labels_
            larger = sk == np.argmax(np.bincount(sk))
            assert np.array_equal(larger, admitted)
            s, _ = restated_clip_scales(g)
            assert clip == np.median(np.sqrt((g.astype(np.float64) ** 2).sum(1))) and (s[admitted] <= 1).all()
            assert np.allclose(out, (s[f:, None] * g[f:].astype(np.float64)).mean(axis=0), rtol=1e-12, atol=0)


def test_the_sanitisation_rules():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    d = np.array([[inf, 0.1, 0.5, inf, 0.7],
                  [0.1, inf, -0.0, inf, nan],
                  [0.5, -0.0, inf, inf, -3.0],
                  [inf, inf, inf, inf, inf],
                  [0.7, nan, -3.0, inf, inf]], dtype=np.float32)
    w, usable = restated_working_copy(d, fill=2.0)
    assert usable.tolist() == [True, True, True, False, True]
    assert w[4, 1] == 2.0 and w[1, 4] == 2.0 and w[4, 2] == 2.0                 # NaN and a negative entry: fill
    assert w[2, 1] == 0.0 and not np.signbit(w[2, 1]) and not np.signbit(w[1, 2])  # -0.0 counts as +0.0
    assert np.array_equal(w, w.T)
    pair, height, size, _ = restated_linkage(d, 'average', fill=2.0)
    assert pair.tolist() == [[1, 2], [0, 1], [0, 4]] and size.tolist() == [2, 3, 4]
    assert height[0] == 0.0 and height[1] == (np.float64(np.float32(0.1)) + np.float64(np.float32(0.5))) / 2.0
    for c in (1, 2, 3, 4):
        labels, sizes = restated_cut(pair, usable, c)
        assert labels[3] == -1 and sorted(set(labels[usable])) == list(range(c)) and sizes.sum() == 4
    labels, _ = restated_cut(pair, usable, 3)
    assert labels.tolist() == [0, 1, 1, -1, 2]                                  # numbered by lowest row
    # the entry is read from the LOWER triangle: garbage above the diagonal changes nothing
    noisy = d.copy()
    noisy[np.triu_indices(5, 1)] = 9.0
    assert np.array_equal(restated_working_copy(noisy)[0], w)
    # a different fill moves the last merge
    assert restated_linkage(d, 'average', fill=0.25)[1][-1] < height[-1]
    # nobody usable, one usable
    none = np.full((4, 4), inf, dtype=np.float32)
    assert not restated_select(none).any()
    one = none.copy()
    one[2, 1] = nan
    assert not restated_select(one).any()
    out, admitted, _ = restated_clipped_clustering(np.zeros((4, 6), np.float32))
    assert not admitted.any() and not out.any()


def test_the_tie_goes_to_the_cluster_of_the_lowest_usable_row():
    inf = np.float32(np.inf)
    # rows {1, 3} against rows {2, 4}, row 0 not usable: two clusters of two; the lowest usable row is 1
    d = np.full((5, 5), 1.0, dtype=np.float32)
    d[0, :] = d[:, 0] = inf
    np.fill_diagonal(d, inf)
    d[3, 1] = d[1, 3] = 0.1
    d[4, 2] = d[2, 4] = 0.1
    for method in METHODS:
        assert np.flatnonzero(restated_select(d, method)).tolist() == [1, 3]
    # the same with the other pair first: the rule follows the lowest usable row, not the merge order
    d[3, 1] = d[1, 3] = 0.2
    for method in METHODS:
        assert np.flatnonzero(restated_select(d, method)).tolist() == [1, 3]
    # all distances equal: every choice is a tie broken by index -- (0, 1), (0, 2), ... -- and the last row stands alone
    e = np.full((6, 6), 0.5, dtype=np.float32)
    np.fill_diagonal(e, inf)
    pair, height, size, _ = restated_linkage(e, 'average')
    assert pair.tolist() == [[0, k] for k in range(1, 6)] and (height == 0.5).all()
    assert np.flatnonzero(restated_select(e)).tolist() == [0, 1, 2, 3, 4]


# ---- the surface ------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_new_entry_points_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    assert '#define BYZ_ABI_VERSION 1\n' in text
    assert 'BYZ_K_MISC = 8, BYZ_K_PLANE_SPLIT = 9, BYZ_K_COUNT = 10' in text          # the timing enum did not change
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    fields = re.search(r'typedef struct byz_clipped_clustering_params \{(.*?)\}', code, flags=re.S).group(1)
    assert re.findall(r'(\w+);', fields) == ['clip', 'adaptive', 'method', 'fill']
    for name in ('byz_linkage_dev', 'byz_clipped_clustering_select_dev', 'byz_clipped_clustering_dev'):      # no doubles by value
        assert not re.search(r'\bdouble\s+\w+\s*[,)]', re.search(r'int\s+%s\s*\((.*?)\)' % name, code, flags=re.S).group(1))
    assert re.search(r'#define BYZ_LINKAGE_AVERAGE 0\n#define BYZ_LINKAGE_COMPLETE 1\n#define BYZ_LINKAGE_SINGLE 2\n', text)


def test_the_ctypes_table_lists_them():
    import ctypes
    from attacking_federate_learning_amd import _native
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS, name
    i64, vp, f64, i = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    P = ctypes.POINTER
    params = P(_native.ClippedClusteringParams)
    assert _native._PROTOTYPES['byz_linkage_dev'] == [vp, vp, i64, i, P(f64), vp, vp, vp, vp, vp]
    assert _native._PROTOTYPES['byz_linkage_cut_dev'] == [vp, vp, i64, vp, i64, vp, vp, vp]
    assert _native._PROTOTYPES['byz_clipped_clustering_select_dev'] == [vp, vp, i64, i, P(f64), vp, vp]
    assert _native._PROTOTYPES['byz_clipped_clustering_dev'] == [vp, vp, i64, i64, i64, params, vp, vp, vp, vp, vp]
    assert _native._PROTOTYPES['byz_clipped_clustering_info'] == [vp, P(i64), P(i64), P(f64), P(f64), P(f64)]
    assert _native._PROTOTYPES['byz_clipped_clustering_host'] == [vp, vp, i64, i64, params, vp, vp, vp, vp]
    assert _native._PROTOTYPES['byz_clipped_clustering_sharded_dev'] == [vp, vp, i64, i64, i64, params, vp, vp, vp, vp, vp, vp]
    assert [f[0] for f in _native.ClippedClusteringParams._fields_] == ['clip', 'adaptive', 'method', 'fill']
    assert ctypes.sizeof(_native.ClippedClusteringParams) == 24


def test_the_source_is_on_the_build_list():
    from attacking_federate_learning_amd import build_native
    assert 'linkage.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['linkage.hip']


def test_python_surface():
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.clipped_clustering)) == (
        "(users_grads, users_count, corrupted_count, clip=None, method='average', distances=None, norm_history=None, "
        'max_tau=100000.0, return_info=False)')
    assert str(inspect.signature(defences.linkage_labels)) == "(distances, n_clusters=2, method='average', fill=2.0)"
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert defences.clipped_clustering not in defences.defend.values()
    doc = defences.clipped_clustering.__doc__
    assert 'UNCLIPPED' in doc and 'Blades clips first' in doc and 'ALWAYS rejects somebody' in doc
    assert 'ONE synchronisation' in doc and 'lowest usable row' in doc
    assert str(inspect.signature(Engine.linkage)) == "(self, distances, method='average', fill=2.0)"
    assert callable(Engine.linkage_cut) and callable(Engine.clipped_clustering_select) and callable(Engine.clipped_clustering)
    assert callable(Engine.clipped_clustering_info) and callable(Engine.linkage_info)
    assert str(inspect.signature(DeviceServer.defend_clipped_clustering)) == "(self, method='average', max_tau=100000.0)"
    assert 'clipped_clustering_norms' in DeviceServer.defend_clipped_clustering.__doc__
    assert callable(ShardedAggregator.clipped_clustering) and callable(HipKernels.clipped_clustering_select)


def test_the_refusals_that_need_no_gpu():
    from attacking_federate_learning_amd.engine import Engine
    assert Engine._linkage_args(2, 'average', 2.0) == (0, 2.0)
    assert Engine._linkage_args(16384, 'complete', 0.0) == (1, 0.0)
    assert Engine._linkage_args(100, 'single', 1) == (2, 1.0)
    for n, method, fill in ((1, 'average', 2.0), (10, 'ward', 2.0), (10, 0, 2.0), (10, 'average', -1.0),
                            (10, 'average', float('nan')), (10, 'average', float('inf'))):
        with pytest.raises(ValueError):
            Engine._linkage_args(n, method, fill)
    with pytest.raises(NotImplementedError):
        Engine._linkage_args(16385, 'average', 2.0)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    from attacking_federate_learning_amd import defences
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_clipped_clustering', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.clipped_clustering is defences.clipped_clustering and mod.linkage_labels is defences.linkage_labels
    assert 'clipped_clustering' not in mod.defend


def test_the_documents_name_the_new_entry_points():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert name in integration, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '3.4o' in design and 'nearest-partner' in design
    papers = open(os.path.join(ROOT, 'PAPERS.md')).read()
    assert 'Voigt' in papers and 'llner' in papers
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'defences.clipped_clustering' in readme and 'linkage.hip' in readme
