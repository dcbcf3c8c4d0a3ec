"""FLAME (Nguyen et al., USENIX Security 2022) without a GPU: the numpy restatement of the clustering rule against scikit-learn's
HDBSCAN, csrc/flame_tree.hpp on the host (plain and under the host sanitizers), and the surface -- header, ctypes table,
signatures, the refusals that need no device.

The rule (include/byzagg.h): with m = min_cluster_size, 2 m > n, two clusters cannot coexist and HDBSCAN with
metric='precomputed', allow_single_cluster=True admits exactly the connected component of at least m vertices of the mutual
reachability graph cut at the smallest threshold that has one.  tests/test_gpu_flame.py imports restated_flame_select."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, 'attacking_federate_learning_amd', 'csrc')

NEW_SYMBOLS = ('byz_cosine_distances_dev', 'byz_cosine_from_gram_dev', 'byz_flame_core_distances_dev', 'byz_flame_select_dev', 'byz_flame_dev', 'byz_flame_info',
               'byz_flame_host', 'byz_flame_sharded_dev')


# ---- the restatement ------------------------------------------------------------------------------------------------------
def restated_cosine(g):
    """The cosine distances of g's rows in fp64 (diagonal +inf; a zero or non-finite row's row and column +inf)."""
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(all='ignore'):
        gram = g @ g.T
        diag = np.diagonal(gram).copy()
        ok = np.isfinite(diag) & (diag > 0)
        root = np.sqrt(np.where(ok, diag, 1.0))
        c = np.maximum(0.0, 1.0 - gram / (root[:, None] * root[None, :]))
    c[~np.isfinite(c)] = np.inf
    c[~ok, :] = np.inf
    c[:, ~ok] = np.inf
    np.fill_diagonal(c, np.inf)
    return c


def restated_core(c, ms):
    """core_i: the ms-th smallest off-diagonal entry of row i (ms = 0: 0); a NaN sorts behind +inf, -inf counts as +inf.  In c's
    own dtype, a block of rows at a time (the largest case is 16,384 x 16,384)."""
    c = np.asarray(c)
    n = c.shape[0]
    core = np.zeros(n, dtype=c.dtype)
    if ms == 0:
        return core
    for r0 in range(0, n, 1024):
        blk = np.array(c[r0:r0 + 1024])
        blk[blk == -np.inf] = np.inf
        rows = np.arange(blk.shape[0])
        blk[rows, r0 + rows] = np.nan                  # the diagonal sorts last, behind the n - 1 others (NaN: np.sort's order)
        if ms == 1:                                    # the row minimum; np.fmin passes over a NaN unless there is nothing else
            core[r0:r0 + 1024] = np.fmin.reduce(blk, axis=1)
        else:
            core[r0:r0 + 1024] = np.partition(blk, ms - 1, axis=1)[:, ms - 1]
    return core


def restated_flame_select(c, m, ms):
    """(mask, w_star) of the rule on the symmetric matrix c (any float dtype, diagonal ignored): Prim on the mutual
    reachability R_ij = max(c_ij, core_i, core_j), the tree's edges ascending through a union-find until a component holds m
    vertices, edges tied at that weight still merged, non-finite weights never.  Only comparisons of c's own values: exact in
    any dtype.  Nobody admitted: w_star = +inf."""
    c = np.asarray(c)
    n = c.shape[0]
    assert c.shape == (n, n) and 2 * m > n and 2 <= m <= n and 0 <= ms <= n - 1
    core = restated_core(c, ms)
    outside = np.ones(n, dtype=bool)
    block = np.zeros(n, dtype=c.dtype)                 # +inf at the tree's vertices: their keys are never touched again
    key = np.full(n, np.inf, dtype=c.dtype)            # (of the vertices outside the tree; +inf inside)
    parent = np.zeros(n, dtype=np.int64)
    outside[0], block[0] = False, np.inf
    u, edges = 0, []
    with np.errstate(invalid='ignore'):
        for _ in range(n - 1):
            row = np.maximum(np.maximum(c[u], core[u]), core)
            if np.isneginf(row).any():
                row[np.isneginf(row)] = np.inf
            np.maximum(row, block, out=row)
            better = row < key                                        # (a NaN is never better: it merges nothing anyway)
            np.copyto(key, row, where=better)
            np.copyto(parent, u, where=better)
            u = int(np.argmin(key))
            if not key[u] < np.inf:                                   # only infinite keys are left: any vertex outside
                u = int(np.flatnonzero(outside)[0])
            edges.append((float(key[u]), int(parent[u]), u))
            key[u] = block[u] = np.inf
            outside[u] = False
    edges.sort(key=lambda e: e[0])
    root, size = list(range(n)), [1] * n

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x
    w_star = None
    for w, a, b in edges:
        if not np.isfinite(w) or (w_star is not None and w != w_star):
            break
        ra, rb = find(a), find(b)
        if ra != rb:
            if size[ra] < size[rb]:
                ra, rb = rb, ra
            root[rb] = ra
            size[ra] += size[rb]
            if w_star is None and size[ra] >= m:
                w_star = w
    if w_star is None:
        return np.zeros(n, dtype=bool), np.inf
    return np.array([size[find(v)] >= m for v in range(n)]), float(w_star)


def family(kind, n, d, rng):
    """The four families of the issue: gaussian rows, a tight shifted third, rows rounded to halves (distances tie), a quarter
    of the rows duplicates."""
    g = rng.standard_normal((n, d)).astype(np.float32)
    if kind == 1:
        f = n // 3
        g[:f] = g[:f] * 0.1 + (rng.standard_normal(d) * 3).astype(np.float32)
    elif kind == 2:
        g = np.round(g * 2) / 2
        g[np.abs(g).sum(1) == 0, 0] = 1
    elif kind == 3:
        g[:max(1, n // 4)] = g[0]
    return g


def test_the_restatement_is_hdbscan_on_every_case():
    sklearn_cluster = pytest.importorskip('sklearn.cluster')
    rng = np.random.default_rng(2022)
    cases = 0
    for trial in range(120):
        n, d = int(rng.integers(5, 60)), int(rng.integers(3, 40))
        g = family(trial % 4, n, d, rng)
        c = restated_cosine(g)
        assert np.isfinite(c[~np.eye(n, dtype=bool)]).all()
        np.fill_diagonal(c, 0.0)                       # scikit-learn asks for a zero diagonal; the restatement ignores it
        m = n // 2 + 1
        for ms in (0, 1, 2):
            model = sklearn_cluster.HDBSCAN(min_cluster_size=m, min_samples=ms + 1, allow_single_cluster=True, metric='precomputed',
                                            copy=True)
            labels = model.fit(c.copy()).labels_
            mask, w_star = restated_flame_select(c, m, ms)
            assert np.array_equal(labels == 0, mask), (trial, n, d, ms, int((labels == 0).sum()), int(mask.sum()))
            assert set(labels) <= {-1, 0}
            cases += 1
    assert cases >= 300


def test_the_rule_on_hand_made_matrices():
    inf = np.inf
    # two tight pairs and a loner: nobody reaches 3 before the pairs join at 0.5
    c = np.array([[inf, 0.1, 0.5, 0.6, 0.9], [0.1, inf, 0.55, 0.7, 0.9], [0.5, 0.55, inf, 0.1, 0.9], [0.6, 0.7, 0.1, inf, 0.9],
                  [0.9, 0.9, 0.9, 0.9, inf]])
    mask, w = restated_flame_select(c, 3, 0)
    assert mask.tolist() == [True, True, True, True, False] and w == 0.5
    # ties at w*: the edge that completes the component and its equals all count
    c = np.full((6, 6), 2.0)
    c[:4, :4] = 0.25
    np.fill_diagonal(c, inf)
    mask, w = restated_flame_select(c, 4, 1)
    assert mask.tolist() == [True] * 4 + [False] * 2 and w == 0.25
    # more than n - m broken rows: nobody, never NaN
    c = np.full((5, 5), 0.5)
    c[2:] = inf
    c[:, 2:] = inf
    mask, w = restated_flame_select(c, 3, 1)
    assert not mask.any() and w == inf
    # n = 2
    mask, w = restated_flame_select(np.array([[inf, 0.75], [0.75, inf]]), 2, 1)
    assert mask.all() and w == 0.75
    # min_samples raises the threshold: core distances enter the reachability
    c = np.array([[inf, 0.0, 0.0, 1.0], [0.0, inf, 0.0, 1.0], [0.0, 0.0, inf, 1.0], [1.0, 1.0, 1.0, inf]])
    assert restated_flame_select(c, 3, 1)[1] == 0.0 and restated_flame_select(c, 3, 3)[1] == 1.0


def test_the_cosine_restatement_breaks_zero_and_non_finite_rows():
    g = np.random.default_rng(3).standard_normal((6, 9)).astype(np.float32)
    g[1] = 0
    g[4, 2] = np.nan
    c = restated_cosine(g)
    off = ~np.eye(6, dtype=bool)
    assert np.isinf(c[1]).all() and np.isinf(c[:, 1]).all() and np.isinf(c[4]).all() and np.isinf(c[:, 4]).all()
    live = [0, 2, 3, 5]
    assert np.isfinite(c[np.ix_(live, live)][~np.eye(4, dtype=bool)]).all() and np.isinf(np.diagonal(c)).all()
    assert np.array_equal(c, c.T) and (c[off] >= 0).all()


# ---- csrc/flame_tree.hpp on the host ----------------------------------------------------------------------------------------
def _build_and_run(tmp_path, extra):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if compiler is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'flame_tree_check')
    build = subprocess.run([compiler, '-std=c++17', '-O1', '-Wall', '-I', CSRC] + extra +
                           [os.path.join(HERE, 'flame_tree_check.cpp'), '-o', exe], capture_output=True, text=True)
    return build, exe


def test_flame_tree_header_on_the_host(tmp_path):
    build, exe = _build_and_run(tmp_path, [])
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith('flame_tree ok'), run.stdout


def test_flame_tree_header_under_the_host_sanitizers(tmp_path):
    """The stand-alone program again with AddressSanitizer and UndefinedBehaviorSanitizer (a host build: nothing here is loaded
    into Python).  Whether the compiler has the sanitizers' runtime is asked of a trivial program first, so that a failure of
    the real build under these flags is a failure and not a skip."""
    flags = ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if compiler is None:
        pytest.skip('no host C++ compiler')
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    probed = subprocess.run([compiler, '-std=c++17'] + flags + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp_path / 'probe')], capture_output=True).returncode != 0:
        pytest.skip('the host compiler has no sanitizer runtime: ' + probed.stderr[-200:])
    build, exe = _build_and_run(tmp_path, flags)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith('flame_tree ok'), run.stdout


# ---- the surface ------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_new_entry_points_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    assert '#define BYZ_ABI_VERSION 1\n' in text
    assert 'BYZ_K_MISC = 8, BYZ_K_PLANE_SPLIT = 9, BYZ_K_COUNT = 10' in text          # the timing enum did not change
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    assert 'byz_flame_params' in code
    fields = re.search(r'typedef struct byz_flame_params \{(.*?)\}', code, flags=re.S).group(1)
    assert re.findall(r'(\w+);', fields) == ['lambda', 'min_samples', 'min_cluster_size', 'seed', 'round', 'column_offset']
    assert not re.search(r'\bdouble\s+\w+\s*[,)]', re.search(r'int\s+byz_flame_dev\s*\((.*?)\)', code, flags=re.S).group(1))


def test_the_ctypes_table_lists_them():
    import ctypes
    from attacking_federate_learning_amd import _native
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS, name
    i64, vp, f64 = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    P = ctypes.POINTER
    assert _native._PROTOTYPES['byz_cosine_distances_dev'] == [vp, vp, i64, i64, i64, vp, vp]
    assert _native._PROTOTYPES['byz_cosine_from_gram_dev'] == [vp, vp, i64, vp, vp]
    assert _native._PROTOTYPES['byz_flame_core_distances_dev'] == [vp, vp, i64, i64, vp, vp]
    assert _native._PROTOTYPES['byz_flame_select_dev'] == [vp, vp, i64, i64, i64, vp, vp]
    assert _native._PROTOTYPES['byz_flame_dev'] == [vp, vp, i64, i64, i64, P(_native.FlameParams), vp, vp, vp, vp]
    assert _native._PROTOTYPES['byz_flame_info'] == [vp, P(i64), P(i64), P(f64), P(f64)]
    assert _native._PROTOTYPES['byz_flame_host'] == [vp, vp, i64, i64, P(_native.FlameParams), vp, vp, vp]
    assert _native._PROTOTYPES['byz_flame_sharded_dev'] == [vp, vp, i64, i64, i64, P(_native.FlameParams), vp, vp, vp, vp, vp, vp]
    assert [f[0] for f in _native.FlameParams._fields_] == ['lam', 'min_samples', 'min_cluster_size', 'seed', 'round', 'column_offset']
    assert ctypes.sizeof(_native.FlameParams) == 48


def test_the_source_is_on_the_build_list():
    from attacking_federate_learning_amd import build_native
    assert 'flame.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['flame.hip']
    assert os.path.exists(os.path.join(CSRC, 'flame_tree.hpp'))


def test_python_surface():
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.flame)) == (
        '(users_grads, users_count, corrupted_count, lam=0.001, min_samples=1, min_cluster_size=None, seed=0, round=0, '
        'distances=None, return_info=False)')
    assert str(inspect.signature(defences.cosine_distances)) == '(users_grads)'
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    for fn in (defences.flame, defences.cosine_distances):
        assert fn not in defences.defend.values()
    assert 'flame' not in defences.defend and 'cosine_distances' not in defences.defend
    doc = defences.flame.__doc__
    assert '`hdbscan`' in doc and 'scikit-learn' in doc and 'one more' in doc
    assert "package's default" in doc and 'tunes it per task' in doc
    assert 'MODELS' in doc and '`distances=`' in doc
    assert str(inspect.signature(Engine.cosine_distances)) == '(self, g)'
    assert list(inspect.signature(Engine.flame_select).parameters)[:4] == ['self', 'distances', 'min_samples', 'min_cluster_size']
    assert inspect.signature(Engine.flame_select).parameters['min_samples'].default == 1
    assert inspect.signature(Engine.flame_select).parameters['min_cluster_size'].default is None
    assert callable(Engine.flame) and callable(Engine.flame_info) and callable(Engine.cosine_from_gram)
    assert str(inspect.signature(DeviceServer.defend_flame)) == '(self, lam=0.001, min_samples=1, seed=0)'
    assert 'flame_round' in DeviceServer.defend_flame.__doc__
    assert list(inspect.signature(ShardedAggregator.flame).parameters)[:5] == [
        'self', 'g_local', 'users_count', 'corrupted_count', 'column_offset']
    assert callable(HipKernels.cosine_from_gram) and callable(HipKernels.flame_select)


def test_the_refusals_that_need_no_gpu():
    from attacking_federate_learning_amd.engine import Engine
    assert Engine._flame_sizes(20, 1, None) == (1, 11)
    assert Engine._flame_sizes(5, 0, 5) == (0, 5)
    assert Engine._flame_sizes(16384, 32, None) == (32, 8193)
    for n, ms, m in ((20, 1, 10), (20, 1, 21), (20, 1, 1), (1, 0, None), (20, -1, None), (5, 5, None)):
        with pytest.raises(ValueError):
            Engine._flame_sizes(n, ms, m)
    with pytest.raises(NotImplementedError):
        Engine._flame_sizes(100, 33, None)
    with pytest.raises(NotImplementedError):
        Engine._flame_sizes(16385, 1, None)
    for lam in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            Engine._noise_params(lam, 0, 0, 0)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    from attacking_federate_learning_amd import defences
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_flame', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.flame is defences.flame and mod.cosine_distances is defences.cosine_distances and 'flame' not in mod.defend


def test_the_documents_name_the_new_entry_points():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert name in integration, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '3.4m' in design and 'minimum spanning tree' in design
    papers = open(os.path.join(ROOT, 'PAPERS.md')).read()
    assert 'Campello' in papers and 'Moulavi' in papers and 'Nguyen' in papers
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'defences.flame' in readme and 'not an answer to the drift attack' in readme
