"""Auror without a GPU: a numpy restatement of include/byzagg.h's rule (tests/test_gpu_auror.py holds the device to it), the
restatement against scikit-learn's Lloyd iterations and on planted poisoning, its edge cases, csrc/two_means.hpp on the host
(tests/two_means_check.cpp, built with the host sanitizers), and the surface: header, ctypes table, build list, Python layers,
documents.

The restatement sums in numpy's order, the device in its own; a sum of m fp32 values in fp64 is within m * 2^-53 * max|x| of
exact in any order.  So it also returns the smallest margins any of its decisions had -- min |x - t| over every sweep and
min |gap - alpha| -- and a comparison with another order of summation is sound where those margins exceed margin_bound()."""
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

NEW_SYMBOLS = ('byz_auror_votes_dev', 'byz_auror_select_dev', 'byz_auror_dev', 'byz_auror_info', 'byz_auror_host')


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def restated_auror_votes(g, alpha, max_iter=32):
    """include/byzagg.h's votes on an n x D float32 matrix, every column at once.  -> dict: votes (int64 n), bad (int32 n),
    counts (int64 4: indicative, clustered, capped, 0), gap (float64 D), t, m1, side, sweeps (per column), and the margins
    margin_t = min |x - t| over every finite value of every sweep, margin_alpha = min |gap - alpha| over the clustered columns."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    n, d = g.shape
    x = g.astype(np.float64)
    fin = np.isfinite(g)
    bad = (~fin).any(axis=1)
    m = fin.sum(axis=0)
    mn = np.where(fin, x, np.inf).min(axis=0, initial=np.inf)
    mx = np.where(fin, x, -np.inf).max(axis=0, initial=-np.inf)
    clustered = (m >= 2) & (mn < mx)
    c0, c1 = np.where(clustered, mn, 0.0), np.where(clustered, mx, 0.0)
    t = 0.5 * (c0 + c1)
    m1 = np.full(d, -1, dtype=np.int64)
    capped = np.zeros(d, dtype=bool)
    sweeps = np.zeros(d, dtype=np.int64)
    active = clustered.copy()
    margin_t = np.inf
    for k in range(1, int(max_iter) + 1):
        cols = np.flatnonzero(active)
        if cols.size == 0:
            break
        xa, fa = x[:, cols], fin[:, cols]
        ta = 0.5 * (c0[cols] + c1[cols])
        margin_t = min(margin_t, float(np.abs(xa - ta)[fa].min()))
        up = fa & (xa > ta)
        m1a = up.sum(axis=0)
        assert (m1a >= 1).all() and (m1a < m[cols]).all()        # min <= t < max: neither cluster is empty
        s1 = np.where(up, xa, 0.0).sum(axis=0)
        s0 = np.where(fa & ~up, xa, 0.0).sum(axis=0)
        c1[cols], c0[cols], t[cols] = s1 / m1a, s0 / (m[cols] - m1a), ta
        settled = (m1a == m1[cols]) if k >= 2 else np.zeros(cols.size, dtype=bool)
        m1[cols], sweeps[cols] = m1a, k
        if k == int(max_iter):
            capped[cols[~settled]] = True
            active[cols] = False
        else:
            active[cols[settled]] = False
    gap = np.where(clustered, c1 - c0, 0.0)
    indicative = clustered & (gap > alpha)
    margin_alpha = float(np.abs(gap[clustered] - alpha).min()) if clustered.any() else np.inf
    m0 = m - m1
    side = np.where(indicative & (m1 != m0), np.where(m1 < m0, 1, 0), -1)
    upper = fin & (x > t)
    vote = fin & (((side == 1) & upper) | ((side == 0) & ~upper))
    counts = np.array([indicative.sum(), clustered.sum(), capped.sum(), 0], dtype=np.int64)
    return dict(votes=vote.sum(axis=1).astype(np.int64), bad=bad.astype(np.int32), counts=counts, gap=gap, t=t, m1=m1, side=side,
                sweeps=sweeps, indicative=indicative, margin_t=margin_t, margin_alpha=margin_alpha, labels=upper)


def restated_auror_select(votes, bad, counts, tau):
    """-> the kept flags (bool n)"""
    votes, bad = np.asarray(votes), np.asarray(bad)
    voted_out = (votes.astype(np.float64) > tau * float(counts[0])) if counts[0] > 0 else np.zeros(votes.size, dtype=bool)
    return ~((bad != 0) | voted_out)


def restated_auror(g, alpha, tau=0.5, max_iter=32):
    got = restated_auror_votes(g, alpha, max_iter)
    kept = restated_auror_select(got['votes'], got['bad'], got['counts'], tau)
    out = g[kept].astype(np.float64).mean(axis=0) if kept.any() else np.zeros(g.shape[1])
    return out, kept, got


def margin_bound(g):
    """n * 2^-51 * max|x|: four times what two orders of an n-term fp64 sum of fp32 values can differ by"""
    finite = np.abs(g[np.isfinite(g)])
    return g.shape[0] * 2.0 ** -51 * (float(finite.max()) if finite.size else 0.0)


def planted_case(n, d, seed):
    """honest rows 0.1 x normals; n // 5 attackers with +0.5 on a random tenth of the columns -> (g, attackers, columns)"""
    rng = np.random.default_rng(seed)
    g = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    attackers = np.sort(rng.choice(n, n // 5, replace=False))
    columns = np.sort(rng.choice(d, d // 10, replace=False))
    g[np.ix_(attackers, columns)] += np.float32(0.5)
    return g, attackers, columns


def quarter_case(n, d, seed):
    """values k / 4, |k| <= 8: every sum is exact and values land on the thresholds"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-8, 9, size=(n, d)) / 4.0).astype(np.float32)


PLANTED = [(100, 4000), (1000, 2000), (4097, 500)]


# ---- the restatement against scikit-learn and on planted poisoning ---------------------------------------------------------------
def test_the_restatement_s_labels_are_scikit_learn_s_lloyd_iterations():
    cluster = pytest.importorskip('sklearn.cluster')
    rng = np.random.default_rng(5)
    for trial in range(12):
        n = int(rng.integers(5, 400))
        col = rng.standard_normal(n).astype(np.float32)
        if trial % 2:
            col[: n // 4] += np.float32(3.0)
        got = restated_auror_votes(col[:, None], 0.0, max_iter=300)
        assert got['counts'][2] == 0                           # not capped: Lloyd's fixed point
        x = col.astype(np.float64)[:, None]
        km = cluster.KMeans(n_clusters=2, init=np.array([[x.min()], [x.max()]]), n_init=1, algorithm='lloyd', tol=0, max_iter=300).fit(x)
        assert np.array_equal(km.labels_ == 1, got['labels'][:, 0]), trial
        assert abs((km.cluster_centers_[1, 0] - km.cluster_centers_[0, 0]) - got['gap'][0]) <= 1e-12


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('n,d', PLANTED)
def test_planted_attackers_are_removed_and_nobody_else(n, d, seed):
    g, attackers, columns = planted_case(n, d, seed)
    out, kept, got = restated_auror(g, alpha=0.3, tau=0.5)
    assert np.array_equal(np.flatnonzero(~kept), attackers)                    # every attacker, no honest row
    assert np.array_equal(np.flatnonzero(got['indicative']), columns)          # exactly the planted columns
    assert got['counts'][0] == columns.size and got['counts'][2] == 0 and not got['bad'].any()
    assert got['sweeps'].max() <= 32
    assert min(got['margin_t'], got['margin_alpha']) > margin_bound(g)         # (the device tests lean on this)


def test_a_small_alpha_makes_every_column_indicative_and_removes_honest_rows():
    """What the rule does not do: a unimodal column splits into centres about 1.6 sigma apart."""
    g = np.random.default_rng(7).standard_normal((200, 300)).astype(np.float32)
    got = restated_auror_votes(g, 1.0)
    assert got['counts'][0] == 300 and 1.4 < np.median(got['gap']) < 1.8
    assert restated_auror_votes(g, 2.5)['counts'][0] == 0


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------
def test_columns_that_are_not_clustered():
    nan, inf = np.nan, np.inf
    g = np.array([[1.0, nan, 3.0, -0.0, 5.0],
                  [nan, nan, 3.0, 0.0, 5.0],
                  [inf, -inf, 3.0, 0.0, 9.0]], dtype=np.float32)
    got = restated_auror_votes(g, 0.0)
    # column 0: m = 1; column 1: m = 0; column 2: constant; column 3: -0 == +0, constant; column 4: clustered
    assert got['counts'].tolist() == [1, 1, 0, 0] and got['gap'].tolist() == [0.0, 0.0, 0.0, 0.0, 4.0]
    assert got['bad'].tolist() == [1, 1, 1] and got['votes'].tolist() == [0, 0, 1]
    assert not restated_auror_select(got['votes'], got['bad'], got['counts'], 0.5).any()


def test_non_finite_values_abstain_and_flag_their_row():
    g, attackers, columns = planted_case(60, 200, 3)
    clean = restated_auror_votes(g, 0.3)
    honest = np.setdiff1d(np.arange(60), attackers)
    h0, h1 = honest[0], honest[1]
    free = np.setdiff1d(np.arange(200), columns)
    g[h0, free[0]], g[h1, free[1]] = np.nan, -np.inf
    got = restated_auror_votes(g, 0.3)
    assert np.flatnonzero(got['bad']).tolist() == sorted([h0, h1])
    assert np.array_equal(got['votes'], clean['votes']) and np.array_equal(got['counts'], clean['counts'])
    kept = restated_auror_select(got['votes'], got['bad'], got['counts'], 0.5)
    assert np.array_equal(np.flatnonzero(~kept), np.union1d(attackers, [h0, h1]))


def test_denormals_and_signed_zeros():
    tiny = np.float32(1e-45)
    g = np.array([[tiny], [2 * tiny], [3 * tiny], [np.float32(1e-40)]], dtype=np.float32)
    got = restated_auror_votes(g, 0.0)
    assert got['counts'][0] == 1 and got['votes'].tolist() == [0, 0, 0, 1] and got['gap'][0] > 0
    z = np.array([[-0.0], [0.0], [1.0]], dtype=np.float32)
    got = restated_auror_votes(z, 0.25)
    assert got['votes'].tolist() == [0, 0, 1] and got['gap'][0] == 1.0


def test_a_value_on_the_threshold_stays_below_and_equal_clusters_cast_no_vote():
    got = restated_auror_votes(np.array([[0.0], [1.0], [2.0]], dtype=np.float32), 0.5)
    assert got['m1'][0] == 1 and got['votes'].tolist() == [0, 0, 1] and got['margin_t'] == 0.0
    even = restated_auror_votes(np.array([[-2.0], [-2.0], [2.0], [2.0]], dtype=np.float32), 1.0)
    assert even['counts'][0] == 1 and even['side'][0] == -1 and not even['votes'].any()
    at_alpha = restated_auror_votes(np.array([[0.0]] * 5 + [[4.0]], dtype=np.float32), 4.0)
    assert at_alpha['counts'][0] == 0 and at_alpha['margin_alpha'] == 0.0      # gap == alpha: not indicative


def test_tau_zero_tau_one_and_no_indicative_column():
    g, attackers, columns = planted_case(50, 400, 4)
    got = restated_auror_votes(g, 0.3)
    g2 = g.copy()
    stray = np.setdiff1d(np.arange(50), attackers)[0]
    g2[stray, columns[0]] += np.float32(0.5)                   # an honest row with ONE vote
    one = restated_auror_votes(g2, 0.3)
    assert one['votes'][stray] == 1
    assert not restated_auror_select(one['votes'], one['bad'], one['counts'], 0.0)[stray]      # tau = 0: any vote removes
    assert restated_auror_select(one['votes'], one['bad'], one['counts'], 0.5)[stray]
    assert restated_auror_select(got['votes'], got['bad'], got['counts'], 1.0).all()           # tau = 1: votes never exceed
    none = restated_auror_votes(g, 5.0)
    assert none['counts'][0] == 0 and not none['votes'].any()
    assert restated_auror_select(none['votes'], none['bad'], none['counts'], 0.0).all()        # nobody removed for votes


def test_everybody_removed_gives_zeros():
    g = np.full((4, 6), np.nan, dtype=np.float32)
    out, kept, got = restated_auror(g, 0.1)
    assert not kept.any() and got['bad'].all() and (out == 0).all() and got['counts'].tolist() == [0, 0, 0, 0]


def test_the_cap_and_the_capped_count():
    col = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 8.0], dtype=np.float32)[:, None]
    free = restated_auror_votes(col, 1.0, max_iter=32)
    assert free['counts'][2] == 0 and free['sweeps'][0] >= 2
    one = restated_auror_votes(col, 1.0, max_iter=1)
    assert one['counts'].tolist() == [1, 1, 1, 0] and one['sweeps'][0] == 1 and one['t'][0] == 4.0 and one['m1'][0] == 1
    two = restated_auror_votes(col, 1.0, max_iter=2)
    assert two['sweeps'][0] == 2 and two['counts'][2] == (0 if free['sweeps'][0] == 2 else 1)
    g = np.random.default_rng(9).standard_normal((300, 50)).astype(np.float32)
    capped = restated_auror_votes(g, 0.0, max_iter=3)
    full = restated_auror_votes(g, 0.0, max_iter=64)
    assert capped['counts'][2] == int((full['sweeps'] > 3).sum()) > 0 and full['counts'][2] == 0


def test_two_rounds_accumulated_are_the_sums_of_the_rounds():
    a, _, _ = planted_case(40, 300, 11)
    b, _, _ = planted_case(40, 300, 12)
    b[3, 7] = np.nan
    ra, rb = restated_auror_votes(a, 0.3), restated_auror_votes(b, 0.3)
    both = restated_auror_votes(np.concatenate([a, b], axis=1), 0.3)           # column-local: two rounds are more columns
    assert np.array_equal(both['votes'], ra['votes'] + rb['votes']) and np.array_equal(both['counts'], ra['counts'] + rb['counts'])
    assert np.array_equal(both['bad'], np.maximum(ra['bad'], rb['bad']))


# ---- the rule's header on the host ------------------------------------------------------------------------------------------------
def test_the_column_rule_on_the_host_under_the_sanitizers(tmp_path):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if compiler is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'two_means_check')
    base = [compiler, '-std=c++17', '-O1', '-g', '-Wall', '-Wno-unknown-pragmas', '-I', CSRC, os.path.join(HERE, 'two_means_check.cpp'),
            '-o', exe]
    build = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], capture_output=True, text=True)
    if build.returncode != 0 and 'sanitize' in build.stderr + build.stdout:
        build = subprocess.run(base, capture_output=True, text=True)           # (a compiler without the sanitizer runtimes)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith('two_means ok'), run.stdout


# ---- the surface ------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_new_entry_points_and_states_the_rule():
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    assert '#define BYZ_ABI_VERSION 1\n' in text
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    fields = re.search(r'typedef struct byz_auror_params \{(.*?)\}', code, flags=re.S).group(1)
    assert re.findall(r'(\w+)\s+(\w+);', fields) == [('double', 'alpha'), ('double', 'tau'), ('int64_t', 'max_iter'),
                                                     ('int64_t', 'accumulate')]
    for phrase in ('t = 0.5 * (c0 + c1)', 'a value equal to t is in cluster 0', 'NO answer to the drift attack', 'CAPPED',
                   'never NaN', 'Integer'):
        assert phrase in text, phrase


def test_the_ctypes_table_lists_them():
    import ctypes
    from attacking_federate_learning_amd import _native
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS, name
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    P = ctypes.POINTER
    params = P(_native.AurorParams)
    assert _native._PROTOTYPES['byz_auror_votes_dev'] == [vp, vp, i64, i64, i64, params, vp, vp, vp, vp, vp]
    assert _native._PROTOTYPES['byz_auror_select_dev'] == [vp, vp, vp, vp, i64, params, vp, vp]
    assert _native._PROTOTYPES['byz_auror_dev'] == [vp, vp, i64, i64, i64, params, vp, vp, vp, vp, vp, vp, vp]
    assert _native._PROTOTYPES['byz_auror_info'] == [vp] + [P(i64)] * 5
    assert _native._PROTOTYPES['byz_auror_host'] == [vp, vp, i64, i64, params, vp, vp, vp, vp, vp, vp]
    assert ctypes.sizeof(_native.AurorParams) == 32 and _native.AurorParams.max_iter.offset == 16


def test_the_sources_are_on_the_build_list_and_the_rule_header_is_plain_cxx():
    from attacking_federate_learning_amd import build_native
    assert 'auror.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['auror.hip']
    kernel = open(os.path.join(CSRC, 'auror.hip')).read()
    assert 'colsel::for_height' in kernel and 'colsel::column_tile' in kernel and 'two_means_votes_kernel' in kernel
    assert not re.search(r'atomicAdd\([^;]*(float|double)', kernel)            # integers only
    header = open(os.path.join(CSRC, 'two_means.hpp')).read()
    assert '__HIPCC__' in header and 'hip_runtime' not in header


def test_the_report_joins_the_typed_block():
    text = open(os.path.join(CSRC, 'device_scalars.hpp')).read()
    assert re.search(r'struct AurorReport \{', text) and re.search(r'AurorReport auror;', text)
    assert 'sizeof(AurorReport)' in text and 'BYZ_AT(auror.kept_f64)' in text and re.search(r'kReportAuror\b', text)


def test_python_surface():
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.auror)) == (
        '(users_grads, users_count, corrupted_count, alpha, tau=0.5, max_iter=32, history=None, return_info=False)')
    assert inspect.signature(defences.auror).parameters['alpha'].default is inspect.Parameter.empty       # no default
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert defences.auror not in defences.defend.values()
    doc = defences.auror.__doc__
    assert 'drift attack' in doc and 'NO default' in doc and '1.6 sigma' in doc and 'not used' in doc
    assert str(inspect.signature(defences.AurorHistory.__init__)) == '(self, n)' and callable(defences.AurorHistory.reset)
    for name in ('auror_votes', 'auror_select', 'auror', 'auror_info'):
        assert callable(getattr(Engine, name)), name
    assert str(inspect.signature(Engine.auror_info)) == '(self)'
    assert str(inspect.signature(DeviceServer.defend_auror)) == '(self, alpha, tau=0.5, max_iter=32, history=True)'
    assert callable(ShardedAggregator.auror) and callable(HipKernels.auror_votes)
    # the rule of a pre-aggregation: then(matrix, users_count, corrupted_count, **then_kwargs) with alpha= among them
    parameters = list(inspect.signature(defences.auror).parameters.values())
    assert [p.name for p in parameters[:4]] == ['users_grads', 'users_count', 'corrupted_count', 'alpha']
    assert all(p.default is not inspect.Parameter.empty for p in parameters[4:])
    for pre in (defences.nnm, defences.bucketing, defences.robust_lr, defences.sparsefed, defences.weak_dp):
        sig = inspect.signature(pre).parameters
        assert 'then' in sig and any(p.kind is inspect.Parameter.VAR_KEYWORD for p in sig.values())


def test_then_composition_hands_alpha_through():
    """nnm(..., then=auror, alpha=...) calls then(mixed, users_count, corrupted_count, alpha=...): shown on a stand-in engine-free
    `then` with auror's own signature bound, so that a missing alpha fails the way Python fails it."""
    from attacking_federate_learning_amd import defences
    sig = inspect.signature(defences.auror)
    sig.bind('mixed', 10, 2, alpha=0.3)
    sig.bind('mixed', 10, 2, alpha=0.3, tau=0.25, max_iter=8)
    with pytest.raises(TypeError):
        sig.bind('mixed', 10, 2)


def test_the_refusals_that_need_no_gpu():
    from attacking_federate_learning_amd.engine import Engine
    p = Engine._auror_params(100, 0.3)
    assert (p.alpha, p.tau, p.max_iter, p.accumulate) == (0.3, 0.5, 32, 0)
    assert Engine._auror_params(16384, 0.0, 1.0, 1, accumulate=True).accumulate == 1
    for n, alpha, tau, cap in ((0, 0.3, 0.5, 32), (10, -0.1, 0.5, 32), (10, np.nan, 0.5, 32), (10, np.inf, 0.5, 32),
                               (10, 0.3, -0.01, 32), (10, 0.3, 1.01, 32), (10, 0.3, np.nan, 32), (10, 0.3, 0.5, 0)):
        with pytest.raises(ValueError):
            Engine._auror_params(n, alpha, tau, cap)
    with pytest.raises(NotImplementedError):
        Engine._auror_params(16385, 0.3)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    from attacking_federate_learning_amd import defences
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_auror', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.auror is defences.auror and mod.AurorHistory is defences.AurorHistory and 'auror' not in mod.defend


def test_the_documents_name_the_new_entry_points():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert name in integration, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '3.4s' in design and 'two_means_votes_kernel' in design and 'byz_auror_votes_dev' in design
    papers = open(os.path.join(ROOT, 'PAPERS.md')).read()
    assert 'AUROR' in papers and 'ACSAC 2016' in papers
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'defences.auror' in readme and 'auror.hip' in readme
    assert 'auror_timing.md' in open(os.path.join(ROOT, 'profiles', 'INDEX.md')).read()
