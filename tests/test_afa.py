"""AFA without a GPU: a numpy restatement of include/byzagg.h's rule in the stated orders (what tests/test_gpu_afa.py holds the
kernels to, integers exactly and doubles as bits), what the rule does to the drift attack and to sign flips on planted
matrices, the margins that make its decisions independent of the Gram's rounding, the reputation's arithmetic, and the
surface: header, ctypes table, build list, typed report, Python signatures, documents.

What the rule does NOT catch is stated here too (test_what_is_not_caught): rows of pure noise at three times the honest scale
are mostly kept, because they drag the aggregate with them."""
import functools
import inspect
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('byz_afa_select_dev', 'byz_afa_dev', 'byz_afa_info', 'byz_afa_host')
THREADS, WAVE = 1024, 64


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def block_sum(terms, kept):
    """A sum over the kept rows in the header's one order: 1024 chains (chain t: the kept rows t, t + 1024, ... ascending, from
    +0.0), every aligned group of 64 chains folded 32, 16, 8, 4, 2, 1, the 16 groups' sums folded 8, 4, 2, 1."""
    n = terms.size
    chain = np.zeros(THREADS)
    for lo in range(0, n, THREADS):
        rows = np.arange(lo, min(n, lo + THREADS))
        rows = rows[kept[rows]]
        chain[rows - lo] = chain[rows - lo] + terms[rows]
    c = chain.reshape(THREADS // WAVE, WAVE).copy()
    for h in (32, 16, 8, 4, 2, 1):
        c[:, :h] = c[:, :h] + c[:, h:2 * h]
    w = c[:, 0].copy()
    for h in (8, 4, 2, 1):
        w[:h] = w[:h] + w[h:2 * h]
    return w[0]


def initial_u(c, w):
    """u_k = sum of w_j * C[k][j] over the usable j: 64 chains by column modulo 64, ascending, folded 32 ... 1 (w: 0 = excluded)"""
    n = c.shape[0]
    chain = np.zeros((n, WAVE))
    with np.errstate(invalid='ignore', over='ignore'):
        for lo in range(0, n, WAVE):
            cols = np.arange(lo, min(n, lo + WAVE))
            cols = cols[w[cols] > 0]
            chain[:, cols - lo] = chain[:, cols - lo] + w[cols][None, :] * c[:, cols]
        for h in (32, 16, 8, 4, 2, 1):
            chain[:, :h] = chain[:, :h] + chain[:, h:2 * h]
    return chain[:, 0].copy()


def median_of(values):
    """np.median's two middle order statistics, spelled out"""
    a = np.sort(values)
    m = a.size
    return a[(m - 1) // 2] if m % 2 else (a[m // 2 - 1] + a[m // 2]) / 2.0


def restated_afa_select(c, weights=None, xi0=2.0, delta_xi=0.5, max_rounds=0):
    """include/byzagg.h's selection, operation for operation.  -> dict: kept (bool), round_of, score, the report's fields, the
    weights w_k * kept_k, and for the tests of the margins: `branches` (the side of every round that removed somebody),
    `removed_per_round`, `margin_thr` = min |s_k - thr| / sd and `margin_side` = min |mean - med| / sd over the rounds with sd > 0."""
    c = np.asarray(c, dtype=np.float64)
    n = c.shape[0]
    w_in = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    diag = np.diagonal(c)
    with np.errstate(invalid='ignore'):
        usable = np.isfinite(diag) & (diag > 0) & np.isfinite(w_in) & (w_in > 0)
    w = np.where(usable, w_in, 0.0)
    r = np.where(usable, np.sqrt(np.where(usable, diag, 1.0)), 0.0)
    u = initial_u(c, w)
    kept = usable.copy()
    round_of = np.where(usable, -1, 0).astype(np.int32)
    score = np.zeros(n)
    info = dict(rounds=0, branch=0, degenerate=False, mean=0.0, med=0.0, sd=0.0, thr=0.0)
    branches, removed_per_round, margin_thr, margin_side = [], [], np.inf, np.inf
    xi, m = float(xi0), int(kept.sum())
    for rnd in range(1, n + 1):
        if m == 0:
            break
        info['rounds'] = rnd
        a = block_sum(w * u, kept)
        if not (np.isfinite(a) and a > 0):
            info['degenerate'] = True
            break
        s = np.zeros(n)
        s[kept] = u[kept] / (r[kept] * np.sqrt(a))
        score[kept] = s[kept]
        mean = block_sum(s, kept) / float(m)
        dev = np.zeros(n)
        dev[kept] = s[kept] - mean
        sd = np.sqrt(block_sum(dev * dev, kept) / float(m))
        med = median_of(s[kept])
        lower = bool(mean < med)
        thr = med - xi * sd if lower else med + xi * sd
        gone = kept & ((s < thr) if lower else (s > thr))
        info.update(mean=mean, med=med, sd=sd, thr=thr)
        if sd > 0:
            margin_thr = min(margin_thr, np.abs(s[kept] - thr).min() / sd)
            margin_side = min(margin_side, abs(mean - med) / sd)
        if not gone.any():
            break
        info['branch'] = -1 if lower else 1
        branches.append(info['branch'])
        removed_per_round.append(int(gone.sum()))
        round_of[gone] = rnd
        kept &= ~gone
        m -= int(gone.sum())
        if max_rounds and rnd >= max_rounds:
            break
        for q in np.flatnonzero(gone):
            u[kept] = u[kept] - w[q] * c[q][kept]
        xi = xi + delta_xi
    w_out = np.where(kept, w, 0.0)
    info.update(kept=int(kept.sum()), removed=int((usable & ~kept).sum()), excluded=int((~usable).sum()),
                divisor=block_sum(w_out, kept))
    return dict(info, kept_flags=kept, round_of=round_of, score=score, weights=w_out, branches=branches,
                removed_per_round=removed_per_round, margin_thr=margin_thr, margin_side=margin_side)


REPORT_FIELDS = ('rounds', 'kept', 'removed', 'excluded', 'branch', 'degenerate')
STAT_FIELDS = ('mean', 'med', 'sd', 'thr', 'divisor')


# ---- the planted matrices -----------------------------------------------------------------------------------------------------
def planted(n, d, kind, seed, f=None):
    """n x d fp32: honest rows mu + N(0, 1) with mu ~ 0.2 N(0, 1); the first f = n // 5 rows are the attackers:
    'drift'  the honest rows' mean - 1.0 * std, copied f times (A Little Is Enough);
    'flip'   sign-flipped rows of the honest kind, unscaled;
    'noise'  pure noise at three times the honest scale."""
    rng = np.random.default_rng(seed)
    f = n // 5 if f is None else f
    mu = 0.2 * rng.standard_normal(d)
    honest = mu[None, :] + rng.standard_normal((n - f, d))
    if kind == 'drift':
        bad = np.tile(honest.mean(axis=0) - 1.0 * honest.std(axis=0), (f, 1))
    elif kind == 'flip':
        bad = -(mu[None, :] + rng.standard_normal((f, d)))
    elif kind == 'noise':
        bad = 3.0 * rng.standard_normal((f, d))
    else:
        raise ValueError(kind)
    return np.vstack([bad, honest]).astype(np.float32), f


def gram64(g):
    g = np.asarray(g, dtype=np.float64)
    return g @ g.T


WIDE_SHAPES = ((65, 2000), (64, 2000), (130, 777))
THIN_SIZES = (2, 3, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)


@functools.lru_cache(maxsize=None)
def wide_case(n, d, kind, seed):
    g, f = planted(n, d, kind, seed)
    return g, f, restated_afa_select(gram64(g))


@functools.lru_cache(maxsize=None)
def thin_gram(n):
    """the Gram of the GPU tests' selections: built on the host in fp64 from a thin fp32 matrix, n x 32, 'noise', seed 7"""
    return gram64(planted(n, 32, 'noise', 7)[0])


@functools.lru_cache(maxsize=None)
def thin_case(n):
    return restated_afa_select(thin_gram(n))


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
def test_the_restatement_s_median_is_numpy_s_and_its_sums_are_sums():
    rng = np.random.default_rng(0)
    for m in (1, 2, 3, 64, 65, 1000, 2049):
        v = rng.standard_normal(m)
        assert median_of(v) == np.median(v)
        kept = rng.random(m) < 0.7
        assert abs(block_sum(v, kept) - v[kept].sum()) <= 1e-12 * np.abs(v).sum()
    c = gram64(rng.standard_normal((130, 50)))
    w = rng.random(130)
    w[[3, 77]] = 0.0
    assert np.allclose(initial_u(c, w), c @ w, rtol=1e-13, atol=1e-10)


# ---- the drift attack and the sign flips --------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('n,d', WIDE_SHAPES)
@pytest.mark.parametrize('kind', ['drift', 'flip'])
def test_no_attacker_is_kept(kind, n, d, seed):
    g, f, got = wide_case(n, d, kind, seed)
    kept = got['kept_flags']
    assert not kept[:f].any(), np.flatnonzero(kept[:f])
    lost = int((~kept[f:]).sum())
    print('afa %s %dx%d seed %d: %d rounds, removed per round %s, %d honest rows lost' % (
        kind, n, d, seed, got['rounds'], got['removed_per_round'], lost))
    assert lost <= (3 if n == 130 else 2)
    assert got['excluded'] == 0 and not got['degenerate'] and got['kept'] + got['removed'] == n
    # the upper branch takes the drift attack's copies, the lower one the flipped rows: both as the FIRST round
    assert got['branches'][0] == (1 if kind == 'drift' else -1)


def test_a_case_with_three_or_more_rounds_is_among_them():
    rounds = [wide_case(n, d, kind, seed)[2]['rounds'] for kind in ('drift', 'flip') for n, d in WIDE_SHAPES for seed in (0, 1, 2)]
    assert max(rounds) >= 3, rounds


def test_what_is_not_caught():
    """Rows of pure noise at three times the honest scale are NOT caught: they carry three times the weight in the aggregate,
    so their cosine with it is no outlier.  That is the rule's, not the kernels': norm clipping belongs in front (weak_dp,
    centered_clip)."""
    for n, d in WIDE_SHAPES:
        g, f, = planted(n, d, 'noise', 0)
        kept = restated_afa_select(gram64(g))['kept_flags']
        print('afa noise x3 %dx%d: %d of %d noise rows kept' % (n, d, int(kept[:f].sum()), f))
        assert kept[:f].sum() > f // 2


# ---- the margins of the decisions ---------------------------------------------------------------------------------------------
def test_every_decision_has_a_margin():
    """|s_k - thr| / sd and |mean - med| / sd above 1e-3 in every round of every case: the kernels' comparisons then do not
    depend on the last bits of the Gram (tests/test_gpu_afa.py measures the device Gram's error and holds it below 1e-5)."""
    worst_thr, worst_side = np.inf, np.inf
    for kind in ('drift', 'flip'):
        for n, d in WIDE_SHAPES:
            for seed in (0, 1, 2):
                got = wide_case(n, d, kind, seed)[2]
                worst_thr, worst_side = min(worst_thr, got['margin_thr']), min(worst_side, got['margin_side'])
                assert got['margin_thr'] > 1e-3 and got['margin_side'] > 1e-3, (kind, n, d, seed, got['margin_thr'], got['margin_side'])
    for n in THIN_SIZES[1:]:
        got = thin_case(n)
        print('afa thin n = %d: %d rounds, removed per round %s, margins %.3g %.3g' % (
            n, got['rounds'], got['removed_per_round'], got['margin_thr'], got['margin_side']))
        worst_thr, worst_side = min(worst_thr, got['margin_thr']), min(worst_side, got['margin_side'])
        assert got['margin_thr'] > 1e-3 and got['margin_side'] > 1e-3, (n, got['margin_thr'], got['margin_side'])
    print('afa margins: worst |s - thr| / sd = %.3g, worst |mean - med| / sd = %.3g' % (worst_thr, worst_side))


def test_two_rows_tie_and_take_the_upper_branch():
    """n = 2 is the one exception to the margin: mean = med exactly; the equal case takes the upper branch and removes nobody"""
    got = thin_case(2)
    assert got['mean'] == got['med'] and got['margin_side'] == 0.0
    assert got['thr'] == got['med'] + 2.0 * got['sd'] and got['thr'] > got['med']
    assert got['rounds'] == 1 and got['kept'] == 2 and got['branch'] == 0 and got['branches'] == []


def test_the_thin_cases_remove_several_rows_a_round():
    sizes = [max(thin_case(n)['removed_per_round'], default=0) for n in THIN_SIZES]
    assert max(sizes) >= 16, sizes              # a multi-row update: more than one batch of the kernel's row reads


def test_excluded_rows_and_weights_in_the_restatement():
    c = thin_gram(65).copy()
    c[5, 5] = 0.0
    c[9, :] = c[:, 9] = np.nan
    c[11, 11] = np.inf
    w = np.linspace(0.5, 2.0, 65)
    w[[20, 21]] = 0.0
    w[22] = np.nan
    got = restated_afa_select(c, w)
    assert got['excluded'] == 6 and (got['round_of'][[5, 9, 11, 20, 21, 22]] == 0).all()
    assert not got['kept_flags'][[5, 9, 11, 20, 21, 22]].any() and np.isfinite(got['score']).all()
    assert (got['weights'][got['kept_flags']] == w[got['kept_flags']]).all() and got['divisor'] > 0
    nobody = restated_afa_select(np.zeros((7, 7)))
    assert nobody['excluded'] == 7 and nobody['rounds'] == 0 and nobody['kept'] == 0 and nobody['divisor'] == 0.0
    one = restated_afa_select(c, max_rounds=1)
    full = restated_afa_select(c)
    assert one['rounds'] == 1 and one['removed'] == full['removed_per_round'][0] and full['rounds'] > 1


# ---- the reputation -----------------------------------------------------------------------------------------------------------
def test_the_binomial_tail_is_the_incomplete_beta_function():
    from attacking_federate_learning_amd.defences import AfaReputation
    assert AfaReputation.bad_probability(3, 3) == 0.5 and AfaReputation.bad_probability(1, 1) == 0.5
    assert AfaReputation.bad_probability(3, 9) == 1981 / 2048
    try:
        from scipy.special import betainc
    except ImportError:
        return                                  # (the comparison needs scipy; the exact values above do not)
    for a in range(1, 12):
        for b in range(1, 12):
            assert abs(AfaReputation.bad_probability(a, b) - betainc(a, b, 0.5)) <= 1e-14, (a, b)


def test_a_client_removed_six_times_running_is_blocked_in_the_sixth_round():
    """From (3, 3), after r removals the client stands at (3, 3 + r) and I_0.5 = P(Bin(5 + r, 1/2) >= 3): 42/64, 99/128, 219/256,
    466/512, 968/1024 = 0.9453 < 0.95 <= 1981/2048 = 0.9673: the sixth removal blocks, the fifth does not."""
    from attacking_federate_learning_amd.defences import AfaReputation
    tails = [1 - sum(math.comb(5 + r, j) for j in range(3)) / 2 ** (5 + r) for r in range(1, 7)]
    assert [t >= 0.95 for t in tails] == [False] * 5 + [True] and tails[4] == 968 / 1024 and tails[5] == 1981 / 2048
    rep = AfaReputation(4)
    assert (rep.weights() == 0.5).all()
    for rnd in range(1, 7):
        fresh = rep.update(kept=[0, 1, 2])      # client 3 is removed every round
        assert fresh.tolist() == ([3] if rnd == 6 else []), rnd
        assert rep.weights()[3] == (0.0 if rnd == 6 else 3 / (6 + rnd))
    assert rep.blocked.tolist() == [False, False, False, True]
    assert rep.alpha.tolist() == [9, 9, 9, 3] and rep.beta.tolist() == [3, 3, 3, 9]
    # blocked: its weight is 0, the rule sees it as excluded, and nothing moves its counts any more
    c = thin_gram(65)[:4, :4]
    got = restated_afa_select(c, rep.weights())
    assert got['round_of'][3] == 0 and got['excluded'] == 1 and not got['kept_flags'][3]
    rep.update(kept=np.flatnonzero(got['kept_flags']), excluded=np.flatnonzero(got['round_of'] == 0))
    assert rep.alpha[3] == 3 and rep.beta[3] == 9 and rep.alpha[:3].tolist() == (9 + got['kept_flags'][:3]).tolist()
    # an excluded client that is not blocked is left alone as well
    rep2 = AfaReputation(3, alpha0=2, beta0=1, delta=0.9)
    rep2.update(kept=[0], excluded=[2])
    assert rep2.alpha.tolist() == [3, 2, 2] and rep2.beta.tolist() == [1, 2, 1]
    assert np.array_equal(rep2.weights(), np.array([3 / 4, 2 / 4, 2 / 3]))


# ---- the surface --------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_new_entry_points_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    assert '#define BYZ_ABI_VERSION 1\n' in text
    assert 'BYZ_K_MISC = 8, BYZ_K_PLANE_SPLIT = 9, BYZ_K_COUNT = 10' in text          # the timing enum did not change
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    fields = re.search(r'typedef struct byz_afa_params \{(.*?)\}', code, flags=re.S).group(1)
    assert re.findall(r'(\w+)\s+(\w+);', fields) == [('double', 'xi0'), ('double', 'delta_xi'), ('int64_t', 'max_rounds')]
    assert '1024 chains' in text and 'Both comparisons are strict' in text and 'everybody is excluded' in text


def test_the_ctypes_table_lists_them():
    import ctypes
    from attacking_federate_learning_amd import _native
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS, name
    i64, vp, f64 = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    P = ctypes.POINTER
    params = P(_native.AfaParams)
    assert _native._PROTOTYPES['byz_afa_select_dev'] == [vp, vp, i64, vp, params, vp, vp, vp, vp]
    assert _native._PROTOTYPES['byz_afa_dev'] == [vp, vp, i64, i64, i64, vp, params, vp, vp, vp, vp, vp, vp]
    assert _native._PROTOTYPES['byz_afa_info'] == [vp, P(i64), P(f64), P(f64)]
    assert _native._PROTOTYPES['byz_afa_host'] == [vp, vp, i64, i64, vp, params, vp, vp, vp, vp, vp]
    assert ctypes.sizeof(_native.AfaParams) == 24 and _native.AfaParams.max_rounds.offset == 16


def test_the_source_is_on_the_build_list():
    from attacking_federate_learning_amd import build_native
    assert 'afa.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['afa.hip']


def test_the_report_joins_the_typed_block():
    text = open(os.path.join(ROOT, 'attacking_federate_learning_amd', 'csrc', 'device_scalars.hpp')).read()
    assert re.search(r'struct AfaReport \{', text) and re.search(r'AfaReport afa;', text)
    assert 'sizeof(AfaReport)' in text and 'BYZ_AT(afa.thr)' in text and 'BYZ_AT(afa.divisor)' in text
    assert re.search(r'kReportAfa\b', text)


def test_python_surface():
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.afa)) == (
        '(users_grads, users_count, corrupted_count, weights=None, xi=2.0, delta_xi=0.5, gram=None, reputation=None)')
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert defences.afa not in defences.defend.values()
    doc = defences.afa.__doc__
    assert 'drift attack' in doc and 'KEPT' in doc and 'not used' in doc
    assert str(inspect.signature(Engine.afa_select)) == (
        '(self, gram, weights=None, xi=2.0, delta_xi=0.5, max_rounds=None, on_device=False, like=None)')
    assert str(inspect.signature(Engine.afa_info)) == '(self)' and callable(Engine.afa)
    assert str(inspect.signature(defences.AfaReputation.__init__)) == '(self, n, alpha0=3, beta0=3, delta=0.95)'
    assert str(inspect.signature(DeviceServer.defend_afa)) == '(self, xi=2.0, delta_xi=0.5, reputation=True)'
    assert callable(ShardedAggregator.afa) and callable(HipKernels.afa_select)
    # the rule of a pre-aggregation: called as then(matrix, users_count, corrupted_count), every other parameter defaulted
    parameters = list(inspect.signature(defences.afa).parameters.values())
    assert [p.name for p in parameters[:3]] == ['users_grads', 'users_count', 'corrupted_count']
    assert all(p.default is not inspect.Parameter.empty for p in parameters[3:])
    for pre in (defences.nnm, defences.bucketing, defences.robust_lr, defences.sparsefed, defences.weak_dp):
        assert 'then' in inspect.signature(pre).parameters


def test_the_refusals_that_need_no_gpu():
    from attacking_federate_learning_amd.engine import Engine
    p = Engine._afa_params(2, 2.0, 0.5, None)
    assert (p.xi0, p.delta_xi, p.max_rounds) == (2.0, 0.5, 0)
    assert Engine._afa_params(16384, 0.0, 0.0, 7).max_rounds == 7
    for n, xi, delta, cap in ((1, 2.0, 0.5, None), (10, -1.0, 0.5, None), (10, 2.0, -0.5, None), (10, np.nan, 0.5, None),
                              (10, 2.0, np.inf, None), (10, 2.0, 0.5, -1)):
        with pytest.raises(ValueError):
            Engine._afa_params(n, xi, delta, cap)
    with pytest.raises(NotImplementedError):
        Engine._afa_params(16385, 2.0, 0.5, None)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    from attacking_federate_learning_amd import defences
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_afa', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.afa is defences.afa and mod.AfaReputation is defences.AfaReputation and 'afa' not in mod.defend


def test_the_documents_name_the_new_entry_points():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert name in integration, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '3.4r' in design and 'byz_afa_select_dev' in design
    papers = open(os.path.join(ROOT, 'PAPERS.md')).read()
    assert 'AFA' in papers and '1909.05125' in papers
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'defences.afa' in readme and 'afa.hip' in readme
    assert 'afa_timing.md' in open(os.path.join(ROOT, 'profiles', 'INDEX.md')).read()
