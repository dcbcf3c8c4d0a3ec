"""The attacks of Fang, Cao, Jia and Gong (USENIX Security 2020) without a GPU: the numpy restatement of the three rules of
include/byzagg.h (A: trimmed mean / median with full knowledge, B: with partial knowledge, C: Krum) that tests/test_gpu_fang.py
holds the kernels to, the restatement's own properties, csrc/philox.hpp's philox_uniform on the host
(tests/fang_uniform_check.cpp, compiled as plain C++17) and the public surface.

The restatement.  G is n x d float32; rows 0 .. c - 1 are the attacker's, the others benign.
  A  mean = np.mean(G, axis=0) (no_defense's bits), lo / hi = np.fmin.reduce / np.fmax.reduce over G[c:]; mean > 0: the interval
     is [lo / b, lo] (lo > 0) or [b lo, lo], otherwise [hi, b hi] (hi > 0) or [hi, hi / b]; ends in fp64 from the fp32 extreme.
     (For hi <= 0 the paper's set is written with its ends in order, A <= B: hi / b lies ABOVE a negative hi.)
  B  mu, sigma = np.mean, np.var ** 0.5 over G[:c]; mu > 0: [mu - k_hi sigma, mu - k_lo sigma], otherwise [mu + k_lo sigma,
     mu + k_hi sigma]; ends (double)mu -+ k * (double)sigma.
  the draw  u = (word + 0.5) * 2^-32, value = fl32(A + u * (B - A)); an end that is not finite: the extreme (lo, hi, the k_lo end).
     The word of (row i, global column j) is tests/test_weak_dp.py's restated_words(., seed, round | i << 32, .).
  C  s = +1 where mean > 0 else -1; from q_i = |g_i|^2, t_i = g_i . s and the benign rows' distance block: lambda_0 = min_i S_i /
     ((n - 2c - 1) sqrt(d)) + sqrt(max_i q_i) / sqrt(d), S_i the fp64 sum in column order of row i of the block without its diagonal
     and the first of its largest entries; lambda_k = lambda_0 / 2^k; the matrix of a step has fl32(sqrt(max((q_i + (2 lambda) t_i)
     + (lambda lambda) d, 0))) in the attackers' rows and columns, 0 between attackers, +inf on the diagonal; the loop stops at the
     first k at which Krum picks a row < c, or after the first lambda_k < threshold."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import faithful
from tests.test_weak_dp import restated_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, 'attacking_federate_learning_amd', 'csrc')

NEW_SYMBOLS = ('byz_column_extremes_dev', 'byz_fang_fill_dev', 'byz_fang_trmean_attack_dev', 'byz_fang_trmean_attack_host',
               'byz_fang_krum_attack_dev', 'byz_fang_krum_info')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def restated_mean(g):
    """np.mean(g, axis=0) as the operations numpy performs over the OUTER axis: the sequential fp32 chain from +0.0 in row order,
    divided by float(n) -- no_defense's bits.  (numpy itself leaves that order where the matrix has ONE column: the reduction is
    then over contiguous memory and pairwise; the chain is the contract, test_the_chain_is_numpys_mean holds the two together.)"""
    with np.errstate(all='ignore'):
        return faithful.attack_statistics_sequential(g)[0]


def restated_column_extremes(g, c):
    """(mean, lo, hi) as float32 vectors."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    mean = restated_mean(g)
    benign = g[c:]
    if benign.shape[0] == 0:
        nan = np.full(g.shape[1], np.nan, dtype=np.float32)
        return mean, nan, nan.copy()
    with np.errstate(all='ignore'):
        return mean, np.fmin.reduce(benign, axis=0), np.fmax.reduce(benign, axis=0)


def restated_full_intervals(mean, lo, hi, b=2.0):
    """(A, B, extreme): the fp64 ends and the float32 extreme of every column under rule A."""
    mean, lo, hi = (np.asarray(v, dtype=np.float32) for v in (mean, lo, hi))
    lo64, hi64, b = lo.astype(np.float64), hi.astype(np.float64), float(b)
    with np.errstate(all='ignore'):
        a_down, b_down = np.where(lo > 0, lo64 / b, b * lo64), lo64
        a_up, b_up = hi64, np.where(hi > 0, b * hi64, hi64 / b)
    down = mean > 0
    return np.where(down, a_down, a_up), np.where(down, b_down, b_up), np.where(down, lo, hi).astype(np.float32)


def restated_partial_intervals(mu, sigma, k_lo=3.0, k_hi=4.0):
    """(A, B, extreme) under rule B; the extreme is the k_lo end, rounded to float32."""
    mu, sigma = np.asarray(mu, dtype=np.float32), np.asarray(sigma, dtype=np.float32)
    mu64, near, far = mu.astype(np.float64), float(k_lo) * sigma.astype(np.float64), float(k_hi) * sigma.astype(np.float64)
    down = mu > 0
    with np.errstate(all='ignore'):
        A, B = np.where(down, mu64 - far, mu64 + near), np.where(down, mu64 - near, mu64 + far)
        return A, B, np.where(down, B, A).astype(np.float32)


def restated_draw(words, A, B, extreme):
    """philox_uniform on arrays."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    u = (np.asarray(words).astype(np.float64) + 0.5) * 2.0 ** -32
    with np.errstate(all='ignore'):
        value = (A + u * (B - A)).astype(np.float32)
    return np.where(np.isfinite(A) & np.isfinite(B), value, np.asarray(extreme, dtype=np.float32))


def restated_fang_rows(A, B, extreme, c, seed=0, round=0, column_offset=0):
    """The c attacker rows drawn from the columns' intervals."""
    assert 0 <= int(round) < 1 << 32
    d = len(A)
    return np.stack([restated_draw(restated_words(d, seed, int(round) | i << 32, column_offset), A, B, extreme)
                     for i in range(c)]) if c else np.empty((0, d), dtype=np.float32)


def restated_fang_trmean(g, c, b=2.0, partial=False, seed=0, round=0, column_offset=0, k_lo=3.0, k_hi=4.0):
    """The attacked matrix: rows 0 .. c - 1 redrawn, the others as they are."""
    g = np.array(g, dtype=np.float32)
    if c == 0:
        return g
    if partial:
        with np.errstate(all='ignore'):
            A, B, e = restated_partial_intervals(*faithful.attack_statistics_sequential(g[:c]), k_lo, k_hi)
    else:
        A, B, e = restated_full_intervals(*restated_column_extremes(g, c), b=b)
    g[:c] = restated_fang_rows(A, B, e, c, seed, round, column_offset)
    return g


def rank_trimmed_mean_f64(g, trim):
    """Yin et al.'s trimmed mean, rank_trimmed_mean's rule, in fp64: the mean of np.sort(col)[trim : n - trim]."""
    s = np.sort(np.asarray(g, dtype=np.float64), axis=0)
    kept = s[trim:s.shape[0] - trim]
    return np.cumsum(kept, axis=0)[-1] / kept.shape[0]          # (one order of addition for both sides of a comparison)


def restated_sign(mean):
    return np.where(np.asarray(mean, dtype=np.float32) > 0, np.float32(1), np.float32(-1)).astype(np.float32)


def restated_row_sums(block):
    """S_i of every row of the benign block."""
    block = np.asarray(block, dtype=np.float32)
    m = block.shape[0]
    out = np.zeros(m, dtype=np.float64)
    for i in range(m):
        others = np.delete(block[i], i)
        if others.size >= 2:
            rest = np.delete(others, int(np.argmax(others))).astype(np.float64)
            out[i] = np.cumsum(rest)[-1]
    return out


def restated_lambda0(block, q, n, c, d):
    root = np.sqrt(np.float64(d))
    return float(restated_row_sums(block).min() / (np.float64(n - 2 * c - 1) * root) + np.sqrt(np.float64(np.max(q))) / root)


def restated_krum_matrix(block, q, t, lam, n, c, d):
    """The n x n float32 matrix of one step."""
    q, t, lam = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64), np.float64(lam)
    dist = np.zeros((n, n), dtype=np.float32)
    dist[c:, c:] = block
    sq = (q + (np.float64(2.0) * lam) * t) + (lam * lam) * np.float64(d)
    v = np.sqrt(np.maximum(sq, 0.0)).astype(np.float32)
    dist[c:, :c] = v[:, None]
    dist[:c, c:] = v[None, :]
    dist[np.arange(c), np.arange(c)] = np.inf
    return dist


def cpu_krum(dist, c):
    n = dist.shape[0]
    return int(faithful.krum_pick(dist, faithful.visit_order(n), n, c))


def restated_fang_krum(block, q, t, n, c, d, threshold=1e-5, krum=cpu_krum):
    """{lambda0, lambdas (every lambda tried), lambda, steps, chosen, succeeded, dist (the last step's matrix)}."""
    if c < 1 or n <= 2 * c + 1:
        raise ValueError('n = %d rows must exceed 2 c + 1 with c = %d >= 1' % (n, c))
    lam0 = restated_lambda0(block, q, n, c, d)
    lam, tried = lam0, []
    while True:
        dist = restated_krum_matrix(block, q, t, lam, n, c, d)
        chosen = krum(dist, c)
        tried.append(lam)
        succeeded = 0 <= chosen < c
        if succeeded or lam < threshold:
            break
        lam = lam / 2.0
    return {'lambda0': lam0, 'lambdas': tried, 'lambda': lam, 'steps': len(tried), 'chosen': chosen, 'succeeded': succeeded,
            'dist': dist}


def restated_krum_attack_matrix(g, c, threshold=1e-5):
    """The whole of rule C on a matrix, t and q in numpy's fp64: (attacked matrix, info)."""
    g = np.array(g, dtype=np.float32)
    n, d = g.shape
    s = restated_sign(restated_mean(g))
    g64 = g[c:].astype(np.float64)
    info = restated_fang_krum(faithful.distance_matrix(g[c:]), (g64 * g64).sum(axis=1), g64 @ s.astype(np.float64), n, c, d, threshold)
    g[:c] = (-np.float32(info['lambda'])) * s
    return g, info


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def seeded(seed, n=20, d=64, shift=0.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)) + shift).astype(np.float32)


def krum_case(seed, n, c, d, mu=0.5):
    """Benign rows N(mu, I) with |mu_j| = `mu` and seeded signs.  mu = 0.5: large against the spread of the column MEAN (1 /
    sqrt(n)), so s is the sign of mu, yet the cluster's distance from the zero gradient, sqrt(d (1 + mu^2)), is of the order of
    the benign rows' own distances sqrt(2 d): a row -lambda s near the origin is nearer to the benign rows than they are to
    their farthest neighbours, which is what Krum can be made to pick.  mu = 20: every -lambda s, the origin included, lies 20
    sqrt(d) from a cluster of diameter sqrt(2 d), and no lambda succeeds."""
    rng = np.random.default_rng(seed)
    centre = mu * rng.choice([-1.0, 1.0], size=d)
    return (rng.standard_normal((n, d)) + centre).astype(np.float32)


KRUM_CASES = [(7001, 12, 2, 40), (7002, 64, 15, 1000)]


# ---- csrc/philox.hpp's philox_uniform on the host ---------------------------------------------------------------------------------
UNIFORM_CASES = ((0, 0, 0, 0, 0.5, 1.0), (12345, 7, 3, 10, -2.0, -1.0), (12345, 7, 3, 11, float(np.float32(0.1)) / 2, float(np.float32(0.1))),
                 (12345, 7, 4, 11, float(np.float32(0.1)) / 2, float(np.float32(0.1))),
                 (0x9e3779b97f4a7c15, 0xffffffff, 799, (1 << 34) + 2, -1e30, 1e30), (1, 2, 1, 5, 3.0, 3.0))


def _build_and_run(tmp_path, extra):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if compiler is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'fang_uniform_check')
    build = subprocess.run([compiler, '-std=c++17', '-O1', '-Wall', '-ffp-contract=off', '-I', CSRC] + extra +
                           [os.path.join(HERE, 'fang_uniform_check.cpp'), '-o', exe], capture_output=True, text=True)
    return build, exe


def _check_program_output(stdout):
    lines = stdout.splitlines()
    assert lines[0].startswith('uniform ok'), stdout
    assert len(lines) == 1 + len(UNIFORM_CASES)
    for line, (seed, rnd, row, column, A, B) in zip(lines[1:], UNIFORM_CASES):
        word, value = (int(v, 16) for v in line.split())
        want_word = int(restated_words(1, seed, rnd | row << 32, column)[0])
        assert word == want_word, (line, want_word)
        assert value == int(bits(restated_draw(np.array([want_word]), np.array([A]), np.array([B]), np.zeros(1)))[0]), line


def test_the_uniform_draw_on_the_host(tmp_path):
    build, exe = _build_and_run(tmp_path, [])
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    _check_program_output(run.stdout)


def test_the_uniform_draw_under_the_host_sanitizers(tmp_path):
    """The stand-alone program again with AddressSanitizer and UndefinedBehaviorSanitizer (a host build: nothing here is loaded
    into Python)."""
    build, exe = _build_and_run(tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    if build.returncode != 0:
        pytest.skip('the host compiler has no sanitizer runtime: ' + build.stderr[-200:])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    _check_program_output(run.stdout)


# ---- the draw ------------------------------------------------------------------------------------------------------------------
def test_the_chain_is_numpys_mean():
    for seed, n, d in ((1, 20, 64), (2, 9, 2), (3, 17, 257)):
        g = seeded(seed, n, d)
        assert np.array_equal(bits(restated_mean(g)), bits(np.mean(g, axis=0)))
        mu, sigma = faithful.attack_statistics_sequential(g[:5])
        assert np.array_equal(bits(mu), bits(np.mean(g[:5], axis=0))) and np.array_equal(bits(sigma), bits(np.var(g[:5], axis=0) ** 0.5))
    assert np.array_equal(bits(restated_mean(np.full((3, 2), -0.0, dtype=np.float32))), bits(np.zeros(2, dtype=np.float32)))


@pytest.mark.parametrize('partial', [False, True])
def test_every_draw_lies_inside_its_rounded_interval(partial):
    for seed in range(6):
        g, c = seeded(100 + seed, shift=0.3 * (seed - 2)), 4
        if partial:
            A, B, e = restated_partial_intervals(*faithful.attack_statistics_sequential(g[:c]))
        else:
            A, B, e = restated_full_intervals(*restated_column_extremes(g, c))
        assert np.all(A <= B)
        rows = restated_fang_rows(A, B, e, c, seed=seed, round=3)
        assert np.all(rows >= A.astype(np.float32)[None, :]) and np.all(rows <= B.astype(np.float32)[None, :])
        assert np.array_equal(bits(restated_fang_trmean(g, c, partial=partial, seed=seed, round=3)[:c]), bits(rows))
        assert np.array_equal(bits(restated_fang_trmean(g, c, partial=partial, seed=seed, round=3)[c:]), bits(g[c:]))


def test_attacker_rows_draw_different_words():
    words = np.stack([restated_words(64, 5, 9 | i << 32, 0) for i in range(4)])
    for i in range(4):
        for j in range(i):
            assert not np.any(words[i] == words[j])
    g = seeded(7)
    rows = restated_fang_trmean(g, 4, seed=5, round=9)[:4]
    assert len({rows[i].tobytes() for i in range(4)}) == 4
    assert not np.array_equal(bits(rows), bits(restated_fang_trmean(g, 4, seed=5, round=10)[:4]))
    assert not np.array_equal(bits(rows), bits(restated_fang_trmean(g, 4, seed=6, round=9)[:4]))


@pytest.mark.parametrize('partial', [False, True])
def test_any_split_of_the_columns_concatenates_to_the_one_call_matrix(partial):
    g, c = seeded(11, d=67), 3
    whole = restated_fang_trmean(g, c, partial=partial, seed=2, round=1, column_offset=5)
    for cuts in ((1,), (2, 3), (5, 6, 7, 30), (3, 66)):
        edges = (0,) + cuts + (67,)
        parts = [restated_fang_trmean(g[:, a:b], c, partial=partial, seed=2, round=1, column_offset=5 + a)
                 for a, b in zip(edges[:-1], edges[1:])]
        assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(whole))


def test_the_four_branches_of_the_full_knowledge_interval():
    f = np.float32
    mean = np.array([1, 1, -1, -1, 0.0, -0.0, np.nan], dtype=f)
    lo = np.array([2, -2, 7, 7, 3, 3, 3], dtype=f)
    hi = np.array([9, 9, 4, -4, 5, 5, -5], dtype=f)
    A, B, e = restated_full_intervals(mean, lo, hi, b=2.0)
    assert A.tolist() == [1.0, -4.0, 4.0, -4.0, 5.0, 5.0, -5.0]         # lo / b, b lo, hi, hi / b; mean = 0, -0.0, NaN: hi's side
    assert B.tolist() == [2.0, -2.0, 8.0, -2.0, 10.0, 10.0, -2.5]
    assert e.tolist() == [2.0, -2.0, 4.0, -4.0, 5.0, 5.0, -5.0]
    # lo = 0 and hi = 0 take the "<= 0" branches and give the end itself
    A, B, e = restated_full_intervals(np.array([1, -1], dtype=f), np.zeros(2, dtype=f), np.zeros(2, dtype=f))
    assert A.tolist() == [0.0, 0.0] and B.tolist() == [0.0, 0.0]
    # the ends are fp64 products of the fp32 extreme: 0.1f / 2 is not fl32(0.05)
    A, _, _ = restated_full_intervals(np.ones(1, dtype=f), np.array([0.1], dtype=f), np.ones(1, dtype=f))
    assert A[0] == float(f(0.1)) / 2.0


def test_a_nan_is_skipped_in_the_extremes_and_a_column_without_a_number_gives_nan():
    g = seeded(13, n=9, d=6)
    g[4, 0] = np.nan
    g[3:, 1] = np.nan
    g[0, 2] = np.nan                                    # an attacker's NaN reaches the mean alone
    g[8, 3] = np.inf
    mean, lo, hi = restated_column_extremes(g, 3)
    assert lo[0] == np.delete(g[3:, 0], 1).min() and hi[0] == np.delete(g[3:, 0], 1).max()
    assert np.isnan(lo[1]) and np.isnan(hi[1])
    assert np.isnan(mean[2]) and lo[2] == g[3:, 2].min()
    assert hi[3] == np.inf and np.isfinite(lo[3])
    out = restated_fang_trmean(g, 3, seed=1)
    assert np.all(np.isnan(out[:3, 1]))                 # the extreme itself: NaN, and no other column gained one
    assert not np.isnan(out[:3, [0, 2, 4, 5]]).any()
    # mean = +inf > 0 goes below lo; mean of column 2 is NaN: above hi
    assert np.all(out[:3, 3] <= lo[3]) and np.all(out[:3, 2] >= hi[2])


def test_an_infinite_extreme_gives_the_extreme():
    f = np.float32
    A, B, e = restated_full_intervals(np.array([1, -1, 1, -1], dtype=f), np.array([-np.inf, 0, np.inf, 0], dtype=f),
                                      np.array([0, np.inf, 0, -np.inf], dtype=f))
    got = restated_draw(np.array([0, 1, 2, 0xffffffff]), A, B, e)
    assert got.tolist() == [-np.inf, np.inf, np.inf, -np.inf]
    # a finite extreme whose far end overflows fp64 is not finite either
    A, B, e = restated_full_intervals(np.array([-1], dtype=f), np.zeros(1, dtype=f), np.array([3e38], dtype=f), b=1e308)
    assert not np.isfinite(B[0]) and restated_draw(np.array([7]), A, B, e)[0] == f(3e38)


def test_one_attacker_with_partial_knowledge_gets_the_end_itself():
    g = seeded(17)
    out = restated_fang_trmean(g, 1, partial=True, seed=3)
    assert np.array_equal(bits(out[0]), bits(g[0]))     # sigma = 0: [mu, mu], mu the row itself
    A, B, e = restated_partial_intervals(g[0], np.zeros_like(g[0]))
    assert np.array_equal(A, B) and np.array_equal(bits(e), bits(g[0]))


def test_the_trimmed_mean_can_only_move_the_attackers_way():
    """Full knowledge.  Where mean_j > 0 every attacker value is <= the smallest benign one, so the kept ranks c .. n - c - 1 of
    the attacked column are the n - 2c smallest BENIGN values; rank k of the honest column has at most c attacker values below
    it and is therefore >= the (k - c)-th smallest benign value: term by term the attacked sum is <= the honest one, and
    rounding is monotone.  The other columns mirror it.  No exception is allowed."""
    n, c, d = 20, 4, 64
    for seed in range(24):
        g = seeded(200 + seed, n, d, shift=0.25 * ((seed % 5) - 2))
        mean = np.mean(g, axis=0)
        honest, attacked = rank_trimmed_mean_f64(g, c), rank_trimmed_mean_f64(restated_fang_trmean(g, c, seed=seed, round=seed), c)
        down = mean > 0
        assert down.any() or seed % 5 == 0
        assert np.all(attacked[down] <= honest[down]) and np.all(attacked[~down] >= honest[~down])
        median_h, median_a = np.median(g.astype(np.float64), axis=0), np.median(restated_fang_trmean(g, c, seed=seed).astype(np.float64), axis=0)
        assert np.all(median_a[down] <= median_h[down]) and np.all(median_a[~down] >= median_h[~down])


# ---- the Krum attack ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed, n, c, d', KRUM_CASES)
def test_lambda0_is_theorem_one_by_brute_force(seed, n, c, d):
    g = krum_case(seed, n, c, d)
    block = faithful.distance_matrix(g[c:])
    g64 = g[c:].astype(np.float64)
    q = (g64 * g64).sum(axis=1)
    m = n - c
    sums = [np.sort(np.delete(block[i], i).astype(np.float64))[:n - c - 2].sum() for i in range(m)]
    want = min(sums) / ((n - 2 * c - 1) * np.sqrt(float(d))) + max(np.sqrt(q)) / np.sqrt(float(d))
    assert restated_lambda0(block, q, n, c, d) == want


@pytest.mark.parametrize('seed, n, c, d', KRUM_CASES)
def test_the_krum_attack_halves_lambda_until_krum_picks_an_attacker(seed, n, c, d):
    g = krum_case(seed, n, c, d)
    attacked, info = restated_krum_attack_matrix(g, c)
    assert info['succeeded'] and 0 <= info['chosen'] < c and info['steps'] >= 2
    assert info['lambdas'] == [info['lambda0'] / 2.0 ** k for k in range(info['steps'])] and info['lambda'] == info['lambdas'][-1]
    # the loop stopped at the FIRST such k: Krum on every earlier step's matrix picks a benign row
    s = restated_sign(np.mean(g, axis=0))
    g64 = g[c:].astype(np.float64)
    block, q, t = faithful.distance_matrix(g[c:]), (g64 * g64).sum(axis=1), g64 @ s.astype(np.float64)
    for lam in info['lambdas'][:-1]:
        assert cpu_krum(restated_krum_matrix(block, q, t, lam, n, c, d), c) >= c
    # the formula is the distance: Krum on the attacked rows themselves picks an attacker, and that row is -lambda s
    assert np.array_equal(bits(attacked[:c]), bits(np.tile(-np.float32(info['lambda']) * s, (c, 1))))
    assert np.array_equal(bits(attacked[c:]), bits(g[c:]))
    want = np.sqrt(((attacked[c:].astype(np.float64) - attacked[0].astype(np.float64)) ** 2).sum(axis=1))
    assert np.allclose(info['dist'][c:, 0], want, rtol=1e-6)
    assert 0 <= faithful.krum(attacked, n, c, return_index=True) < c


def test_the_krum_attack_gives_up_below_the_threshold():
    n, c, d = 12, 2, 40
    for g in (krum_case(7003, n, c, d, mu=20.0), np.tile(krum_case(7004, 1, 0, d, mu=1.0), (n, 1))):
        attacked, info = restated_krum_attack_matrix(g, c, threshold=1e-3)
        assert not info['succeeded'] and info['chosen'] >= c
        assert info['lambda'] < 1e-3 <= info['lambdas'][-2] and info['lambda'] == info['lambda0'] / 2.0 ** (info['steps'] - 1)
        assert np.isfinite(attacked).all() and np.all(np.abs(attacked[:c]) == np.float32(info['lambda']))


def test_the_krum_attack_needs_more_than_2c_plus_1_rows():
    g = krum_case(7005, 5, 2, 8)
    with pytest.raises(ValueError):
        restated_krum_attack_matrix(g, 2)
    with pytest.raises(ValueError):
        restated_krum_attack_matrix(g, 0)
    restated_krum_attack_matrix(krum_case(7005, 6, 2, 8), 2)


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_new_entry_points_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    assert '#define BYZ_ABI_VERSION 1\n' in text
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    assert 'byz_fang_params' in code and not re.search(r'\bbyz_fang_\w*sharded', code)
    assert 'NO SHARDED ENTRY POINT for A and B' in text and 'copies of it here' in text
    assert 'philox_uniform' in open(os.path.join(CSRC, 'philox.hpp')).read()


def test_the_ctypes_table_lists_them():
    import ctypes
    from attacking_federate_learning_amd import _native
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS, name
    i64, vp, P = ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER
    assert _native._PROTOTYPES['byz_fang_trmean_attack_dev'] == [vp, vp, i64, i64, i64, i64, P(_native.FangParams), vp]
    assert [f[0] for f in _native.FangParams._fields_] == ['b', 'k_lo', 'k_hi', 'partial', 'seed', 'round', 'column_offset']
    assert ctypes.sizeof(_native.FangParams) == 56 and _native.FangParams.seed.offset == 32


def test_the_source_is_on_the_build_list():
    from attacking_federate_learning_amd import build_native
    assert 'fang.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['fang.hip']
    source = open(os.path.join(CSRC, 'fang.hip')).read()
    for kernel in ('column_extremes_kernel', 'fang_fill_kernel', 'sign_vector_kernel', 'fang_krum_fill_kernel'):
        assert '__global__' in source and kernel in source, kernel


def test_python_surface():
    from attacking_federate_learning_amd import defences, malicious
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    for name in ('column_extremes', 'fang_trmean_attack', 'fang_krum_attack', 'fang_krum_info'):
        assert callable(getattr(Engine, name)), name
    assert str(inspect.signature(Engine.fang_trmean_attack)) == (
        '(self, g, n_malicious, b=2.0, partial=False, seed=0, round=0, column_offset=0, k_lo=3.0, k_hi=4.0)')
    assert str(inspect.signature(Engine.fang_krum_attack)) == (
        '(self, g, n_malicious, threshold=1e-05, return_info=False, return_working=False)')
    assert str(inspect.signature(DeviceServer.attack_fang_trimmed_mean)) == '(self, n_malicious, b=2.0, partial=False, seed=0)'
    assert str(inspect.signature(DeviceServer.attack_fang_krum)) == '(self, n_malicious, threshold=1e-05)'
    assert 'fang_round' in DeviceServer.attack_fang_trimmed_mean.__doc__
    assert str(inspect.signature(malicious.FangTrimmedMeanAttack.__init__)) == '(self, b=2.0, partial=False, seed=0)'
    assert str(inspect.signature(malicious.FangKrumAttack.__init__)) == '(self, threshold=1e-05)'
    assert issubclass(malicious.FangTrimmedMeanAttack, malicious.Attack) and issubclass(malicious.FangKrumAttack, malicious.Attack)
    assert 'ITS OWN row' in malicious.FangTrimmedMeanAttack.__doc__ and 'DriftAttack' in malicious.FangTrimmedMeanAttack.__doc__
    assert list(inspect.signature(malicious.FangTrimmedMeanAttack.attack).parameters) == ['self', 'users', 'benign_users']
    assert malicious.FangKrumAttack().num_std is None and malicious.FangTrimmedMeanAttack().num_std is None
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    with pytest.raises(ValueError):
        Engine._fang_params(1.0, False, 0, 0, 0)
    with pytest.raises(ValueError):
        Engine._fang_params(float('inf'), False, 0, 0, 0)
    with pytest.raises(ValueError):
        Engine._fang_params(2.0, False, 0, 1 << 32, 0)
    with pytest.raises(ValueError):
        Engine._fang_params(2.0, True, 0, 0, 0, k_lo=4.0, k_hi=3.0)
    with pytest.raises(ValueError):
        Engine._fang_params(2.0, False, 0, 0, -1)
    p = Engine._fang_params(2.5, True, (1 << 64) + 5, 7, 9)
    assert (p.b, p.k_lo, p.k_hi, p.partial, p.seed, p.round, p.column_offset) == (2.5, 3.0, 4.0, 1, 5, 7, 9)
    # full knowledge without the benign gradients is refused before anything reaches the engine
    class User:
        grads = np.zeros(4, dtype=np.float32)
    with pytest.raises(ValueError):
        malicious.FangKrumAttack()._matrix([User()], None, needs_benign=True)
    assert malicious.FangKrumAttack().bind(np.ones((3, 4)))._matrix([User()], None, needs_benign=True).shape == (4, 4)


def test_the_dropin_shim_re_exports_both_classes():
    import importlib.util
    from attacking_federate_learning_amd import malicious
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'malicious.py')
    spec = importlib.util.spec_from_file_location('shim_malicious_fang', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.FangTrimmedMeanAttack is malicious.FangTrimmedMeanAttack and mod.FangKrumAttack is malicious.FangKrumAttack
    assert mod.DriftAttack is malicious.DriftAttack


def test_the_documents_name_the_new_entry_points():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert name in integration, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'column_extremes_kernel' in design and 'fang_krum_fill_kernel' in design and 'all-reduce of t and q' in design
    assert 'Fang, Cao, Jia' in open(os.path.join(ROOT, 'PAPERS.md')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'fang_trmean_attack' in readme and 'fang_krum_attack' in readme
