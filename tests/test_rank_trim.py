"""The coordinate-wise median and the rank-trimmed mean (Yin et al. 2018) on the CPU: the numpy restatement
the GPU tests hold the kernels to, checked against first principles here; that they are a different rule from the reference's
trimmed_mean; and the surface (header, ctypes table, Engine, defences, drop-in shim, ShardedAggregator)."""
import inspect
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement (imported by tests/test_gpu_rank_trim.py) ---------------------------------------------------------
def restated_median(g):
    """np.median of every column of a float32 matrix (NaN if the column holds one)."""
    g = np.asarray(g, dtype=np.float32)
    with np.errstate(all='ignore'):
        return np.median(g, axis=0).astype(np.float32)


def kept_rows(g, b, presorted=False):
    """np.sort(col)[b : n - b] of every column (NaN of either sign behind +inf), as a float32 matrix.  presorted: g already
    is np.sort(g, axis=0) (the GPU tests check several trim counts against one sort)."""
    g = np.asarray(g, dtype=np.float32)
    n = g.shape[0]
    assert 0 <= b and 2 * b < n
    return (g if presorted else np.sort(g, axis=0))[b:n - b]


def restated_rank_trimmed_mean(g, b):
    """fl32(mean of kept in fp64): numpy's pairwise fp64 sum, within (n - 1) 2^-53 sum|x| of the exact one."""
    kept = kept_rows(g, b).astype(np.float64)
    with np.errstate(all='ignore'):
        return (kept.sum(axis=0) / kept.shape[0]).astype(np.float32)


def exact_rank_trimmed_mean(g, b):
    """The exactly rounded mean of kept (math.fsum), one column at a time: what the accuracy bar is stated against."""
    kept = kept_rows(g, b)
    out = np.empty(kept.shape[1], dtype=np.float64)
    for c in range(kept.shape[1]):
        col = [float(x) for x in kept[:, c]]
        if any(math.isnan(x) for x in col) or (math.inf in col and -math.inf in col):
            out[c] = math.nan
        elif math.inf in col or -math.inf in col:
            out[c] = math.inf if math.inf in col else -math.inf
        else:
            out[c] = math.fsum(col) / len(col)
    return out


def bar(ref, mabs):
    """|out - ref| <= 2^-23 |ref| + 2^-30 mabs + 2^-149 (one fp32 rounding with a factor two to spare; a fixed-order fp64 sum
    of up to 2^20 terms eight times over)."""
    return 2.0 ** -23 * np.abs(ref) + 2.0 ** -30 * mabs + 2.0 ** -149


def within_bar(out, g, b, ref=None, presorted=False):
    """Per element: equal non-finite results, the finite ones within the bar.  `ref` defaults to the fp64 numpy mean of kept
    (its own error, (n - 1) 2^-53 mabs, is far inside the bar's second term)."""
    kept = kept_rows(g, b, presorted).astype(np.float64)
    with np.errstate(all='ignore'):
        if ref is None:
            ref = kept.sum(axis=0) / kept.shape[0]
        mabs = np.abs(kept).sum(axis=0) / kept.shape[0]
    out = np.asarray(out, dtype=np.float64)
    finite = np.isfinite(ref)
    if not np.array_equal(np.isnan(out), np.isnan(ref)):
        return False
    if not np.array_equal(out[~finite & ~np.isnan(ref)], ref[~finite & ~np.isnan(ref)]):
        return False
    return bool(np.all(np.abs(out[finite] - ref[finite]) <= bar(ref[finite], mabs[finite])))


def same_median(got, want):
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and bool(np.all(got[~nan] == want[~nan]))


def negative_nan():
    return np.frombuffer(np.uint32(0xffc00000).tobytes(), dtype=np.float32)[0]


# ---- the restatement against first principles ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3, 10, 11, 64, 65])
def test_the_median_is_the_middle_value_or_the_fp32_mean_of_the_two(n):
    rng = np.random.default_rng(n)
    g = rng.standard_normal((n, 37)).astype(np.float32)
    s = np.sort(g, axis=0)
    want = s[n // 2] if n % 2 else ((s[n // 2 - 1] + s[n // 2]) * np.float32(0.5)).astype(np.float32)
    assert np.array_equal(restated_median(g), want)


def test_the_median_of_a_column_with_a_nan_is_nan_and_flt_max_overflows_as_numpy_does():
    g = np.arange(12, dtype=np.float32).reshape(4, 3)
    g[1, 0] = np.nan
    g[2, 1] = negative_nan()
    big = np.finfo(np.float32).max
    g[:, 2] = [big, big, -1.0, big]
    with np.errstate(all='ignore'):
        out = restated_median(g)
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == np.inf


@pytest.mark.parametrize('n,b', [(1, 0), (2, 0), (9, 0), (9, 2), (9, 4), (10, 4), (200, 48), (201, 100)])
def test_the_rank_trimmed_mean_against_a_per_column_loop(n, b):
    rng = np.random.default_rng(100 * n + b)
    g = (rng.standard_normal((n, 23)) * 10).astype(np.float32)
    g[:, 1] = np.round(g[:, 1] * 4) / 4          # ties across the rank edges
    want = np.empty(23, dtype=np.float32)
    for c in range(23):
        col = sorted(float(x) for x in g[:, c])[b:n - b]
        want[c] = np.float32(math.fsum(col) / len(col))
    got = restated_rank_trimmed_mean(g, b)
    assert within_bar(got, g, b, ref=exact_rank_trimmed_mean(g, b))
    assert np.allclose(got, want, rtol=2e-7, atol=0)
    if b == 0:
        assert np.allclose(got, g.astype(np.float64).mean(axis=0), rtol=2e-7)
    if n % 2 == 1 and b == (n - 1) // 2:
        assert np.array_equal(got, restated_median(g))


def test_the_bar_is_reachable_by_the_kernels_formula():
    """A numpy model of S = sum{lo < x < hi} + c_lo lo + c_hi hi with a sequential fp64 sum stays well inside the bar on plain,
    tied and cancelling columns, so the bar is not so tight that only one summation order meets it."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for trial in range(60):
        n = int(rng.integers(3, 400))
        b = int(rng.integers(0, (n - 1) // 2 + 1))
        col = rng.standard_normal(n).astype(np.float32)
        if trial % 3 == 1:
            col = (np.round(col * 4) / 4).astype(np.float32)
        if trial % 3 == 2:
            col = (col - col.mean() + np.float32(1e-3)).astype(np.float32)
        s = np.sort(col)
        lo, hi = s[b], s[n - 1 - b]
        kept = s[b:n - b]
        if lo == hi:
            out = lo
        else:
            total = 0.0
            for x in kept[(kept > lo) & (kept < hi)]:
                total += float(x)
            total += float(np.sum(kept == lo)) * float(lo) + float(np.sum(kept == hi)) * float(hi)
            out = np.float32(total / len(kept))
        ref = math.fsum(float(x) for x in kept) / len(kept)
        mabs = math.fsum(abs(float(x)) for x in kept) / len(kept)
        worst = max(worst, abs(float(out) - ref) / float(bar(np.float64(ref), mabs)))
    assert worst <= 0.6, worst


def test_non_finite_values_are_trimmed_when_they_fit_and_poison_the_column_otherwise():
    n, b = 11, 2
    g = np.tile(np.arange(n, dtype=np.float32)[:, None], (1, 8))
    g[0, 0] = np.nan; g[5, 0] = negative_nan()                   # two NaNs, both signs: trimmed (b = 2)
    g[0, 1] = np.nan; g[5, 1] = negative_nan(); g[7, 1] = np.nan   # three: one survives
    g[3, 2] = np.inf; g[4, 2] = np.inf                           # trimmed
    g[3, 3] = np.inf; g[4, 3] = np.inf; g[9, 3] = np.inf         # one +inf kept -> +inf
    g[1, 4] = -np.inf; g[2, 4] = -np.inf; g[6, 4] = -np.inf      # one -inf kept -> -inf
    g[0:3, 5] = -np.inf; g[8:11, 5] = np.inf                     # both kept -> NaN
    g[2, 6] = np.nan; g[3, 6] = np.inf; g[4, 6] = np.inf          # NaN above the infs: NaN and one inf trimmed, one inf kept
    with np.errstate(all='ignore'):
        out = restated_rank_trimmed_mean(g, b)
    ref = exact_rank_trimmed_mean(g, b)
    assert np.isfinite(out[0]) and np.isnan(out[1]) and np.isfinite(out[2])
    assert out[3] == np.inf and out[4] == -np.inf and np.isnan(out[5]) and out[6] == np.inf and np.isfinite(out[7])
    assert within_bar(out, g, b, ref=ref)
    # a NaN-free reading of column 0: the values 0..10 without rows 0 and 5, then the two smallest dropped
    assert out[0] == np.float32(np.mean([3, 4, 6, 7, 8, 9, 10]))


# ---- a different rule from trimmed_mean; robust where the mean is not ---------------------------------------------------------
def test_it_is_not_the_around_the_median_trimmed_mean():
    from oracle import faithful
    n, f = 21, 5
    col = np.concatenate([np.linspace(0.0, 1.0, 16), np.linspace(50.0, 90.0, 5)]).astype(np.float32)   # skewed to the right
    g = np.tile(col[:, None], (1, 4))
    theirs = faithful.trimmed_mean(g, n, f)          # keeps the n - f - 1 = 15 values closest to the median
    ours = restated_rank_trimmed_mean(g, f)          # keeps ranks 5 .. 15
    ref = exact_rank_trimmed_mean(g, f)
    mabs = np.abs(kept_rows(g, f)).mean(axis=0)
    assert np.all(np.abs(theirs.astype(np.float64) - ref) > 1e4 * bar(ref, mabs))
    assert within_bar(ours, g, f)


def test_the_drift_attack_moves_the_mean_but_not_these_two():
    from oracle import faithful
    rng = np.random.default_rng(11)
    n, d, f = 100, 256, 24
    g = rng.standard_normal((n, d)).astype(np.float32)
    honest_median = restated_median(g[f:])
    g[:f] = faithful.drift_vector(g[:f].copy(), 40.0)          # every malicious row: mean - 40 stdev
    moved = np.abs(faithful.no_defense(g, n, f) - g[f:].mean(axis=0))
    assert np.median(moved) > 5.0
    assert np.abs(restated_median(g) - honest_median).max() < 1.0
    assert np.abs(restated_rank_trimmed_mean(g, f) - g[f:].mean(axis=0)).max() < 1.0


# ---- the surface ------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ('byz_coordinate_median_dev', 'byz_rank_trimmed_mean_dev', 'byz_coordinate_median_host',
               'byz_rank_trimmed_mean_host')


def test_the_new_names_and_their_signatures():
    from attacking_federate_learning_amd import _native, defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.coordinate_median)) == '(users_grads, users_count, corrupted_count)'
    assert str(inspect.signature(defences.rank_trimmed_mean)) == '(users_grads, users_count, corrupted_count)'
    assert str(inspect.signature(Engine.coordinate_median)) == '(self, g, row_index=None, validate_index=True)'
    assert str(inspect.signature(Engine.rank_trimmed_mean)) == '(self, g, trim_count, row_index=None, validate_index=True)'
    assert str(inspect.signature(ShardedAggregator.coordinate_median)) == \
        '(self, g_local, users_count=None, corrupted_count=None, gather=False, total_columns=None)'
    assert str(inspect.signature(ShardedAggregator.rank_trimmed_mean)) == \
        '(self, g_local, users_count, corrupted_count, gather=False, total_columns=None)'
    assert callable(HipKernels.coordinate_median) and callable(HipKernels.rank_trimmed_mean)
    header = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS, name
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
    assert len(_native._PROTOTYPES['byz_coordinate_median_dev']) == 8
    assert len(_native._PROTOTYPES['byz_rank_trimmed_mean_dev']) == 9
    assert len(_native._PROTOTYPES['byz_coordinate_median_host']) == 5
    assert len(_native._PROTOTYPES['byz_rank_trimmed_mean_host']) == 6
    assert re.search(r'#define BYZ_ABI_VERSION 1\b', header)


def test_the_library_exports_them():
    from attacking_federate_learning_amd import _native, build_native
    build_native.build()
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.byz_abi_version() == 1


def test_neither_is_a_defend_key():
    from attacking_federate_learning_amd import defences
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert defences.coordinate_median not in defences.defend.values()
    assert defences.rank_trimmed_mean not in defences.defend.values()


def test_the_dropin_shim_re_exports_them():
    import importlib.util
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_rank', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.coordinate_median) and callable(mod.rank_trimmed_mean)
    assert 'coordinate_median' not in mod.defend and 'rank_trimmed_mean' not in mod.defend


def test_the_drop_in_asserts_the_row_count_before_anything_runs():
    from attacking_federate_learning_amd import defences
    g = np.zeros((4, 8), dtype=np.float32)
    with pytest.raises(AssertionError):
        defences.rank_trimmed_mean(g, 4, 2)
