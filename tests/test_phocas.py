"""The mean of the values nearest a given centre, Phocas and MeaMed (Xie, Koyejo and Gupta 2018) on the CPU: the
numpy restatement the GPU tests hold csrc/centre_window.hip to, checked against first principles here; that Phocas is neither the
rank-trimmed mean nor the mean around the median; that the tie rule (equal distances go to the earlier row) shows in the
result; the non-finite cases of the contract; and the surface (header, ctypes table, Engine, defences, ShardedAggregator)."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests.test_rank_trim import bar, negative_nan, restated_median, restated_rank_trimmed_mean

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement (imported by tests/test_gpu_phocas.py) ------------------------------------------------------------------
def window_order(g, centre):
    """(a, order): a = |fl32(col - c)| and np.argsort(a, kind='stable') per column -- ties by row, every NaN behind +inf in row
    order.  What restated_window needs and `keep` does not enter (the GPU tests check several keeps against one sort)."""
    g = np.asarray(g, dtype=np.float32)
    c = np.asarray(centre, dtype=np.float32).reshape(1, -1)
    assert c.shape[1] == g.shape[1]
    with np.errstate(all='ignore'):
        a = np.abs(np.subtract(g, c, dtype=np.float32))
    return a, np.argsort(a, axis=0, kind='stable')


def restated_window(g, centre, keep, ordered=None):
    """(out, radius, kept): kept = order[:keep] (the row numbers, keep x cols), radius = a[order[keep - 1]] and
    out = fl32(fp64 sum of col[kept] / keep) (numpy's pairwise fp64 sum: within (keep - 1) 2^-53 sum|x| of the exact one).
    ordered: window_order(g, centre) when the caller has it already."""
    g = np.asarray(g, dtype=np.float32)
    assert 1 <= keep <= g.shape[0]
    a, order = window_order(g, centre) if ordered is None else ordered
    with np.errstate(all='ignore'):
        kept = order[:keep]
        radius = np.take_along_axis(a, order[keep - 1:keep], axis=0)[0]
        out = (np.take_along_axis(g, kept, axis=0).astype(np.float64).sum(axis=0) / keep).astype(np.float32)
    return out, radius, kept


def restated_window_mean(g, centre, keep):
    return restated_window(g, centre, keep)[0]


def restated_phocas(g, b):
    """Phocas by definition: the window of n - b values around the b-trimmed mean (tests/test_rank_trim.py's restatement)."""
    g = np.asarray(g, dtype=np.float32)
    return restated_window_mean(g, restated_rank_trimmed_mean(g, b), g.shape[0] - b)


def window_within_bar(out, g, kept, ref=None):
    """Per column: equal non-finite results, the finite ones within |out - ref| <= 2^-23 |ref| + 2^-30 mabs + 2^-149, the
    bar of the rank-trimmed mean.  `ref` defaults to the fp64 numpy mean of col[kept]; `kept` is restated_window's."""
    vals = np.take_along_axis(np.asarray(g, dtype=np.float32), kept, axis=0).astype(np.float64)
    with np.errstate(all='ignore'):
        if ref is None:
            ref = vals.sum(axis=0) / vals.shape[0]
        mabs = np.abs(vals).sum(axis=0) / vals.shape[0]
    out = np.asarray(out, dtype=np.float64)
    finite = np.isfinite(ref)
    if not np.array_equal(np.isnan(out), np.isnan(ref)):
        return False
    if not np.array_equal(out[~finite & ~np.isnan(ref)], ref[~finite & ~np.isnan(ref)]):
        return False
    return bool(np.all(np.abs(out[finite] - ref[finite]) <= bar(ref[finite], mabs[finite])))


def same_radius(got, want):
    """The radius' bits as integers; where the restatement's is NaN any NaN will do."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def tie_case(n, d, seed, scale=1.0):
    """The tie recipe: quarter-integer data, uniform in [-10, 10], and a quarter-integer GIVEN centre, uniform in [-2, 2]:
    c + t and c - t are both there, at the window's edge more often than not."""
    rng = np.random.default_rng(seed)
    g = (rng.integers(-40, 41, size=(n, d)) / 4.0).astype(np.float32)
    c = (rng.integers(-8, 9, size=d) / 4.0).astype(np.float32)
    return (g * np.float32(scale)).astype(np.float32), (c * np.float32(scale)).astype(np.float32)


def order_matters(g, c, keep):
    """(forward, reversed, differ): the restatement on the rows as they lie, on the rows reversed, and the columns where the
    two choices of the tied rows differ by more than twice the bar."""
    fwd, _, kept = restated_window(g, c, keep)
    rev = restated_window_mean(g[::-1], c, keep)
    vals = np.take_along_axis(g, kept, axis=0).astype(np.float64)
    twice = 2.0 * bar(np.abs(vals.mean(axis=0)), np.abs(vals).mean(axis=0))
    return fwd, rev, np.abs(fwd.astype(np.float64) - rev.astype(np.float64)) > twice


def shifted_case(n, b, d=512, seed=0):
    """Quarter-integer values in [-10, 10], the first b rows shifted by +7: the separation test's data."""
    rng = np.random.default_rng(seed + 1000 * n)
    g = (rng.integers(-40, 41, size=(n, d)) / 4.0).astype(np.float32)
    g[:b] += np.float32(7.0)
    return g


# ---- the restatement against first principles ---------------------------------------------------------------------------
def brute_window(col, c, keep):
    """One column by hand: Python's stable sort of the rows by |fl32(x - c)|, then math.fsum."""
    d = [abs(float(np.float32(x) - np.float32(c))) for x in col]
    rows = sorted(range(len(col)), key=lambda r: d[r])[:keep]
    return math.fsum(float(col[r]) for r in rows) / keep, math.fsum(abs(float(col[r])) for r in rows) / keep, d[rows[-1]], rows


@pytest.mark.parametrize('n', [1, 2, 5, 64, 257])
def test_the_window_mean_against_a_per_column_loop(n):
    rng = np.random.default_rng(n)
    d = 24
    g = (rng.standard_normal((n, d)) * 3).astype(np.float32)
    g[:, ::3] = np.round(g[:, ::3] * 4) / 4                    # ties in the distance, c + t against c - t among them
    c = (rng.standard_normal(d)).astype(np.float32)
    c[::3] = np.round(c[::3] * 4) / 4
    for keep in sorted({1, min(2, n), max(1, n // 2), max(1, n - 1), n}):
        out, radius, kept = restated_window(g, c, keep)
        ref = np.empty(d)
        for j in range(d):
            ref[j], mabs, rad, rows = brute_window(g[:, j], c[j], keep)
            assert list(kept[:, j]) == rows, (n, keep, j)
            assert np.float32(rad) == radius[j]
            assert abs(float(out[j]) - ref[j]) <= bar(abs(ref[j]), mabs), (n, keep, j)
        assert window_within_bar(out, g, kept, ref=ref)


@pytest.mark.parametrize('n,b', [(1, 0), (2, 0), (5, 2), (64, 15), (257, 61)])
def test_phocas_is_the_trimmed_mean_then_the_nearest_n_minus_b(n, b):
    rng = np.random.default_rng(10 * n + b)
    g = (rng.standard_normal((n, 19)) * 2).astype(np.float32)
    g[:, ::4] = np.round(g[:, ::4] * 4) / 4
    got = restated_phocas(g, b)
    for j in range(19):
        col = sorted(float(x) for x in g[:, j])[b:n - b]
        centre = np.float32(math.fsum(col) / len(col))
        if centre != restated_rank_trimmed_mean(g, b)[j]:
            continue                                        # (the fp64 numpy sum rounded the other way: another centre)
        ref, mabs, _, _ = brute_window(g[:, j], centre, n - b)
        assert abs(float(got[j]) - ref) <= bar(abs(ref), mabs), (n, b, j)
    if b == 0:
        assert np.allclose(got, g.astype(np.float64).mean(axis=0), rtol=2e-7, atol=1e-30)


@pytest.mark.parametrize('n,b', [(11, 2), (64, 15), (257, 61)])
def test_phocas_is_neither_the_trimmed_mean_nor_the_mean_around_the_median(n, b):
    g = shifted_case(n, b)
    ph = restated_phocas(g, b)
    rtm = restated_rank_trimmed_mean(g, b)
    meamed = restated_window_mean(g, restated_median(g), n - b)
    assert np.count_nonzero(ph != rtm) >= 0.9 * 512, np.count_nonzero(ph != rtm)
    assert np.count_nonzero(ph != meamed) >= 0.15 * 512, np.count_nonzero(ph != meamed)


TIE_SHAPES = [(64, 40), (257, 196), (1000, 760), (4097, 3000)]


@pytest.mark.parametrize('n,keep', TIE_SHAPES)
def test_the_tie_rule_shows_in_the_result(n, keep):
    g, c = tie_case(n, 256, seed=n)
    fwd, rev, differ = order_matters(g, c, keep)
    assert np.count_nonzero(fwd != rev) >= 0.2 * 256, np.count_nonzero(fwd != rev)
    assert np.count_nonzero(differ) >= 0.2 * 256, np.count_nonzero(differ)


def test_non_finite_values_and_centres():
    n, keep = 9, 6
    col = np.array([0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0], dtype=np.float32)
    g = np.tile(col[:, None], (1, 8))
    c = np.zeros(8, dtype=np.float32)
    g[1, 0] = np.nan                                           # a NaN where a kept value was: NaN sorts last, is trimmed (keep 6)
    g[[1, 2, 3, 4], 1] = [np.nan, negative_nan(), np.nan, np.nan]   # four NaNs, five numbers: one NaN is kept
    g[1, 2] = np.inf                                           # an infinity beyond keep: trimmed
    g[[3, 5, 6, 7], 3] = np.inf                                # four +inf, five numbers: one kept
    g[[3, 5, 6, 7], 4] = [-np.inf, np.inf, np.inf, np.inf]     # the first infinity in row order is -inf: kept alone
    g[[3, 5, 6, 7, 8], 5] = [-np.inf, np.inf, np.inf, np.inf, np.inf]   # four numbers: -inf and +inf both kept
    c[6] = np.nan                                              # a NaN centre: every distance NaN, the first `keep` rows
    c[7] = np.inf                                              # an infinite centre: every distance +inf, the first `keep` rows
    out, radius, kept = restated_window(g, c, keep)
    assert out[0] == np.float32(np.mean([0, -1, 2, -2, 3, -3])) and radius[0] == 3.0
    assert np.isnan(out[1]) and np.isnan(radius[1]) and list(kept[:, 1]) == [0, 5, 6, 7, 8, 1]
    assert out[2] == np.float32(np.mean([0, -1, 2, -2, 3, -3])) and radius[2] == 3.0
    assert out[3] == np.inf and radius[3] == np.inf and list(kept[:, 3]) == [0, 1, 2, 4, 8, 3]
    assert out[4] == -np.inf and radius[4] == np.inf
    assert np.isnan(out[5]) and radius[5] == np.inf and list(kept[:, 5]) == [0, 1, 2, 4, 3, 5]
    assert out[6] == np.float32(col[:keep].astype(np.float64).mean()) and np.isnan(radius[6])
    assert out[7] == np.float32(col[:keep].astype(np.float64).mean()) and radius[7] == np.inf
    assert list(kept[:, 6]) == list(range(keep)) and list(kept[:, 7]) == list(range(keep))
    assert window_within_bar(out, g, kept)                     # (the helper takes NaN for NaN and an infinity for itself)
    wrong = out.copy()
    wrong[5] = np.inf
    assert not window_within_bar(wrong, g, kept)
    g[2, 7] = np.inf                                           # inf - inf: a NaN distance, behind the +inf ones
    assert list(restated_window(g, c, keep)[2][:, 7]) == [0, 1, 3, 4, 5, 6]


# ---- the surface ------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = {'byz_window_mean_dev': 11, 'byz_phocas_dev': 11, 'byz_window_mean_host': 8, 'byz_phocas_host': 8}


def test_the_new_names_and_their_signatures():
    from attacking_federate_learning_amd import _native, build_native, defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(Engine.window_mean)) == \
        '(self, g, centre, keep, row_index=None, validate_index=True, return_radius=False)'
    assert str(inspect.signature(Engine.phocas)) == '(self, g, trim_count, row_index=None, validate_index=True)'
    assert str(inspect.signature(defences.phocas)) == '(users_grads, users_count, corrupted_count)'
    assert str(inspect.signature(defences.mean_around)) == \
        "(users_grads, users_count, corrupted_count, centre='median', keep=None)"
    assert str(inspect.signature(ShardedAggregator.phocas)) == \
        '(self, g_local, users_count, corrupted_count, gather=False, total_columns=None)'
    assert str(inspect.signature(ShardedAggregator.window_mean)) == \
        '(self, g_local, centre_local, keep, gather=False, total_columns=None)'
    assert callable(HipKernels.phocas) and callable(HipKernels.window_mean)
    header = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    for name, count in NEW_SYMBOLS.items():
        assert name in _native.EXPORTED_SYMBOLS, name
        assert len(_native._PROTOTYPES[name]) == count, name
        declared = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, header)
        assert declared and len(declared.group(1).split(',')) == count, name
    assert re.search(r'#define BYZ_ABI_VERSION 1\b', header)
    assert 'centre_window.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['centre_window.hip']
    assert os.path.exists(os.path.join(build_native.CSRC, 'centre_window.hip'))


def test_the_library_exports_them():
    from attacking_federate_learning_amd import _native, build_native
    build_native.build()
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_neither_is_a_defend_key_and_the_dropin_shim_re_exports_them():
    import importlib.util
    from attacking_federate_learning_amd import defences
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert defences.phocas not in defences.defend.values()
    assert defences.mean_around not in defences.defend.values()
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_phocas', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.phocas) and callable(mod.mean_around)
    assert list(mod.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert mod.defend == defences.defend


def test_argument_errors_on_the_host_path_are_raised_before_anything_runs():
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import Engine
    eng = object.__new__(Engine)                      # no context, no library: whatever reaches for one fails otherwise
    g = np.zeros((10, 8), dtype=np.float32)
    c = np.zeros(8, dtype=np.float32)
    for call in (lambda: Engine.window_mean(eng, g, c, 0), lambda: Engine.window_mean(eng, g, c, 11),
                 lambda: Engine.window_mean(eng, g, c, None), lambda: Engine.window_mean(eng, g, None, 3),
                 lambda: Engine.window_mean(eng, g, np.zeros(7, dtype=np.float32), 3),
                 lambda: Engine.window_mean(eng, g, c, 3, row_index=[]),
                 lambda: Engine.window_mean(eng, g, c, 4, row_index=[1, 2, 3]),
                 lambda: Engine.phocas(eng, g, 5), lambda: Engine.phocas(eng, g, -1), lambda: Engine.phocas(eng, g, None),
                 lambda: Engine.phocas(eng, g, 1, row_index=[]), lambda: Engine.phocas(eng, g, 1, row_index=[4, 5]),
                 lambda: defences.mean_around(g, 10, 2, centre='mean'), lambda: defences.mean_around(g, 10, 2, keep=0),
                 lambda: defences.mean_around(g, 10, 2, keep=11)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(AssertionError):
        defences.phocas(g, 10, 5)
