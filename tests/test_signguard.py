"""SignGuard without a GPU: the numpy restatement of the contract (include/byzagg.h) that
tests/test_gpu_signguard.py holds the kernels to, its own properties, the comparison with scikit-learn where that is
installed, and the public surface (names and signatures at every layer, not a `defend` key).

The restatement: the census is vectorised numpy on the bits; the norms, their median, the norm filter, the three features and
the bandwidth follow the header operation by operation in fp64; the mean shift is a plain loop over the seeds; the sum is
tests/test_fltrust.py's restated_scaled_sum with w and K.

The margin.  The restatement also returns the smallest RELATIVE distance from its threshold of any comparison it makes:
membership d^2 <= h^2, the stop test, suppression, the orphan test, the nearest centre against the second nearest, the norm
filter, x / h against the half-integer its rounding turns on, and the coordinates that decide the order of two centres with
equal member counts.  Device and numpy add a centre's members in different orders, so their decisions can be asked to agree
only where that margin is clear: every input a GPU test uses has margin >= 1e-9, asserted here.  An honest equality (two
centres with the SAME members are the same bits on either side) is resolved by the stated tie rules and is no near miss."""
import functools
import inspect
import os
import re

import numpy as np
import pytest

from tests.test_fltrust import restated_scaled_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (rows, columns): the kernel's boundaries (tests/test_gpu_signguard.py says which)
SHAPES = [(1, 777), (2, 4096), (7, 1023), (9, 1025), (33, 2051), (100, 5000), (1000, 2048), (4097, 300), (20000, 64), (16, 1)]
WIDE = (13, 600_000)
# shapes whose window is too narrow (or whose rows too few) for an estimated bandwidth to mean anything: a fixed one
FIXED_BANDWIDTH = {(1, 777): 0.25, (2, 4096): 0.25, (20000, 64): 0.3, (16, 1): 0.25}
MARGIN = 1e-9
MIN_BANDWIDTH = 2.0 ** -20
MAX_SHIFTS = 300


# ---- the inputs ------------------------------------------------------------------------------------------------------
def alie(n, d, seed, mal_prop=0.24, z=1.0):
    """Honest rows s + noise; the first int(mal_prop * n) rows are the "A Little Is Enough" vector mean - z * std of the honest
    ones, which is what the reference's malicious.DriftAttack produces."""
    rng = np.random.default_rng(seed)
    s = (0.5 * rng.standard_normal(d)).astype(np.float32)
    g = (s[None, :] + rng.standard_normal((n, d))).astype(np.float32)
    f = int(n * mal_prop)
    if f:
        honest = g[f:].astype(np.float64)
        g[:f] = (honest.mean(axis=0) - z * honest.std(axis=0)).astype(np.float32)[None, :]
    return g


def window_of(d, frac=0.1, seed=0):
    from attacking_federate_learning_amd.engine import signguard_window
    return signguard_window(d, frac, seed)


def sample_of(n, n_samples=50, seed=0):
    from attacking_federate_learning_amd.engine import signguard_sample
    return signguard_sample(n, n_samples, seed)


# ---- the restatement -------------------------------------------------------------------------------------------------
def restated_census(g, c0, m):
    """(pos, zero, neg) as int64 over the columns [c0, c0 + m), decided on the bits, and q = the fp64 sums of squares."""
    g = np.asarray(g, dtype=np.float32)
    bits = np.ascontiguousarray(g[:, c0:c0 + m]).view(np.uint32)
    mag = bits & np.uint32(0x7fffffff)
    by_sign = (mag > 0) & (mag <= np.uint32(0x7f800000))
    minus = (bits >> np.uint32(31)) != 0
    pos = (by_sign & ~minus).sum(axis=1).astype(np.int64)
    neg = (by_sign & minus).sum(axis=1).astype(np.int64)
    zero = (mag == 0).sum(axis=1).astype(np.int64)
    x = g.astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        q = (x * x).sum(axis=1)
    return pos, zero, neg, q


class Margin:
    """The smallest relative distance of a compared value from its threshold."""

    def __init__(self):
        self.value = np.inf

    def see(self, a, b):
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
        ok = np.isfinite(a) & np.isfinite(b)
        if ok.any():
            scale = np.maximum(np.abs(a[ok]), np.abs(b[ok]))
            rel = np.where(scale > 0, np.abs(a[ok] - b[ok]) / np.where(scale > 0, scale, 1.0), 0.0)
            self.value = min(self.value, float(rel.min()))


def sqdist(x, c):
    d = x - c
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def restated_features(pos, zero, neg, m):
    m = np.float64(m)
    cols = []
    for c in (pos, zero, neg):
        share = np.asarray(c, dtype=np.float64) / m
        cols.append(share / (share.max() + 1e-8))
    return np.stack(cols, axis=1)


def restated_bandwidth(x, sample):
    """The mean, in sample order, of the k-th smallest distance from a sampled row to the sampled rows, itself included."""
    xs = x[np.asarray(sample)]
    s = len(xs)
    k = max(1, s // 2)
    total = 0.0
    for i in range(s):
        total = total + np.sort(np.sqrt(sqdist(xs, xs[i])))[k - 1]
    return total / s


def restated_mean_shift(x, h, margin):
    """(labels, clusters, seeds): flat-kernel mean shift from the bin seeds, scikit-learn's order, suppression and labels."""
    n = len(x)
    if not (np.isfinite(h) and h >= MIN_BANDWIDTH):
        return np.zeros(n, dtype=np.int32), 1, 0
    h2, stop = h * h, 1e-3 * h
    v = x / h
    margin.see(v, np.floor(v) + 0.5)
    bins = np.unique(np.round(v), axis=0)                       # ties to even; lexicographic: the packed keys' order
    centres, members = [], []
    for b in bins:
        c = h * b
        last = 0
        for _ in range(MAX_SHIFTS):
            d2 = sqdist(x, c)
            margin.see(d2, h2)
            inside = d2 <= h2
            last = int(inside.sum())
            if last == 0:
                break
            new = np.zeros(3)
            for row in x[inside]:                               # a fixed order: row order
                new = new + row
            new = new / last
            move = np.sqrt(sqdist(new, c))
            c = new
            if move != 0.0:
                margin.see(move, stop)
            if move <= stop:
                break
        if last > 0:
            centres.append(c)
            members.append(last)
    if not centres:
        return np.full(n, -1, dtype=np.int32), 0, len(bins)
    centres, members = np.array(centres), np.array(members)
    order = sorted(range(len(centres)), key=lambda i: (members[i], tuple(centres[i])), reverse=True)
    centres, members = centres[order], members[order]
    for a in range(len(centres) - 1):                           # neighbours in the order: equal counts, coordinates deciding
        if members[a] == members[a + 1] and not np.array_equal(centres[a], centres[a + 1]):
            k = int(np.argmax(centres[a] != centres[a + 1]))
            margin.see(centres[a][k], centres[a + 1][k])
    standing = np.ones(len(centres), dtype=bool)
    for a in range(len(centres)):
        if standing[a]:
            d2 = sqdist(centres[a + 1:], centres[a])
            live = standing[a + 1:]
            pairs = d2[live]
            pairs = pairs[pairs != 0.0]                         # (the same members: the same bits, an honest equality)
            if pairs.size:
                margin.see(pairs, h2)
            standing[a + 1:] &= ~(d2 <= h2)
    final = centres[standing]
    d2 = np.stack([sqdist(x, c) for c in final], axis=1)        # n x clusters
    labels = np.argmin(d2, axis=1).astype(np.int32)             # the first on ties
    best = d2[np.arange(n), labels]
    if d2.shape[1] > 1:
        rest = np.sort(d2, axis=1)[:, 1]
        margin.see(best, rest)
    margin.see(best, h2)
    labels[~(best <= h2)] = -1
    return labels, len(final), len(bins)


def restated_select(pos, zero, neg, q, m, lower=0.1, upper=3.0, bandwidth=None, sample=None):
    """The selection from the counts and squared norms: a dict with keep, weights, labels, median_norm (M), kept (K),
    bandwidth (h), seeds, clusters, norm_failed_rows, outside_rows and margin."""
    q = np.asarray(q, dtype=np.float64)
    n = len(q)
    margin = Margin()
    finite = np.isfinite(q)
    with np.errstate(invalid='ignore'):
        norm = np.sqrt(q)
    M = float(np.median(norm[finite])) if finite.any() else np.nan
    with np.errstate(invalid='ignore'):
        norm_ok = finite & (lower * M < norm) & (norm < upper * M)
        margin.see(norm[finite], lower * M)
        margin.see(norm[finite], upper * M)
    x = restated_features(pos, zero, neg, m)
    h = float(bandwidth) if bandwidth is not None and bandwidth > 0 else float(restated_bandwidth(x, sample))
    labels, clusters, seeds = restated_mean_shift(x, h, margin)
    rows = np.bincount(labels[labels >= 0], minlength=max(clusters, 1))
    benign = int(np.argmax(rows)) if (labels >= 0).any() else -1            # the lowest label on ties
    in_cluster = (labels == benign) & (benign >= 0)
    keep = norm_ok & in_cluster
    with np.errstate(invalid='ignore', divide='ignore'):
        w = np.where(keep, np.minimum(1.0, M / norm), 0.0)
    return {'keep': keep.astype(np.int32), 'weights': w, 'labels': labels, 'median_norm': M, 'kept': int(keep.sum()),
            'kept_rows': int(keep.sum()), 'bandwidth': h, 'seeds': seeds, 'clusters': clusters,
            'norm_failed_rows': int((~norm_ok).sum()), 'outside_rows': int((~in_cluster).sum()), 'margin': margin.value}


def restated_signguard(g, window, sample=None, lower=0.1, upper=3.0, bandwidth=None):
    """(out, info) of the whole rule on the matrix g with the window (c0, m)."""
    c0, m = window
    pos, zero, neg, q = restated_census(g, c0, m)
    info = restated_select(pos, zero, neg, q, m, lower, upper, bandwidth, sample)
    info.update(pos=pos, zero=zero, neg=neg, q=q)
    return restated_scaled_sum(g, info['weights'], float(info['kept'])), info


@functools.lru_cache(maxsize=None)
def case(n, d):
    """The inputs of one shape and their restatement, computed once and never written to: (g, window, sample, bandwidth,
    out, info)."""
    g = alie(n, d, seed=n + d)
    window, sample = window_of(d, seed=n + d), sample_of(n, seed=n + d)
    bandwidth = FIXED_BANDWIDTH.get((n, d))
    out, info = restated_signguard(g, window, sample, bandwidth=bandwidth)
    for a in (g, sample, out, info['keep'], info['weights'], info['labels'], info['q']):
        a.setflags(write=False)
    return g, window, sample, bandwidth, out, info


# ---- the generator keeps its promises --------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', SHAPES + [WIDE])
def test_the_generator_is_clear_of_every_threshold_and_the_rule_catches_the_attack(n, d):
    g, window, sample, bandwidth, out, info = case(n, d)
    f = int(n * 0.24)
    print((n, d), 'margin', info['margin'], 'clusters', info['clusters'], 'seeds', info['seeds'], 'h', info['bandwidth'],
          'kept', info['kept'], 'of', n - f, 'honest')
    assert info['margin'] >= MARGIN, info['margin']
    assert np.isfinite(out).all()
    if (n, d) not in FIXED_BANDWIDTH and f > 0:
        # the attack the rule is for, wherever the window is wide enough to tell the shares apart
        assert info['clusters'] >= 2
        assert info['keep'][:f].sum() == 0
        assert info['keep'][f:].sum() >= 0.9 * (n - f)


# ---- against scikit-learn --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', [(9, 1025), (33, 2051), (100, 5000), (1000, 2048)])
def test_the_labels_are_scikit_learns(n, d):
    cluster = pytest.importorskip('sklearn.cluster')
    g, window, sample, _, _, info = case(n, d)
    x = restated_features(info['pos'], info['zero'], info['neg'], window[1])
    h = info['bandwidth']
    # estimate_bandwidth takes the expanded |a|^2 - 2ab + |b|^2 for its distances at this sample size: an absolute error of a
    # few 2^-52 on squares of order h^2 >= 1e-6
    assert np.isclose(h, cluster.estimate_bandwidth(x[sample], quantile=0.5, n_samples=None), rtol=1e-8, atol=0.0)
    ms = cluster.MeanShift(bandwidth=h, bin_seeding=True, cluster_all=False).fit(x)
    ours, theirs = info['labels'], ms.labels_
    assert np.array_equal(ours == -1, theirs == -1)
    pairs = {(int(a), int(b)) for a, b in zip(ours, theirs)}
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})       # equal up to the labelling
    assert info['clusters'] == len(ms.cluster_centers_)


# ---- the restatement's own properties -------------------------------------------------------------------------------
def test_one_cluster_and_open_bounds_give_the_mean_of_the_rows_clipped_to_the_median_norm():
    g = alie(40, 500, seed=3)
    out, info = restated_signguard(g, (0, 500), lower=0.0, upper=np.inf, bandwidth=10.0)
    assert info['clusters'] == 1 and info['kept'] == 40
    x = g.astype(np.float64)
    norm = np.sqrt((x * x).sum(axis=1))
    M = np.median(norm)
    want = (x * np.minimum(1.0, M / norm)[:, None]).mean(axis=0)
    assert np.allclose(out, want, rtol=1e-6, atol=1e-7)
    assert info['median_norm'] == M


def test_a_row_scaled_by_ten_fails_the_norm_filter():
    g = alie(30, 800, seed=4, mal_prop=0.0)
    g[7] *= 10.0
    _, info = restated_signguard(g, (100, 80), bandwidth=10.0)
    assert info['keep'][7] == 0 and info['norm_failed_rows'] == 1 and info['kept'] == 29
    g[9] *= 0.05                                                # and one below a tenth of the median
    _, info = restated_signguard(g, (100, 80), bandwidth=10.0)
    assert info['keep'][[7, 9]].tolist() == [0, 0] and info['norm_failed_rows'] == 2


def test_rows_with_nan_or_inf_are_never_kept_and_the_output_has_no_nan():
    g = alie(30, 800, seed=5)
    g[8, 3], g[12, 700], g[20, 150] = np.nan, np.inf, -np.inf
    out, info = restated_signguard(g, (100, 80), sample=sample_of(30, seed=5))
    assert info['keep'][[8, 12, 20]].tolist() == [0, 0, 0] and info['weights'][[8, 12, 20]].tolist() == [0.0, 0.0, 0.0]
    assert np.isfinite(out).all() and info['kept'] > 0
    pos, zero, neg, _ = restated_census(g, 100, 80)
    assert (pos + zero + neg)[[8, 12]].tolist() == [80, 80] and (pos + zero + neg)[20] == 80   # (inf counts by its sign)
    bad = np.full((4, 50), np.nan, dtype=np.float32)
    out, info = restated_signguard(bad, (0, 50), bandwidth=1.0)
    assert np.array_equal(out, np.zeros(50, dtype=np.float32)) and info['kept'] == 0 and np.isnan(info['median_norm'])


def test_the_census_is_decided_on_the_bits():
    row = np.array([0.0, -0.0, 1e-45, -1e-45, np.inf, -np.inf, np.nan, -np.nan, 1.0, -2.0], dtype=np.float32)
    pos, zero, neg, _ = restated_census(row[None, :], 0, 10)
    assert (int(pos[0]), int(zero[0]), int(neg[0])) == (3, 2, 3)            # the two NaNs count nowhere
    pos, zero, neg, _ = restated_census(row[None, :], 2, 3)
    assert (int(pos[0]), int(zero[0]), int(neg[0])) == (2, 0, 1)


def test_identical_rows_are_one_cluster_with_a_zero_bandwidth():
    g = np.repeat(alie(1, 300, seed=6), 12, axis=0)
    out, info = restated_signguard(g, (10, 30), sample=sample_of(12, seed=6))
    assert info['bandwidth'] == 0.0 and info['clusters'] == 1 and info['seeds'] == 0
    assert (info['labels'] == 0).all() and info['kept'] == 12
    assert np.array_equal(out, g[0])                            # M / norm = 1: the rows' mean, each weight exactly 1


def test_one_row():
    g = alie(1, 300, seed=7)
    out, info = restated_signguard(g, (0, 30), sample=sample_of(1, seed=7))
    assert info['kept'] == 1 and info['labels'].tolist() == [0] and np.array_equal(out, g[0])


def test_the_window_at_both_ends_and_the_whole_row():
    from attacking_federate_learning_amd.engine import signguard_window
    g = alie(20, 400, seed=8)
    for window in ((0, 40), (360, 40), (0, 400)):
        pos, zero, neg, _ = restated_census(g, *window)
        assert ((pos + zero + neg) == window[1]).all()
        out, info = restated_signguard(g, window, sample=sample_of(20, seed=8))
        assert np.isfinite(out).all() and info['kept'] > 0
    assert signguard_window(400, 1.0, 3) == (0, 400)            # frac = 1 is the whole row
    starts = {signguard_window(11, 0.1, seed)[0] for seed in range(200)}
    assert starts == set(range(11))                             # m = 1: both ends of [0, D - m] are drawn
    assert signguard_window(5, 0.1, 0)[1] == 1                  # m is never 0
    with pytest.raises(ValueError):
        signguard_window(10, 0.0)


def test_the_sample_is_distinct_rows():
    from attacking_federate_learning_amd.engine import signguard_sample
    s = signguard_sample(1000, 50, 1)
    assert s.dtype == np.int32 and len(s) == 50 == len(set(s.tolist())) and 0 <= s.min() and s.max() < 1000
    assert signguard_sample(7, 50, 1).tolist() == list(range(7))
    assert not np.array_equal(s, signguard_sample(1000, 50, 2))


def test_no_row_kept_gives_zeros():
    g = alie(10, 200, seed=9, mal_prop=0.0)
    out, info = restated_signguard(g, (0, 20), lower=0.0, upper=1e-3, bandwidth=10.0)        # nobody is that short
    assert info['kept'] == 0 and info['norm_failed_rows'] == 10
    assert np.array_equal(out, np.zeros(200, dtype=np.float32))


# ---- the surface ----------------------------------------------------------------------------------------------------
def test_the_new_names_and_their_signatures():
    from attacking_federate_learning_amd import _native, defences, engine
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.signguard)) == \
        '(users_grads, users_count, corrupted_count, frac=0.1, lower=0.1, upper=3.0, bandwidth=None, n_samples=50, seed=0, ' \
        'window=None, sample=None, return_info=False)'
    assert 'ICDCS 2022' in defences.signguard.__doc__ and 'every round' in defences.signguard.__doc__
    assert str(inspect.signature(engine.signguard_window)) == '(n_cols, frac=0.1, seed=0)'
    assert str(inspect.signature(engine.signguard_sample)) == '(n, n_samples=50, seed=0)'
    assert 'frac = 1' in engine.signguard_window.__doc__
    assert str(inspect.signature(Engine.row_signs)) == '(self, g, window_start, window_len)'
    assert str(inspect.signature(Engine.signguard_info)) == '(self)'
    assert str(inspect.signature(Engine.signguard)) == \
        '(self, g, frac=0.1, lower=0.1, upper=3.0, bandwidth=None, n_samples=50, seed=0, window=None, sample=None, ' \
        'return_info=False)'
    assert callable(Engine.signguard_select)
    assert str(inspect.signature(DeviceServer.defend_signguard)) == \
        '(self, frac=0.1, lower=0.1, upper=3.0, bandwidth=None, n_samples=50, seed=None)'
    assert callable(HipKernels.row_signs) and callable(HipKernels.signguard_select) and callable(ShardedAggregator.signguard)
    counts = {'byz_row_signs_dev': 10, 'byz_signguard_select_dev': 11, 'byz_signguard_dev': 12, 'byz_signguard_info': 8,
              'byz_signguard_host': 10, 'byz_signguard_sharded_dev': 16}
    header = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    for name, count in counts.items():
        assert name in _native.EXPORTED_SYMBOLS, name
        assert len(_native._PROTOTYPES[name]) == count, name
        proto = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, header)
        assert proto, name
        assert len(proto.group(1).split(',')) == count, name          # the header and the binding agree on the arguments
    assert re.search(r'#define BYZ_ABI_VERSION 1\b', header)
    assert re.search(r'#define BYZ_SIGNGUARD_MAX_SAMPLES %d\b' % _native.SIGNGUARD_MAX_SAMPLES, header)
    fields = [name for name, _ in _native.SignGuardParams._fields_]
    struct = re.search(r'typedef struct byz_signguard_params \{(.*?)\} byz_signguard_params;', header, re.S).group(1)
    assert fields == re.findall(r'(\w+)\s*[,;]', re.sub(r'/\*.*?\*/', '', struct, flags=re.S))


def test_signguard_is_not_a_defend_key():
    from attacking_federate_learning_amd import defences
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert not any('sign' in k.lower() for k in defences.defend)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_sg', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.signguard) and 'signguard' not in mod.defend


def test_the_source_is_built_without_fused_multiply_add():
    from attacking_federate_learning_amd import build_native
    assert 'signguard.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['signguard.hip']
