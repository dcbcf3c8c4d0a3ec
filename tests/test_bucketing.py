"""s-bucketing (Karimireddy, He and Jaggi, "Byzantine-Robust Learning on Heterogeneous Datasets via Bucketing", ICLR 2022): the
numpy restatement of include/byzagg.h's contract, its properties, and the surface every layer has to carry.  No GPU here;
tests/test_gpu_bucketing.py holds the kernel to the restatement bit for bit."""
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ('byz_bucket_means_dev', 'byz_bucket_means_host')


# ---- the restatement ------------------------------------------------------------------------------------------------
def column_mean(rows):
    """np.mean(rows, axis=0) as numpy reduces an OUTER axis: the rows added in order, sequential fp32 from +0.0, then one
    division -- the arithmetic the contract states.  A matrix of ONE column is the exception: numpy sees an (m, 1) array as m
    contiguous values and sums them pairwise (2 ulp away from the chain in test_gpu_bucketing's 17 x 1 case, where the kernel
    has no_defense's bits); with a column of zeros beside it numpy reduces the outer axis again."""
    if rows.shape[1] == 1:
        return np.mean(np.concatenate([rows, np.zeros_like(rows)], axis=1), axis=0)[:1]
    return np.mean(rows, axis=0)


def restated_buckets(g, s, perm=None):
    """Row b: np.mean(g[perm[b*s:(b+1)*s]], axis=0); perm=None is the identity.  The last bucket may be short."""
    g = np.asarray(g, dtype=np.float32)
    n = g.shape[0]
    assert 1 <= s <= n
    perm = np.arange(n) if perm is None else np.asarray(perm)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([column_mean(g[perm[b * s:(b + 1) * s]]) for b in range(-(-n // s))])


def chained_buckets(g, s, perm):
    """The contract's arithmetic spelt out: per bucket a sequential fp32 chain from +0.0 in list order, then / float(c_b)."""
    out = []
    for b in range(-(-g.shape[0] // s)):
        rows = perm[b * s:(b + 1) * s]
        total = np.zeros(g.shape[1], dtype=np.float32)
        for r in rows:
            total = total + g[r]
        out.append(total / np.float32(len(rows)))
    return np.stack(out)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def heterogeneous(n, d, f, seed):
    """Honest rows of different scales and offsets (non-IID clients), the first f rows one vector (identical Byzantine rows)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d)).astype(np.float32)
    g *= (1.0 + 0.5 * rng.permutation(n) / n).astype(np.float32)[:, None]
    g += rng.standard_normal((n, 1)).astype(np.float32)
    if f:
        g[:f] = np.float32(-7.0)
    return g


# ---- properties of the restatement ------------------------------------------------------------------------------------
def test_one_bucket_is_the_column_mean_and_buckets_of_one_are_the_permuted_rows():
    from attacking_federate_learning_amd.engine import bucketing_permutation
    g = heterogeneous(37, 211, 0, seed=1)
    assert np.array_equal(bits(restated_buckets(g, 37)), bits(np.mean(g, axis=0)[None, :]))
    perm = bucketing_permutation(37, seed=5)
    assert np.array_equal(restated_buckets(g, 1, perm), g[perm])


def test_the_restatement_is_the_sequential_chain_at_every_width():
    """np.mean over the rows IS the chain the header states, one column included (column_mean says why that needs care)."""
    from attacking_federate_learning_amd.engine import bucketing_permutation
    for d in (1, 2, 3, 257):
        for n in (8, 9, 17, 100):
            g = np.random.default_rng(100 * n + d).standard_normal((n, d)).astype(np.float32)
            perm = bucketing_permutation(n, seed=d)
            for s in sorted({s for s in (1, 2, 3, 8, 9, n) if s <= n}):
                assert np.array_equal(bits(restated_buckets(g, s, perm)), bits(chained_buckets(g, s, perm))), (n, d, s)


def test_shapes_and_the_short_last_bucket():
    g = heterogeneous(17, 5, 0, seed=2)
    for s, want in ((1, 17), (2, 9), (3, 6), (8, 3), (9, 2), (16, 2), (17, 1)):
        y = restated_buckets(g, s)
        assert y.shape == (want, 5)
        tail = g[(want - 1) * s:]
        assert 1 <= len(tail) <= s and np.array_equal(bits(y[-1]), bits(np.mean(tail, axis=0)))


def test_the_size_weighted_mean_of_the_buckets_is_the_column_mean():
    from attacking_federate_learning_amd.engine import bucketing_permutation
    n, d = 101, 333
    g = heterogeneous(n, d, 0, seed=3)
    want = g.astype(np.float64).mean(axis=0)
    for s in (2, 3, 10, 50):
        y = restated_buckets(g, s, bucketing_permutation(n, seed=s)).astype(np.float64)
        sizes = np.full(y.shape[0], s, dtype=np.float64)
        sizes[-1] = n - s * (y.shape[0] - 1)
        got = (y * sizes[:, None]).sum(axis=0) / n
        # every bucket mean is one fp32 sum of at most s terms and one division: relative error (s + 1) eps/2 of values O(4)
        assert np.max(np.abs(got - want)) <= 4.0 * (s + 1) * np.finfo(np.float32).eps


def test_a_nan_row_touches_its_own_bucket_only():
    from attacking_federate_learning_amd.engine import bucketing_permutation
    n, d, s = 23, 40, 3
    g = heterogeneous(n, d, 0, seed=4)
    perm = bucketing_permutation(n, seed=9)
    nan_row, inf_row = perm[1], perm[2 * s]           # members of buckets 0 and 2
    g[nan_row, :] = np.nan
    g[inf_row, 7] = np.inf
    y = restated_buckets(g, s, perm)
    bad = np.zeros_like(y, dtype=bool)
    bad[0, :] = True
    bad[2, 7] = True
    assert np.array_equal(~np.isfinite(y), bad)
    assert np.isnan(y[0]).all() and y[2, 7] == np.inf


def test_identical_byzantine_rows_spoil_at_most_f_buckets():
    from attacking_federate_learning_amd.engine import bucketing_permutation
    n, d, f, s = 40, 64, 6, 2
    g = heterogeneous(n, d, f, seed=5)
    for seed in range(20):
        perm = bucketing_permutation(n, seed)
        holds_bad = {int(b) for b in np.nonzero(perm < f)[0] // s}
        assert 1 <= len(holds_bad) <= f
        y = restated_buckets(g, s, perm)
        # a bucket without a Byzantine row is a mean of honest rows: nowhere near the planted -7
        clean = np.array([b not in holds_bad for b in range(n // s)])
        assert np.all(y[clean].mean(axis=1) > -3.5) and np.all(y[~clean].mean(axis=1) < -2.0)


def test_bucketing_permutation_is_a_seeded_permutation():
    from attacking_federate_learning_amd.engine import bucketing_permutation
    for n in (1, 2, 9, 1000):
        p = bucketing_permutation(n, seed=3)
        assert p.dtype == np.int32 and p.shape == (n,) and np.array_equal(np.sort(p), np.arange(n))
        assert np.array_equal(p, bucketing_permutation(n, seed=3))
        assert np.array_equal(p, np.random.default_rng(3).permutation(n).astype(np.int32))
    assert np.array_equal(bucketing_permutation(50), bucketing_permutation(50, seed=0))
    assert not np.array_equal(bucketing_permutation(50, seed=0), bucketing_permutation(50, seed=1))


# ---- the surface ------------------------------------------------------------------------------------------------------
def header_prototypes():
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(',') if a.strip() and a.strip() != 'void']
            for m in re.finditer(r'\bint\s+(byz_\w+)\s*\(([^;]*?)\)\s*;', text, flags=re.S)}


def test_the_header_declares_both_entry_points_and_the_binding_matches_their_arity():
    from attacking_federate_learning_amd import _native
    protos = header_prototypes()
    for name in ENTRY_POINTS:
        assert name in protos, name
        assert name in _native._PROTOTYPES, name
        assert len(_native._PROTOTYPES[name]) == len(protos[name]), name
    assert 'byz_bucket_means_sharded_dev' not in protos          # column-local: no sharded entry point
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    assert 'BYZ_K_MISC = 8, BYZ_K_PLANE_SPLIT = 9, BYZ_K_COUNT = 10' in text          # the timing enum did not change
    from attacking_federate_learning_amd import build_native
    assert 'bucketing.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['bucketing.hip']


def test_the_python_layers_carry_the_names_and_signatures():
    from attacking_federate_learning_amd import defences, engine
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator

    def leading(fn, *names):
        params = list(inspect.signature(fn).parameters)
        assert params[:len(names)] == list(names), (fn.__qualname__, params)

    def default(fn, name):
        return inspect.signature(fn).parameters[name].default

    leading(Engine.bucket_means, 'self', 'g', 's', 'perm')
    assert default(Engine.bucket_means, 'perm') is None
    leading(engine.bucketing_permutation, 'n', 'seed')
    assert default(engine.bucketing_permutation, 'seed') == 0
    leading(defences.bucketing, 'users_grads', 'users_count', 'corrupted_count', 's', 'then', 'perm', 'seed')
    assert default(defences.bucketing, 'then') is None and default(defences.bucketing, 's') == 2
    assert default(defences.bucketing, 'perm') is None and default(defences.bucketing, 'seed') == 0
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(defences.bucketing).parameters.values())
    assert defences.bucketing_permutation is engine.bucketing_permutation
    leading(DeviceServer.defend_bucketing, 'self', 'then', 's', 'seed')
    assert default(DeviceServer.defend_bucketing, 's') == 2 and default(DeviceServer.defend_bucketing, 'seed') is None
    leading(HipKernels.bucket_means, 'self', 'g_local', 's', 'perm')
    leading(ShardedAggregator.bucketing, 'self', 'g_local', 'users_count', 'corrupted_count', 's', 'perm', 'seed')
    assert default(ShardedAggregator.bucketing, 's') == 2
    assert 'defend' in defences.bucketing.__doc__ and 's = 2' in defences.bucketing.__doc__
    assert 'same' in ShardedAggregator.bucketing.__doc__.lower()


def test_defend_keeps_its_four_keys():
    from attacking_federate_learning_amd import defences
    assert sorted(defences.defend) == ['Bulyan', 'Krum', 'NoDefense', 'TrimmedMean']
