"""Nearest-neighbour mixing (Allouah et al., "Fixing by Mixing", AISTATS 2023): the numpy restatement of include/byzagg.h's
contract, its properties, and the surface every layer has to carry.  No GPU here; tests/test_gpu_nnm.py holds the kernels to the
restatement bit for bit."""
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ('byz_nnm_neighbours_dev', 'byz_nnm_mix_dev', 'byz_nnm_dev', 'byz_nnm_info', 'byz_nnm_host',
                'byz_nnm_sharded_dev')


# ---- the restatement ------------------------------------------------------------------------------------------------
def ordered_bits(d):
    """fp32 values -> uint32 whose unsigned order is the contract's: by value, -0.0 as +0.0, every NaN behind +inf."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    bits = d.view(np.uint32).copy()
    bits[bits == np.uint32(0x80000000)] = 0
    negative = (bits & np.uint32(0x80000000)) != 0
    out = np.where(negative, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    out[np.isnan(d)] = np.uint32(0xffffffff)
    return out


def restated_order(dist):
    """Row i: the other rows j ascending by (ordered distance bits, j) -- an (n, n - 1) array."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    n = dist.shape[0]
    keys = (ordered_bits(dist).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
    keys[np.arange(n), np.arange(n)] = np.uint64(0xffffffffffffffff)       # the diagonal is no candidate
    return np.argsort(keys, axis=1, kind='stable')[:, :n - 1]


def restated_neighbours(dist, k, order=None):
    """list_i: the first k - 1 candidates of row i in key order, those at a non-finite distance dropped, i added, ascending."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    n = dist.shape[0]
    assert 1 <= k <= n
    if order is None:
        order = restated_order(dist)
    lists = []
    for i in range(n):
        taken = order[i, :k - 1]
        taken = taken[np.isfinite(dist[i, taken])]
        lists.append(np.sort(np.append(taken, i)).astype(np.int64))
    return lists


def lists_as_matrix(lists, k):
    """(n x k int32 with -1 behind every list, n int32 lengths): the form byz_nnm_neighbours_dev writes."""
    nbr = np.full((len(lists), k), -1, dtype=np.int32)
    for i, rows in enumerate(lists):
        nbr[i, :len(rows)] = rows
    return nbr, np.asarray([len(rows) for rows in lists], dtype=np.int32)


def restated_mix(g, lists):
    """Y[i] = np.mean(g[list_i], axis=0); the row itself where the list is {i}."""
    out = np.empty_like(g)
    for i, rows in enumerate(lists):
        out[i] = g[i] if len(rows) == 1 else np.mean(g[rows], axis=0)
    return out


def numpy_distances(g):
    """Unsquared L2 distances with a +inf diagonal (what byz_pairwise_distances_dev writes, up to rounding)."""
    with np.errstate(invalid='ignore', over='ignore'):
        g64 = g.astype(np.float64)
        sq = (g64 * g64).sum(axis=1)
        d2 = sq[:, None] + sq[None, :] - 2.0 * (g64 @ g64.T)
        dist = np.sqrt(np.maximum(d2, 0.0)).astype(np.float32)
        dist[np.isnan(d2)] = np.nan
    np.fill_diagonal(dist, np.inf)
    return dist


def attacked(n, d, f, seed):
    """Honest rows of different scales, the first f rows one vector (the attack's mean - 1.5 std)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d)).astype(np.float32)
    g *= (1.0 + 0.5 * rng.permutation(n) / n).astype(np.float32)[:, None]
    if f:
        head = g[:f]
        g[:f] = (head.mean(axis=0) - 1.5 * head.std(axis=0)).astype(np.float32)
    return g


# ---- properties of the restatement ------------------------------------------------------------------------------------
def test_k_all_is_the_column_mean_and_k_one_is_the_matrix():
    g = attacked(37, 211, 8, seed=1)
    dist = numpy_distances(g)
    every = restated_mix(g, restated_neighbours(dist, 37))
    assert np.array_equal(every, np.broadcast_to(np.mean(g, axis=0), g.shape))
    assert np.array_equal(restated_mix(g, restated_neighbours(dist, 1)), g)


def test_lists_are_ascending_contain_their_row_and_have_k_entries():
    g = attacked(50, 64, 12, seed=2)
    dist = numpy_distances(g)
    for k in (1, 2, 38, 49, 50):
        lists = restated_neighbours(dist, k)
        for i, rows in enumerate(lists):
            assert i in rows and len(rows) == k
            assert np.all(np.diff(rows) > 0)
        nbr, counts = lists_as_matrix(lists, k)
        assert nbr.shape == (50, k) and np.all(counts == k) and np.all(nbr >= 0)


def test_ties_among_identical_rows_follow_the_key_order():
    """Rows 0..4 are one vector: every other row sees five equal distances, and a cut inside them takes the lowest indices;
    -0.0 ties with +0.0 and a NaN sorts behind +inf."""
    n = 9
    dist = np.full((n, n), 5.0, dtype=np.float32)
    dist[:5, :5] = 0.0
    dist[5:, :5] = 1.0                       # the identical rows are everybody's nearest
    dist[:5, 5:] = 1.0
    np.fill_diagonal(dist, np.inf)
    lists = restated_neighbours(dist, 4)     # 3 candidates out of 5 tied ones
    assert lists[7].tolist() == [0, 1, 2, 7]
    assert lists[2].tolist() == [0, 1, 2, 3]           # row 2's candidates at distance 0 are 0, 1, 3, 4
    dist[6, 3] = -0.0                        # below 1.0, and equal to +0.0: row 3 first, then the rows at 1.0 by index
    dist[6, 0] = np.nan
    assert restated_neighbours(dist, 4)[6].tolist() == [1, 2, 3, 6]
    order = restated_order(dist)
    assert order[6, -1] == 0                 # the NaN behind the +inf-free rest
    dist[6, 8] = np.inf
    assert restated_order(dist)[6, -2:].tolist() == [8, 0]


def test_a_row_with_a_nan_or_an_inf_is_solo_and_in_nobodys_list():
    g = attacked(30, 40, 7, seed=3)
    g[11, 5] = np.nan
    g[17, 0] = np.inf
    g[23, 39] = -np.inf
    dist = numpy_distances(g)
    for k in (23, 30):
        lists = restated_neighbours(dist, k)
        for bad in (11, 17, 23):
            assert lists[bad].tolist() == [bad]
        for i, rows in enumerate(lists):
            if i not in (11, 17, 23):
                assert not set(rows.tolist()) & {11, 17, 23}
                assert len(rows) == min(k, 27)
        mixed = restated_mix(g, lists)
        assert np.array_equal(mixed[[11, 17, 23]].view(np.uint32), g[[11, 17, 23]].view(np.uint32))
        assert np.isfinite(np.delete(mixed, [11, 17, 23], axis=0)).all()


def test_mixing_reduces_the_honest_rows_spread():
    rng = np.random.default_rng(4)
    n, d, f = 60, 500, 14
    centre = rng.standard_normal(d).astype(np.float32)
    g = (centre + rng.standard_normal((n, d))).astype(np.float32)
    g[:f] = (centre - 8.0).astype(np.float32)          # the attacked rows, far away and identical
    mixed = restated_mix(g, restated_neighbours(numpy_distances(g), n - f))
    honest = slice(f, n)
    spread = lambda m: float(np.mean(np.linalg.norm(m[honest] - m[honest].mean(axis=0), axis=1)))    # noqa: E731
    assert spread(mixed) < 0.25 * spread(g)
    # an honest row's n - f nearest rows are the honest rows: nothing of the attack reaches it
    assert np.allclose(mixed[honest], g[honest].mean(axis=0), atol=1e-5)


# ---- the surface ------------------------------------------------------------------------------------------------------
def header_prototypes():
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(',') if a.strip() and a.strip() != 'void']
            for m in re.finditer(r'\bint\s+(byz_\w+)\s*\(([^;]*?)\)\s*;', text, flags=re.S)}


def test_the_header_declares_every_entry_point_and_the_binding_matches_its_arity():
    from attacking_federate_learning_amd import _native
    protos = header_prototypes()
    for name in ENTRY_POINTS:
        assert name in protos, name
        assert name in _native._PROTOTYPES, name
        assert len(_native._PROTOTYPES[name]) == len(protos[name]), name
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    assert 'BYZ_K_MISC = 8, BYZ_K_PLANE_SPLIT = 9, BYZ_K_COUNT = 10' in text          # the timing enum did not change


def test_the_python_layers_carry_the_names_and_signatures():
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator

    def leading(fn, *names):
        params = list(inspect.signature(fn).parameters)
        assert params[:len(names)] == list(names), (fn.__qualname__, params)

    leading(Engine.nnm_neighbours, 'self', 'distances', 'k')
    leading(Engine.nnm_mix, 'self', 'g', 'neighbours', 'counts')
    leading(Engine.nnm, 'self', 'g', 'users_count', 'corrupted_count', 'distances', 'return_neighbours')
    leading(Engine.nnm_info, 'self')
    leading(defences.nnm, 'users_grads', 'users_count', 'corrupted_count', 'then', 'distances')
    assert inspect.signature(defences.nnm).parameters['then'].default is None
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(defences.nnm).parameters.values())
    leading(DeviceServer.defend_nnm, 'self', 'then')
    leading(HipKernels.nnm_neighbours, 'self', 'dist', 'k')
    leading(HipKernels.nnm_mix, 'self', 'g_local', 'neighbours')
    leading(ShardedAggregator.nnm, 'self', 'g_local', 'users_count', 'corrupted_count')
    assert 'defend' in defences.nnm.__doc__


def test_defend_keeps_its_four_keys():
    from attacking_federate_learning_amd import defences
    assert sorted(defences.defend) == ['Bulyan', 'Krum', 'NoDefense', 'TrimmedMean']
