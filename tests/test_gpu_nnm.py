"""Nearest-neighbour mixing on the GPU against tests/test_nnm.py's numpy restatement.  Every comparison is exact: the lists
are a total order on the engine's own distance bits, and the mix is ONE fp32 accumulator chain in row order, which is numpy's
np.mean(g[list], axis=0).  No tolerance appears anywhere."""
import ctypes

import numpy as np
import pytest

from tests.test_nnm import lists_as_matrix, restated_mix, restated_neighbours, restated_order

pytestmark = pytest.mark.gpu

MAL_PROP = 0.24


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def attacked(n, d, f, seed):
    """Honest rows of different scales, the first f rows one vector (the attack's mean - 1.5 std)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d)).astype(np.float32)
    g *= (1.0 + 0.5 * rng.permutation(n) / n).astype(np.float32)[:, None]
    if f:
        head = g[:f]
        g[:f] = (head.mean(axis=0) - 1.5 * head.std(axis=0)).astype(np.float32)
    return g


_CASES = {}


def case(eng, n, d):
    """(g, f, k, lists, want) for the attacked matrix of this shape, computed once: the lists are the restatement's on the
    engine's own distance matrix, `want` the restated mix.  Shared, and never written to."""
    if (n, d) not in _CASES:
        f = int(n * MAL_PROP)
        g = attacked(n, d, f, seed=n + d)
        dist = eng.pairwise_distances(g)
        lists = restated_neighbours(dist.numpy(), n - f)
        want = restated_mix(g, lists)
        for a in (g, want):
            a.setflags(write=False)
        _CASES[(n, d)] = (g, f, n - f, lists, want)
    return _CASES[(n, d)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- lists --------------------------------------------------------------------------------------------------------------
# (1025 rows are 33 bitmap words: one thread of the take kernel's compaction holds a single word, every later thread none)
@pytest.mark.parametrize('n', [1, 2, 3, 31, 33, 100, 257, 1000, 1025, 4100])
def test_lists_are_the_restatement_on_the_engines_own_distances(eng, n):
    d = 200
    f = int(n * MAL_PROP)
    g = attacked(n, d, f, seed=n)
    dist = eng.pairwise_distances(g)
    host = dist.numpy()
    order = restated_order(host)
    for k in sorted({1, 2, n - f, n - 1, n} & set(range(1, n + 1))):
        nbr, counts = eng.nnm_neighbours(dist, k)
        want_nbr, want_counts = lists_as_matrix(restated_neighbours(host, k, order), k)
        assert np.array_equal(nbr.numpy(), want_nbr), k
        assert np.array_equal(counts.numpy(), want_counts), k
        assert eng.nnm_info() == (0, 0)
    # a dense host matrix goes the same way and comes back as numpy
    nbr, counts = eng.nnm_neighbours(host, n - f)
    want_nbr, want_counts = lists_as_matrix(restated_neighbours(host, n - f, order), n - f)
    assert np.array_equal(nbr, want_nbr) and np.array_equal(counts, want_counts)


def test_exact_ties_at_the_cut_fall_by_row_index(eng):
    """f identical rows: every honest row sees f equal distances; k - 1 cuts through them."""
    n, d, f = 100, 200, 24
    g = attacked(n, d, f, seed=5)
    g[f:] *= np.float32(40.0)                # the identical rows are every honest row's nearest
    dist = eng.pairwise_distances(g)
    host = dist.numpy()
    assert len(np.unique(host[f + 1, :f])) == 1
    k = 11
    nbr, counts = eng.nnm_neighbours(dist, k)
    assert np.array_equal(nbr.numpy(), lists_as_matrix(restated_neighbours(host, k), k)[0])
    assert nbr.numpy()[f + 1].tolist() == list(range(10)) + [f + 1]


# ---- mix ----------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 777), (2, 1), (7, 63), (31, 129), (33, 2051), (100, 5000), (257, 1025), (1000, 2048), (4100, 200)]


@pytest.mark.parametrize('n,d', SHAPES)
def test_mix_is_numpys_mean_of_the_listed_rows(eng, torch, n, d):
    g, f, k, lists, want = case(eng, n, d)
    gt = torch.from_numpy(g).to(torch.device('cuda', eng.device))
    got, nbr = eng.nnm(gt, n, f, return_neighbours=True)
    assert np.array_equal(nbr.cpu().numpy(), lists_as_matrix(lists, k)[0])
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    # the host matrix, and the two steps apart on a Distances handle
    assert np.array_equal(bits(eng.nnm(g, n, f)), bits(want))
    dist = eng.pairwise_distances(gt)
    assert torch.equal(eng.nnm(gt, n, f, distances=dist), got)


def test_strided_view_misaligned_base_and_a_guard_band_round_the_output(eng, torch):
    n, d = 33, 2051
    g, f, k, lists, want = case(eng, n, d)
    device = torch.device('cuda', eng.device)
    nbr, counts = lists_as_matrix(lists, k)
    big = torch.full((n, d + 13), float('nan'), dtype=torch.float32, device=device)
    for first in (0, 5):                     # ld > n_cols on an aligned base; then a base pointer 20 bytes off
        view = big[:, first:first + d]
        view.copy_(torch.from_numpy(g))
        assert view.stride(0) == d + 13 and (view.data_ptr() % 16 == 0) == (first == 0)
        assert np.array_equal(bits(eng.nnm_mix(view, nbr, counts).cpu().numpy()), bits(want))
        assert np.array_equal(bits(eng.nnm_mix(view, nbr).cpu().numpy()), bits(want))      # the lengths read off the -1 tails
    gt = torch.from_numpy(g).to(device)
    guard = torch.full((n + 2, d + 9), 12345.0, dtype=torch.float32, device=device)
    out = guard[1:n + 1, 3:3 + d]
    eng.nnm_mix(gt, torch.from_numpy(nbr).to(device), torch.from_numpy(counts).to(device), out=out)
    eng.synchronize()
    host = guard.cpu().numpy()
    assert np.array_equal(bits(host[1:n + 1, 3:3 + d]), bits(want))
    host[1:n + 1, 3:3 + d] = 12345.0
    assert np.all(host == np.float32(12345.0))


# ---- the chain is one chain ---------------------------------------------------------------------------------------------
def test_k_all_is_no_defense_in_every_row_and_column_panels_are_the_one_call(eng, torch):
    from attacking_federate_learning_amd import defences
    n, d = 1000, 2048
    g, f, k, lists, want = case(eng, n, d)
    device = torch.device('cuda', eng.device)
    gt = torch.from_numpy(g).to(device)
    mean = defences.no_defense(gt, n, 0)
    every = eng.nnm(gt, n, 0)
    assert torch.equal(every, mean[None, :].expand(n, d))
    assert torch.equal(eng.nnm(gt, n, n - 1), gt)            # k = 1
    nbr, counts = lists_as_matrix(lists, k)
    nbr_t, counts_t = torch.from_numpy(nbr).to(device), torch.from_numpy(counts).to(device)
    one = eng.nnm_mix(gt, nbr_t, counts_t)
    panels = torch.full((n, d), float('nan'), dtype=torch.float32, device=device)
    for lo, hi in ((0, 1001), (1001, d)):                    # (the second panel starts 4 bytes off a 16-byte boundary)
        eng.nnm_mix(gt[:, lo:hi], nbr_t, counts_t, out=panels[:, lo:hi])
    assert torch.equal(panels, one)
    assert np.array_equal(bits(one.cpu().numpy()), bits(want))


# ---- non-finite rows ------------------------------------------------------------------------------------------------------
def test_non_finite_rows_come_back_verbatim_and_reach_nobody(eng, torch):
    n, d, f = 100, 300, 24
    g = attacked(n, d, f, seed=9)
    bad = [31, 57, 88]
    g[31, 7] = np.nan
    g[57, 0] = np.inf
    g[88, d - 1] = -np.inf
    gt = torch.from_numpy(g).to(torch.device('cuda', eng.device))
    host = eng.pairwise_distances(gt).numpy()
    good = np.setdiff1d(np.arange(n), bad)
    for k, short in ((n - f, 3), (n, n)):    # n - 1 candidates wanted, 96 finite ones there: the divisor is k_i = 97
        lists = restated_neighbours(host, k)
        assert all(lists[b].tolist() == [b] for b in bad)
        assert all(len(lists[i]) == min(k, n - 3) for i in good)
        got, nbr = eng.nnm(gt, n, n - k, return_neighbours=True)
        assert eng.nnm_info() == (3, short)
        got = got.cpu().numpy()
        assert np.array_equal(nbr.cpu().numpy(), lists_as_matrix(lists, k)[0])
        assert np.array_equal(bits(got[bad]), bits(g[bad]))
        assert np.isfinite(got[good]).all()
        assert np.array_equal(bits(got), bits(restated_mix(g, lists)))


# ---- composition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', [(100, 5000), (1000, 2048)])
@pytest.mark.parametrize('rule', ['coordinate_median', 'trimmed_mean', 'krum', 'geometric_median'])
def test_a_rule_behind_the_mixing_sees_the_restated_matrix(eng, torch, rule, n, d):
    from attacking_federate_learning_amd import defences
    g, f, k, lists, want = case(eng, n, d)
    then = getattr(defences, rule)
    expect = np.asarray(then(np.array(want), n, f))
    got = defences.nnm(g, n, f, then=then)
    assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(expect))
    gt = torch.from_numpy(g).to(torch.device('cuda', eng.device))
    on_device = defences.nnm(gt, n, f, then=then)
    assert on_device.is_cuda and np.array_equal(bits(on_device.cpu().numpy()), bits(expect))
    assert np.array_equal(bits(defences.nnm(g, n, f)), bits(want))


def test_device_server_moves_the_weights_as_defend_would(eng, torch):
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.server import DeviceServer
    n, d = 100, 5000
    g, f, k, lists, want = case(eng, n, d)
    device = torch.device('cuda', eng.device)
    w0 = np.random.default_rng(3).standard_normal(d).astype(np.float32)
    server = DeviceServer(n, w0, MAL_PROP, 0.1, 0.9, torch_device=device, engine=eng)
    server.users_grads.data.copy_(torch.from_numpy(g))
    server.velocity.fill_(0.25)
    agg = server.defend_nnm(defences.trimmed_mean)
    expect = defences.trimmed_mean(np.array(want), n, f)
    assert np.array_equal(bits(agg.cpu().numpy()), bits(expect))
    w = torch.from_numpy(w0).to(device)
    v = torch.full_like(w, 0.25)
    eng.server_update(w, v, torch.from_numpy(expect).to(device), 0.9, 0.1)
    assert torch.equal(server.current_weights, w) and torch.equal(server.velocity, v)
    with pytest.raises(TypeError):
        server.defend_nnm(None)


# ---- sharded ----------------------------------------------------------------------------------------------------------------
def column_bounds(d, world):
    base, extra = divmod(d, world)
    out, start = [], 0
    for r in range(world):
        stop = start + base + (1 if r < extra else 0)
        out.append((start, stop))
        start = stop
    return out


def test_columns_layout_looped_over_three_uneven_shards_equals_one_gpu(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d = 257, 1025
    g, f, k, lists, want = case(eng, n, d)
    device = torch.device('cuda', eng.device)
    gt = torch.from_numpy(g).to(device)
    want_y, want_nbr = eng.nnm(gt, n, f, return_neighbours=True)
    kern = HipKernels(eng)
    slices = []
    for lo, hi in column_bounds(d, 3):
        view = torch.empty((n, -(-(hi - lo) // 4) * 4), dtype=torch.float32, device=device)[:, :hi - lo]
        view.copy_(gt[:, lo:hi])
        slices.append(view)
    gram = None
    for v in slices:
        part = kern.gram(v)
        gram = part if gram is None else gram.add_(part)
    dist = eng.distances_from_gram(gram, n)
    count = eng.near_pairs_count()
    if count:
        sq = None
        for v in slices:
            part = eng.near_pairs_sqdist(v, count)
            sq = part if sq is None else sq.add_(part)
        eng.near_pairs_apply(sq, dist)
    nbr, counts = kern.nnm_neighbours(dist, k)
    assert np.array_equal(nbr.numpy(), want_nbr.cpu().numpy())
    mixed = torch.cat([kern.nnm_mix(v, nbr, counts) for v in slices], dim=1)
    assert torch.equal(mixed, want_y)
    # the aggregator at world size one: the same composition behind one name
    y, lists_dev = ShardedAggregator(kern).nnm(gt, n, f, return_neighbours=True)
    assert torch.equal(y, want_y) and np.array_equal(lists_dev.numpy(), want_nbr.cpu().numpy())


def test_the_sharded_entry_point_with_a_pass_through_all_reduce(eng):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    n, d, f = 100, 777, 24
    k = n - f
    g = attacked(n, d, f, seed=21)
    cb = _native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 0)
    cb_ptr = ctypes.cast(cb, ctypes.c_void_p)
    gd = eng.to_device(g)
    dist = eng.empty((n, n), np.float32)
    _check(eng.lib.byz_pairwise_distances_sharded_dev(eng.ctx, _vp(gd.ptr), n, d, d, cb_ptr, None, _vp(dist.ptr), None))
    eng.check()
    lists = restated_neighbours(dist.numpy(), k)
    y = eng.empty((n, d), np.float32)
    nbr = eng.empty((n, k), np.int32)
    _check(eng.lib.byz_nnm_sharded_dev(eng.ctx, _vp(gd.ptr), n, d, d, n, f, cb_ptr, None, _vp(y.ptr), d, _vp(nbr.ptr), None))
    eng.check()
    assert np.array_equal(nbr.numpy(), lists_as_matrix(lists, k)[0])
    assert np.array_equal(bits(y.numpy()), bits(restated_mix(g, lists)))
    failing = _native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 7)
    rc = eng.lib.byz_nnm_sharded_dev(eng.ctx, _vp(gd.ptr), n, d, d, n, f, ctypes.cast(failing, ctypes.c_void_p), None, _vp(y.ptr), d,
                                     None, None)
    assert rc == _native.E_COLLECTIVE


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_errors(eng):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    n, d = 10, 16
    g = attacked(n, d, 2, seed=1)
    dist = eng.pairwise_distances(g)
    for k in (0, n + 1):
        with pytest.raises(ValueError):
            eng.nnm_neighbours(dist, k)
        with pytest.raises(ValueError):
            eng.nnm(g, n, n - k)
        with pytest.raises(ValueError):
            eng.nnm(eng.to_device(g), n, n - k)
    # 16,385 rows: refused on the argument alone, before any pointer is looked at -- no matrix exists behind these
    some = eng.empty((4,), np.float32)
    big = 16385
    lib, ctx, p = eng.lib, eng.ctx, _vp(some.ptr)
    assert lib.byz_nnm_neighbours_dev(ctx, p, big, big - 1, p, None, None) == _native.E_UNSUPPORTED
    assert lib.byz_nnm_mix_dev(ctx, p, big, 8, 8, p, None, big - 1, p, 8, None) == _native.E_UNSUPPORTED
    assert lib.byz_nnm_dev(ctx, p, big, 8, 8, big, 1, p, 8, None, None) == _native.E_UNSUPPORTED
    assert lib.byz_nnm_host(ctx, p, big, 8, big, 1, p, None) == _native.E_UNSUPPORTED
    # the output must not overlap the matrix, and must be wide enough
    gd = eng.to_device(g)
    nbr, counts = eng.nnm_neighbours(dist, 5)
    assert lib.byz_nnm_mix_dev(ctx, _vp(gd.ptr), n, d, d, _vp(nbr.ptr), _vp(counts.ptr), 5, _vp(gd.ptr), d, None) == _native.E_INVALID
    y = eng.empty((n, d), np.float32)
    assert lib.byz_nnm_mix_dev(ctx, _vp(gd.ptr), n, d, d, _vp(nbr.ptr), _vp(counts.ptr), 5, _vp(y.ptr), d - 1, None) == _native.E_INVALID
