"""Multi-Krum on an MI355X (Blanchard et al. 2017, section 4): every row scored the Krum way, the m best
in ranking order, their mean in ascending row order.

The contract (include/byzagg.h) is checked against its numpy restatement (tests/test_multi_krum.py) on the engine's own
distance matrix: the selection exactly, the aggregate bit for bit against np.mean(G[np.sort(selection)], axis=0).  The
inputs carry the attack's f identical rows (malicious.py:26-27), ties through rows 0 and 1, NaN and huge scores, more rows
than the LDS-resident selection kernels hold, and the two multi-GPU layouts looped over their shards on one GPU."""
import ctypes

import numpy as np
import pytest

from tests.test_multi_krum import restated_ranking, restated_scores, visit_positions

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


def engine_scores(eng, dist, users_count, corrupted_count):
    """scores_dev of byz_krum_select_dev on a Distances handle (and Krum's index)."""
    from attacking_federate_learning_amd.engine import _check, _vp
    buf = eng.empty((dist.n,), np.float32)
    idx = ctypes.c_int32(-2)
    _check(eng.lib.byz_krum_select_dev(eng.ctx, _vp(dist.ptr), dist.n, int(users_count), int(corrupted_count),
                                       ctypes.byref(idx), _vp(buf.ptr), None))
    return buf.numpy(), int(idx.value)


def np_mean_rows(g, rows):
    return np.mean(g[np.sort(np.asarray(rows))], axis=0)


@pytest.mark.parametrize('n,d', [(10, 3000), (100, 5000), (1000, 2048), (4000, 1024)])
def test_default_m_is_the_restated_selection_and_numpys_mean(eng, torch, n, d):
    f = int(n * MAL_PROP)
    g = attacked(n, d, f, seed=n)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    out, sel = eng.multi_krum(gt, n, f, return_selection=True)
    sel = sel.cpu().numpy()
    dist = eng.pairwise_distances(gt).numpy()
    scores = restated_scores(dist, n, f)
    want = restated_ranking(scores, n - f)
    assert sel.tolist() == want.tolist()
    assert np.array_equal(out.cpu().numpy(), np_mean_rows(g, sel))
    # the engine's scores are the restatement's bits, so the ranking is a ranking of the same numbers
    handle = eng.pairwise_distances(gt)
    got_scores, _ = engine_scores(eng, handle, n, f)
    assert np.array_equal(got_scores, scores)


@pytest.mark.parametrize('n,d', [(23, 2048), (300, 4000), (2500, 1500)])
def test_m_one_is_krum_and_m_all_is_no_defense(eng, torch, n, d):
    from attacking_federate_learning_amd import defences
    f = int(n * MAL_PROP)
    g = attacked(n, d, f, seed=100 + n)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    idx = defences.krum(g, n, f, return_index=True)
    assert idx >= 0
    out1, sel1 = eng.multi_krum(gt, n, f, m=1, return_selection=True)
    assert sel1.cpu().numpy().tolist() == [idx]
    assert np.array_equal(out1.cpu().numpy(), g[idx])
    out_n, sel_n = eng.multi_krum(gt, n, f, m=n, return_selection=True)
    assert sorted(sel_n.cpu().numpy().tolist()) == list(range(n))
    assert np.array_equal(out_n.cpu().numpy(), defences.no_defense(g, n, f))
    assert np.array_equal(out_n.cpu().numpy(), np.mean(g, axis=0))


def test_a_single_row(eng):
    g = attacked(1, 777, 0, seed=1)
    out, sel = eng.multi_krum(g, 1, 0, return_selection=True)
    assert sel.tolist() == [0]
    assert np.array_equal(out, g[0])


@pytest.mark.parametrize('m', [1, 2, 3, 4, 6])
def test_m_cuts_through_a_tie_class_with_rows_zero_and_one(eng, m):
    from attacking_federate_learning_amd import defences
    n, d, f = 50, 1000, 5
    g = attacked(n, d, 0, seed=7)
    for r in (1, 4, 7):
        g[r] = g[0]                                    # one tie class: rows 0, 1, 4, 7 score exactly alike
    dist = defences._krum_create_distances(g)
    scores, _ = engine_scores(eng, dist, n, f)
    assert scores[0] == scores[1] == scores[4] == scores[7]
    sel = defences.multi_krum(g, n, f, m=m, return_index=True)
    want = restated_ranking(restated_scores(dist.numpy(), n, f), m)
    assert sel.tolist() == want.tolist()
    assert sel.tolist()[:min(m, 4)] == [1, 0, 4, 7][:min(m, 4)]      # by visit position: 1, 0, 2, 3, ...
    out = defences.multi_krum(g, n, f, m=m)
    assert np.array_equal(out, np_mean_rows(g, sel))


def test_nan_inf_and_huge_scores_rank_by_the_engines_own_scores(eng):
    """A distance matrix whose row 5 is NaN, row 9 +inf and row 12 1e19 (a score of 3.4e20 >= 1e20): the engine's own
    scores_dev ranked by np.lexsort is the selection for every m; on a gradient matrix with a NaN entry the whole call."""
    from attacking_federate_learning_amd.engine import Distances
    n, d, f = 40, 256, 6
    g = attacked(n, d, 0, seed=11)
    dense = eng.pairwise_distances(g).numpy()
    dense[12, :] = dense[:, 12] = 1e19
    dense[9, :] = dense[:, 9] = np.inf
    dense[5, :] = dense[:, 5] = np.nan
    np.fill_diagonal(dense, np.inf)
    handle = Distances(eng.to_device(dense), n)
    scores, krum_idx = engine_scores(eng, handle, n, f)
    assert np.isnan(scores[5]) and np.isposinf(scores[9]) and scores[12] >= 1e20 and np.isfinite(scores[12])
    nan = np.isnan(scores)
    want = np.lexsort((visit_positions(n), np.where(nan, 0.0, scores), nan))
    for m in (1, 7, n - f, n):
        assert eng.multi_krum_select(handle, n, f, m=m).tolist() == want[:m].tolist(), m
        assert eng.multi_krum_select(dense, n, f, m=m).tolist() == want[:m].tolist(), m
    assert want[0] == krum_idx
    # every NaN after every number, +inf and >= 1e20 by value
    assert want[-1] == 5 and want[-2] == 9 and want[-3] == 12
    g[5, 3] = np.nan
    g[12] = 1e19
    out, sel = eng.multi_krum(g, n, f, m=n, return_selection=True)
    assert sel[-1] == 5
    assert np.array_equal(out, np.mean(g, axis=0), equal_nan=True)


def test_beyond_the_lds_resident_selection(eng, torch):
    """16,400 rows: the row sort in global memory (large_rows.hip).  The C oracle's faithful scores are the reference's fp32
    sums (cast to double); checked against scores_dev first, then ranked."""
    from oracle import scale
    n, d = 16400, 512
    f = int(n * MAL_PROP)
    g = attacked(n, d, f, seed=16400)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    handle = eng.pairwise_distances(gt)
    dist = handle.numpy()
    idx, _, ref_scores = scale.krum_pick(dist, n, f, with_scores=True)
    got_scores, krum_idx = engine_scores(eng, handle, n, f)
    assert np.array_equal(ref_scores.astype(np.float32), got_scores)
    assert np.array_equal(ref_scores.astype(np.float32).astype(np.float64), ref_scores)
    assert krum_idx == idx
    want = restated_ranking(got_scores, n - f)
    sel = eng.multi_krum_select(handle, n, f)
    assert sel.tolist() == want.tolist()
    out, sel2 = eng.multi_krum(gt, n, f, return_selection=True)
    assert sel2.cpu().numpy().tolist() == want.tolist()
    assert np.array_equal(out.cpu().numpy(), np_mean_rows(g, want))


def test_one_row_more_than_the_compaction_has_threads(eng, torch):
    """1025 rows: the first size at which a thread of the take kernel's compaction (1024 threads) owns two rows, so that
    thread 512 owns one and every later thread none.  The selection against the restated ranking of the engine's own scores,
    the ascending list through the aggregate it is walked for, numpy's mean of the sorted selection bit for bit."""
    n, d = 1025, 64
    f = int(n * MAL_PROP)
    g = attacked(n, d, f, seed=1025)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    handle = eng.pairwise_distances(gt)
    scores, krum_idx = engine_scores(eng, handle, n, f)
    assert np.array_equal(scores, restated_scores(handle.numpy(), n, f))
    for m in (1, 513, 1025):
        want = restated_ranking(scores, m)
        assert eng.multi_krum_select(handle, n, f, m=m).tolist() == want.tolist(), m
        out, sel = eng.multi_krum(gt, n, f, m=m, return_selection=True)
        assert sel.cpu().numpy().tolist() == want.tolist(), m
        assert np.array_equal(out.cpu().numpy(), np_mean_rows(g, want)), m
    assert restated_ranking(scores, 1).tolist() == [krum_idx]


def test_distances_handle_strided_view_host_matrix_and_return_index(eng, torch):
    from attacking_federate_learning_amd import defences
    n, d, f = 200, 3001, 40
    g = attacked(n, d, f, seed=3)
    device = 'cuda:%d' % eng.device
    gt = torch.from_numpy(g).to(device)
    want_out, want_sel = eng.multi_krum(gt, n, f, return_selection=True)
    want_out, want_sel = want_out.cpu().numpy(), want_sel.cpu().numpy()
    assert np.array_equal(want_out, np_mean_rows(g, want_sel))
    # host numpy: the drop-in path
    out_h, sel_h = eng.multi_krum(g, n, f, return_selection=True)
    assert np.array_equal(out_h, want_out) and np.array_equal(sel_h, want_sel)
    assert np.array_equal(defences.multi_krum(g, n, f), want_out)
    assert np.array_equal(defences.multi_krum(g, n, f, return_index=True), want_sel)
    # a strided view (ld > n_cols)
    buf = torch.zeros((n, d + 5), dtype=torch.float32, device=device)
    view = buf[:, 1:d + 1]
    view.copy_(gt)
    out_v, sel_v = eng.multi_krum(view, n, f, return_selection=True)
    assert np.array_equal(out_v.cpu().numpy(), want_out) and np.array_equal(sel_v.cpu().numpy(), want_sel)
    # a Distances handle, on a host matrix and on a device one
    handle = defences._krum_create_distances(g)
    assert np.array_equal(defences.multi_krum(g, n, f, distances=handle), want_out)
    assert np.array_equal(defences.multi_krum(g, n, f, distances=handle, return_index=True), want_sel)
    out_d, sel_d = eng.multi_krum(gt, n, f, distances=handle, return_selection=True)
    assert np.array_equal(out_d.cpu().numpy(), want_out) and np.array_equal(sel_d.cpu().numpy(), want_sel)
    # the reference's dict form with a row removed: keys in dict order, the selection in the dict's row names
    small = g[:12]
    dd = defences._krum_create_distances(small).to_dict()
    del dd[3]
    for row in dd.values():
        row.pop(3)
    sel_dict = defences.multi_krum(small, 12, 2, m=4, distances=dd, return_index=True)
    assert 3 not in sel_dict.tolist() and len(sel_dict) == 4
    # the row-list mean alone, in list order, on its own
    rows = np.asarray([7, 3, 150, 3], dtype=np.int32)
    got = eng.mean_rows(gt, rows).cpu().numpy()
    want = np.float32(0.0) + g[7] + g[3] + g[150] + g[3]
    assert np.array_equal(got, want / np.float32(4))


def column_bounds(d, world):
    base, extra = divmod(d, world)
    out, start = [], 0
    for r in range(world):
        stop = start + base + (1 if r < extra else 0)
        out.append((start, stop))
        start = stop
    return out


def ceil4(x):
    return -(-x // 4) * 4


@pytest.mark.parametrize('world', [2, 3])
def test_columns_layout_looped_over_uneven_shards_equals_one_gpu(eng, torch, world):
    from attacking_federate_learning_amd.sharded import HipKernels
    n, d = 300, 10001
    f = int(n * MAL_PROP)
    g = attacked(n, d, f, seed=300 + world)
    g[f + 3] = g[f + 7] + np.float32(1e-4) * np.random.default_rng(1).standard_normal(d).astype(np.float32)
    device = torch.device('cuda', eng.device)
    gt = torch.from_numpy(g).to(device)
    want_out, want_sel = eng.multi_krum(gt, n, f, return_selection=True)
    kern = HipKernels(eng)
    slices = []
    for lo, hi in column_bounds(d, world):
        view = torch.empty((n, ceil4(hi - lo)), dtype=torch.float32, device=device)[:, :hi - lo]
        view.copy_(gt[:, lo:hi])
        slices.append(view)
    gram = None
    for v in slices:
        part = kern.gram(v)
        gram = part if gram is None else gram.add_(part)
    dist = eng.distances_from_gram(gram, n)
    count = eng.near_pairs_count()
    assert count >= 1
    sq = None
    for v in slices:
        part = eng.near_pairs_sqdist(v, count)
        sq = part if sq is None else sq.add_(part)
    eng.near_pairs_apply(sq, dist)
    sel = kern.multi_krum_select(dist, n, f)
    assert sel.tolist() == want_sel.cpu().numpy().tolist()
    out = torch.cat([kern.mean_rows(v, np.sort(sel)) for v in slices])
    assert torch.equal(out, want_out)


def test_clients_layout_looped_over_uneven_shards_equals_one_gpu(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels
    n, d, world = 520, 6000, 3
    f = int(n * MAL_PROP)
    g = attacked(n, d, f, seed=520)
    device = torch.device('cuda', eng.device)
    gt = torch.from_numpy(g).to(device)
    want_out, want_sel = eng.multi_krum(gt, n, f, return_selection=True)
    kern = HipKernels(eng)
    rows_per = [n // world + (1 if r < n % world else 0) for r in range(world)]
    rows_per[0] += 5
    rows_per[-1] -= 5
    n_max = max(rows_per)
    starts = np.concatenate([[0], np.cumsum(rows_per)])
    row_index = torch.from_numpy(np.concatenate(
        [r * n_max + np.arange(rows_per[r]) for r in range(world)]).astype(np.int32)).to(device)
    panel = torch.full((world * n_max, d), float('nan'), dtype=torch.float32, device=device)
    for r in range(world):
        panel[r * n_max:r * n_max + rows_per[r]] = gt[int(starts[r]):int(starts[r + 1])]
    gram = None
    for share in range(world):
        part = kern.gram_share(panel, row_index, world, share)
        gram = part if gram is None else gram.add_(part)
    eng.check()
    dist = eng.distances_from_gram(gram, n)
    count = eng.near_pairs_count()
    if count:
        eng.near_pairs_apply(eng.near_pairs_sqdist(panel, count, row_index=row_index), dist)
    sel = kern.multi_krum_select(dist, n, f)
    assert sel.tolist() == want_sel.cpu().numpy().tolist()
    rows = np.sort(sel)
    picked = gt[torch.from_numpy(rows.astype(np.int64)).to(device)]     # owner order of ascending rows = ascending
    outs = []
    for lo, hi in column_bounds(d, world):
        view = torch.empty((len(rows), ceil4(hi - lo)), dtype=torch.float32, device=device)[:, :hi - lo]
        view.copy_(picked[:, lo:hi])
        outs.append(kern.mean_rows(view, np.arange(len(rows), dtype=np.int32)))
    assert torch.equal(torch.cat(outs), want_out)


def test_sharded_aggregator_at_world_size_one(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d = 120, 4099
    f = int(n * MAL_PROP)
    g = attacked(n, d, f, seed=120)
    gt = torch.from_numpy(g).to(torch.device('cuda', eng.device))
    want_out, want_sel = eng.multi_krum(gt, n, f, m=50, return_selection=True)
    agg = ShardedAggregator(HipKernels(eng))
    out, sel = agg.multi_krum(gt, n, f, m=50, return_selection=True)
    assert sel.tolist() == want_sel.cpu().numpy().tolist() and torch.equal(out, want_out)
    out_c, sel_c = agg.multi_krum_clients(gt, [n], n, f, m=50, return_selection=True)
    assert sel_c.tolist() == want_sel.cpu().numpy().tolist() and torch.equal(out_c, want_out)


def test_two_ranks_through_the_c_abi(eng):
    """byz_multi_krum_sharded_dev on two contexts with a summing callback (tests/test_gpu_sharded_cabi.py's pattern): the
    restated selection on the sharded distances on both ranks, each rank's columns of numpy's mean of those rows."""
    from attacking_federate_learning_amd.engine import _check, _vp
    from tests.test_gpu_sharded_cabi import Rank, TwoRankAllReduce, attacked_matrix, distances_sharded, run_ranks
    n, d, f, cut, m = 200, 3000, 40, 1100, 150
    g = attacked_matrix(n, d, f, seed=77)
    ranks = [Rank(g[:, :cut]), Rank(g[:, cut:])]
    try:
        ar0 = TwoRankAllReduce(ranks)
        cbs0 = [ar0.callback_for(r) for r in range(2)]
        dists = run_ranks(ranks, lambda r, rank: distances_sharded(rank, cbs0[r]))
        want_sel = restated_ranking(restated_scores(dists[0], n, f), m)
        ar = TwoRankAllReduce(ranks)
        cbs = [ar.callback_for(r) for r in range(2)]

        def work(r, rank):
            out = rank.eng.empty((rank.d,), np.float32)
            sel = rank.eng.empty((m,), np.int32)
            _check(rank.eng.lib.byz_multi_krum_sharded_dev(rank.eng.ctx, _vp(rank.g.ptr), rank.n, rank.d, rank.d, n, f, m, 1,
                                                           ctypes.cast(cbs[r], ctypes.c_void_p), None, _vp(out.ptr),
                                                           _vp(sel.ptr), None))
            rank.eng.check()
            return out.numpy(), sel.numpy()
        res = run_ranks(ranks, work)
        assert ar.calls[0] == ar.calls[1] and ar.calls[0][0] == n * n
        for r in range(2):
            assert res[r][1].tolist() == want_sel.tolist()
        assert np.array_equal(np.concatenate([res[0][0], res[1][0]]), np_mean_rows(g, want_sel))
    finally:
        for rank in ranks:
            rank.close()


def test_errors(eng, torch):
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import _check, _vp
    n, d, f = 30, 500, 5
    g = attacked(n, d, f, seed=30)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    for m in (0, -1, n + 1):
        with pytest.raises(ValueError):
            eng.multi_krum(gt, n, f, m=m)
        with pytest.raises(ValueError):
            eng.multi_krum(g, n, f, m=m)
        with pytest.raises(ValueError):
            defences.multi_krum(g, n, f, m=m, return_index=True)
    with pytest.raises(AssertionError):
        defences.multi_krum(g, 10, 5)
    with pytest.raises(AssertionError):
        eng.multi_krum(gt, 10, 5)
    out = eng.empty((d,), np.float32)
    with pytest.raises(AssertionError):
        _check(eng.lib.byz_multi_krum_dev(eng.ctx, _vp(gt.data_ptr()), n, d, d, 10, 5, 3, 1, _vp(out.ptr), None, None))
    # without check_assert the same call goes through (krum(..., return_index=True) does not assert either)
    _check(eng.lib.byz_multi_krum_dev(eng.ctx, _vp(gt.data_ptr()), n, d, d, 10, 5, 3, 0, _vp(out.ptr), None, None))
    eng.check()
    assert len(defences.multi_krum(g, 10, 5, return_index=True)) == 5
