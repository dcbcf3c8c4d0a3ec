"""DnC on an MI355X, held to the numpy restatement of tests/test_dnc.py -- never to the code under test:
the scores within 1e-9 of the restatement's largest finite score, the selection equal to the restatement's wherever its gap at
the cut exceeds 1e-6 of that score in every iteration (asserted for every input here, not skipped), the aggregate the bits of
np.mean(G[good], axis=0); non-finite rows, strided views, host input, determinism, several iterations, sub_dim >= D, the
columns layout over 2-4 shards (one with no sampled column) and through the C ABI's callback, and the argument checks."""
import ctypes

import numpy as np
import pytest

from tests.test_dnc import ATTACKED_SHAPES, gap_at_cut, restated_dnc, restated_scores, sampled
from tests.test_geometric_median import attacked

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-9          # of the restatement's largest finite score
GAP_NEEDED = 1e-6         # the restatement's gap at the cut, same unit, for the selection to be compared


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def top_score(s):
    finite = s[np.isfinite(s)]
    return float(finite.max()) if finite.size and finite.max() > 0 else 1.0


def scores_close(got, want):
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf)
    worst = float(np.abs(got[~inf] - want[~inf]).max()) / top_score(want) if (~inf).any() else 0.0
    print('dnc scores: largest discrepancy %.3e of the top score (n = %d)' % (worst, len(want)))
    assert worst <= SCORE_TOL, worst
    return worst


def check_whole_call(eng, torch, g, f, lists, power_iters=32):
    """scores, selection and aggregate of one input against the restatement; returns the device results."""
    lists = np.asarray(lists, dtype=np.int64)
    lists = lists.reshape(1, -1) if lists.ndim == 1 else lists
    want_out, want_good, want_scores = restated_dnc(g, f, lists, power_iters)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    for cols, ws in zip(lists, want_scores):
        scores_close(eng.dnc_scores(gt, cols, power_iters=power_iters).cpu().numpy(), ws)
        assert gap_at_cut(ws, f) > GAP_NEEDED, gap_at_cut(ws, f)
    out, good = eng.dnc(gt, f, lists, power_iters=power_iters, return_selection=True)
    assert good.cpu().numpy().tolist() == want_good.tolist()
    assert np.array_equal(eng.dnc_select(gt, f, lists, power_iters=power_iters).cpu().numpy(), want_good)
    assert np.array_equal(out.cpu().numpy(), want_out, equal_nan=True)
    assert eng.dnc_info()[0] == len(want_good)
    return out, good


@pytest.mark.parametrize('n,d,b,seed', ATTACKED_SHAPES)
def test_attacked_matrices_match_the_restatement(eng, torch, n, d, b, seed):
    g = attacked(n, d, seed, mal_prop=0.24)
    f = int(n * 0.24)
    out, good = check_whole_call(eng, torch, g, f, sampled(d, b, seed + 100))
    assert good.cpu().numpy().tolist() == list(range(f, n))
    assert np.array_equal(out.cpu().numpy(), np.mean(g[f:], axis=0))


def test_pure_noise_matches_the_restatement(eng, torch):
    g = np.random.default_rng(4).standard_normal((100, 5000)).astype(np.float32)
    cols = sampled(5000, 1000, 104)
    for power_iters in (16, 32):
        check_whole_call(eng, torch, g, 24, cols, power_iters=power_iters)


@pytest.mark.parametrize('n,d,b', [(1, 77, 30), (2, 300, 100), (23, 2048, 500), (4000, 600, 256), (10000, 257, 128),
                                   (20000, 64, 48)])
def test_row_counts_from_one_to_twenty_thousand(eng, torch, n, d, b):
    g = attacked(n, d, seed=n + d, mal_prop=0.24)
    f = int(n * 0.24)
    check_whole_call(eng, torch, g, f, sampled(d, b, n))


def test_one_row_more_than_the_compaction_has_threads(eng, torch):
    """1025 rows: the first size at which a thread of the compaction (1024 threads) owns two rows, so that thread 512 owns
    one and every later thread none.  The whole call against the restatement, then the list as the kernel leaves it: the
    kept rows ascending, -1 behind the count."""
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    n, d, b, remove_count = 1025, 96, 32, 300
    g = attacked(n, d, seed=n + d, mal_prop=0.24)
    cols = sampled(d, b, n)
    want_good = restated_dnc(g, remove_count, cols)[1]
    assert len(want_good) == 725
    check_whole_call(eng, torch, g, remove_count, cols)
    assert eng.dnc_info()[0] == 725
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    cols_dev = eng.to_device(np.asarray(cols, dtype=np.int64))
    good = eng.empty((n,), np.int32)
    params = _native.DncParams(1, b, 32, remove_count)
    _check(eng.lib.byz_dnc_select_dev(eng.ctx, _vp(gt.data_ptr()), n, d, d, ctypes.byref(params), _vp(cols_dev.ptr), _vp(good.ptr),
                                      None, None))
    assert eng.dnc_info()[0] == 725
    good = good.numpy()
    assert good[:725].tolist() == want_good.tolist() and (np.diff(good[:725]) > 0).all()
    assert (good[725:] == -1).all()


def test_remove_count_zero_is_no_defense(eng, torch):
    g = attacked(300, 5000, seed=3)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    out, good = eng.dnc(gt, 0, sampled(5000, 400, 5), return_selection=True)
    assert torch.equal(out, eng.no_defense(gt)) and good.cpu().numpy().tolist() == list(range(300))
    assert np.array_equal(out.cpu().numpy(), np.mean(g, axis=0))


def test_power_iters_zero_and_an_all_equal_matrix(eng, torch):
    g = attacked(60, 700, seed=7)
    cols = sampled(700, 200, 8)
    want, _ = restated_scores(g, cols, power_iters=0)
    scores_close(eng.dnc_scores(g, cols, power_iters=0), want)
    flat = np.full((9, 40), 2.5, dtype=np.float32)
    assert np.array_equal(eng.dnc_scores(flat, np.arange(40)), np.zeros(9))
    out, good = eng.dnc(flat, 3, np.arange(40), return_selection=True)
    assert good.tolist() == [0, 1, 2, 3, 4, 5] and np.array_equal(out, flat[0])


def test_non_finite_rows(eng, torch):
    g = attacked(120, 4100, seed=11)
    f = 28
    cols = sampled(4100, 900, 12)
    other = np.setdiff1d(np.arange(4100), cols)
    g[5, cols[17]] = np.nan
    g[40, cols[3]] = np.inf
    g[77, cols[800]] = -np.inf
    g[90, other[10]] = np.nan                      # not sampled: row 90 stays active and reaches the mean
    want_out, want_good, (ws,) = restated_dnc(g, f + 2, cols)
    assert 90 in want_good.tolist() and not {5, 40, 77} & set(want_good.tolist())
    out, good = check_whole_call(eng, torch, g, f + 2, cols)
    assert eng.dnc_info() == (120 - f - 2, 3)
    assert np.isnan(out.cpu().numpy()[other[10]])
    # fewer removed than are inactive: the lowest-indexed inactive rows stay, as the ranking says
    out, good = eng.dnc(g, 2, cols, return_selection=True)
    want_out, want_good, _ = restated_dnc(g, 2, cols)
    assert good.tolist() == want_good.tolist() and 5 in good.tolist()
    assert np.array_equal(out, want_out, equal_nan=True)
    # no active row
    bad = np.full((6, 300), np.inf, dtype=np.float32)
    assert np.isinf(eng.dnc_scores(bad, np.arange(300))).all()
    out, good = eng.dnc(bad, 2, np.arange(300), return_selection=True)
    assert good.tolist() == [0, 1, 2, 3] and eng.dnc_info() == (4, 6)


def test_strided_views_and_host_matrices_give_the_same_bits(eng, torch):
    n, d = 500, 3000
    g = attacked(n, d, seed=12)
    f = 120
    lists = np.stack([sampled(d, 700, 13), sampled(d, 700, 14)])
    dev = torch.device('cuda', eng.device)
    dense = torch.from_numpy(g).to(dev)
    want, wgood = eng.dnc(dense, f, lists, return_selection=True)
    ws = eng.dnc_scores(dense, lists[0])
    view = torch.empty((n, d + 5), dtype=torch.float32, device=dev)[:, 1:d + 1]
    view.copy_(dense)
    assert view.stride(0) == d + 5
    got, good = eng.dnc(view, f, lists, return_selection=True)
    assert torch.equal(got, want) and torch.equal(good, wgood)
    assert torch.equal(eng.dnc_scores(view, lists[0]), ws)
    host, hgood = eng.dnc(g, f, lists, return_selection=True)
    assert np.array_equal(host, want.cpu().numpy()) and np.array_equal(hgood, wgood.cpu().numpy())
    assert np.array_equal(eng.dnc_scores(g, lists[0]), ws.cpu().numpy())
    # the column lists on the device, and the drop-in function on the same samples
    from attacking_federate_learning_amd import defences
    lt = torch.from_numpy(lists).to(dev)
    assert torch.equal(eng.dnc(dense, f, lt), want)
    assert np.array_equal(defences.dnc(g, n, f, columns=lists), host)
    assert np.array_equal(defences.dnc(g, n, f, columns=lists, return_index=True), hgood)
    drawn = defences.dnc(g, n, f, niters=2, sub_dim=700, seed=9)
    assert np.array_equal(drawn, restated_dnc(g, f, defences.dnc_columns(d, 700, 2, 9))[0])
    with pytest.raises(ValueError):
        eng.dnc(dense, f, [3, 2, 5])
    with pytest.raises(ValueError):
        eng.dnc(g, f, [0, d])


def test_two_calls_are_bitwise_equal(eng, torch):
    g = attacked(2500, 3000, seed=13)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    lists = np.stack([sampled(3000, 1000, 20 + t) for t in range(2)])
    a, ga = eng.dnc(gt, 600, lists, return_selection=True)
    sa = eng.dnc_scores(gt, lists[1])
    b, gb = eng.dnc(gt, 600, lists, return_selection=True)
    assert torch.equal(a, b) and torch.equal(ga, gb) and torch.equal(sa, eng.dnc_scores(gt, lists[1]))


def test_three_iterations_intersect(eng, torch):
    g = attacked(200, 6000, seed=21)
    f = 48
    lists = np.stack([sampled(6000, 800, 30 + t) for t in range(3)])
    check_whole_call(eng, torch, g, f, lists)
    noise = np.random.default_rng(22).standard_normal((60, 2000)).astype(np.float32)
    lists = np.stack([sampled(2000, 300, 40 + t) for t in range(3)])
    out, good = check_whole_call(eng, torch, noise, 10, lists)
    assert len(good) < 50                          # the iterations disagree on noise: a real intersection


def test_an_empty_intersection_is_nan_with_a_count_of_zero(eng, torch):
    g = np.zeros((3, 4), dtype=np.float32)
    g[:, 0] = [0.0, 5.0, -5.1]
    g[:, 2] = [7.0, 0.1, -7.0]
    lists = [[0, 1], [2, 3]]
    assert restated_dnc(g, 2, lists)[1].size == 0
    out, good = eng.dnc(torch.from_numpy(g).to('cuda:%d' % eng.device), 2, lists, return_selection=True)
    assert good.numel() == 0 and torch.isnan(out).all() and eng.dnc_info()[0] == 0
    out, good = eng.dnc(g, 2, lists, return_selection=True)
    assert good.size == 0 and np.isnan(out).all()


def test_sub_dim_at_least_the_width_takes_every_column(eng, torch):
    from attacking_federate_learning_amd import defences
    g = attacked(80, 900, seed=23)
    f = 19
    assert np.array_equal(defences.dnc_columns(900, 10000, 1, 0), np.arange(900)[None])
    check_whole_call(eng, torch, g, f, np.arange(900))
    assert np.array_equal(defences.dnc(g, 80, f), restated_dnc(g, f, np.arange(900))[0])


# ---- the columns layout ---------------------------------------------------------------------------------------------
def run_sharded(g, cuts, lists, f, power_iters=32):
    """One rank (its own context, its own thread) per column slice; the all-reduce sums the ranks' buffers on the host."""
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    from tests.test_gpu_sharded_cabi import Rank, TwoRankAllReduce, run_ranks
    bounds = list(zip(cuts[:-1], cuts[1:]))
    ranks = [Rank(np.ascontiguousarray(g[:, lo:hi])) for lo, hi in bounds]
    try:
        ar = TwoRankAllReduce(ranks)
        cbs = [ar.callback_for(r) for r in range(len(ranks))]
        params = _native.DncParams(len(lists), lists.shape[1], power_iters, f)

        def work(r, rank):
            lo, hi = bounds[r]
            local = [row[(row >= lo) & (row < hi)] - lo for row in lists]
            counts = (ctypes.c_int64 * len(local))(*[len(c) for c in local])
            flat = np.concatenate(local).astype(np.int64)
            cols = rank.eng.to_device(flat) if flat.size else None
            out = rank.eng.empty((rank.d,), np.float32)
            good = rank.eng.empty((rank.n,), np.int32)
            _check(rank.eng.lib.byz_dnc_sharded_dev(rank.eng.ctx, _vp(rank.g.ptr), rank.n, rank.d, rank.d, ctypes.byref(params),
                                                    _vp(cols.ptr) if cols is not None else None, counts,
                                                    ctypes.cast(cbs[r], ctypes.c_void_p), None, _vp(out.ptr), _vp(good.ptr), None))
            kept, _ = rank.eng.dnc_info()
            return out.numpy(), good.numpy()[:kept], [len(c) for c in local]
        return run_ranks(ranks, work), ar.calls
    finally:
        for rank in ranks:
            rank.close()


@pytest.mark.parametrize('shards', [2, 3, 4])
def test_column_shards_give_the_same_selection_and_the_concatenated_aggregate(eng, torch, shards):
    n, d, f, power_iters = 200, 3000, 48, 32
    g = attacked(n, d, seed=17 + shards)
    # the last shard owns columns that no iteration samples
    lists = np.stack([sampled(d - 400, 500, 50 + t) for t in range(2)])
    cuts = {2: [0, 2600, d], 3: [0, 1001, 2600, d], 4: [0, 700, 1400, 2600, d]}[shards]
    want_out, want_good, want_scores = restated_dnc(g, f, lists, power_iters)
    assert all(gap_at_cut(s, f) > GAP_NEEDED for s in want_scores)
    res, calls = run_sharded(g, cuts, lists, f, power_iters)
    assert res[-1][2] == [0, 0]                                   # a shard with no sampled column
    assert all(c == calls[0] for c in calls) and calls[0] == [n] * (2 * (power_iters + 3))
    for out, good, _ in res:
        assert good.tolist() == want_good.tolist()
    assert np.array_equal(np.concatenate([r[0] for r in res]), want_out)
    one_gpu = eng.dnc(torch.from_numpy(g).to('cuda:%d' % eng.device), f, lists)
    assert np.array_equal(one_gpu.cpu().numpy(), want_out)


def test_one_rank_through_the_c_abi_callback_and_the_aggregator(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _DeviceF64, _vp
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d, f = 150, 4099, 36
    g = attacked(n, d, seed=16)
    g[9, 100] = np.nan
    rest = np.setdiff1d(np.arange(d), [100])                   # column 100 (the NaN's) in both samples, 600 columns each
    lists = np.stack([np.union1d(rest[sampled(d - 1, 599, 60 + t)], [100]) for t in range(2)])
    assert lists.shape == (2, 600)
    want_out, want_good, _ = restated_dnc(g, f, lists)
    assert 9 not in want_good.tolist()
    gt = torch.from_numpy(g).to(torch.device('cuda', eng.device))
    calls = []

    def reduce(t):
        assert t.dtype == torch.float64 and t.is_cuda
        calls.append(int(t.numel()))
    out, good = HipKernels(eng).dnc(gt, f, list(lists), lists.shape[1], all_reduce=reduce, return_selection=True)
    assert calls == [n] * (2 * 35)
    assert good.cpu().numpy().tolist() == want_good.tolist() and np.array_equal(out.cpu().numpy(), want_out, equal_nan=True)
    agg = ShardedAggregator(HipKernels(eng))
    got = agg.dnc(gt, n, f, columns=lists)
    assert np.array_equal(got.cpu().numpy(), want_out, equal_nan=True)
    assert agg.dnc(gt, n, f, columns=lists, return_index=True).cpu().numpy().tolist() == want_good.tolist()
    # the view torch gets of the library's buffer in the callback
    probe = torch.arange(7, dtype=torch.float64, device=gt.device)
    seen = torch.as_tensor(_DeviceF64(probe.data_ptr(), 7), device=gt.device)
    assert seen.data_ptr() == probe.data_ptr() and torch.equal(seen, probe)
    # a failing all-reduce
    cb = ctypes.cast(_native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 5), ctypes.c_void_p)
    params = _native.DncParams(1, 600, 4, f)
    cols = eng.to_device(lists[0])
    counts = (ctypes.c_int64 * 1)(600)
    out = eng.empty((d,), np.float32)
    rc = eng.lib.byz_dnc_sharded_dev(eng.ctx, _vp(gt.data_ptr()), n, d, d, ctypes.byref(params), _vp(cols.ptr), counts, cb, None,
                                     _vp(out.ptr), None, None)
    assert rc == _native.E_COLLECTIVE and 'all-reduce returned 5' in _native.last_error()
    eng.synchronize()


def test_argument_errors(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    g = attacked(30, 500, seed=18)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    out = eng.empty((500,), np.float32)
    cols = eng.to_device(np.arange(0, 400, 2, dtype=np.int64))
    lib, ctx, ptr = eng.lib, eng.ctx, _vp(gt.data_ptr())
    P = _native.DncParams

    def call(params, n=30, d=500, ld=500, columns=cols.ptr):
        return lib.byz_dnc_dev(ctx, ptr, n, d, ld, ctypes.byref(params), _vp(columns), _vp(out.ptr), None, None)
    for bad in (P(0, 200, 32, 5), P(1, 0, 32, 5), P(1, 501, 32, 5), P(1, 200, -1, 5), P(1, 200, 32, -1), P(1, 200, 32, 30)):
        assert call(bad) == _native.E_INVALID
    ok = P(1, 200, 32, 5)
    assert call(ok, n=0) == _native.E_INVALID
    assert call(ok, ld=499) == _native.E_INVALID
    assert call(ok, columns=None) == _native.E_INVALID
    assert lib.byz_dnc_dev(ctx, ptr, 30, 500, 500, None, _vp(cols.ptr), _vp(out.ptr), None, None) == _native.E_INVALID
    assert call(P(1, 1, 32, 5), n=(1 << 20) + 1, d=1, ld=1) == _native.E_UNSUPPORTED
    assert call(P(1, 1025, 32, 5), n=1 << 18, d=2000, ld=2000) == _native.E_UNSUPPORTED      # 2^18 * 1025 > 2^28 sampled values
    assert call(P(2, 200, 32768, 5)) == _native.E_UNSUPPORTED                               # 2 * 32769 products
    assert lib.byz_dnc_scores_dev(ctx, ptr, 30, 500, 500, _vp(cols.ptr), 200, 32, None, None) == _native.E_INVALID
    assert lib.byz_dnc_select_dev(ctx, ptr, 30, 500, 500, ctypes.byref(ok), _vp(cols.ptr), None, None, None) == _native.E_INVALID
    host_cols = np.arange(0, 400, 2, dtype=np.int64)
    host_cols[7] = host_cols[6]                                       # not strictly ascending: the host entry checks
    res = np.empty(500, dtype=np.float32)
    rc = lib.byz_dnc_host(ctx, g.ctypes.data_as(ctypes.c_void_p), 30, 500, ctypes.byref(ok), host_cols.ctypes.data_as(ctypes.c_void_p),
                          res.ctypes.data_as(ctypes.c_void_p), None, None)
    assert rc == _native.E_INVALID
    assert call(ok) == _native.OK
    eng.check()
    with pytest.raises(ValueError):
        eng.dnc(gt, 30, np.arange(10))
    with pytest.raises(NotImplementedError):
        eng.dnc(gt, 5, np.arange(10), power_iters=1 << 17)
