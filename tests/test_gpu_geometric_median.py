"""The geometric median on an MI355X (smoothed Weiszfeld, RFA), held to the numpy restatement of
tests/test_geometric_median.py: the median within rtol 1e-6 (atol 1e-6 max|G|), the objective within 1e-8, the iteration
count wherever no stop ratio of the restatement lies within 1 % of ftol; the weighted mean bit for bit; non-finite rows,
strided views, determinism, the columns layout looped over its shards and through the C ABI's callback."""
import ctypes

import numpy as np
import pytest

from tests.test_geometric_median import attacked, restated_geometric_median, restated_wmean

pytestmark = pytest.mark.gpu

MAX_ITER = 65536          # BYZ_GEOMED_MAX_ITER (include/byzagg.h)


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def close(got, want, g):
    scale = float(np.nanmax(np.abs(g[np.isfinite(g)]))) if np.isfinite(g).any() else 1.0
    return np.allclose(got, want, rtol=1e-6, atol=1e-6 * scale)


def iterations_decided(ratios, ftol):
    return all(abs(r - ftol) > 0.01 * ftol for r in ratios)


def check_against_restatement(got, info, g, ftol=1e-6, **kw):
    want, winfo = restated_geometric_median(g, ftol=ftol, **kw)
    assert close(got, want, g), np.abs(got - want).max()
    assert info['excluded_rows'] == winfo['excluded_rows']
    assert info['objective'] == pytest.approx(winfo['objective'], rel=1e-8, abs=1e-300)
    if iterations_decided(winfo['ratios'], ftol):
        assert info['iterations'] == winfo['iterations'], (info['iterations'], winfo['ratios'])
    return want, winfo


@pytest.mark.parametrize('n,d', [(1, 777), (2, 4096), (23, 2048), (100, 5000), (1000, 2048), (4000, 1024), (10000, 257),
                                 (20000, 64)])
def test_matches_the_restatement(eng, torch, n, d):
    g = attacked(n, d, seed=n + d)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    out, info = eng.geometric_median(gt, return_info=True)
    _, winfo = check_against_restatement(out.cpu().numpy(), info, g)
    w = info['weights'].cpu().numpy()
    assert np.allclose(w, winfo['weights'], rtol=1e-6, atol=1e-12) and w.sum() == pytest.approx(1.0, rel=1e-12)


def test_weighted_mean_is_the_sequential_fp64_loop_bit_for_bit(eng, torch):
    rng = np.random.default_rng(5)
    for n, d in [(37, 3001), (300, 70000), (9, 5)]:
        g = rng.standard_normal((n, d)).astype(np.float32)
        w = rng.random(n) * 3.0
        w[::4] = 0.0
        g[4] = np.inf                                     # a row of infs under a zero weight
        gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
        got = eng.weighted_mean(gt, torch.from_numpy(w).to(gt.device)).cpu().numpy()
        assert np.array_equal(got, restated_wmean(g, w))
        assert np.array_equal(eng.weighted_mean(g, w), restated_wmean(g, w))
    assert np.isnan(eng.weighted_mean(g, np.zeros(len(g)))).all()
    with pytest.raises(ValueError):
        eng.weighted_mean(g, -np.ones(len(g)))


def test_row_sqdist_is_fp64_on_the_difference(eng, torch):
    rng = np.random.default_rng(6)
    g = (1e3 + rng.standard_normal((50, 9000))).astype(np.float32)
    z = (g[7] + np.float32(1e-3)).astype(np.float32)        # near one row: the Gram identity would cancel here
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    got = eng.row_sqdist(gt, torch.from_numpy(z).to(gt.device)).cpu().numpy()
    want = ((g.astype(np.float64) - z.astype(np.float64)) ** 2).sum(axis=1)
    assert np.allclose(got, want, rtol=1e-12)
    assert np.array_equal(got, eng.row_sqdist(gt, torch.from_numpy(z).to(gt.device)).cpu().numpy())


def test_max_iter_zero_is_no_defense(eng, torch):
    g = attacked(300, 5000, seed=3)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    out, info = eng.geometric_median(gt, max_iter=0, return_info=True)
    assert torch.equal(out, eng.no_defense(gt))
    assert info['iterations'] == 0
    assert np.allclose(info['weights'].cpu().numpy(), 1.0 / 300, rtol=1e-15)


def test_ftol_zero_runs_every_iteration(eng, torch):
    g = attacked(64, 3000, seed=4)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    out, info = eng.geometric_median(gt, max_iter=7, ftol=0.0, return_info=True)
    want, winfo = restated_geometric_median(g, max_iter=7, ftol=0.0)
    assert info['iterations'] == 7 == winfo['iterations']
    assert close(out.cpu().numpy(), want, g)
    one = g[:1].copy()
    out1, info1 = eng.geometric_median(one, max_iter=9, ftol=0.0, return_info=True)
    assert info1['iterations'] == 1 and info1['objective'] == 0.0 and np.array_equal(out1, one[0])


def test_non_finite_rows_are_excluded(eng, torch):
    g = attacked(120, 4100, seed=11)
    g[5, 17] = np.nan
    g[40, 17] = np.inf
    g[77, 17] = -np.inf
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    out, info = eng.geometric_median(gt, return_info=True)
    check_against_restatement(out.cpu().numpy(), info, g)
    assert info['excluded_rows'] == 3
    assert info['weights'].cpu().numpy()[[5, 40, 77]].tolist() == [0.0, 0.0, 0.0]
    bad = np.full((6, 300), np.inf, dtype=np.float32)
    bad[::2] = np.nan
    out, info = eng.geometric_median(bad, return_info=True)
    assert np.isnan(out).all() and info['iterations'] == 0 and info['excluded_rows'] == 6


def test_strided_views_and_host_matrices_give_the_same_bits(eng, torch):
    # d % 4 == 0: the dense copy takes the dwordx4 rowsq, the view (ld = d + 5, 4 bytes past an aligned start) the scalar one
    n, d = 500, 3000
    g = attacked(n, d, seed=12)
    dev = torch.device('cuda', eng.device)
    dense = torch.from_numpy(g).to(dev)
    want, winfo = eng.geometric_median(dense, return_info=True)
    view = torch.empty((n, d + 5), dtype=torch.float32, device=dev)[:, 1:d + 1]
    view.copy_(dense)
    got, info = eng.geometric_median(view, return_info=True)
    assert torch.equal(got, want) and info['iterations'] == winfo['iterations']
    assert torch.equal(info['weights'], winfo['weights'])
    host, hinfo = eng.geometric_median(g, return_info=True)
    assert np.array_equal(host, want.cpu().numpy()) and np.array_equal(hinfo['weights'], winfo['weights'].cpu().numpy())


def test_two_calls_are_bitwise_equal(eng, torch):
    g = attacked(2500, 3000, seed=13)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    a, ia = eng.geometric_median(gt, return_info=True)
    b, ib = eng.geometric_median(gt, return_info=True)
    assert torch.equal(a, b) and torch.equal(ia['weights'], ib['weights'])
    assert ia['objective'] == ib['objective'] and ia['iterations'] == ib['iterations']


def test_the_median_resists_a_distant_attack(eng, torch):
    from attacking_federate_learning_amd import defences
    n, d = 400, 2000
    f = int(n * 0.24)
    g = attacked(n, d, seed=14, shift=1e3)
    out = defences.geometric_median(g, n, f, max_iter=50)
    honest = eng.geometric_median(g[f:], max_iter=50)
    spread = float(np.sqrt(((g[f:] - g[f:].mean(axis=0)) ** 2).sum(axis=1)).mean())
    assert np.linalg.norm(out - honest) <= 2.0 * spread
    moved = np.abs(eng.no_defense(g) - g[f:].mean(axis=0)).mean()
    assert moved == pytest.approx(0.24 * 1e3, rel=0.05)


def column_bounds(d):
    """Three uneven column slices."""
    cuts = [0, d // 3 + 1, d // 2 + 7, d]
    return list(zip(cuts[:-1], cuts[1:]))


def test_hip_kernels_over_uneven_column_shards_match_one_gpu(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels
    n, d = 300, 10001
    g = attacked(n, d, seed=15)
    dev = torch.device('cuda', eng.device)
    gt = torch.from_numpy(g).to(dev)
    want, winfo = eng.geometric_median(gt, return_info=True)
    kern = HipKernels(eng)
    slices = [gt[:, lo:hi] for lo, hi in column_bounds(d)]
    z = [kern.no_defense(v) for v in slices]
    F, d_rows, iterations = None, None, 0

    def distances(z):
        sq = sum(kern.row_sqdist(v, zz) for v, zz in zip(slices, z))
        dd = torch.sqrt(sq)
        return dd, float(dd.sum().item())
    d_rows, F = distances(z)
    for k in range(1, 11):
        beta = 1.0 / torch.clamp(d_rows, min=1e-6)
        z = [kern.weighted_mean(v, beta) for v in slices]
        d_rows, f_new = distances(z)
        stop = abs(F - f_new) <= 1e-6 * f_new
        F, iterations = f_new, k
        if stop:
            break
    got = torch.cat(z).cpu().numpy()
    assert close(got, want.cpu().numpy(), g)
    assert iterations == winfo['iterations']
    assert F == pytest.approx(winfo['objective'], rel=1e-8)


def test_sharded_aggregator_at_world_size_one(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    g = attacked(150, 4099, seed=16)
    g[9, 100] = np.nan
    gt = torch.from_numpy(g).to(torch.device('cuda', eng.device))
    want, winfo = eng.geometric_median(gt, return_info=True)
    got, info = ShardedAggregator(HipKernels(eng)).geometric_median(gt, return_info=True)
    assert close(got.cpu().numpy(), want.cpu().numpy(), g)
    assert info['iterations'] == winfo['iterations'] and info['excluded_rows'] == winfo['excluded_rows'] == 1


@pytest.mark.parametrize('nan_rank', [None, 0, 1])
def test_two_ranks_through_the_c_abi(eng, torch, nan_rank):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    from tests.test_gpu_sharded_cabi import Rank, TwoRankAllReduce, run_ranks
    n, d, cut, max_iter = 200, 3000, 1100, 10
    g = attacked(n, d, seed=17)
    if nan_rank is not None:
        g[13, 50 if nan_rank == 0 else 2000] = np.nan
    want, winfo = restated_geometric_median(g)
    ranks = [Rank(g[:, :cut]), Rank(g[:, cut:])]
    try:
        ar = TwoRankAllReduce(ranks)
        cbs = [ar.callback_for(r) for r in range(2)]
        params = _native.GeomedParams(1e-6, max_iter, 1e-6)

        def work(r, rank):
            out = rank.eng.empty((rank.d,), np.float32)
            w = rank.eng.empty((rank.n,), np.float64)
            _check(rank.eng.lib.byz_geometric_median_sharded_dev(rank.eng.ctx, _vp(rank.g.ptr), rank.n, rank.d, rank.d,
                                                                 ctypes.byref(params), ctypes.cast(cbs[r], ctypes.c_void_p),
                                                                 None, _vp(out.ptr), _vp(w.ptr), None))
            it, ex, obj = rank.eng.geometric_median_info()
            return out.numpy(), w.numpy(), it, ex, obj
        res = run_ranks(ranks, work)
        assert ar.calls[0] == ar.calls[1] == [n + 1] + [n] * (max_iter + 1)
        assert np.array_equal(res[0][1], res[1][1]) and res[0][2:] == res[1][2:]
        assert close(np.concatenate([res[0][0], res[1][0]]), want, g)
        assert res[0][3] == winfo['excluded_rows'] == (0 if nan_rank is None else 1)
        assert res[0][4] == pytest.approx(winfo['objective'], rel=1e-8)
        if iterations_decided(winfo['ratios'], 1e-6):
            assert res[0][2] == winfo['iterations']
        cb = ctypes.cast(_native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 5), ctypes.c_void_p)
        out = ranks[0].eng.empty((ranks[0].d,), np.float32)
        rc = ranks[0].eng.lib.byz_geometric_median_sharded_dev(ranks[0].eng.ctx, _vp(ranks[0].g.ptr), n, cut, cut,
                                                               ctypes.byref(params), cb, None, _vp(out.ptr), None, None)
        assert rc == _native.E_COLLECTIVE and 'all-reduce returned 5' in _native.last_error()
        ranks[0].eng.synchronize()
    finally:
        for rank in ranks:
            rank.close()


def test_argument_errors(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    g = attacked(30, 500, seed=18)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    out = eng.empty((500,), np.float32)
    lib, ctx, ptr = eng.lib, eng.ctx, _vp(gt.data_ptr())

    def call(params, n=30, d=500, ld=500):
        return lib.byz_geometric_median_dev(ctx, ptr, n, d, ld, ctypes.byref(params), _vp(out.ptr), None, None)
    P = _native.GeomedParams
    for bad in (P(0.0, 10, 1e-6), P(-1.0, 10, 1e-6), P(float('nan'), 10, 1e-6), P(1e-6, -1, 1e-6), P(1e-6, 10, -1e-6),
                P(1e-6, 10, float('nan'))):
        assert call(bad) == _native.E_INVALID
    ok = P(1e-6, 10, 1e-6)
    assert call(ok, n=0) == _native.E_INVALID
    assert call(ok, ld=499) == _native.E_INVALID
    assert call(ok, n=(1 << 20) + 1, d=1, ld=1) == _native.E_UNSUPPORTED
    assert call(P(1e-6, MAX_ITER + 1, 1e-6)) == _native.E_UNSUPPORTED       # (rejected before anything is enqueued)
    assert lib.byz_geometric_median_dev(ctx, ptr, 30, 500, 500, None, _vp(out.ptr), None, None) == _native.E_INVALID
    assert call(ok) == _native.OK
    eng.check()
    with pytest.raises(ValueError):
        eng.geometric_median(gt, nu=0.0)
    with pytest.raises(ValueError):
        eng.geometric_median(g, max_iter=-1)
    with pytest.raises(NotImplementedError):
        eng.geometric_median(gt, max_iter=MAX_ITER + 1)


# ---- the 4-wide paths: what realistic model sizes run ---------------------------------------------------------------
# launch_weighted_mean takes weighted_rows_kernel<4, false> from 4 * 256 * num_cus * 2 = 524,288 columns on (ld % 4 == 0, 16-byte
# aligned G); rowsq takes dwordx4 loads whenever ld % 4 == 0 and G and z are 16-byte aligned
WIDE = 600_000


def test_weighted_mean_of_wide_rows_is_the_sequential_fp64_loop_bit_for_bit(eng, torch):
    rng = np.random.default_rng(21)
    n = 13                                                # a run of eight rows, then a tail of five
    g = rng.standard_normal((n, WIDE)).astype(np.float32)
    g[4] = np.inf                                         # a row of infs under a zero weight
    w = rng.random(n) * 3.0
    w[[1, 4, 10]] = 0.0
    dev = torch.device('cuda', eng.device)
    wt = torch.from_numpy(w).to(dev)
    gt = torch.from_numpy(g).to(dev)
    assert gt.data_ptr() % 16 == 0
    assert np.array_equal(eng.weighted_mean(gt, wt).cpu().numpy(), restated_wmean(g, w))
    # ld % 4 == 0 but n_cols % 4 != 0: the masked tail of the 4-wide kernel
    view = gt[:, :WIDE - 1]
    assert view.stride(0) == WIDE
    assert np.array_equal(eng.weighted_mean(view, wt).cpu().numpy(), restated_wmean(g[:, :WIDE - 1], w))
    # and a width that is not a multiple of 256 * 4 either
    narrow = gt[:, :WIDE - 1027]
    assert np.array_equal(eng.weighted_mean(narrow, wt).cpu().numpy(), restated_wmean(g[:, :WIDE - 1027], w))


@pytest.mark.parametrize('cols', [WIDE, WIDE - 3])
def test_wide_rows_match_the_restatement(eng, torch, cols):
    n = 24
    g = attacked(n, WIDE, seed=22)
    dev = torch.device('cuda', eng.device)
    gt = torch.from_numpy(g).to(dev)[:, :cols]              # ld = WIDE: the 4-wide paths, masked at the end for WIDE - 3
    out, info = eng.geometric_median(gt, return_info=True)
    check_against_restatement(out.cpu().numpy(), info, np.ascontiguousarray(g[:, :cols]))
    # the scalar-load paths (ld odd, 4 bytes past an aligned start) give the same bits
    odd = torch.empty((n, cols + 5), dtype=torch.float32, device=dev)[:, 1:cols + 1]
    odd.copy_(gt)
    out_odd, info_odd = eng.geometric_median(odd, return_info=True)
    assert torch.equal(out_odd, out) and info_odd['iterations'] == info['iterations']
    assert torch.equal(info_odd['weights'], info['weights'])
