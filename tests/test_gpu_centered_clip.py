"""Centered clipping on an MI355X, held to the numpy restatement of tests/test_centered_clip.py: the
vector within rtol 1e-6 (atol 1e-6 max|G|, the geometric median's tolerance), the scales within rtol 1e-12, the clipped and
excluded counts exactly (the inputs keep every row's distance at least 1e-9 tau away from tau in every iteration: asserted).
The shapes cross every kernel boundary: one row, fewer rows than a run of eight scales and a tail behind the runs, one and
several chunks of rowsq, widths that are no multiple of a window or of four, the four-wide update from 524,288 columns."""
import ctypes

import numpy as np
import pytest

from tests.test_centered_clip import median_tau, restated_centered_clip, restated_clip_update
from tests.test_geometric_median import attacked

pytestmark = pytest.mark.gpu

MAX_ITER = 65536          # BYZ_CCLIP_MAX_ITER (include/byzagg.h)


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def close(got, want, g):
    scale = float(np.nanmax(np.abs(g[np.isfinite(g)]))) if np.isfinite(g).any() else 1.0
    return np.allclose(got, want, rtol=1e-6, atol=1e-6 * scale)


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:%d' % eng.device)


def check_against_restatement(out, info, g, **kw):
    want, winfo = restated_centered_clip(g, **kw)
    gaps = winfo['gaps']
    print('gaps', gaps, 'clipped', winfo['clipped_rows'], 'excluded', winfo['excluded_rows'])
    assert all(gap > 1e-9 for gap in gaps), gaps            # a precondition of the inputs, not of the kernels
    out = out.cpu().numpy() if hasattr(out, 'cpu') else out
    scales = info['scales'].cpu().numpy() if hasattr(info['scales'], 'cpu') else info['scales']
    print('max |out - want|', float(np.nanmax(np.abs(out - want))) if out.size else 0.0)
    assert close(out, want, g), np.abs(out - want).max()
    assert np.allclose(scales, winfo['scales'], rtol=1e-12, atol=0.0)
    assert info['clipped_rows'] == winfo['clipped_rows'] and info['excluded_rows'] == winfo['excluded_rows']
    return want, winfo


@pytest.mark.parametrize('n,d', [(1, 777), (2, 4096), (23, 2051), (100, 5000), (1000, 2048), (2000, 600), (4000, 1024),
                                 (4096, 200), (4097, 300), (20000, 64)])
def test_matches_the_restatement(eng, torch, n, d):
    g = attacked(n, d, seed=n + d)
    tau = median_tau(g)
    out, info = eng.centered_clip(on_gpu(torch, eng, g), tau=tau, iters=3, return_info=True)
    _, winfo = check_against_restatement(out, info, g, tau=tau, iters=3)
    if n >= 2:
        assert 0 < winfo['clipped_history'][0] < n            # both branches of the scale are taken: in iteration 0 everywhere
    if n >= 23:
        assert 0 < winfo['clipped_rows'] < n                  # and in the last one too (two rows end up both inside tau)


def test_a_given_start_the_next_round_and_an_aliased_output(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    n, d = 300, 5000
    g = attacked(n, d, seed=31)
    gt = on_gpu(torch, eng, g)
    tau = 0.5 * median_tau(g)
    start = (g[n - 1] + np.float32(1e-2)).astype(np.float32)            # near one honest row
    out, info = eng.centered_clip(gt, tau=tau, iters=3, start=on_gpu(torch, eng, start), return_info=True)
    check_against_restatement(out, info, g, tau=tau, iters=3, start=start)
    host, hinfo = eng.centered_clip(gt, tau=tau, iters=3, start=start, return_info=True)      # a host start, uploaded
    assert torch.equal(host, out) and torch.equal(hinfo['scales'], info['scales'])
    # round two of a server: the previous output is the start
    g2 = attacked(n, d, seed=32)
    out2, info2 = eng.centered_clip(on_gpu(torch, eng, g2), tau=tau, iters=3, start=out, return_info=True)
    check_against_restatement(out2, info2, g2, tau=tau, iters=3, start=out.cpu().numpy())
    # out aliasing start, through the C ABI
    buf = out.clone()
    params = _native.CclipParams(tau, 3)
    _check(eng.lib.byz_centered_clip_dev(eng.ctx, _vp(gt.data_ptr()), n, d, d, ctypes.byref(params), _vp(buf.data_ptr()),
                                         _vp(buf.data_ptr()), None, None))
    eng.synchronize()
    want, _ = eng.centered_clip(gt, tau=tau, iters=3, start=out, return_info=True)
    assert torch.equal(buf, want)


def test_infinite_tau_is_the_mean_and_no_iteration_returns_the_start(eng, torch):
    g = attacked(300, 5000, seed=33)
    gt = on_gpu(torch, eng, g)
    out, info = eng.centered_clip(gt, tau=float('inf'), iters=1, return_info=True)
    assert close(out.cpu().numpy(), eng.no_defense(gt).cpu().numpy(), g)
    assert info['clipped_rows'] == 0 and info['excluded_rows'] == 0
    assert torch.equal(info['scales'], torch.ones_like(info['scales']))
    start = on_gpu(torch, eng, np.random.default_rng(33).standard_normal(5000).astype(np.float32))
    out, info = eng.centered_clip(gt, iters=0, start=start, return_info=True)
    assert torch.equal(out, start) and out.data_ptr() != start.data_ptr()
    assert info['clipped_rows'] == 0 and info['excluded_rows'] == 0
    assert torch.equal(eng.centered_clip(gt, iters=0), torch.zeros_like(start))
    assert np.array_equal(eng.centered_clip(g, iters=0, start=start.cpu().numpy()), start.cpu().numpy())


def test_a_small_tau_clips_every_row(eng, torch):
    g = attacked(150, 3000, seed=34)
    out, info = eng.centered_clip(on_gpu(torch, eng, g), tau=1e-3, iters=3, return_info=True)
    check_against_restatement(out, info, g, tau=1e-3, iters=3)
    assert info['clipped_rows'] == 150
    assert np.linalg.norm(out.cpu().numpy().astype(np.float64)) <= 3e-3 * (1 + 1e-6)


@pytest.mark.parametrize('n', [120, 4200])
def test_non_finite_rows_are_excluded(eng, torch, n):
    g = attacked(n, 1100, seed=35)
    tau = median_tau(g)
    g[5, 17] = np.nan
    g[40, 17] = np.inf
    g[77, 17] = -np.inf
    out, info = eng.centered_clip(on_gpu(torch, eng, g), tau=tau, iters=3, return_info=True)
    check_against_restatement(out, info, g, tau=tau, iters=3)
    assert info['excluded_rows'] == 3 and torch.isfinite(out).all()
    assert info['scales'].cpu().numpy()[[5, 40, 77]].tolist() == [0.0, 0.0, 0.0]


def test_nothing_but_non_finite_rows_returns_the_start(eng, torch):
    bad = np.full((6, 300), np.inf, dtype=np.float32)
    bad[::2] = np.nan
    start = np.random.default_rng(36).standard_normal(300).astype(np.float32)
    for matrix in (bad, on_gpu(torch, eng, bad)):
        out, info = eng.centered_clip(matrix, start=start, return_info=True)
        out = out.cpu().numpy() if hasattr(out, 'cpu') else out
        assert np.array_equal(out, start) and info['excluded_rows'] == 6 and info['clipped_rows'] == 0


@pytest.mark.parametrize('n,d', [(500, 3000), (4500, 260)])
def test_the_call_is_the_composition_of_its_pieces(eng, torch, n, d):
    # row_sqdist, the scales, clip_update, three times
    g = attacked(n, d, seed=37)
    gt = on_gpu(torch, eng, g)
    tau = median_tau(g)
    out, info = eng.centered_clip(gt, tau=tau, iters=3, return_info=True)
    v = torch.zeros(d, dtype=torch.float32, device=gt.device)
    for _ in range(3):
        dist = torch.sqrt(eng.row_sqdist(gt, v))
        scales = torch.where(dist > tau, tau / dist, torch.ones_like(dist))
        v = eng.clip_update(gt, v, scales)
    assert close(out.cpu().numpy(), v.cpu().numpy(), g)
    assert np.allclose(info['scales'].cpu().numpy(), scales.cpu().numpy(), rtol=1e-12, atol=0.0)


@pytest.mark.parametrize('n,d', [(500, 3000), (3000, 520), (4500, 260)])
def test_two_calls_strided_views_and_host_matrices_give_the_same_bits(eng, torch, n, d):
    # d % 4 == 0: the dense copy takes dwordx4 loads, the view (ld = d + 5, 4 bytes past an aligned start) scalar ones
    g = attacked(n, d, seed=38)
    tau = median_tau(g)
    dense = on_gpu(torch, eng, g)
    want, winfo = eng.centered_clip(dense, tau=tau, return_info=True)
    again, ainfo = eng.centered_clip(dense, tau=tau, return_info=True)
    assert torch.equal(again, want) and torch.equal(ainfo['scales'], winfo['scales'])
    view = torch.empty((n, d + 5), dtype=torch.float32, device=dense.device)[:, 1:d + 1]
    view.copy_(dense)
    got, info = eng.centered_clip(view, tau=tau, return_info=True)
    assert torch.equal(got, want) and torch.equal(info['scales'], winfo['scales'])
    assert (info['clipped_rows'], info['excluded_rows']) == (winfo['clipped_rows'], winfo['excluded_rows'])
    host, hinfo = eng.centered_clip(g, tau=tau, return_info=True)
    assert np.array_equal(host, want.cpu().numpy()) and np.array_equal(hinfo['scales'], winfo['scales'].cpu().numpy())


def test_clip_update_alone(eng, torch):
    rng = np.random.default_rng(39)
    # (7, 129): no whole run of eight rows, the tail loop alone; (16, 1): whole runs, no tail, one column
    for n, d in [(37, 3001), (300, 70000), (9, 5), (7, 129), (16, 1)]:
        g = rng.standard_normal((n, d)).astype(np.float32)
        v = rng.standard_normal(d).astype(np.float32)
        s = rng.random(n)
        s[::4] = 0.0
        g[4] = np.inf                                     # a row of infs under a zero scale
        want = restated_clip_update(g, v, s)
        gt = on_gpu(torch, eng, g)
        got = eng.clip_update(gt, on_gpu(torch, eng, v), on_gpu(torch, eng, s)).cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got, want)     # the restatement is the kernel's arithmetic: bits
        assert np.array_equal(eng.clip_update(g, v, s), want)


def test_wide_rows_take_the_four_wide_update(eng, torch):
    # launch_clip_update takes weighted_rows_kernel<4, true> from 4 * 256 * num_cus * 2 = 524,288 columns on (ld % 4 == 0,
    # aligned G): the weighted mean's template and launch rule
    n, wide = 13, 600_000
    rng = np.random.default_rng(40)
    g = rng.standard_normal((n, wide)).astype(np.float32)
    g[4] = np.inf
    v = rng.standard_normal(wide).astype(np.float32)
    s = rng.random(n)
    s[[1, 4, 10]] = 0.0
    gt, vt, st = on_gpu(torch, eng, g), on_gpu(torch, eng, v), on_gpu(torch, eng, s)
    for cols in (wide, wide - 1, wide - 1027):                       # whole, a masked tail, no multiple of 1024
        got = eng.clip_update(gt[:, :cols], vt[:cols].contiguous(), st).cpu().numpy()
        assert np.array_equal(got, restated_clip_update(g[:, :cols], v[:cols], s))
    odd = torch.empty((n, wide + 5), dtype=torch.float32, device=gt.device)[:, 1:wide + 1]
    odd.copy_(gt)
    assert torch.equal(eng.clip_update(odd, vt, st), eng.clip_update(gt, vt, st))      # the scalar kernel: the same bits


def test_argument_errors(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    g = attacked(30, 500, seed=41)
    gt = on_gpu(torch, eng, g)
    out = eng.empty((500,), np.float32)
    lib, ctx, ptr = eng.lib, eng.ctx, _vp(gt.data_ptr())

    def call(params, n=30, d=500, ld=500, out_ptr=None):
        return lib.byz_centered_clip_dev(ctx, ptr, n, d, ld, ctypes.byref(params), None, out_ptr or _vp(out.ptr), None, None)
    P = _native.CclipParams
    for bad in (P(0.0, 3), P(-1.0, 3), P(float('nan'), 3), P(10.0, -1)):
        assert call(bad) == _native.E_INVALID
    ok = P(10.0, 3)
    assert call(ok, n=0) == _native.E_INVALID
    assert call(ok, ld=499) == _native.E_INVALID
    assert call(ok, out_ptr=_vp(gt.data_ptr() + 4000)) == _native.E_INVALID           # the output inside the matrix
    assert call(ok, n=(1 << 20) + 1, d=1, ld=1) == _native.E_UNSUPPORTED
    assert call(P(10.0, MAX_ITER + 1)) == _native.E_UNSUPPORTED          # (rejected before anything is enqueued)
    assert lib.byz_centered_clip_dev(ctx, ptr, 30, 500, 500, None, None, _vp(out.ptr), None, None) == _native.E_INVALID
    assert call(P(float('inf'), 3)) == _native.OK and call(ok) == _native.OK
    eng.check()
    for kw in (dict(tau=0.0), dict(tau=-2.0), dict(tau=float('nan')), dict(iters=-1)):
        with pytest.raises(ValueError):
            eng.centered_clip(gt, **kw)
        with pytest.raises(ValueError):
            eng.centered_clip(g, **kw)
    with pytest.raises(NotImplementedError):
        eng.centered_clip(gt, iters=MAX_ITER + 1)


def test_the_defences_entry_clips_a_distant_attack(eng, torch):
    from attacking_federate_learning_amd import defences
    n, d = 400, 2000
    f = int(n * 0.24)
    g = attacked(n, d, seed=42, shift=1e3)
    tau = median_tau(g[f:])
    out = defences.centered_clip(g, n, f, tau=tau, iters=3)
    assert np.array_equal(out, eng.centered_clip(g, tau=tau, iters=3))
    honest = g[f:].astype(np.float64).mean(axis=0)
    assert np.linalg.norm(out - honest) <= 3 * tau
    assert np.linalg.norm(eng.no_defense(g) - honest) >= 0.2 * 1e3 * np.sqrt(d)


# ---- the columns layout -----------------------------------------------------------------------------------------------
def test_sharded_aggregator_over_uneven_column_shards_matches_one_gpu(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator

    class LoopedKernels(HipKernels):
        """Every shard on this GPU: row_sqdist sums the shards' parts, as the all-reduce over the ranks would."""

        def __init__(self, engine, bounds):
            super().__init__(engine)
            self.bounds = bounds

        def row_sqdist(self, g, z):
            return sum(self.engine.row_sqdist(g[:, lo:hi], z[lo:hi].contiguous()) for lo, hi in self.bounds)

        def clip_update(self, g, v, scales):
            return torch.cat([self.engine.clip_update(g[:, lo:hi], v[lo:hi].contiguous(), scales) for lo, hi in self.bounds])

    n, d = 300, 5000
    g = attacked(n, d, seed=43)
    g[9, 100] = np.nan
    gt = on_gpu(torch, eng, g)
    tau = median_tau(attacked(n, d, seed=43))
    start = on_gpu(torch, eng, np.random.default_rng(43).standard_normal(d).astype(np.float32) * np.float32(0.1))
    want, winfo = eng.centered_clip(gt, tau=tau, start=start, return_info=True)
    for cuts in ([0, d], [0, d // 3 + 1, d], [0, d // 3 + 1, d // 2 + 7, d]):
        kern = LoopedKernels(eng, list(zip(cuts[:-1], cuts[1:])))
        got, info = ShardedAggregator(kern).centered_clip(gt, tau=tau, start=start, return_info=True)
        assert close(got.cpu().numpy(), want.cpu().numpy(), g)
        assert np.allclose(info['scales'].cpu().numpy(), winfo['scales'].cpu().numpy(), rtol=1e-12, atol=0.0)
        assert info['clipped_rows'] == winfo['clipped_rows'] and info['excluded_rows'] == winfo['excluded_rows'] == 1


@pytest.mark.parametrize('iters', [0, 3])
def test_two_ranks_through_the_c_abi(eng, torch, iters):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    from tests.test_gpu_sharded_cabi import Rank, TwoRankAllReduce, run_ranks
    n, d, cut = 200, 3000, 1100
    g = attacked(n, d, seed=44)
    tau = median_tau(g)
    start = np.random.default_rng(44).standard_normal(d).astype(np.float32) * np.float32(0.1)
    want, winfo = restated_centered_clip(g, tau=tau, iters=iters, start=start)
    ranks = [Rank(g[:, :cut]), Rank(g[:, cut:])]
    starts = [start[:cut], start[cut:]]
    try:
        ar = TwoRankAllReduce(ranks)
        cbs = [ar.callback_for(r) for r in range(2)]
        params = _native.CclipParams(tau, iters)

        def work(r, rank):
            out = rank.eng.empty((rank.d,), np.float32)
            st = rank.eng.to_device(starts[r])
            s = rank.eng.empty((rank.n,), np.float64)
            _check(rank.eng.lib.byz_centered_clip_sharded_dev(rank.eng.ctx, _vp(rank.g.ptr), rank.n, rank.d, rank.d,
                                                              ctypes.byref(params), ctypes.cast(cbs[r], ctypes.c_void_p),
                                                              None, _vp(st.ptr), _vp(out.ptr), _vp(s.ptr), None))
            clipped, excluded = rank.eng.centered_clip_info()
            return out.numpy(), s.numpy(), clipped, excluded
        res = run_ranks(ranks, work)
        assert ar.calls[0] == ar.calls[1] == [n] * iters          # one all-reduce of n doubles per distance computation
        assert np.array_equal(res[0][1], res[1][1]) and res[0][2:] == res[1][2:]
        assert close(np.concatenate([res[0][0], res[1][0]]), want, g)
        assert np.allclose(res[0][1], winfo['scales'], rtol=1e-12, atol=0.0)
        assert res[0][2:] == (winfo['clipped_rows'], winfo['excluded_rows'])
        cb = ctypes.cast(_native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 5), ctypes.c_void_p)
        out = ranks[0].eng.empty((ranks[0].d,), np.float32)
        rc = ranks[0].eng.lib.byz_centered_clip_sharded_dev(ranks[0].eng.ctx, _vp(ranks[0].g.ptr), n, cut, cut,
                                                            ctypes.byref(_native.CclipParams(tau, 3)), cb, None, None,
                                                            _vp(out.ptr), None, None)
        assert rc == _native.E_COLLECTIVE and 'all-reduce returned 5' in _native.last_error()
        ranks[0].eng.synchronize()
    finally:
        for rank in ranks:
            rank.close()


# ---- the server keeps the centre --------------------------------------------------------------------------------------
def test_device_server_feeds_each_round_the_last_aggregate(eng, torch):
    from attacking_federate_learning_amd.server import DeviceServer
    n, d = 50, 4000
    rng = np.random.default_rng(45)
    weights = rng.standard_normal(d).astype(np.float32)
    dev = 'cuda:%d' % eng.device
    server = DeviceServer(n, weights, 0.24, 0.1, 0.9, torch_device=dev, engine=eng)
    assert torch.equal(server.clip_centre, torch.zeros(d, dtype=torch.float32, device=dev))
    w, vel = on_gpu(torch, eng, weights), torch.zeros(d, dtype=torch.float32, device=dev)
    centre = None
    for seed in (46, 47):
        g = attacked(n, d, seed=seed)
        tau = median_tau(g)
        server.users_grads.data.copy_(on_gpu(torch, eng, g))
        agg = server.defend_centered_clip(tau=tau, iters=3)
        want = eng.centered_clip(on_gpu(torch, eng, g), tau=tau, iters=3, start=centre)
        assert torch.equal(agg, want)
        eng.server_update(w, vel, want, 0.9, 0.1)
        assert torch.equal(server.current_weights, w) and torch.equal(server.velocity, vel)
        assert torch.equal(server.clip_centre, agg)
        centre = want
    check, _ = restated_centered_clip(g, tau=tau, iters=3, start=None)
    assert not close(agg.cpu().numpy(), check, g)                    # round two did start from round one's aggregate
