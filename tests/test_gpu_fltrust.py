"""FLTrust on an MI355X, held to the numpy restatement of tests/test_fltrust.py.

The bounds.  row_dots against numpy's fp64 sums: |p - p_ref| <= d 2^-53 sum_c |x_c| |r_c| a row (the classical bound of a
length-d sum, whatever its order), likewise q.  The trust kernel from the device's own sums: ts and w within rtol 1e-12 (centered
clipping's tolerance for its scales), T within rtol 2 n 2^-53, the counts exactly (every |c_i| >= 1e-9: asserted on the inputs).
scaled_rows_sum from the device's own w and T: the bits of the sequential restatement.  The whole call: the vector within
rtol 1e-6, atol 1e-6 max|G| (tests/test_gpu_centered_clip.py's tolerance), ts within atol 4 d 2^-53, the counts exactly.

The shapes cross every kernel boundary: one row, fewer rows than a wave's eight, one more than eight, one more than a block of
32, one and several chunks, widths one short of a window of 1024, one past it and no multiple of four, more than 4096 rows,
many rows, one column; 600,000 columns take the four-wide second pass, and a view with an odd leading dimension the scalar
loads of both passes."""
import ctypes
import functools

import numpy as np
import pytest

from tests.test_fltrust import (SHAPES, restated_dots, restated_fltrust, restated_scaled_sum, restated_trust, trusted)

pytestmark = pytest.mark.gpu

WIDE = (13, 600_000)          # walk_shape's four-wide form starts at 4 * 256 * num_cus * 2 = 524,288 columns
U = 2.0 ** -53


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


@functools.lru_cache(maxsize=None)
def case(n, d):
    """The inputs of one shape and their restatement, computed once and never written to."""
    g, r = trusted(n, d, seed=n + d)
    p, q, q0 = restated_dots(g, r)
    out, info = restated_fltrust(g, r)
    for a in (g, r, p, q, out, info['trust'], info['weights'], info['cosines']):
        a.setflags(write=False)
    return g, r, (p, q, q0), out, info


def close(got, want, g):
    scale = float(np.nanmax(np.abs(g[np.isfinite(g)]))) if np.isfinite(g).any() else 1.0
    return np.allclose(got, want, rtol=1e-6, atol=1e-6 * scale)


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:%d' % eng.device)


def odd_view(torch, dense):
    """The same values behind a leading dimension of d + 5, one float past an aligned start: scalar loads."""
    n, d = dense.shape
    view = torch.empty((n, d + 5), dtype=torch.float32, device=dense.device)[:, 1:d + 1]
    view.copy_(dense)
    return view


def device_sums(torch, eng, gt, rt):
    """(p, q, q0) as the device computes them: row_dots, and rowsq of the 1 x d matrix r."""
    p, q = eng.row_dots(gt, rt)
    q0 = eng.row_sqdist(rt.reshape(1, -1), torch.zeros_like(rt))
    return p.cpu().numpy(), q.cpu().numpy(), float(q0.cpu().numpy()[0])


def check_against_restatement(out, info, g, want, winfo):
    out = out.cpu().numpy() if hasattr(out, 'cpu') else out
    ts = info['trust'].cpu().numpy() if hasattr(info['trust'], 'cpu') else info['trust']
    d = g.shape[1]
    print('max |out - want|', float(np.abs(out - want).max()), 'max |ts - want|', float(np.abs(ts - winfo['trust']).max()),
          'trusted', winfo['trusted_rows'], 'excluded', winfo['excluded_rows'])
    assert not np.isnan(out).any()
    assert close(out, want, g), np.abs(out - want).max()
    assert np.allclose(ts, winfo['trust'], rtol=0.0, atol=4 * d * U)
    assert info['trusted_rows'] == winfo['trusted_rows'] and info['excluded_rows'] == winfo['excluded_rows']
    assert info['root_ok'] == winfo['root_ok']
    return want, winfo


# ---- 1: the fused row pass ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', SHAPES + [WIDE])
def test_row_dots_against_the_fp64_sums(eng, torch, n, d):
    g, r, (p_ref, q_ref, _), _, _ = case(n, d)
    gt, rt = on_gpu(torch, eng, g), on_gpu(torch, eng, r)
    p, q = eng.row_dots(gt, rt)
    x, rd = np.abs(g.astype(np.float64)), np.abs(r.astype(np.float64))
    p_bound, q_bound = d * U * (x * rd[None, :]).sum(axis=1), d * U * (x * x).sum(axis=1)
    p_err, q_err = np.abs(p.cpu().numpy() - p_ref), np.abs(q.cpu().numpy() - q_ref)
    print('p: worst error / bound', float((p_err / p_bound).max()), 'q:', float((q_err / q_bound).max()))
    assert (p_err <= p_bound).all() and (q_err <= q_bound).all()
    again_p, again_q = eng.row_dots(gt, rt)
    assert torch.equal(again_p, p) and torch.equal(again_q, q)                  # two calls: equal bits
    view_p, view_q = eng.row_dots(odd_view(torch, gt), rt)
    assert torch.equal(view_p, p) and torch.equal(view_q, q)                    # a strided view and its dense copy: equal bits
    if n * d <= 1 << 20:
        host_p, host_q = eng.row_dots(g, r)                                     # a host matrix, staged
        assert np.array_equal(host_p, p.cpu().numpy()) and np.array_equal(host_q, q.cpu().numpy())


# ---- 2: the trust kernel from the device's own sums ---------------------------------------------------------------------
@pytest.mark.parametrize('n,d', SHAPES)
def test_the_trust_kernel_alone(eng, torch, n, d):
    g, r, _, _, _ = case(n, d)
    gt, rt = on_gpu(torch, eng, g), on_gpu(torch, eng, r)
    p, q, q0 = device_sums(torch, eng, gt, rt)
    ts, w, total, winfo = restated_trust(p, q, q0)
    assert (np.abs(winfo['cosines']) >= 1e-9).all()          # a precondition of the inputs, not of the kernel
    _, info = eng.fltrust(gt, rt, return_info=True)
    assert np.allclose(info['trust'].cpu().numpy(), ts, rtol=1e-12, atol=0.0)
    assert np.allclose(info['weights'].cpu().numpy(), w, rtol=1e-12, atol=0.0)
    print('T', info['trust_sum'], 'restated', total)
    assert abs(info['trust_sum'] - total) <= 2 * n * U * total
    assert (info['trusted_rows'], info['excluded_rows'], info['root_ok']) == (winfo['trusted_rows'], 0, True)
    assert eng.fltrust_info() == (info['trusted_rows'], 0, True, info['trust_sum'])


# ---- 3: the second pass -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', [(9, 1025), (33, 2051), (4097, 300), (16, 1), WIDE])
def test_scaled_rows_sum_from_the_devices_own_weights(eng, torch, n, d):
    g, r, _, _, _ = case(n, d)
    gt = on_gpu(torch, eng, g)
    _, info = eng.fltrust(gt, on_gpu(torch, eng, r), return_info=True)
    w, total = info['weights'], info['trust_sum']
    want = restated_scaled_sum(g, w.cpu().numpy(), total)
    got = eng.scaled_rows_sum(gt, w, total)
    assert np.array_equal(got.cpu().numpy(), want)            # the restatement is the kernel's arithmetic: bits
    assert torch.equal(eng.scaled_rows_sum(odd_view(torch, gt), w, total), got)                 # the scalar kernel: the same bits
    assert torch.equal(eng.scaled_rows_sum(gt, w, 0.0), torch.zeros_like(got))                  # a zero divisor: zeros


def test_scaled_rows_sum_alone(eng, torch):
    rng = np.random.default_rng(39)
    # (7, 129): no whole run of eight rows, the tail loop alone; (16, 1): whole runs, no tail, one column
    for n, d in [(37, 3001), (300, 70000), (9, 5), (7, 129), (16, 1)]:
        g = rng.standard_normal((n, d)).astype(np.float32)
        w = rng.random(n)
        w[::4] = 0.0
        g[4] = np.inf                                     # a row of infs under a zero weight
        total = float(w.sum())
        want = restated_scaled_sum(g, w, total)
        got = eng.scaled_rows_sum(on_gpu(torch, eng, g), on_gpu(torch, eng, w), on_gpu(torch, eng, np.array([total]))).cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got, want)
        assert np.array_equal(eng.scaled_rows_sum(g, w, total), want)                       # host inputs, staged
        assert np.array_equal(eng.scaled_rows_sum(g, w, 0.0), np.zeros(d, dtype=np.float32))


def test_wide_rows_take_the_four_wide_sum(eng, torch):
    n, wide = WIDE
    rng = np.random.default_rng(40)
    g = rng.standard_normal((n, wide)).astype(np.float32)
    g[4] = np.inf
    w = rng.random(n)
    w[[1, 4, 10]] = 0.0
    total = float(w.sum())
    gt, wt = on_gpu(torch, eng, g), on_gpu(torch, eng, w)
    for cols in (wide, wide - 1, wide - 1027):                       # whole, a masked tail, no multiple of 1024
        got = eng.scaled_rows_sum(gt[:, :cols], wt, total).cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got, restated_scaled_sum(g[:, :cols], w, total))


# ---- 4: the whole call --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', SHAPES + [WIDE])
def test_matches_the_restatement(eng, torch, n, d):
    g, r, _, want, winfo = case(n, d)
    gt, rt = on_gpu(torch, eng, g), on_gpu(torch, eng, r)
    out, info = eng.fltrust(gt, rt, return_info=True)
    check_against_restatement(out, info, g, want, winfo)
    if n >= 7:
        assert 0 < info['trusted_rows'] < n                  # both branches of the ReLU are taken
    assert torch.equal(eng.fltrust(gt, rt), out)
    view, vinfo = eng.fltrust(odd_view(torch, gt), rt, return_info=True)        # ld > n_cols, odd: the scalar path
    assert torch.equal(view, out) and torch.equal(vinfo['trust'], info['trust']) and torch.equal(vinfo['weights'], info['weights'])
    assert (vinfo['trusted_rows'], vinfo['trust_sum']) == (info['trusted_rows'], info['trust_sum'])


# ---- 5: the call is the composition of its pieces -----------------------------------------------------------------------
@pytest.mark.parametrize('n,d', [(500, 3000), (4500, 260)])
def test_the_call_is_the_composition_of_its_pieces(eng, torch, n, d):
    g, r, _, _, _ = case(n, d)
    gt, rt = on_gpu(torch, eng, g), on_gpu(torch, eng, r)
    out, info = eng.fltrust(gt, rt, return_info=True)
    p, q = eng.row_dots(gt, rt)
    q0 = eng.row_sqdist(rt.reshape(1, -1), torch.zeros_like(rt))[0]
    norm, root_norm = torch.sqrt(q), torch.sqrt(q0)
    c = p / (norm * root_norm)
    trust = torch.where(c > 0, c, torch.zeros_like(c))
    weights = trust * (root_norm / norm)
    print('max |ts - pieces|', float((trust - info['trust']).abs().max()), 'max |w - pieces|', float((weights - info['weights']).abs().max()))
    assert torch.equal(trust, info['trust']) and torch.equal(weights, info['weights'])
    assert torch.equal(eng.scaled_rows_sum(gt, weights, info['trust_sum']), out)


# ---- 6: the other entry points ------------------------------------------------------------------------------------------
def test_host_inputs_an_aliased_output_and_an_overlapping_one(eng, torch):
    from attacking_federate_learning_amd import _native, defences
    from attacking_federate_learning_amd.engine import _check, _vp
    n, d = 300, 5000
    g, r, _, _, _ = case(n, d)
    gt, rt = on_gpu(torch, eng, g), on_gpu(torch, eng, r)
    want, winfo = eng.fltrust(gt, rt, return_info=True)
    host, hinfo = eng.fltrust(g, r, return_info=True)                        # a host matrix and a host root
    assert np.array_equal(host, want.cpu().numpy())
    assert np.array_equal(hinfo['trust'], winfo['trust'].cpu().numpy()) and np.array_equal(hinfo['weights'], winfo['weights'].cpu().numpy())
    assert (hinfo['trusted_rows'], hinfo['excluded_rows'], hinfo['root_ok'], hinfo['trust_sum']) == \
        (winfo['trusted_rows'], winfo['excluded_rows'], winfo['root_ok'], winfo['trust_sum'])
    assert torch.equal(eng.fltrust(gt, r), want)                             # a device matrix and a host root, uploaded
    assert np.array_equal(eng.fltrust(g, rt), host)
    assert np.array_equal(defences.fltrust(g, n, int(0.24 * n), r), host)
    dout, dinfo = defences.fltrust(gt, n, int(0.24 * n), rt, return_info=True)
    assert torch.equal(dout, want) and dinfo['trusted_rows'] == winfo['trusted_rows']
    # out aliasing root, through the C ABI
    buf = rt.clone()
    lib, ctx = eng.lib, eng.ctx
    _check(lib.byz_fltrust_dev(ctx, _vp(gt.data_ptr()), n, d, d, _vp(buf.data_ptr()), _vp(buf.data_ptr()), None, None, None))
    eng.synchronize()
    assert torch.equal(buf, want)
    # out inside the matrix
    out = eng.empty((d,), np.float32)
    assert lib.byz_fltrust_dev(ctx, _vp(gt.data_ptr()), n, d, d, _vp(rt.data_ptr()), _vp(gt.data_ptr() + 4000), None, None,
                               None) == _native.E_INVALID
    assert 'overlaps' in _native.last_error()
    assert lib.byz_fltrust_dev(ctx, _vp(gt.data_ptr()), n, d, d, None, _vp(out.ptr), None, None, None) == _native.E_INVALID
    assert lib.byz_fltrust_dev(ctx, _vp(gt.data_ptr()), 0, d, d, _vp(rt.data_ptr()), _vp(out.ptr), None, None, None) == _native.E_INVALID
    assert lib.byz_fltrust_dev(ctx, _vp(gt.data_ptr()), n, d, d - 1, _vp(rt.data_ptr()), _vp(out.ptr), None, None, None) == _native.E_INVALID
    assert lib.byz_fltrust_dev(ctx, _vp(gt.data_ptr()), (1 << 20) + 1, 1, 1, _vp(rt.data_ptr()), _vp(out.ptr), None, None,
                               None) == _native.E_UNSUPPORTED
    eng.check()
    with pytest.raises(ValueError):
        eng.fltrust(gt, rt[:-1].contiguous())
    with pytest.raises(ValueError):
        eng.fltrust(g, r[:-1])


# ---- 7: the edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [120, 4200])
def test_non_finite_rows_are_excluded(eng, torch, n):
    g, r = trusted(n, 1100, seed=35)
    g[5, 17] = np.nan
    g[40, 17] = np.inf
    g[77, 17] = -np.inf
    out, info = eng.fltrust(on_gpu(torch, eng, g), on_gpu(torch, eng, r), return_info=True)
    check_against_restatement(out, info, g, *restated_fltrust(g, r))
    assert info['excluded_rows'] == 3 and torch.isfinite(out).all()
    assert info['trust'].cpu().numpy()[[5, 40, 77]].tolist() == [0.0, 0.0, 0.0]
    assert info['weights'].cpu().numpy()[[5, 40, 77]].tolist() == [0.0, 0.0, 0.0]


def test_no_trusted_row_and_a_broken_root_are_the_zero_step(eng, torch):
    bad = np.full((6, 300), np.inf, dtype=np.float32)
    bad[::2] = np.nan
    root = np.random.default_rng(36).standard_normal(300).astype(np.float32)
    zeros = np.zeros(300, dtype=np.float32)
    for matrix in (bad, on_gpu(torch, eng, bad)):                           # nothing but non-finite rows
        out, info = eng.fltrust(matrix, root, return_info=True)
        out = out.cpu().numpy() if hasattr(out, 'cpu') else out
        assert np.array_equal(out, zeros)
        assert (info['excluded_rows'], info['trusted_rows'], info['root_ok'], info['trust_sum']) == (6, 0, True, 0.0)
    g, r = trusted(30, 300, seed=37)
    gt = on_gpu(torch, eng, g)
    broken = r.copy()
    broken[5] = np.nan
    for bad_root in (zeros, broken, np.full(300, np.inf, dtype=np.float32)):                 # a zero root, a non-finite one
        out, info = eng.fltrust(gt, on_gpu(torch, eng, bad_root), return_info=True)
        assert torch.equal(out, torch.zeros_like(out))
        assert not info['root_ok'] and info['trusted_rows'] == 0 and info['trust_sum'] == 0.0
        assert torch.equal(info['trust'], torch.zeros_like(info['trust']))
    negative = (-np.abs(g)).astype(np.float32)                              # every cosine negative
    out, info = eng.fltrust(on_gpu(torch, eng, negative), on_gpu(torch, eng, np.abs(r)), return_info=True)
    assert torch.equal(out, torch.zeros_like(out))
    assert (info['trusted_rows'], info['excluded_rows'], info['root_ok'], info['trust_sum']) == (0, 0, True, 0.0)


# ---- 8: the columns layout ----------------------------------------------------------------------------------------------
def test_sharded_aggregator_over_uneven_column_shards_matches_one_gpu(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator

    class LoopedKernels(HipKernels):
        """Every shard on this GPU: the row sums add the shards' parts, as the all-reduce over the ranks would."""

        def __init__(self, engine, bounds):
            super().__init__(engine)
            self.bounds = bounds

        def row_dots(self, g, r):
            parts = [self.engine.row_dots(g[:, lo:hi], r[lo:hi].contiguous()) for lo, hi in self.bounds]
            return sum(p for p, _ in parts), sum(q for _, q in parts)

        def row_sqdist(self, g, z):
            return sum(self.engine.row_sqdist(g[:, lo:hi], z[lo:hi].contiguous()) for lo, hi in self.bounds)

        def scaled_rows_sum(self, g, weights, divisor):
            return torch.cat([self.engine.scaled_rows_sum(g[:, lo:hi], weights, divisor) for lo, hi in self.bounds])

    n, d = 300, 5000
    g, r = (a.copy() for a in case(n, d)[:2])
    g[9, 100] = np.nan
    gt, rt = on_gpu(torch, eng, g), on_gpu(torch, eng, r)
    want, winfo = eng.fltrust(gt, rt, return_info=True)
    for cuts in ([0, d], [0, d // 3 + 1, d], [0, d // 3 + 1, d // 2 + 7, d]):
        kern = LoopedKernels(eng, list(zip(cuts[:-1], cuts[1:])))
        got, info = ShardedAggregator(kern).fltrust(gt, rt, return_info=True)
        assert close(got.cpu().numpy(), want.cpu().numpy(), g)
        ts, wts = info['trust'].cpu().numpy(), winfo['trust'].cpu().numpy()
        print('shards', len(cuts) - 1, 'max |ts - one GPU|', float(np.abs(ts - wts).max()))
        if len(cuts) == 2:
            assert np.array_equal(ts, wts)                 # one shard: the same sums, the same scores
        # several shards move rowsq's chunk boundaries: p and q are other roundings of the same sums (item 4's bound), the
        # trusted set is the same
        assert np.allclose(ts, wts, rtol=0.0, atol=4 * d * U) and np.array_equal(ts > 0, wts > 0)
        assert info['trusted_rows'] == winfo['trusted_rows'] and info['excluded_rows'] == winfo['excluded_rows'] == 1
        # T: n scores each within 4 d 2^-53, and the order of the sum
        assert info['root_ok'] and abs(info['trust_sum'] - winfo['trust_sum']) <= n * 4 * d * U + 2 * n * U * winfo['trust_sum']


def test_two_ranks_through_the_c_abi(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    from tests.test_gpu_sharded_cabi import Rank, TwoRankAllReduce, run_ranks
    n, d, cut = 200, 3000, 1100
    g, r, _, want, winfo = case(n, d)
    ranks = [Rank(g[:, :cut]), Rank(g[:, cut:])]
    roots = [r[:cut], r[cut:]]
    try:
        ar = TwoRankAllReduce(ranks)
        cbs = [ar.callback_for(k) for k in range(2)]

        def work(k, rank):
            out = rank.eng.empty((rank.d,), np.float32)
            root = rank.eng.to_device(roots[k])
            ts = rank.eng.empty((rank.n,), np.float64)
            w = rank.eng.empty((rank.n,), np.float64)
            _check(rank.eng.lib.byz_fltrust_sharded_dev(rank.eng.ctx, _vp(rank.g.ptr), rank.n, rank.d, rank.d, _vp(root.ptr),
                                                        ctypes.cast(cbs[k], ctypes.c_void_p), None, _vp(out.ptr), _vp(ts.ptr),
                                                        _vp(w.ptr), None))
            return out.numpy(), ts.numpy(), w.numpy(), rank.eng.fltrust_info()
        res = run_ranks(ranks, work)
        assert ar.calls[0] == ar.calls[1] == [2 * n + 1]          # exactly one all-reduce, of 2 n + 1 doubles, per rank
        assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2]) and res[0][3] == res[1][3]
        assert close(np.concatenate([res[0][0], res[1][0]]), want, g)
        assert np.allclose(res[0][1], winfo['trust'], rtol=0.0, atol=4 * d * U)
        assert res[0][3][:3] == (winfo['trusted_rows'], winfo['excluded_rows'], True)
        cb = ctypes.cast(_native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 5), ctypes.c_void_p)
        out = ranks[0].eng.empty((ranks[0].d,), np.float32)
        root = ranks[0].eng.to_device(roots[0])
        rc = ranks[0].eng.lib.byz_fltrust_sharded_dev(ranks[0].eng.ctx, _vp(ranks[0].g.ptr), n, cut, cut, _vp(root.ptr), cb, None,
                                                      _vp(out.ptr), None, None, None)
        assert rc == _native.E_COLLECTIVE and 'all-reduce returned 5' in _native.last_error()
        ranks[0].eng.synchronize()
    finally:
        for rank in ranks:
            rank.close()


# ---- 9: the server's round ----------------------------------------------------------------------------------------------
def test_device_server_takes_the_momentum_step_on_the_aggregate(eng, torch):
    from attacking_federate_learning_amd.server import DeviceServer
    n, d = 50, 4000
    rng = np.random.default_rng(45)
    weights = rng.standard_normal(d).astype(np.float32)
    dev = 'cuda:%d' % eng.device
    server = DeviceServer(n, weights, 0.24, 0.1, 0.9, torch_device=dev, engine=eng)
    w, vel = on_gpu(torch, eng, weights), torch.zeros(d, dtype=torch.float32, device=dev)
    for seed in (46, 47):
        g, r = trusted(n, d, seed=seed)
        rt = on_gpu(torch, eng, r)
        server.users_grads.data.copy_(on_gpu(torch, eng, g))
        agg = server.defend_fltrust(rt)
        want = eng.fltrust(on_gpu(torch, eng, g), rt)
        assert torch.equal(agg, want) and torch.equal(rt.cpu(), torch.from_numpy(r))          # the root is left alone
        eng.server_update(w, vel, want, 0.9, 0.1)
        assert torch.equal(server.current_weights, w) and torch.equal(server.velocity, vel)
