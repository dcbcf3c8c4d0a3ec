"""The global top-k over two ranks through the C ABI alone (needs an MI355X): byz_topk_sparsify_sharded_dev with the host's
all-reduce as a callback, two contexts on two threads (tests/test_gpu_sharded_cabi.py's Rank, TwoRankAllReduce and run_ranks).
The concatenated out and residual are the single call's bits, the all-reduce lengths are the constants include/byzagg.h
states (2048, 1024, 1024 and rank_count doubles) on both ranks whatever the data, a failing callback is BYZ_E_COLLECTIVE."""
import ctypes

import numpy as np
import pytest

from tests import views_arena
from tests.test_geometric_median import attacked
from tests.test_gpu_centered_clip import close
from tests.test_gpu_sharded_cabi import Rank, TwoRankAllReduce, run_ranks
from tests.test_sparsefed import planted, restated_topk

pytestmark = pytest.mark.gpu

N_TOTAL = 5000
LENGTHS = [2048, 1024, 1024, 2]          # the four all-reduces of a call over two ranks


def sharded_call(rank, r, cb, x_slice, add_slice, n_total, k, in_place=False):
    from attacking_federate_learning_amd.engine import _check, _vp
    eng = rank.eng
    n_local = x_slice.size
    x = eng.to_device(x_slice)
    add = eng.to_device(add_slice) if add_slice is not None else None
    out = add if in_place and add is not None else eng.empty((n_local,), np.float32)
    res = x if in_place else eng.empty((n_local,), np.float32)
    _check(eng.lib.byz_topk_sparsify_sharded_dev(eng.ctx, _vp(x.ptr), _vp(add.ptr) if add is not None else None, n_local, n_total,
                                                 k, r, 2, ctypes.cast(cb, ctypes.c_void_p), None, _vp(out.ptr), _vp(res.ptr), None))
    info = eng.topk_info()
    return out.numpy(), res.numpy(), info


def vectors():
    x = planted(N_TOTAL, seed=1)
    add = planted(N_TOTAL, seed=2)[::-1].copy()
    equal = np.full(N_TOTAL, -2.5, dtype=np.float32)
    equal[::2] = 2.5
    late = (0.01 * np.random.default_rng(3).uniform(0.1, 1.0, N_TOTAL)).astype(np.float32)
    late[[7, 30]] = [9.0, -8.0]                               # two above the threshold on rank 0 ...
    late[[1200, 3000, 4100, 4998, 4999]] = 0.5                # ... and the threshold's ties on rank 1 alone (cut at 1100)
    return x, add, equal, late


@pytest.mark.parametrize('cut', [1100, 4999])
def test_two_ranks_select_the_single_calls_set_bit_for_bit(eng, cut):
    x, add, equal, late = vectors()
    cases = [(x, None, N_TOTAL // 3), (x, add, 777), (x, add, 0), (x, add, N_TOTAL), (x, None, 1),
             (equal, None, 1700), (equal, None, cut + 1), (equal, np.zeros(N_TOTAL, dtype=np.float32), cut - 1),
             (late, None, 4), (late, None, 2), (late, None, 7)]
    ranks = [Rank(np.zeros((1, 4), dtype=np.float32)) for _ in range(2)]
    try:
        for case, (v, a, k) in enumerate(cases):
            want_out, want_res, want = restated_topk(v, k, add=a, return_info=True)
            single = eng.topk_sparsify(v, k, add=a)
            assert views_arena.same_bits(single[0], want_out) and views_arena.same_bits(single[1], want_res)
            slices = [(v[:cut], None if a is None else a[:cut]), (v[cut:], None if a is None else a[cut:])]
            ar = TwoRankAllReduce(ranks)
            cbs = [ar.callback_for(r) for r in range(2)]
            res = run_ranks(ranks, lambda r, rank: sharded_call(rank, r, cbs[r], slices[r][0], slices[r][1], N_TOTAL, k,
                                                                in_place=case % 2 == 1))
            print('case', case, 'k', k, 'cut', cut, 'info', res[0][2], 'calls', ar.calls)
            assert ar.calls[0] == ar.calls[1] == LENGTHS                      # constants of the build, whatever the data
            assert views_arena.same_bits(np.concatenate([res[0][0], res[1][0]]), want_out)
            assert views_arena.same_bits(np.concatenate([res[0][1], res[1][1]]), want_res)
            for r in range(2):                                                # the global figures, on both ranks
                assert {key: res[r][2][key] for key in ('selected', 'threshold_key', 'ties', 'ties_taken')} == \
                       {key: want[key] for key in ('selected', 'threshold_key', 'ties', 'ties_taken')}
        # the tie cases took what they were written for: a quota split across the cut, ties on rank 1 alone
        assert restated_topk(equal, cut + 1, return_info=True)[2]['ties_taken'] == cut + 1
        info = restated_topk(late, 4, return_info=True)[2]
        assert info['ties'] == 5 and info['ties_taken'] == 2 and np.flatnonzero(info['mask']).tolist() == [7, 30, 1200, 3000]
    finally:
        for rank in ranks:
            rank.close()


def test_a_failing_callback_and_bad_shapes(eng):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    x = eng.to_device(planted(1000, seed=4))
    out, res = eng.empty((1000,), np.float32), eng.empty((1000,), np.float32)
    fail = _native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 5)
    ok = _native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 0)

    def call(cb, n_local, n_total, k, rank, world):
        return eng.lib.byz_topk_sparsify_sharded_dev(eng.ctx, _vp(x.ptr), None, n_local, n_total, k, rank, world,
                                                     ctypes.cast(cb, ctypes.c_void_p) if cb is not None else None, None,
                                                     _vp(out.ptr), _vp(res.ptr), None)
    assert call(fail, 1000, 5000, 10, 0, 2) == _native.E_COLLECTIVE and 'all-reduce returned 5' in _native.last_error()
    eng.synchronize()
    assert call(ok, 1001, 1000, 10, 0, 2) == _native.E_INVALID                 # n_local > n_total
    for args in ((ok, 1000, 5000, 5001, 0, 2), (ok, 1000, 5000, -1, 0, 2), (ok, 1000, 5000, 10, 2, 2), (ok, 1000, 5000, 10, -1, 2),
                 (ok, 1000, 5000, 10, 0, 0), (None, 1000, 5000, 10, 0, 2)):
        assert call(*args) == _native.E_INVALID, args[1:]
    # one rank of one with an all-reduce that has nothing to add is the single call
    assert call(ok, 1000, 1000, 100, 0, 1) == 0
    want = restated_topk(planted(1000, seed=4), 100)
    assert views_arena.same_bits(out.numpy(), want[0]) and views_arena.same_bits(res.numpy(), want[1])


def test_the_engine_wraps_a_python_all_reduce_and_never_unwinds_through_c(eng):
    import torch
    from attacking_federate_learning_amd.engine import EngineError
    v = planted(3000, seed=5)
    xt = torch.from_numpy(v.copy()).to('cuda:%d' % eng.device)
    seen = []
    out, res, info = eng.topk_sparsify_sharded(xt, 300, 3000, 0, 1, all_reduce=lambda t: seen.append((t.dtype, t.numel())),
                                               return_info=True)
    assert seen == [(torch.float64, 2048), (torch.float64, 1024), (torch.float64, 1024), (torch.float64, 1)]
    want = restated_topk(v, 300, return_info=True)
    assert views_arena.same_bits(out.cpu().numpy(), want[0]) and views_arena.same_bits(res.cpu().numpy(), want[1])
    assert info['ties_taken'] == want[2]['ties_taken']

    def broken(t):
        raise RuntimeError('the communicator is gone')
    with pytest.raises(EngineError):
        eng.topk_sparsify_sharded(xt, 300, 3000, 0, 1, all_reduce=broken)
    eng.synchronize()
    for bad in ((300, 2999, 0, 1), (300, 3000, 1, 1), (3001, 3000, 0, 1)):
        with pytest.raises(ValueError):
            eng.topk_sparsify_sharded(xt, *bad)


def test_the_sharded_aggregator_at_world_one(eng):
    import torch
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d, k = 25, 3000, 200
    g = attacked(n, d, seed=6)
    g[3] *= np.float32(30.0)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    memory = (0.05 * np.random.default_rng(7).standard_normal(d)).astype(np.float32)
    agg = ShardedAggregator(HipKernels(eng))
    # clip = inf: every scale is exactly 1 on both routes, so the two entries agree bit for bit
    mem = torch.from_numpy(memory.copy()).to(gt.device)
    step, res = agg.sparsefed(gt, n, 5, k, clip=np.inf, residual_local=mem)
    want_step, want_res = defences.sparsefed(gt, n, 5, k=k, clip=np.inf, residual=torch.from_numpy(memory.copy()).to(gt.device),
                                             return_residual=True)
    assert res is mem and torch.equal(step.view(torch.int32), want_step.view(torch.int32))
    assert torch.equal(res.view(torch.int32), want_res.view(torch.int32))
    # a finite clip: the aggregator forms its scales in torch (tests/test_gpu_centered_clip.py holds the two routes to a
    # tolerance), so the top-k is held to the restatement on the aggregator's own clipped mean, bit for bit
    own = agg.centered_clip(gt, tau=2.0, iters=1)
    assert close(own.cpu().numpy(), eng.centered_clip(gt, tau=2.0, iters=1).cpu().numpy(), g)
    step, res = agg.sparsefed(gt, n, 5, k, clip=2.0, residual_local=torch.from_numpy(memory.copy()).to(gt.device))
    want_step, want_res = restated_topk(memory, k, add=own.cpu().numpy())
    assert views_arena.same_bits(step.cpu().numpy(), want_step) and views_arena.same_bits(res.cpu().numpy(), want_res)
    step, res = agg.sparsefed(gt, n, 5, k, clip=2.0)                              # no memory given: zeros
    assert views_arena.same_bits(step.cpu().numpy(), restated_topk(own.cpu().numpy(), k)[0])
