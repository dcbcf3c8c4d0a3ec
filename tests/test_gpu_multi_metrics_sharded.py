"""Multi-Metrics over column shards.  The case has n = 130 rows, beyond the small-N distance kernel, so that the
one call and the shards both form the Euclidean matrix from the Gram; its restated boundary gap (computed on the CPU) is
above 1e-6, because the sum of three shards' Grams and L1 sums is not the one call's bit for bit.

Three uneven shards are looped on ONE GPU through byz_multi_metrics_sharded_dev, the all-reduce formed by the callback: a first
pass over the shards adds every shard's buffer into the running sum of that all-reduce (its own results are discarded), a
second pass replaces the buffer by the sum, which is what every rank of a real all-reduce sees.  Exactly two all-reduces per
call, n x n doubles each: the Gram, then the L1 sums."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_multi_metrics import bits, on_gpu
from tests.test_multi_metrics import boundary_gap, planted, restated_multi_metrics

pytestmark = pytest.mark.gpu

N, D, F, SEED = 130, 513, 30, 2
BOUNDS = [0, 140, 377, D]


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


@pytest.fixture(scope='module')
def case():
    g = planted(N, D, F, SEED)
    _, flags, scores, info = restated_multi_metrics(g, 0.3)
    assert boundary_gap(scores, flags) > 1e-6 and info['degenerate'] == 0       # the precondition, computed on the CPU
    return g, flags


def test_three_uneven_column_shards_through_the_c_abi(eng, torch, case):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _DeviceF64, _check, _vp
    g, restated_flags = case
    keep = int(0.3 * N)
    dev = 'cuda:%d' % eng.device
    shards = [on_gpu(torch, eng, g[:, lo:hi]) for lo, hi in zip(BOUNDS[:-1], BOUNDS[1:])]
    want, winfo = eng.multi_metrics(on_gpu(torch, eng, g), p=0.3, return_info=True)
    assert np.array_equal(winfo['chosen_rows'], np.flatnonzero(restated_flags)) and not (winfo['chosen_rows'] >= N - F).any()

    sums, calls, state = {}, [], {'replace': False, 'index': 0}

    def all_reduce(user, buf, count, stream):
        t = torch.as_tensor(_DeviceF64(buf, count), device=dev)
        k = state['index']
        state['index'] += 1
        calls.append(int(count))
        if state['replace']:
            t.copy_(sums[k])
        else:
            sums[k] = t.clone() if k not in sums else sums[k] + t
        torch.cuda.synchronize()
        return 0
    cb = _native.ALLREDUCE_F64_FN(all_reduce)
    outs, flags = [], []
    for replace in (False, True):
        state['replace'] = replace
        for shard in shards:
            state['index'] = 0
            out = torch.empty(shard.shape[1], dtype=torch.float32, device=dev)
            chosen = torch.full((N,), -1, dtype=torch.int32, device=dev)
            _check(eng.lib.byz_multi_metrics_sharded_dev(eng.ctx, _vp(shard.data_ptr()), N, shard.shape[1], shard.stride(0), keep,
                                                         ctypes.cast(cb, ctypes.c_void_p), None, _vp(out.data_ptr()),
                                                         _vp(chosen.data_ptr()), None))
            eng.synchronize()
            assert state['index'] == 2
            if replace:
                outs.append(out.cpu().numpy())
                flags.append(chosen.cpu().numpy())
                info = eng.multi_metrics_info()
                assert info['kept'] == winfo['kept'] and info['usable'] == N and info['degenerate'] == 0
    assert calls == [N * N, N * N] * 6                     # two all-reduces a call: the Gram, then the L1 sums
    for chosen in flags:
        assert np.array_equal(np.flatnonzero(chosen), winfo['chosen_rows'])          # the one-GPU call's set on every shard
    got, ref = np.concatenate(outs), want.cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-6
    assert np.array_equal(bits(got), bits(ref))            # (the same rows: the mean is local to a column)

    # a failing callback is reported
    bad = ctypes.cast(_native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 5), ctypes.c_void_p)
    out = torch.empty(shards[0].shape[1], dtype=torch.float32, device=dev)
    rc = eng.lib.byz_multi_metrics_sharded_dev(eng.ctx, _vp(shards[0].data_ptr()), N, shards[0].shape[1], shards[0].stride(0), keep, bad,
                                               None, _vp(out.data_ptr()), None, None)
    assert rc == _native.E_COLLECTIVE and 'all-reduce returned 5' in _native.last_error()
    eng.synchronize()


def test_a_rank_local_argument_error_returns_before_any_collective(eng, torch, case):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    g, _ = case
    shard = on_gpu(torch, eng, g[:, :140])
    calls = []

    def all_reduce(user, buf, count, stream):
        calls.append(int(count))
        return 0
    cb = ctypes.cast(_native.ALLREDUCE_F64_FN(all_reduce), ctypes.c_void_p)
    out = torch.full((140,), -3.0, dtype=torch.float32, device=shard.device)

    def call(keep=39, rows=N, ld=140, out_ptr=None, fn=cb):
        return eng.lib.byz_multi_metrics_sharded_dev(eng.ctx, _vp(shard.data_ptr()), rows, 140, ld, keep, fn, None,
                                                     _vp(out.data_ptr() if out_ptr is None else out_ptr), None, None)
    assert call(keep=0) == _native.E_INVALID
    assert call(keep=N + 1) == _native.E_INVALID
    assert call(ld=139) == _native.E_INVALID
    assert call(rows=16385) == _native.E_UNSUPPORTED
    assert call(out_ptr=shard.data_ptr()) == _native.E_INVALID
    assert call(fn=None) == _native.E_INVALID
    eng.synchronize()
    assert calls == [] and (out == -3.0).all()


def test_sharded_aggregator_at_world_size_one(eng, torch, case):
    """ShardedAggregator(HipKernels).multi_metrics with one rank holding every column: the composition of the halves (Gram,
    distances and cosine from it, L1 sums and distances from them, features, selection, mean) equals the one call."""
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    g, _ = case
    gt = on_gpu(torch, eng, g)
    want, winfo = eng.multi_metrics(gt, p=0.3, return_info=True)
    agg = ShardedAggregator(HipKernels(eng))
    got, info = agg.multi_metrics(gt, N, F, p=0.3, return_info=True)
    assert np.array_equal(info['chosen_rows'], winfo['chosen_rows']) and info['kept'] == winfo['kept']
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    with pytest.raises(ValueError):
        agg.multi_metrics(gt, N, F, p=1.5)
