"""ClippedClustering over column shards: {1, 2, 3} uneven shards are looped on ONE GPU through
byz_clipped_clustering_sharded_dev, the all-reduce formed by the Python callback as tests/test_gpu_flame_sharded.py forms it: a
first pass over the shards adds every shard's buffer into the running sum of that all-reduce (its own results are discarded), a
second pass replaces the buffer by the sum, which is what every rank of a real all-reduce sees.  Exactly two all-reduces a call:
n x n doubles (the Gram), then n (the norms).  The planted input's last two merges are far apart (asserted on the CPU), so the
sum of the shards' Grams, which is not the one call's Gram bit for bit, gives the same admitted set."""
import ctypes

import numpy as np
import pytest

from tests.test_clipped_clustering import planted, restated_linkage
from tests.test_flame import restated_cosine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


@pytest.mark.parametrize('bounds', [[0, 1500], [0, 397, 1500], [0, 397, 1101, 1500]])
def test_column_shards_through_the_c_abi(eng, torch, bounds):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _DeviceF64, _check, _vp
    n, d = 63, 1500
    g, f = planted(n, d, seed=1563)
    _, height, _, _ = restated_linkage(restated_cosine(g).astype(np.float32))
    assert (height[-1] - height[-2]) / height[-1] > 0.5    # the precondition, computed on the CPU
    dev = 'cuda:%d' % eng.device
    full = torch.from_numpy(g).to(dev)
    shards = [full[:, lo:hi].contiguous() for lo, hi in zip(bounds[:-1], bounds[1:])]
    want, winfo = eng.clipped_clustering(full, return_info=True)
    assert np.array_equal(winfo['admitted_rows'], np.arange(f, n))

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
            adm = torch.full((n,), -1, dtype=torch.int32, device=dev)
            params = _native.ClippedClusteringParams(0.0, 1, 0, 2.0)
            _check(eng.lib.byz_clipped_clustering_sharded_dev(eng.ctx, _vp(shard.data_ptr()), n, shard.shape[1], shard.stride(0),
                                                              ctypes.byref(params), ctypes.cast(cb, ctypes.c_void_p), None, None,
                                                              _vp(out.data_ptr()), _vp(adm.data_ptr()), None))
            eng.synchronize()
            assert state['index'] == 2                     # the callback: once for the Gram, once for the norms
            if replace:
                outs.append(out.cpu().numpy())
                flags.append(adm.cpu().numpy())
                info = eng.clipped_clustering_info()
                assert info['admitted'] == winfo['admitted'] and abs(info['clip'] / winfo['clip'] - 1.0) < 1e-12
    assert calls == [n * n, n] * (2 * len(shards))
    for adm in flags:
        assert np.array_equal(np.flatnonzero(adm), winfo['admitted_rows'])          # the one-GPU call's set on every shard
    assert np.abs(np.concatenate(outs) - want.cpu().numpy()).max() <= 1e-5
    # a failing callback is reported
    bad = ctypes.cast(_native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 5), ctypes.c_void_p)
    out = torch.empty(shards[0].shape[1], dtype=torch.float32, device=dev)
    params = _native.ClippedClusteringParams(0.0, 1, 0, 2.0)
    rc = eng.lib.byz_clipped_clustering_sharded_dev(eng.ctx, _vp(shards[0].data_ptr()), n, shards[0].shape[1], shards[0].stride(0),
                                                    ctypes.byref(params), bad, None, None, _vp(out.data_ptr()), None, None)
    assert rc == _native.E_COLLECTIVE and 'all-reduce returned 5' in _native.last_error()
    eng.synchronize()


def test_the_sharded_aggregator_with_one_rank_holding_every_column(eng, torch):
    """ShardedAggregator(HipKernels).clipped_clustering without collectives: the composition of the halves (Gram, cosine_from_gram,
    the selection, the norms, the scales, the sum) gives the one call's admitted set and its vector within 1e-5."""
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d = 40, 700
    g, f = planted(n, d, seed=47)
    gt = torch.from_numpy(g).to('cuda:%d' % eng.device)
    want, winfo = eng.clipped_clustering(gt, return_info=True)
    agg = ShardedAggregator(HipKernels(eng))
    got, info = agg.clipped_clustering(gt, n, f, return_info=True)
    assert np.array_equal(info['admitted_rows'], winfo['admitted_rows']) and np.array_equal(info['admitted_rows'], np.arange(f, n))
    assert np.abs(got.cpu().numpy() - want.cpu().numpy()).max() <= 1e-5 and abs(info['clip'] / winfo['clip'] - 1.0) < 1e-12
