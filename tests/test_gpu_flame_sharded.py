"""FLAME over column shards.  Both tests use an input whose restatement is unchanged under 32 seeded symmetric
perturbations of the fp64 cosine matrix by +- the cosine bound (tests/test_gpu_flame.py: the precondition, computed on the CPU),
because the sum of three shards' Grams is not the one call's Gram bit for bit.

Three uneven shards are looped on ONE GPU through byz_flame_sharded_dev, the all-reduce formed by the callback: a first pass
over the shards adds every shard's buffer into the running sum of that all-reduce (its own results are discarded), a second
pass replaces the buffer by the sum, which is what every rank of a real all-reduce sees.  Exactly two all-reduces per call:
n x n doubles, then n."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_flame import bits, honest_and_opposite, on_gpu, stable_under_the_bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def test_three_uneven_column_shards_through_the_c_abi(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _DeviceF64, _check, _vp
    n, d = 63, 1500
    g, f = honest_and_opposite(n, d, seed=1563)
    stable, mask = stable_under_the_bound(g)
    assert stable                                          # the precondition, computed on the CPU
    bounds = [0, 397, 1101, d]
    dev = 'cuda:%d' % eng.device
    shards = [on_gpu(torch, eng, g[:, lo:hi]) for lo, hi in zip(bounds[:-1], bounds[1:])]
    lam, seed, rnd = 0.01, 21, 4
    want, winfo = eng.flame(on_gpu(torch, eng, g), lam=lam, seed=seed, round=rnd, return_info=True)
    assert np.array_equal(winfo['admitted_rows'], np.flatnonzero(mask)) and not mask[:f].any()

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
        for s, shard in enumerate(shards):
            state['index'] = 0
            out = torch.empty(shard.shape[1], dtype=torch.float32, device=dev)
            adm = torch.full((n,), -1, dtype=torch.int32, device=dev)
            params = _native.FlameParams(lam, 1, 0, seed, rnd, bounds[s])
            _check(eng.lib.byz_flame_sharded_dev(eng.ctx, _vp(shard.data_ptr()), n, shard.shape[1], shard.stride(0), ctypes.byref(params),
                                                 ctypes.cast(cb, ctypes.c_void_p), None, None, _vp(out.data_ptr()), _vp(adm.data_ptr()),
                                                 None))
            eng.synchronize()
            assert state['index'] == 2
            if replace:
                outs.append(out.cpu().numpy())
                flags.append(adm.cpu().numpy())
                assert np.array_equal(eng.flame_info()['admitted'], winfo['admitted'])
    assert calls == [n * n, n] * 6                         # two all-reduces a call: the Gram, then the norms
    for adm in flags:
        assert np.array_equal(np.flatnonzero(adm), winfo['admitted_rows'])           # the one-GPU call's set on every shard
    got, ref = np.concatenate(outs), want.cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-5
    # the noise: what each side added to its own clipped mean is the same vector, bit for bit
    clean = eng.flame(on_gpu(torch, eng, g), lam=0.0).cpu().numpy()
    state['replace'] = True
    clean_shards = []
    for s, shard in enumerate(shards):
        state['index'] = 0
        out = torch.empty(shard.shape[1], dtype=torch.float32, device=dev)
        params = _native.FlameParams(0.0, 1, 0, seed, rnd, bounds[s])
        _check(eng.lib.byz_flame_sharded_dev(eng.ctx, _vp(shard.data_ptr()), n, shard.shape[1], shard.stride(0), ctypes.byref(params),
                                             ctypes.cast(cb, ctypes.c_void_p), None, None, _vp(out.data_ptr()), None, None))
        eng.synchronize()
        clean_shards.append(out.cpu().numpy())
    clean_got = np.concatenate(clean_shards)
    same = bits(clean_got) == bits(clean)
    assert same.mean() > 0.9                               # (the means agree to fp64 rounding: nearly every column's bits)
    assert np.array_equal(bits(got[same] - clean_got[same]), bits(ref[same] - clean[same]))
    zero = torch.zeros(d, dtype=torch.float32, device=dev)
    clip = torch.tensor([winfo['clip']], dtype=torch.float64, device=dev)
    noise = eng.gaussian_noise(zero, lam, seed=seed, round=rnd, scale=clip).cpu().numpy()
    assert np.abs((got - clean_got) - noise).max() <= 2.0 ** -20 * max(1.0, float(np.abs(clean_got).max()))
    # a failing callback is reported
    bad = ctypes.cast(_native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 5), ctypes.c_void_p)
    out = torch.empty(shards[0].shape[1], dtype=torch.float32, device=dev)
    params = _native.FlameParams(lam, 1, 0, seed, rnd, 0)
    rc = eng.lib.byz_flame_sharded_dev(eng.ctx, _vp(shards[0].data_ptr()), n, shards[0].shape[1], shards[0].stride(0),
                                       ctypes.byref(params), bad, None, None, _vp(out.data_ptr()), None, None)
    assert rc == _native.E_COLLECTIVE and 'all-reduce returned 5' in _native.last_error()
    eng.synchronize()


def test_sharded_aggregator_at_world_size_one_through_rccl():
    """ShardedAggregator(HipKernels).flame with BYZ_FORCE_COLLECTIVES=1: both all-reduces go through RCCL although there is nobody
    else, and the result equals the single-GPU call.  Own process: torch.distributed state stays out of the test session."""
    env = dict(os.environ, BYZ_FORCE_COLLECTIVES='1', MASTER_ADDR='127.0.0.1', MASTER_PORT='29547', RANK='0', WORLD_SIZE='1',
               LOCAL_RANK='0', HSA_ENABLE_IPC_MODE_LEGACY='0')
    proc = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'flame_rccl_worker.py')], env=env, capture_output=True,
                          text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    report = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith('{')][-1])
    assert report['ok'], report
    assert report['comm'].get('allreduce_flame_gram', {}).get('calls', 0) == 1, report['comm']
    assert report['comm'].get('allreduce_flame_norms', {}).get('calls', 0) == 1, report['comm']
