"""SparseFed timing on one MI355X: the global top-k next to the elementwise yardstick, and the whole round next to the clipped
mean it is built on.

    python scripts/sparsefed_timing.py --mode topk --d 1000000 --k 10000
    python scripts/sparsefed_timing.py --mode topk --d 10000000 --k 100000
    python scripts/sparsefed_timing.py --mode sparsefed --n 1000 --d 1000000 --k 10000
    python scripts/sparsefed_timing.py --mode sparsefed --n 4000 --d 10000000 --k 100000 --steps 3 --warmup 1

topk: through the C ABI (what the call enqueues, without the engine's output allocations), `byz_topk_sparsify_dev` on three
vectors -- normals, an all-equal vector of mixed signs (every key in one bin of every pass: the worst case for the LDS
atomics) and normals of which a quarter are set to one value just inside the k largest (many threshold ties, rationed; the
addition of these two is a zero vector, so that equal values stay equal) --, each with an addition into separate outputs and
in place (residual = x, no addition: the memory changes from call to call, as it does in training), beside
`byz_server_update_dev` on the same length.  The calls alternate: a round times `--steps` calls of each back to back with device events, the figure is the
median over `--rounds` rounds with the lowest and highest beside it.  Per variant also the split the library's timers give
(`byz_timing_read`): column_stats = the three histogram passes and the apply pass, misc = the find, tie-count and tie-scan
kernels; the three histogram passes are three instantiations, so `rocprofv3 --kernel-trace --stats` on this script tells them
apart.  Before anything is timed every variant's selection is checked: exactly k selected, nothing selected below something
that is not.

sparsefed: `byz_sparsefed_dev` (in place on a memory) beside `byz_centered_clip_dev` (iters = 1, no start), the parent's code
path, on scripts/geomed_timing.py's synthetic matrix, alternating in the same way.  One JSON line per run.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geomed_timing import PEAK_HBM, timed  # noqa: E402  (timed: events round `steps` calls after `warmup` calls)

K_COLUMN_STATS, K_MISC = 0, 8      # BYZ_K_COLUMN_STATS, BYZ_K_MISC (include/byzagg.h)


def alternate(calls, steps, warmup, rounds):
    samples = {name: [] for name in calls}
    for r in range(rounds):
        for name, call in calls.items():
            samples[name].append(timed(call, steps, warmup if r == 0 else 0))
    return samples


def summarise(line, samples, base=None):
    for name, ms in samples.items():
        med = statistics.median(ms)
        line[name + '_ms'] = round(med, 4)
        line[name + '_ms_min_max'] = [round(min(ms), 4), round(max(ms), 4)]
        if base is not None:
            line[name + '_vs_' + base] = round(med / statistics.median(samples[base]), 3)


def timer_split(eng, call, steps):
    """ms per call inside the library's column_stats and misc timers."""
    from attacking_federate_learning_amd.engine import _check
    _check(eng.lib.byz_timing_enable(eng.ctx, 1))
    _check(eng.lib.byz_timing_reset(eng.ctx))
    for _ in range(steps):
        call()
    out = []
    for slot in (K_COLUMN_STATS, K_MISC):
        ms, launches = ctypes.c_double(0.0), ctypes.c_int64(0)
        _check(eng.lib.byz_timing_read(eng.ctx, slot, ctypes.byref(ms), ctypes.byref(launches)))
        out.append(round(ms.value / steps, 4))
    _check(eng.lib.byz_timing_enable(eng.ctx, 0))
    return out


def run_topk(args, eng, torch, device):
    from attacking_federate_learning_amd.engine import _check, _vp
    d, k = args.d, args.k
    gen = torch.Generator(device=device).manual_seed(d + k)
    normals = torch.empty(d, dtype=torch.float32, device=device).normal_(generator=gen)
    small = torch.empty(d, dtype=torch.float32, device=device).normal_(generator=gen).mul_(1e-3)
    equal = torch.full((d,), 0.375, dtype=torch.float32, device=device)
    equal[::3] = -0.375
    tied = normals.clone()
    kth = float(tied.abs().kthvalue(d - k // 2).values)      # the (k / 2)-th largest magnitude: k / 2 - 1 values lie above it
    tied[torch.randperm(d, device=device, generator=gen)[:d // 4]] = kth
    data = {'normals': normals, 'equal': equal, 'ties': tied}
    zeros = torch.zeros_like(small)
    adds = {'normals': small, 'equal': zeros, 'ties': zeros}      # (a zero addition: the equal values stay equal, the ties tied)
    stream = torch.cuda.current_stream(device).cuda_stream
    out, res = torch.empty_like(normals), torch.empty_like(normals)
    w, vel = torch.zeros_like(normals), torch.zeros_like(normals)
    work = {name: v.clone() for name, v in data.items()}

    def topk(x, add, o, r):
        return lambda: _check(eng.lib.byz_topk_sparsify_dev(eng.ctx, _vp(x.data_ptr()), _vp(add.data_ptr()) if add is not None else None,
                                                            d, k, _vp(o.data_ptr()), _vp(r.data_ptr()), _vp(stream)))
    line = {'mode': 'topk', 'd': d, 'k': k, 'steps': args.steps, 'warmup': args.warmup, 'rounds': args.rounds}
    for name, v in data.items():
        topk(v, adds[name], out, res)()
        info = eng.topk_info()
        wv = v + adds[name]
        sel = out.view(torch.int32) != 0
        assert int(sel.sum()) <= k and torch.equal((out.view(torch.int32) | res.view(torch.int32)), wv.view(torch.int32))
        if bool((~sel).any()) and bool(sel.any()):
            assert float(wv.abs()[sel].min()) >= float(wv.abs()[~sel].max())
        line[name + '_info'] = info
    calls = {'server_update': lambda: _check(eng.lib.byz_server_update_dev(eng.ctx, _vp(w.data_ptr()), _vp(vel.data_ptr()),
                                                                            _vp(normals.data_ptr()), d, 0.9, 0.1, _vp(stream)))}
    for name, v in data.items():
        calls[name + '_add'] = topk(v, adds[name], out, res)
        # in place: after the first call the memory holds the unselected values, the k selected are zeros (a steady state)
        calls[name + '_in_place'] = topk(work[name], None, out, work[name])
    samples = alternate(calls, args.steps, args.warmup, args.rounds)
    summarise(line, samples, base='server_update')
    for name in calls:
        if name != 'server_update':
            line[name + '_column_stats_misc_ms'] = timer_split(eng, calls[name], args.steps)
    # bytes: (3 + 1) reads of x (and add) and one write of out and residual; + 1 read when the ties are rationed
    line['algorithmic_bytes_add'] = 4 * 8 * d + 8 * d
    line['normals_add_hbm_frac'] = round(line['algorithmic_bytes_add'] / (line['normals_add_ms'] * 1e-3) / PEAK_HBM, 4)
    return line


def run_sparsefed(args, eng, torch, device):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    n, d, k = args.n, args.d, args.k
    f = int(n * 0.24)
    gen = torch.Generator(device=device).manual_seed(n + d)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    g.normal_(generator=gen)
    g.mul_(torch.linspace(1.0, 1.5, n, device=device)[torch.randperm(n, device=device, generator=gen)][:, None])
    if f:
        g[:f] = g[0]
    torch.cuda.synchronize()
    clip = float(torch.linalg.vector_norm(g[n // 2].double()))      # about half of the rows are clipped
    stream = torch.cuda.current_stream(device).cuda_stream
    agg, out = torch.empty(d, dtype=torch.float32, device=device), torch.empty(d, dtype=torch.float32, device=device)
    memory = torch.zeros(d, dtype=torch.float32, device=device)
    cparams, sparams = _native.CclipParams(clip, 1), _native.SparsefedParams(clip, k)
    calls = {
        'centered_clip': lambda: _check(eng.lib.byz_centered_clip_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, ctypes.byref(cparams), None,
                                                                      _vp(agg.data_ptr()), None, _vp(stream))),
        'sparsefed': lambda: _check(eng.lib.byz_sparsefed_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, ctypes.byref(sparams),
                                                              _vp(memory.data_ptr()), _vp(out.data_ptr()), _vp(stream))),
    }
    calls['centered_clip']()
    calls['sparsefed']()
    info = eng.topk_info()
    assert info['selected'] == k and int((out != 0).sum()) <= k
    assert torch.equal(out.view(torch.int32) | memory.view(torch.int32), agg.view(torch.int32))      # the memory was zero
    line = {'mode': 'sparsefed', 'n': n, 'd': d, 'k': k, 'clip': round(clip, 3), 'steps': args.steps, 'warmup': args.warmup,
            'rounds': args.rounds, 'topk_info': info, 'clipped_excluded_rows': list(eng.centered_clip_info())}
    samples = alternate(calls, args.steps, args.warmup, args.rounds)
    summarise(line, samples, base='centered_clip')
    line['centered_clip_hbm_frac'] = round(2 * 4.0 * n * d / (line['centered_clip_ms'] * 1e-3) / PEAK_HBM, 4)
    return line


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', default='topk', choices=['topk', 'sparsefed'])
    p.add_argument('--n', type=int, default=1000)
    p.add_argument('--d', type=int, default=1_000_000)
    p.add_argument('--k', type=int, default=10_000)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from attacking_federate_learning_amd.engine import get_engine
    eng = get_engine()
    device = torch.device('cuda', eng.device)
    line = run_topk(args, eng, torch, device) if args.mode == 'topk' else run_sparsefed(args, eng, torch, device)
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
