"""Clip-and-noise timing on one MI355X: the noise kernel next to the elementwise yardstick, and the whole defence next to the
clipped mean it is built on.  Every figure of a run comes from ONE process:

    python scripts/weak_dp_timing.py                     # noise at 1e6 and 1e7, weak_dp at 1000 x 1e6 and 4000 x 1e7
    python scripts/weak_dp_timing.py --mode noise --d 10000000
    python scripts/weak_dp_timing.py --mode weak_dp --n 1000 --d 1000000

noise: through the C ABI (what the call enqueues, without the engine's output allocations), `byz_gaussian_noise_dev` out of
place and in place on a 16-byte aligned vector (the dwordx4 instantiation), on a view one float off (the scalar
instantiation) and with a device scale, `byz_noise_words_dev` (the generator alone: no fp64 transform, no read) and
`byz_server_update_dev` on the same length.  By bytes the noise moves 8 B per element and server_update 20 B; the noise pays
an fp64 log, sqrt, sin and cos per two outputs.  The calls alternate: a round times `--steps` calls of each back to back
with device events, the figure is the median over `--rounds` rounds with the lowest and highest beside it.  Before anything
is timed the sample mean and variance of the noise at x = 0 are checked to six standard errors.

weak_dp: `byz_weak_dp_dev` in the fixed and in the adaptive mode beside `byz_centered_clip_dev` (iters = 1, no start), the
code path it extends, on scripts/geomed_timing.py's synthetic matrix, alternating in the same way; sigma = 0 must return the
clipped mean's bits.  One JSON line per measurement.
"""
import argparse
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geomed_timing import PEAK_HBM  # noqa: E402
from sparsefed_timing import alternate, summarise  # noqa: E402


def run_noise(args, eng, torch, device, d):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    gen = torch.Generator(device=device).manual_seed(d)
    flat = torch.empty(d + 4, dtype=torch.float32, device=device).normal_(generator=gen)
    x, off1 = flat[:d], flat[1:d + 1]
    out, out1 = torch.empty(d + 4, dtype=torch.float32, device=device), torch.empty(d + 4, dtype=torch.float32, device=device)
    work = x.clone()
    words = torch.empty(d, dtype=torch.int32, device=device)
    w, vel = torch.zeros(d, dtype=torch.float32, device=device), torch.zeros(d, dtype=torch.float32, device=device)
    scale = torch.tensor([0.5], dtype=torch.float64, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    params = _native.NoiseParams(0.01, 2019, 3, 0)

    def noise(src, dst, scale_ptr=None, p=params):
        return lambda: _check(eng.lib.byz_gaussian_noise_dev(eng.ctx, _vp(src.data_ptr()), d, ctypes.byref(p), _vp(scale_ptr),
                                                             _vp(dst.data_ptr()), _vp(stream)))
    # the sample's moments at x = 0, sigma = 1: six standard errors
    unit = _native.NoiseParams(1.0, 2019, 3, 0)
    zeros = torch.zeros(d, dtype=torch.float32, device=device)
    noise(zeros, out, p=unit)()
    z = out[:d].double()
    mean, var = float(z.mean()), float(z.var(unbiased=False))
    assert abs(mean) <= 6.0 / math.sqrt(d) and abs(var - 1.0) <= 6.0 * math.sqrt(2.0 / d), (mean, var)
    del zeros, z
    calls = {
        'server_update': lambda: _check(eng.lib.byz_server_update_dev(eng.ctx, _vp(w.data_ptr()), _vp(vel.data_ptr()), _vp(x.data_ptr()),
                                                                      d, 0.9, 0.1, _vp(stream))),
        'noise': noise(x, out),
        'noise_in_place': noise(work, work),
        'noise_scaled': noise(x, out, scale.data_ptr()),
        'noise_misaligned': noise(off1, out1[1:d + 1]),
        'words': lambda: _check(eng.lib.byz_noise_words_dev(eng.ctx, ctypes.byref(params), d, _vp(words.data_ptr()), _vp(stream))),
    }
    line = {'mode': 'noise', 'd': d, 'steps': args.noise_steps, 'warmup': args.warmup, 'rounds': args.rounds,
            'sample_mean': round(mean, 6), 'sample_var': round(var, 6)}
    summarise(line, alternate(calls, args.noise_steps, args.warmup, args.rounds), base='server_update')
    line['noise_hbm_frac'] = round(8.0 * d / (line['noise_ms'] * 1e-3) / PEAK_HBM, 4)
    line['server_update_hbm_frac'] = round(20.0 * d / (line['server_update_ms'] * 1e-3) / PEAK_HBM, 4)
    line['noise_normals_per_ns'] = round(d / (line['noise_ms'] * 1e6), 3)
    return line


def run_weak_dp(args, eng, torch, device, n, d, steps, warmup, rounds):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
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
    cparams = _native.CclipParams(clip, 1)

    def weak_dp(sigma, adaptive):
        p = _native.WeakDpParams(clip, sigma, adaptive, 2019, 3, 0)
        return lambda: _check(eng.lib.byz_weak_dp_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, ctypes.byref(p), _vp(out.data_ptr()),
                                                      _vp(stream)))
    calls = {
        'centered_clip': lambda: _check(eng.lib.byz_centered_clip_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, ctypes.byref(cparams), None,
                                                                      _vp(agg.data_ptr()), None, _vp(stream))),
        'weak_dp': weak_dp(0.01, 0),
        'weak_dp_adaptive': weak_dp(0.01, 1),
    }
    calls['centered_clip']()
    weak_dp(0.0, 0)()
    assert torch.equal(out.view(torch.int32), agg.view(torch.int32))          # before the noise: the clipped mean's bits
    line = {'mode': 'weak_dp', 'n': n, 'd': d, 'clip': round(clip, 3), 'steps': steps, 'warmup': warmup, 'rounds': rounds,
            'fixed_info': eng.weak_dp_info()}
    calls['weak_dp_adaptive']()
    line['adaptive_info'] = eng.weak_dp_info()
    summarise(line, alternate(calls, steps, warmup, rounds), base='centered_clip')
    line['centered_clip_hbm_frac'] = round(2 * 4.0 * n * d / (line['centered_clip_ms'] * 1e-3) / PEAK_HBM, 4)
    del g
    torch.cuda.empty_cache()
    return line


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', default='all', choices=['all', 'noise', 'weak_dp'])
    p.add_argument('--n', type=int, default=1000)
    p.add_argument('--d', type=int, default=1_000_000)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--noise-steps', type=int, default=200, help='calls per timed window of the noise mode')
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from attacking_federate_learning_amd.engine import get_engine
    eng = get_engine()
    device = torch.device('cuda', eng.device)
    if args.mode == 'noise':
        runs = [lambda: run_noise(args, eng, torch, device, args.d)]
    elif args.mode == 'weak_dp':
        runs = [lambda: run_weak_dp(args, eng, torch, device, args.n, args.d, args.steps, args.warmup, args.rounds)]
    else:
        runs = [lambda: run_noise(args, eng, torch, device, 1_000_000), lambda: run_noise(args, eng, torch, device, 10_000_000),
                lambda: run_weak_dp(args, eng, torch, device, 1000, 1_000_000, args.steps, args.warmup, args.rounds),
                lambda: run_weak_dp(args, eng, torch, device, 4000, 10_000_000, 3, 1, 3)]
    for run in runs:
        print(json.dumps(run()), flush=True)

if __name__ == '__main__':
    main()
