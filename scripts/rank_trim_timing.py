"""Timing of the coordinate-wise median and the rank-trimmed mean on one MI355X, next to the two yardsticks that exist without
them: no_defense (one streaming read of the same matrix) and trimmed_mean (the same heights through the median-window kernels).

    python scripts/rank_trim_timing.py --n 1000 --d 1000000
    python scripts/rank_trim_timing.py --n 10000 --d 100000 --mode rank_trimmed_mean     # one part alone (under rocprofv3)

Device-resident synthetic gradients (normal, row scales 1 .. 1.5, the first 0.24 n rows one vector as the attack leaves them);
b = 0.24 n.  Every part is timed over `--steps` calls after `--warmup` with device events on the current stream; one JSON line:
ms per call and the share of HBM, 4 * n * d bytes over the time against 8 TB/s.
"""
import argparse
import json
import os
import sys

PEAK_HBM = 8.0e12
MODES = ['rank_trimmed_mean', 'coordinate_median', 'trimmed_mean', 'no_defense']


def timed(call, steps, warmup):
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=1000)
    p.add_argument('--d', type=int, default=1_000_000)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--mode', default='all', choices=['all'] + MODES)
    p.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from attacking_federate_learning_amd.engine import get_engine

    n, d = args.n, args.d
    f = int(n * 0.24)
    eng = get_engine()
    device = torch.device('cuda', eng.device)
    gen = torch.Generator(device=device).manual_seed(n + d)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    g.normal_(generator=gen)
    g.mul_(torch.linspace(1.0, 1.5, n, device=device)[torch.randperm(n, device=device, generator=gen)][:, None])
    if f:
        g[:f] = g[0]
    torch.cuda.synchronize()

    calls = {'rank_trimmed_mean': lambda: eng.rank_trimmed_mean(g, f), 'coordinate_median': lambda: eng.coordinate_median(g),
             'trimmed_mean': lambda: eng.trimmed_mean(g, n, f), 'no_defense': lambda: eng.no_defense(g)}
    line = {'mode': args.mode, 'n': n, 'd': d, 'b': f, 'steps': args.steps, 'warmup': args.warmup,
            'package_root': os.path.abspath(args.package_root)}
    gbytes = 4.0 * n * d
    for mode in (MODES if args.mode == 'all' else [args.mode]):
        ms = timed(calls[mode], args.steps, args.warmup)
        line[mode + '_ms'], line[mode + '_hbm_frac'] = round(ms, 4), round(gbytes / (ms * 1e-3) / PEAK_HBM, 4)
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
