"""Geometric median timing on one MI355X: the end-to-end call at the default max_iter, each pass over G alone (the row
distances to a vector, the weighted row mean) and no_defense for comparison.

    python scripts/geomed_timing.py --n 4000 --d 10000000
    python scripts/geomed_timing.py --n 1000 --d 1000000
    python scripts/geomed_timing.py --mode rowsq ...       # one part alone (run under rocprofv3 --kernel-trace --stats)
    python scripts/geomed_timing.py --mode no_defense --package-root DIR ...     # no_defense of another checkout (an A/B)

Device-resident synthetic gradients (normal, row scales 1 .. 1.5, the first 0.24 n rows one vector as the attack leaves
them).  Every part is timed over `--steps` calls after `--warmup` with device events on the current stream; one JSON line:
ms per call, and for the two passes their share of HBM, 4 * n * d bytes over the pass time against 8 TB/s.
"""
import argparse
import json
import os
import sys

PEAK_HBM = 8.0e12


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
    p.add_argument('--max-iter', type=int, default=10)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--mode', default='all', choices=['all', 'e2e', 'rowsq', 'wmean', 'no_defense'])
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

    line = {'mode': args.mode, 'n': n, 'd': d, 'max_iter': args.max_iter, 'steps': args.steps, 'warmup': args.warmup,
            'package_root': os.path.abspath(args.package_root)}
    gbytes = 4.0 * n * d
    modes = ['e2e', 'rowsq', 'wmean', 'no_defense'] if args.mode == 'all' else [args.mode]
    if 'e2e' in modes:
        line['e2e_ms'] = round(timed(lambda: eng.geometric_median(g, max_iter=args.max_iter), args.steps, args.warmup), 4)
        _, info = eng.geometric_median(g, max_iter=args.max_iter, return_info=True)
        line['iterations'] = info['iterations']
        line['passes'] = 2 + 2 * info['iterations']
    if 'rowsq' in modes or 'wmean' in modes:
        z = eng.no_defense(g)
        w = torch.linspace(0.5, 1.5, n, device=device, dtype=torch.float64)
    if 'rowsq' in modes:
        ms = timed(lambda: eng.row_sqdist(g, z), args.steps, args.warmup)
        line['rowsq_ms'], line['rowsq_hbm_frac'] = round(ms, 4), round(gbytes / (ms * 1e-3) / PEAK_HBM, 4)
    if 'wmean' in modes:
        # (the engine checks the weights with one small reduction per call; the ABI entry alone is what the loop runs)
        from attacking_federate_learning_amd.engine import _check, _vp
        out = torch.empty(d, dtype=torch.float32, device=device)
        stream = torch.cuda.current_stream(device).cuda_stream

        def wmean():
            _check(eng.lib.byz_weighted_mean_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(w.data_ptr()), _vp(out.data_ptr()),
                                                 _vp(stream)))
        ms = timed(wmean, args.steps, args.warmup)
        line['wmean_ms'], line['wmean_hbm_frac'] = round(ms, 4), round(gbytes / (ms * 1e-3) / PEAK_HBM, 4)
    if 'no_defense' in modes:
        ms = timed(lambda: eng.no_defense(g), args.steps, args.warmup)
        line['no_defense_ms'], line['no_defense_hbm_frac'] = round(ms, 4), round(gbytes / (ms * 1e-3) / PEAK_HBM, 4)
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
