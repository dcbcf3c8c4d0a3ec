"""Timing of the window mean (csrc/centre_window.hip) and of Phocas on one MI355X, next to the rank-trimmed mean that supplies
Phocas' centre and to the two yardsticks that exist without them: no_defense (one streaming read of the same matrix) and
trimmed_mean (the reference's mean around the median, through the median-window kernels and, above 5,632 rows, tall_select).

    python scripts/phocas_timing.py                                  # the four shapes, both kinds of data
    python scripts/phocas_timing.py --shapes 1000x1000000 --mode window_mean --data normal     # one part alone (under rocprofv3)

Device-resident synthetic gradients: `normal` is seeded normals, `attack` the same with rows 0 .. 0.24 n being one vector, as the
drift attack leaves them.  b = 0.24 n; the window's centre is rank_trimmed_mean's result and keep = n - b, so window_mean is
exactly Phocas' second kernel.  All parts run in ONE process: every round times each part over `--steps` calls after `--warmup`
with device events on the current stream, the parts alternating, and the figure is the median of `--rounds` rounds with the lowest
and highest beside it.  One JSON line per (shape, data): ms per call and the share of HBM, 4 * n * d bytes over the time against
8 TB/s (one read of the matrix; a kernel that reads it five times cannot exceed 0.2).
"""
import argparse
import json
import os
import statistics
import sys

PEAK_HBM = 8.0e12
MODES = ['window_mean', 'phocas', 'rank_trimmed_mean', 'trimmed_mean', 'no_defense']
SHAPES = '1000x1000000,2080x500000,4000x250000,10000x100000'


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
    p.add_argument('--shapes', default=SHAPES, help='comma-separated ROWSxCOLS')
    p.add_argument('--data', default='normal,attack')
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--mode', default='all', choices=['all'] + MODES)
    p.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from attacking_federate_learning_amd.engine import get_engine

    eng = get_engine()
    device = torch.device('cuda', eng.device)
    modes = MODES if args.mode == 'all' else [args.mode]
    for shape in args.shapes.split(','):
        n, d = (int(v) for v in shape.split('x'))
        f = int(n * 0.24)
        for data in args.data.split(','):
            gen = torch.Generator(device=device).manual_seed(n + d)
            g = torch.empty((n, d), dtype=torch.float32, device=device)
            g.normal_(generator=gen)
            if data == 'attack' and f:
                g[:f] = g[0]
            centre = eng.rank_trimmed_mean(g, f)
            # what is timed is what the composition test compares: the one call and the two calls give the same bits
            same = torch.equal(eng.phocas(g, f).view(torch.int32), eng.window_mean(g, centre, n - f).view(torch.int32))
            torch.cuda.synchronize()
            calls = {'window_mean': lambda: eng.window_mean(g, centre, n - f), 'phocas': lambda: eng.phocas(g, f),
                     'rank_trimmed_mean': lambda: eng.rank_trimmed_mean(g, f), 'trimmed_mean': lambda: eng.trimmed_mean(g, n, f),
                     'no_defense': lambda: eng.no_defense(g)}
            rounds = {mode: [] for mode in modes}
            for _ in range(args.rounds):
                for mode in modes:
                    rounds[mode].append(timed(calls[mode], args.steps, args.warmup))
            line = {'n': n, 'd': d, 'b': f, 'keep': n - f, 'data': data, 'steps': args.steps, 'warmup': args.warmup,
                    'rounds': args.rounds, 'phocas_is_the_composition': bool(same)}
            gbytes = 4.0 * n * d
            for mode in modes:
                ms = statistics.median(rounds[mode])
                line[mode + '_ms'] = round(ms, 4)
                line[mode + '_ms_range'] = [round(min(rounds[mode]), 4), round(max(rounds[mode]), 4)]
                line[mode + '_hbm_frac'] = round(gbytes / (ms * 1e-3) / PEAK_HBM, 4)
            print(json.dumps(line), flush=True)
            del g, centre
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
