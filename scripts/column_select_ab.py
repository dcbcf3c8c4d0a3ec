"""One build's figures for the three users of csrc/column_select.hpp on one MI355X, for comparing two builds of the library
(profiles/column_select_ab.md): the rank-trimmed mean and the coordinate-wise median (rank_select.hip), the window mean
(centre_window.hip) at one height per geometry, and the trimmed mean of tall columns (tall_select.hip).

    python scripts/column_select_ab.py                                   # this tree's build
    python scripts/column_select_ab.py --package-root ../parent          # another checkout's build, same shapes and seeds

One process times one build: run the two builds in alternating processes and compare the lines.  Device-resident synthetic
gradients as scripts/rank_trim_timing.py makes them (normals, row scales 1 .. 1.5, the first 0.24 n rows one vector), b = 0.24 n,
the window's centre is the rank-trimmed mean and keep = n - b.  The widths put every matrix at 0.8 GB or more, beyond the 256 MiB
Infinity Cache.  Every part is timed over `--steps` calls after `--warmup` with device events, the parts alternating over
`--rounds` rounds; one JSON line per shape: the median ms per call with the lowest and highest round, and the SHA-256 of each
result's bytes, so that two builds' outputs compare as bits at the sizes that are timed.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

SHAPES = '200x1000000,1000x400000,2080x200000,4000x100000,6000x100000,66000x8192'
TALL_SHAPES = '6000x32768,10000x32768'


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


def one_shape(eng, torch, args, root, shape, tall):
    n, d = (int(v) for v in shape.split('x'))
    f = int(n * 0.24)
    device = torch.device('cuda', eng.device)
    gen = torch.Generator(device=device).manual_seed(n + d)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    g.normal_(generator=gen)
    g.mul_(torch.linspace(1.0, 1.5, n, device=device)[torch.randperm(n, device=device, generator=gen)][:, None])
    g[:f] = g[0]
    if tall:
        calls = {'trimmed_mean': lambda: eng.trimmed_mean(g, n, f)}
    else:
        centre = eng.rank_trimmed_mean(g, f)
        calls = {'rank_trimmed_mean': lambda: eng.rank_trimmed_mean(g, f), 'coordinate_median': lambda: eng.coordinate_median(g),
                 'window_mean': lambda: eng.window_mean(g, centre, n - f)}
    line = {'package_root': root, 'n': n, 'd': d, 'b': f, 'steps': args.steps, 'warmup': args.warmup, 'rounds': args.rounds}
    for name, call in calls.items():
        line[name + '_sha256'] = hashlib.sha256(call().cpu().numpy().tobytes()).hexdigest()
    rounds = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, call in calls.items():
            rounds[name].append(timed(call, args.steps, args.warmup))
    for name, ms in rounds.items():
        line[name + '_ms'] = round(statistics.median(ms), 4)
        line[name + '_ms_range'] = [round(min(ms), 4), round(max(ms), 4)]
    return line


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--shapes', default=SHAPES, help='comma-separated ROWSxCOLS for the median, the rank-trimmed mean and the window mean')
    p.add_argument('--tall-shapes', default=TALL_SHAPES, help='comma-separated ROWSxCOLS (more than 5,632 rows) for trimmed_mean')
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    root = os.path.abspath(args.package_root)
    sys.path.insert(0, root)
    import torch
    from attacking_federate_learning_amd.engine import get_engine

    eng = get_engine()
    for shape in args.shapes.split(','):
        print(json.dumps(one_shape(eng, torch, args, root, shape, tall=False)), flush=True)
        torch.cuda.empty_cache()
    for shape in args.tall_shapes.split(','):
        print(json.dumps(one_shape(eng, torch, args, root, shape, tall=True)), flush=True)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
