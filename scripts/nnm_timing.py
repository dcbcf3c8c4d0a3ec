"""Nearest-neighbour mixing timing on one MI355X: the neighbour step and the mix beside their two yardsticks.

    python scripts/nnm_timing.py --n 1000 --d 1000000
    python scripts/nnm_timing.py --n 4000 --d 250000

The neighbour step (keys, sort, take: BYZ_K_ROW_SORT) and the mix (mask and MFMA kernel: BYZ_K_MISC) are timed by the
library's own per-kernel events (byz_timing_*) over `--steps` calls after `--warmup`.  Yardstick (a) is what the library
offered before: n calls of byz_mean_rows_dev on the same lists, enqueued back to back and bracketed by one pair of device
events per step, in the same process on the same matrix.  Yardstick (b) is 2 n^2 d flops at the fp32 matrix peak, 157.3 TF.
One JSON line.
"""
import argparse
import json
import os
import sys

PEAK_F32_MATRIX = 157.3e12


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=1000)
    p.add_argument('--d', type=int, default=1_000_000)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from attacking_federate_learning_amd.engine import _check, _vp, get_engine

    n, d = args.n, args.d
    f = int(n * 0.24)
    k = n - f
    eng = get_engine()
    device = torch.device('cuda', eng.device)
    gen = torch.Generator(device=device).manual_seed(n + d)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    g.normal_(generator=gen)
    g.mul_(torch.linspace(1.0, 1.5, n, device=device)[torch.randperm(n, device=device, generator=gen)][:, None])
    if f:
        g[:f] = g[0]
    y = torch.empty_like(g)
    dist = eng.pairwise_distances(g)
    nbr, counts = eng.nnm_neighbours(dist, k)
    stream = torch.cuda.current_stream(device).cuda_stream
    gp, yp = _vp(g.data_ptr()), _vp(y.data_ptr())

    def neighbours():
        _check(eng.lib.byz_nnm_neighbours_dev(eng.ctx, _vp(dist.ptr), n, k, _vp(nbr.ptr), _vp(counts.ptr), _vp(stream)))

    def mix():
        _check(eng.lib.byz_nnm_mix_dev(eng.ctx, gp, n, d, d, _vp(nbr.ptr), _vp(counts.ptr), k, yp, d, _vp(stream)))

    for _ in range(args.warmup):
        neighbours()
        mix()
    eng.synchronize(stream)
    eng.timing(True)
    for _ in range(args.steps):
        neighbours()
        mix()
    eng.synchronize(stream)
    timers = eng.timing_read()
    eng.timing(False)
    mix_ms = timers['misc']['total_ms'] / args.steps
    nbr_ms = timers['row_sort']['total_ms'] / args.steps

    # (a) n calls of byz_mean_rows_dev on the same lists; row i of the result into row i of y
    nbr_ptr = int(nbr.ptr)

    def mean_rows_step():
        for i in range(n):
            _check(eng.lib.byz_mean_rows_dev(eng.ctx, gp, n, d, d, _vp(nbr_ptr + 4 * i * k), k, _vp(y.data_ptr() + 4 * i * d),
                                             _vp(stream)))

    for _ in range(min(args.warmup, 1)):
        mean_rows_step()
    torch.cuda.synchronize(device)
    events = []
    for _ in range(args.steps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        mean_rows_step()
        stop.record()
        events.append((start, stop))
    torch.cuda.synchronize(device)
    rows_ms = sum(a.elapsed_time(b) for a, b in events) / args.steps
    roof_ms = 2.0 * n * n * d / PEAK_F32_MATRIX * 1e3
    print(json.dumps({'n': n, 'd': d, 'f': f, 'k': k, 'steps': args.steps, 'warmup': args.warmup,
                      'neighbours_ms': round(nbr_ms, 4), 'mix_ms': round(mix_ms, 4),
                      'mean_rows_n_calls_ms': round(rows_ms, 3), 'mix_speedup_over_mean_rows': round(rows_ms / mix_ms, 2),
                      'matrix_roof_ms': round(roof_ms, 4), 'mix_fraction_of_matrix_roof': round(roof_ms / mix_ms, 4)}), flush=True)


if __name__ == '__main__':
    main()
