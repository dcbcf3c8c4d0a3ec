"""Multi-Metrics timing on one MI355X.  Every figure of a run comes from ONE process:

    python scripts/multi_metrics_timing.py                       # 1000 x 1e6 (with torch.cdist, p = 1) and 4000 x 1e7
    python scripts/multi_metrics_timing.py --n 1000 --d 1000000 --cdist

Per size, with device events, the median of `--reps` calls after one warm-up call:
    manhattan   byz_manhattan_distances_dev; its tile kernel alone through the library's timers is `tile_ms` (BYZ_K_DISTANCES of
                a byz_manhattan_sums_dev call minus nothing else: the reduction over the chunks is in it and is n^2 work)
    pairwise    byz_pairwise_distances_dev on the same matrix
    whole       byz_multi_metrics_dev
    cdist       torch.cdist(g, g, p=1), the only route to the L1 matrix before (one call: it is slow)
and the vector-issue floor n (n - 1) d / (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz) for 2 instructions per pair-element, scaled by
`--instructions` / 2 for the count read from the build's disassembly (1.5: one packed subtraction per two terms and one
addition with |.| per term).  One JSON line per size."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, call, reps):
    call()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(stop))
    return statistics.median(out)


def run(args, eng, torch, n, d, with_cdist):
    from attacking_federate_learning_amd.engine import _check, _vp
    device = 'cuda:%d' % eng.device
    gen = torch.Generator(device=device).manual_seed(n)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    mu = torch.empty(d, dtype=torch.float32, device=device).normal_(generator=gen)
    for r0 in range(0, n, 50):                             # (in row blocks: the largest matrix is 160 GB)
        blk = g[r0:r0 + 50]
        blk.normal_(generator=gen)
        blk.mul_(0.5).add_(mu)
    f = n // 4
    g[n - f:] *= -1.0
    dist = torch.empty((n, n), dtype=torch.float32, device=device)
    sums = torch.empty((n, n), dtype=torch.float64, device=device)
    out = torch.empty(d, dtype=torch.float32, device=device)
    flags = torch.empty(n, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(g.device).cuda_stream
    keep = int(0.3 * n)

    def manhattan():
        _check(eng.lib.byz_manhattan_distances_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), _vp(dist.data_ptr()), _vp(stream)))

    def manhattan_sums():
        _check(eng.lib.byz_manhattan_sums_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), _vp(sums.data_ptr()), _vp(stream)))

    def pairwise():
        _check(eng.lib.byz_pairwise_distances_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), _vp(dist.data_ptr()), _vp(stream)))

    def whole():
        _check(eng.lib.byz_multi_metrics_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), keep, _vp(out.data_ptr()),
                                             _vp(flags.data_ptr()), _vp(stream)))
    floor2 = n * (n - 1) * d / (256 * 4 * 16 * 2.4e9) * 1e3
    line = {'n': n, 'd': d, 'reps': args.reps, 'floor_2_instructions_ms': round(floor2, 3),
            'instructions_per_pair_element': args.instructions, 'floor_ms': round(floor2 * args.instructions / 2.0, 3)}
    line['manhattan_ms'] = round(timed(torch, manhattan, args.reps), 3)
    manhattan_sums()
    torch.cuda.synchronize()
    eng.timing(True)
    manhattan_sums()
    torch.cuda.synchronize()
    line['tile_and_reduce_ms'] = round(eng.timing_read().get('distances', {}).get('total_ms', float('nan')), 3)
    eng.timing(False)
    line['floor_over_manhattan'] = round(line['floor_ms'] / line['manhattan_ms'], 3)
    line['floor_2_over_manhattan'] = round(floor2 / line['manhattan_ms'], 3)
    line['pairwise_ms'] = round(timed(torch, pairwise, args.reps), 3)
    line['whole_ms'] = round(timed(torch, whole, args.reps), 3)
    info = eng.multi_metrics_info()
    line['kept'], line['degenerate'], line['attackers_chosen'] = info['kept'], info['degenerate'], int(flags[n - f:].sum().item())
    if with_cdist:
        line['cdist_p1_ms'] = round(timed(torch, lambda: torch.cdist(g, g, p=1), 1), 3)
        line['cdist_over_manhattan'] = round(line['cdist_p1_ms'] / line['manhattan_ms'], 2)
    print(json.dumps(line), flush=True)
    del g, dist, sums, out
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=0)
    ap.add_argument('--d', type=int, default=0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--instructions', type=float, default=1.5)
    ap.add_argument('--cdist', action='store_true')
    args = ap.parse_args()
    import torch
    from attacking_federate_learning_amd.engine import get_engine
    eng = get_engine()
    if args.n:
        run(args, eng, torch, args.n, args.d, args.cdist)
    else:
        run(args, eng, torch, 1000, 1000000, True)
        run(args, eng, torch, 4000, 10000000, False)


if __name__ == '__main__':
    main()
