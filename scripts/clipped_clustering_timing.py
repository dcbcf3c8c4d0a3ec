"""ClippedClustering timing on one MI355X.  Every figure of a run comes from ONE process:

    python scripts/clipped_clustering_timing.py                  # the stage at n = 1000 / 4000 / 10,000, the whole call at 1000 x 1e6
    python scripts/clipped_clustering_timing.py --n 4000 --d 10000000          # the whole call at one size

The stage, per n, on the cosine matrix of n rows of 256 columns with a planted quarter pointing the other way, with device
events, the median of `--reps` calls after one warm-up call:
    select      byz_clipped_clustering_select_dev (average linkage): the working copy, the first caches, the linkage, the cut, the
                pick; `linkage_ms` is the one-workgroup kernel alone and `prepare_cut_ms` the rest, through the library's timers
                (BYZ_K_MISC and BYZ_K_ROW_SORT of one call)
    flame       byz_flame_select_dev on the same matrix (min_samples 1, min_cluster_size n / 2 + 1): FLAME's cluster stage
    scipy       scipy.cluster.hierarchy.linkage(method='average') on the host, the copy of the matrix to the host included
and the rescans of the nearest-partner caches per step, mean and maximum, from byz_linkage_info.
The whole call, per (n, d): byz_clipped_clustering_dev beside byz_flame_dev with lambda = 0.  One JSON line per measurement."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

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


def planted(torch, device, n, d, seed):
    gen = torch.Generator(device=device).manual_seed(seed)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    mu = torch.empty(d, dtype=torch.float32, device=device).normal_(generator=gen)
    for r0 in range(0, n, 50):                             # (in row blocks: the largest matrix is 160 GB)
        blk = g[r0:r0 + 50]
        blk.normal_(generator=gen)
        blk.add_(mu)
    f = n // 4
    g[:f] = g[:f] * 0.1 - 4.0 * mu
    return g, f


def stage(args, eng, torch, n):
    from attacking_federate_learning_amd.engine import _check, _vp
    device = 'cuda:%d' % eng.device
    g, f = planted(torch, device, n, 256, n)
    dist = torch.empty((n, n), dtype=torch.float32, device=device)
    flags = torch.empty(n, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(g.device).cuda_stream
    _check(eng.lib.byz_cosine_distances_dev(eng.ctx, _vp(g.data_ptr()), n, 256, g.stride(0), _vp(dist.data_ptr()), _vp(stream)))
    torch.cuda.synchronize()
    fill = ctypes.c_double(2.0)

    def select():
        _check(eng.lib.byz_clipped_clustering_select_dev(eng.ctx, _vp(dist.data_ptr()), n, 0, ctypes.byref(fill), _vp(flags.data_ptr()),
                                                         _vp(stream)))

    def flame():
        _check(eng.lib.byz_flame_select_dev(eng.ctx, _vp(dist.data_ptr()), n, n // 2 + 1, 1, _vp(flags.data_ptr()), _vp(stream)))
    line = {'stage': True, 'n': n, 'reps': args.reps}
    line['select_ms'] = round(timed(torch, select, args.reps), 3)
    info, cc = eng.linkage_info(), eng.clipped_clustering_info()
    line['attackers_admitted'] = int(flags[:f].sum().item())
    line['admitted'], line['merges'] = cc['admitted'], info['merges']
    line['rescans_per_step'] = round(info['rescans'] / max(info['merges'], 1), 3)
    line['max_rescans_in_a_step'] = info['max_rescans']
    eng.timing(True)
    select()
    torch.cuda.synchronize()
    slots = eng.timing_read()
    eng.timing(False)
    line['linkage_ms'] = round(slots.get('misc', {}).get('total_ms', float('nan')), 3)
    line['prepare_cut_ms'] = round(slots.get('row_sort', {}).get('total_ms', float('nan')), 3)
    line['linkage_us_per_step'] = round(1e3 * line['linkage_ms'] / max(info['merges'], 1), 3)
    line['flame_ms'] = round(timed(torch, flame, args.reps), 3)
    line['select_over_flame'] = round(line['select_ms'] / line['flame_ms'], 2)
    if not args.no_scipy:
        from scipy.cluster.hierarchy import linkage
        from scipy.spatial.distance import squareform
        import numpy as np
        t0 = time.perf_counter()
        host = dist.cpu().numpy().astype(np.float64)
        np.fill_diagonal(host, 0.0)
        linkage(squareform(host, checks=False), method='average')
        line['scipy_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        line['scipy_over_select'] = round(line['scipy_ms'] / line['select_ms'], 1)
    print(json.dumps(line), flush=True)


def whole(args, eng, torch, n, d):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    device = 'cuda:%d' % eng.device
    g, f = planted(torch, device, n, d, n + 1)
    out = torch.empty(d, dtype=torch.float32, device=device)
    flags = torch.empty(n, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(g.device).cuda_stream
    cc = _native.ClippedClusteringParams(0.0, 1, 0, 2.0)
    fl = _native.FlameParams(0.0, 1, 0, 0, 0, 0)

    def clipped_clustering():
        _check(eng.lib.byz_clipped_clustering_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), ctypes.byref(cc), None, None,
                                                  _vp(out.data_ptr()), _vp(flags.data_ptr()), _vp(stream)))

    def flame():
        _check(eng.lib.byz_flame_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), ctypes.byref(fl), None, _vp(out.data_ptr()),
                                     _vp(flags.data_ptr()), _vp(stream)))
    line = {'whole': True, 'n': n, 'd': d, 'reps': args.reps}
    line['clipped_clustering_ms'] = round(timed(torch, clipped_clustering, args.reps), 3)
    line['attackers_admitted'], line['admitted'] = int(flags[:f].sum().item()), int(flags.sum().item())
    eng.timing(True)
    clipped_clustering()
    torch.cuda.synchronize()
    slots = eng.timing_read()
    eng.timing(False)
    line['slots_ms'] = {k: round(v.get('total_ms', 0.0), 3) for k, v in slots.items() if v.get('total_ms', 0.0) > 0}
    line['flame_lam0_ms'] = round(timed(torch, flame, args.reps), 3)
    line['whole_over_flame'] = round(line['clipped_clustering_ms'] / line['flame_lam0_ms'], 3)
    print(json.dumps(line), flush=True)
    del g, out
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=0)
    ap.add_argument('--d', type=int, default=0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-scipy', action='store_true')
    args = ap.parse_args()
    import torch
    from attacking_federate_learning_amd.engine import get_engine
    eng = get_engine()
    if args.n:
        whole(args, eng, torch, args.n, args.d)
    else:
        for n in (1000, 4000, 10000):
            stage(args, eng, torch, n)
        whole(args, eng, torch, 1000, 1000000)


if __name__ == '__main__':
    main()
