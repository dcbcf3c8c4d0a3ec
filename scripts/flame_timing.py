"""FLAME timing on one MI355X.  Every figure of a run comes from ONE process:

    python scripts/flame_timing.py                       # cluster stage at n = 1000, 4000, 10000; flame at 1000 x 1e6, 4000 x 1e7
    python scripts/flame_timing.py --mode cluster --n 4000
    python scripts/flame_timing.py --mode flame --n 1000 --d 1000000

cluster: the cosine conversion and `byz_flame_select_dev` on a synthetic n x n Gram (unit rows, an honest majority and a quarter
pointing the other way), read through the library's timers (`byz_timing_*`): distances = cosine_from_gram_kernel, row_sort = the
core distances, the edge sort and the admission, misc = Prim's one workgroup, whose time over n - 1 is the per-step figure.
Beside it Bulyan's selection loop (bulyan_loop, f = n // 4 - 1) on the same matrix at the same n: the other O(n) dependent chain
of the library.  Medians over `--rounds` rounds of `--steps` calls.

flame: `byz_flame_dev` beside its two existing parts, `byz_pairwise_distances_dev` and `byz_weak_dp_dev` (adaptive), alternating
in the same process with device events.  One JSON line per measurement.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sparsefed_timing import alternate, summarise  # noqa: E402


def read_timers(eng, calls, steps, rounds):
    """{timer: median ms per call} of `calls` (a dict name -> callable), each timed on its own."""
    out = {}
    for name, call in calls.items():
        samples = {}
        call()
        for _ in range(rounds):
            eng.timing(True)
            for _ in range(steps):
                call()
            for timer, rec in eng.timing_read().items():
                samples.setdefault(timer, []).append(rec['total_ms'] / steps)
            eng.timing(False)
        out[name] = {timer: round(statistics.median(ms), 4) for timer, ms in samples.items()}
    return out


def run_cluster(args, eng, torch, device, n):
    from attacking_federate_learning_amd.engine import _check, _vp
    gen = torch.Generator(device=device).manual_seed(n)
    d = 256
    mu = torch.empty(d, dtype=torch.float64, device=device).normal_(generator=gen)
    rows = mu + 0.3 * torch.empty((n, d), dtype=torch.float64, device=device).normal_(generator=gen)
    rows[:n // 4] = -3.0 * mu + 0.3 * torch.empty((n // 4, d), dtype=torch.float64, device=device).normal_(generator=gen)
    gram = (rows @ rows.T).contiguous()
    dist = torch.empty((n, n), dtype=torch.float32, device=device)
    flags = torch.empty(n, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    m = n // 2 + 1

    def cosine():
        _check(eng.lib.byz_cosine_from_gram_dev(eng.ctx, _vp(gram.data_ptr()), n, _vp(dist.data_ptr()), _vp(stream)))

    def select(ms):
        return lambda: _check(eng.lib.byz_flame_select_dev(eng.ctx, _vp(dist.data_ptr()), n, m, ms, _vp(flags.data_ptr()), _vp(stream)))
    cosine()
    select(1)()
    info = eng.flame_info()
    attackers = int(flags[:n // 4].sum().item())
    timers = read_timers(eng, {'cosine': cosine, 'select_ms1': select(1), 'select_ms5': select(5)}, args.steps, args.rounds)
    line = {'mode': 'cluster', 'n': n, 'steps': args.steps, 'rounds': args.rounds, 'admitted': info['admitted'],
            'attackers_admitted': attackers, 'w_star': round(info['w_star'], 6)}
    line['cosine_ms'] = timers['cosine'].get('distances')
    for name in ('select_ms1', 'select_ms5'):
        line[name + '_core_sort_admit_ms'] = timers[name].get('row_sort')
        line[name + '_prim_ms'] = timers[name].get('misc')
    line['prim_us_per_step'] = round(1e3 * line['select_ms1_prim_ms'] / (n - 1), 3)
    line['cluster_stage_ms'] = round(line['cosine_ms'] + line['select_ms1_core_sort_admit_ms'] + line['select_ms1_prim_ms'], 4)
    # Bulyan's selection loop on the same matrix, the same n
    from attacking_federate_learning_amd.engine import Distances

    class Held:
        ptr = dist.data_ptr()
    f = n // 4 - 1
    handle = Distances(Held(), n)
    bulyan = read_timers(eng, {'bulyan': lambda: eng.bulyan_select(handle, n, f, on_device=True)}, max(1, args.steps // 2), args.rounds)
    line['bulyan_loop_ms'] = bulyan['bulyan'].get('bulyan_loop')
    line['bulyan_row_sort_ms'] = bulyan['bulyan'].get('row_sort')
    line['cluster_vs_bulyan_loop'] = round(line['cluster_stage_ms'] / line['bulyan_loop_ms'], 3)
    return line


def run_flame(args, eng, torch, device, n, d, steps, warmup, rounds):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    gen = torch.Generator(device=device).manual_seed(n + d)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    g.normal_(generator=gen)
    g.mul_(0.3)
    mu = torch.empty(d, dtype=torch.float32, device=device).normal_(generator=gen)
    g.add_(mu)
    g[:n // 4].sub_(4.0 * mu)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(device).cuda_stream
    out = torch.empty(d, dtype=torch.float32, device=device)
    dist = torch.empty((n, n), dtype=torch.float32, device=device)
    fp = _native.FlameParams(0.001, 1, 0, 2022, 3, 0)
    wp = _native.WeakDpParams(0.0, 0.001, 1, 2022, 3, 0)
    calls = {
        'pairwise_distances': lambda: _check(eng.lib.byz_pairwise_distances_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(dist.data_ptr()),
                                                                                _vp(stream))),
        'weak_dp_adaptive': lambda: _check(eng.lib.byz_weak_dp_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, ctypes.byref(wp), _vp(out.data_ptr()),
                                                                   _vp(stream))),
        'flame': lambda: _check(eng.lib.byz_flame_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, ctypes.byref(fp), None, _vp(out.data_ptr()), None,
                                                      _vp(stream))),
    }
    calls['flame']()
    line = {'mode': 'flame', 'n': n, 'd': d, 'steps': steps, 'warmup': warmup, 'rounds': rounds, 'info': eng.flame_info()}
    summarise(line, alternate(calls, steps, warmup, rounds))
    line['flame_minus_parts_ms'] = round(line['flame_ms'] - line['pairwise_distances_ms'] - line['weak_dp_adaptive_ms'], 4)
    del g
    torch.cuda.empty_cache()
    return line


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', default='all', choices=['all', 'cluster', 'flame'])
    p.add_argument('--n', type=int, default=1000)
    p.add_argument('--d', type=int, default=1_000_000)
    p.add_argument('--steps', type=int, default=4)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from attacking_federate_learning_amd.engine import get_engine
    eng = get_engine()
    device = torch.device('cuda', eng.device)
    if args.mode == 'cluster':
        runs = [lambda: run_cluster(args, eng, torch, device, args.n)]
    elif args.mode == 'flame':
        runs = [lambda: run_flame(args, eng, torch, device, args.n, args.d, args.steps, args.warmup, args.rounds)]
    else:
        runs = [lambda n=n: run_cluster(args, eng, torch, device, n) for n in (1000, 4000, 10000)]
        runs += [lambda: run_flame(args, eng, torch, device, 1000, 1_000_000, args.steps, args.warmup, args.rounds),
                 lambda: run_flame(args, eng, torch, device, 4000, 10_000_000, 2, 1, 3)]
    for run in runs:
        print(json.dumps(run()), flush=True)


if __name__ == '__main__':
    main()
