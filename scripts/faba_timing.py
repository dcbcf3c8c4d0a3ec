"""FABA timing on one MI355X.  Every figure of a run comes from ONE process:

    python scripts/faba_timing.py --write profiles/faba_timing.md          # the loop at n = 1000 / 4000 / 10,000, the whole call
                                                                           # at 1000 x 1e6 and 4000 x 1e7, the note written
    python scripts/faba_timing.py --n 4000 --d 10000000                    # the whole call at one size

The loop, per n, on the Euclidean matrix of n rows of 256 columns (N(0, 1), the first fifth shifted), r = n // 5, with device
events, the median of `--reps` calls after one warm-up call:
    select      byz_faba_select_dev: the initial sums (BYZ_K_ROW_SORT) and the one-workgroup loop (BYZ_K_MISC), each through the
                library's timers; `loop_us_per_step` = the loop kernel / r
    prim        byz_flame_select_dev on the same matrix (min_samples 1, min_cluster_size n / 2 + 1): its BYZ_K_MISC time is Prim's
                kernel alone, `prim_us_per_step` = that / (n - 1)
The whole call, per (n, d): byz_faba_dev with r = n // 5 beside byz_pairwise_distances_dev + byz_scaled_rows_sum_dev with the
same number of rows kept.  One JSON line per measurement.  `--resources FILE`: the compiler's resource report of faba.hip
(hipcc -Rpass-analysis=kernel-resource-usage), quoted in the note."""
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


def shifted(torch, device, n, d, seed):
    gen = torch.Generator(device=device).manual_seed(seed)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    mu = torch.empty(d, dtype=torch.float32, device=device).normal_(generator=gen)
    for r0 in range(0, n, 50):                             # (in row blocks: the largest matrix is 160 GB)
        g[r0:r0 + 50].normal_(generator=gen)
    for r0 in range(0, n // 5, 50):
        g[r0:min(r0 + 50, n // 5)].add_(0.5 * mu)
    return g


def slots_of(eng, torch, call):
    eng.timing(True)
    call()
    torch.cuda.synchronize()
    slots = eng.timing_read()
    eng.timing(False)
    return {k: v.get('total_ms', 0.0) for k, v in slots.items() if v.get('total_ms', 0.0) > 0}


def stage(args, eng, torch, n):
    from attacking_federate_learning_amd.engine import _check, _vp
    device = 'cuda:%d' % eng.device
    g = shifted(torch, device, n, 256, n)
    dist = torch.empty((n, n), dtype=torch.float32, device=device)
    flags = torch.empty(n, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(g.device).cuda_stream
    _check(eng.lib.byz_pairwise_distances_dev(eng.ctx, _vp(g.data_ptr()), n, 256, g.stride(0), _vp(dist.data_ptr()), _vp(stream)))
    torch.cuda.synchronize()
    r = n // 5

    def select():
        _check(eng.lib.byz_faba_select_dev(eng.ctx, _vp(dist.data_ptr()), n, r, 2, _vp(flags.data_ptr()), None, _vp(stream)))

    def flame():
        _check(eng.lib.byz_flame_select_dev(eng.ctx, _vp(dist.data_ptr()), n, n // 2 + 1, 1, _vp(flags.data_ptr()), _vp(stream)))
    line = {'stage': True, 'n': n, 'r': r, 'reps': args.reps}
    line['select_ms'] = round(timed(torch, select, args.reps), 3)
    info = eng.faba_info()
    line['removed'], line['shifted_rows_kept'] = info['removed'], int(flags[:n // 5].sum().item())
    loops, inits, prims = [], [], []
    for _ in range(args.reps):
        s = slots_of(eng, torch, select)
        loops.append(s.get('misc', float('nan')))
        inits.append(s.get('row_sort', float('nan')))
        prims.append(slots_of(eng, torch, flame).get('misc', float('nan')))
    line['init_ms'] = round(statistics.median(inits), 4)
    line['loop_ms'] = round(statistics.median(loops), 4)
    line['loop_us_per_step'] = round(1e3 * statistics.median(loops) / r, 3)
    line['prim_ms'] = round(statistics.median(prims), 4)
    line['prim_us_per_step'] = round(1e3 * statistics.median(prims) / (n - 1), 3)
    line['step_over_prim_step'] = round(line['loop_us_per_step'] / line['prim_us_per_step'], 3)
    print(json.dumps(line), flush=True)
    return line


def whole(args, eng, torch, n, d):
    from attacking_federate_learning_amd.engine import _check, _vp
    device = 'cuda:%d' % eng.device
    g = shifted(torch, device, n, d, n + 1)
    out = torch.empty(d, dtype=torch.float32, device=device)
    dist = torch.empty((n, n), dtype=torch.float32, device=device)
    flags = torch.empty(n, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(g.device).cuda_stream
    r = n // 5
    weights = torch.ones(n, dtype=torch.float64, device=device)
    weights[:r] = 0.0                                       # the same number of rows kept
    count = torch.tensor([float(n - r)], dtype=torch.float64, device=device)

    def faba():
        _check(eng.lib.byz_faba_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), r, None, _vp(out.data_ptr()), _vp(flags.data_ptr()),
                                    None, _vp(stream)))

    def pieces():
        _check(eng.lib.byz_pairwise_distances_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), _vp(dist.data_ptr()), _vp(stream)))
        _check(eng.lib.byz_scaled_rows_sum_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), _vp(weights.data_ptr()),
                                               _vp(count.data_ptr()), _vp(out.data_ptr()), _vp(stream)))
    line = {'whole': True, 'n': n, 'd': d, 'r': r, 'reps': args.reps}
    line['faba_ms'] = round(timed(torch, faba, args.reps), 3)
    line['kept'], line['shifted_rows_kept'] = int(flags.sum().item()), int(flags[:n // 5].sum().item())
    line['slots_ms'] = {k: round(v, 3) for k, v in slots_of(eng, torch, faba).items()}
    line['distances_and_sum_ms'] = round(timed(torch, pieces, args.reps), 3)
    line['faba_over_pieces'] = round(line['faba_ms'] / line['distances_and_sum_ms'], 4)
    print(json.dumps(line), flush=True)
    del g, out
    torch.cuda.empty_cache()
    return line


def note(stages, wholes, resources):
    met = lambda ok: 'met' if ok else 'missed'     # noqa: E731
    text = ['# FABA: the removal loop and the whole call', '',
            'Written by `scripts/faba_timing.py`: one process on one MI355X, device events, the median of the repetitions after a',
            'warm-up call; the kernels through the library\'s timers (`BYZ_K_ROW_SORT`: the initial sums, `BYZ_K_MISC`: the loop;',
            'FLAME\'s `BYZ_K_MISC` is Prim\'s kernel alone).  Recorded, not gated.', '',
            '## The loop per step, beside Prim\'s step on the same matrix (r = n // 5; expected: within 1.5 times)', '',
            '| n | r | select ms | initial sums ms | loop ms | loop us / step | Prim ms | Prim us / step | ratio | within 1.5 |',
            '|---|---|---|---|---|---|---|---|---|---|']
    for s in stages:
        text.append('| %d | %d | %.3f | %.4f | %.4f | %.3f | %.4f | %.3f | %.3f | %s |' % (
            s['n'], s['r'], s['select_ms'], s['init_ms'], s['loop_ms'], s['loop_us_per_step'], s['prim_ms'], s['prim_us_per_step'],
            s['step_over_prim_step'], met(s['step_over_prim_step'] <= 1.5)))
    text += ['', '## The whole call beside `pairwise_distances` + `scaled_rows_sum` of the same kept count', '',
             '| n x d | r | faba ms | distances + sum ms | faba / pieces | selection adds | timers of one call (ms) |', '|---|---|---|---|---|---|---|']
    for w in wholes:
        text.append('| %d x %d | %d | %.3f | %.3f | %.4f | %.2f %% | %s |' % (
            w['n'], w['d'], w['r'], w['faba_ms'], w['distances_and_sum_ms'], w['faba_over_pieces'], 100.0 * (w['faba_over_pieces'] - 1.0),
            ', '.join('%s %.3f' % kv for kv in sorted(w['slots_ms'].items()))))
    big = [w for w in wholes if w['n'] == 4000]
    if big:
        text += ['', 'Expected at 4000 x 1e7: the selection adds less than 5 %%: %s.' % met(big[0]['faba_over_pieces'] < 1.05)]
    text += ['', '## The compiler\'s resource report (gfx950)', '', '```', resources.strip() or 'not collected', '```', '']
    return '\n'.join(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=0)
    ap.add_argument('--d', type=int, default=0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--write', default='')
    ap.add_argument('--resources', default='')
    ap.add_argument('--skip-large', action='store_true')
    args = ap.parse_args()
    import torch
    from attacking_federate_learning_amd.engine import get_engine
    eng = get_engine()
    if args.n:
        whole(args, eng, torch, args.n, args.d)
        return
    stages = [stage(args, eng, torch, n) for n in (1000, 4000, 10000)]
    wholes = [whole(args, eng, torch, 1000, 1000000)]
    if not args.skip_large:
        wholes.append(whole(args, eng, torch, 4000, 10000000))
    if args.write:
        resources = open(args.resources).read() if args.resources else ''
        with open(args.write, 'w') as fh:
            fh.write(note(stages, wholes, resources))


if __name__ == '__main__':
    main()
