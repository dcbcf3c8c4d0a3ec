"""AFA timing on one MI355X.  Every figure of a run comes from ONE process:

    python scripts/afa_timing.py --write profiles/afa_timing.md           # the selection at n = 1000 / 4000 / 10,000, the whole
                                                                          # call at 1000 x 1e6 and 4000 x 1e7, the note written
    python scripts/afa_timing.py --n 4000 --d 10000000                    # the whole call at one size

The selection, per n, on the fp64 Gram of the drift-attack matrix (n rows of 2048 columns, honest rows mu + N(0, 1) with mu ~
0.2 N(0, 1), the first n // 4 rows ONE vector, the honest mean minus one standard deviation), so that the first round removes
about n / 4 rows at once; device events, the median of `--reps` calls after one warm-up call:
    select      byz_afa_select_dev: the usable rows and the initial u (BYZ_K_ROW_SORT) and the one-workgroup loop (BYZ_K_MISC),
                each through the library's timers
    one round   the same with max_rounds = 1: the loop kernel then runs one round's statistics and median and no update, which
                is a round net of removals; `us_per_removed_row` = (loop - rounds x one round) / rows removed
    faba        byz_faba_select_dev on the Euclidean distances of the same matrix with remove_count = the rows AFA removed:
                its loop (BYZ_K_MISC) per step
The whole call, per (n, d): byz_afa_dev beside byz_gram_dev + byz_scaled_rows_sum_dev with the same number of rows kept.  The
device Gram's error against numpy's on the tests' planted matrices is measured too.  One JSON line per measurement.
`--resources FILE`: the compiler's resource report of afa.hip (hipcc -Rpass-analysis=kernel-resource-usage), quoted in the note."""
import argparse
import ctypes
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


def drift_matrix(torch, device, n, d, seed):
    gen = torch.Generator(device=device).manual_seed(seed)
    f = n // 4
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    mu = torch.empty(d, dtype=torch.float32, device=device).normal_(generator=gen).mul_(0.2)
    total = torch.zeros(d, dtype=torch.float64, device=device)
    square = torch.zeros(d, dtype=torch.float64, device=device)
    for r0 in range(f, n, 50):                             # (in row blocks: the largest matrix is 160 GB)
        block = g[r0:min(r0 + 50, n)]
        block.normal_(generator=gen).add_(mu)
        total += block.sum(dim=0, dtype=torch.float64)
        square += (block.to(torch.float64) ** 2).sum(dim=0)
    mean = total / (n - f)
    std = (square / (n - f) - mean * mean).clamp_min(0).sqrt()
    g[:f] = (mean - std).to(torch.float32)
    return g


def slots_of(eng, torch, call):
    eng.timing(True)
    call()
    torch.cuda.synchronize()
    slots = eng.timing_read()
    eng.timing(False)
    return {k: v.get('total_ms', 0.0) for k, v in slots.items() if v.get('total_ms', 0.0) > 0}


def stage(args, eng, torch, n):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    device = 'cuda:%d' % eng.device
    g = drift_matrix(torch, device, n, 2048, n)
    gram = eng.gram(g)
    dist = torch.empty((n, n), dtype=torch.float32, device=device)
    flags = torch.empty(n, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(g.device).cuda_stream
    _check(eng.lib.byz_pairwise_distances_dev(eng.ctx, _vp(g.data_ptr()), n, 2048, g.stride(0), _vp(dist.data_ptr()), _vp(stream)))
    torch.cuda.synchronize()
    full, single = _native.AfaParams(2.0, 0.5, 0), _native.AfaParams(2.0, 0.5, 1)

    def select(params=full):
        _check(eng.lib.byz_afa_select_dev(eng.ctx, _vp(gram.data_ptr()), n, None, ctypes.byref(params), _vp(flags.data_ptr()), None,
                                          None, _vp(stream)))
    line = {'stage': True, 'n': n, 'attackers': n // 4, 'reps': args.reps}
    line['select_ms'] = round(timed(torch, select, args.reps), 4)
    info = eng.afa_info()
    line.update(rounds=info['rounds'], removed=info['removed'], attackers_kept=int(flags[:n // 4].sum().item()))
    removed = max(info['removed'], 1)

    def faba():
        _check(eng.lib.byz_faba_select_dev(eng.ctx, _vp(dist.data_ptr()), n, removed, 2, _vp(flags.data_ptr()), None, _vp(stream)))
    line['faba_select_ms'] = round(timed(torch, faba, args.reps), 4)
    loops, inits, ones, fabas = [], [], [], []
    for _ in range(args.reps):
        s = slots_of(eng, torch, select)
        loops.append(s.get('misc', float('nan')))
        inits.append(s.get('row_sort', float('nan')))
        ones.append(slots_of(eng, torch, lambda: select(single)).get('misc', float('nan')))
        fabas.append(slots_of(eng, torch, faba).get('misc', float('nan')))
    loop, one, faba_loop = statistics.median(loops), statistics.median(ones), statistics.median(fabas)
    line['init_ms'] = round(statistics.median(inits), 4)
    line['loop_ms'] = round(loop, 4)
    line['one_round_ms'] = round(one, 4)
    line['select_us_per_removed_row'] = round(1e3 * line['select_ms'] / removed, 3)
    line['us_per_removed_row'] = round(1e3 * (loop - info['rounds'] * one) / removed, 3)
    line['faba_loop_ms'] = round(faba_loop, 4)
    line['faba_us_per_step'] = round(1e3 * faba_loop / removed, 3)
    line['select_over_faba_select'] = round(line['select_ms'] / line['faba_select_ms'], 3)
    line['row_over_faba_step'] = round(line['us_per_removed_row'] / line['faba_us_per_step'], 3)
    print(json.dumps(line), flush=True)
    return line


def whole(args, eng, torch, n, d):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    device = 'cuda:%d' % eng.device
    g = drift_matrix(torch, device, n, d, n + 1)
    out = torch.empty(d, dtype=torch.float32, device=device)
    gram = torch.empty((n, n), dtype=torch.float64, device=device)
    flags = torch.empty(n, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(g.device).cuda_stream
    params = _native.AfaParams(2.0, 0.5, 0)

    def afa():
        _check(eng.lib.byz_afa_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), None, ctypes.byref(params), None, _vp(out.data_ptr()),
                                   _vp(flags.data_ptr()), None, None, _vp(stream)))
    line = {'whole': True, 'n': n, 'd': d, 'reps': args.reps}
    line['afa_ms'] = round(timed(torch, afa, args.reps), 3)
    info = eng.afa_info()
    line.update(rounds=info['rounds'], kept=info['kept'], attackers_kept=int(flags[:n // 4].sum().item()))
    weights = flags.to(torch.float64)                      # the same rows kept
    count = weights.sum().reshape(1)

    def pieces():
        _check(eng.lib.byz_gram_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), _vp(gram.data_ptr()), _vp(stream)))
        _check(eng.lib.byz_scaled_rows_sum_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), _vp(weights.data_ptr()),
                                               _vp(count.data_ptr()), _vp(out.data_ptr()), _vp(stream)))
    line['slots_ms'] = {k: round(v, 3) for k, v in slots_of(eng, torch, afa).items()}
    line['gram_and_sum_ms'] = round(timed(torch, pieces, args.reps), 3)
    line['afa_over_pieces'] = round(line['afa_ms'] / line['gram_and_sum_ms'], 4)
    print(json.dumps(line), flush=True)
    del g, out
    torch.cuda.empty_cache()
    return line


def gram_errors(eng, torch):
    """max |C_dev - C_np| / sqrt(C_ii C_jj) on the planted matrices of tests/test_gpu_afa.py's whole calls"""
    import numpy as np
    from tests.test_afa import gram64, planted
    lines = []
    for n, d, kind, seed in ((65, 2000, 'drift', 0), (130, 777, 'drift', 1), (65, 2000, 'flip', 1), (130, 777, 'flip', 0)):
        g, _ = planted(n, d, kind, seed)
        c_dev = eng.gram(torch.from_numpy(g).to('cuda:%d' % eng.device)).cpu().numpy()
        c_np = gram64(g)
        norm = np.sqrt(np.diagonal(c_np))
        lines.append({'gram_error': True, 'n': n, 'd': d, 'kind': kind, 'seed': seed,
                      'error': float((np.abs(c_dev - c_np) / (norm[:, None] * norm[None, :])).max())})
        print(json.dumps(lines[-1]), flush=True)
    return lines


def note(stages, wholes, errors, resources):
    met = lambda ok: 'met' if ok else 'missed'     # noqa: E731
    text = ['# AFA: the selection and the whole call', '',
            'Written by `scripts/afa_timing.py`: one process on one MI355X, device events, the median of the repetitions after a',
            'warm-up call; the kernels through the library\'s timers (`BYZ_K_ROW_SORT`: the usable rows and the initial u,',
            '`BYZ_K_MISC`: the one-workgroup loop; FABA\'s `BYZ_K_MISC` is its loop).  Recorded, not gated.', '',
            '## The selection on the drift-attack Gram (n // 4 attackers), beside `faba_select` removing the same number of rows', '',
            'A round net of removals is the loop kernel with `max_rounds = 1`; a removed row costs (loop - rounds x that) / removed.',
            'Expected from the code: a removed row costs no more than a FABA step.', '',
            '| n | rounds | removed | attackers kept | select ms | initial u ms | loop ms | one round ms | us / removed row | select us / removed row '
            '| faba select ms | faba loop us / step | select / faba select | row / faba step | no more than a step |',
            '|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|']
    for s in stages:
        text.append('| %d | %d | %d | %d | %.4f | %.4f | %.4f | %.4f | %.3f | %.3f | %.4f | %.3f | %.3f | %.3f | %s |' % (
            s['n'], s['rounds'], s['removed'], s['attackers_kept'], s['select_ms'], s['init_ms'], s['loop_ms'], s['one_round_ms'],
            s['us_per_removed_row'], s['select_us_per_removed_row'], s['faba_select_ms'], s['faba_us_per_step'],
            s['select_over_faba_select'], s['row_over_faba_step'], met(s['row_over_faba_step'] <= 1.0)))
    text += ['', '## The whole call beside `gram` + `scaled_rows_sum` of the same kept rows', '',
             'Expected: the selection adds about what FABA\'s adds (0.9 ms at 1000 x 1e6, 0.3 % at 4000 x 1e7, `faba_timing.md`).', '',
             '| n x d | rounds | kept | attackers kept | afa ms | gram + sum ms | afa / pieces | selection adds | timers of one call (ms) |',
             '|---|---|---|---|---|---|---|---|---|']
    for w in wholes:
        text.append('| %d x %d | %d | %d | %d | %.3f | %.3f | %.4f | %.3f ms, %.2f %% | %s |' % (
            w['n'], w['d'], w['rounds'], w['kept'], w['attackers_kept'], w['afa_ms'], w['gram_and_sum_ms'], w['afa_over_pieces'],
            w['afa_ms'] - w['gram_and_sum_ms'], 100.0 * (w['afa_over_pieces'] - 1.0),
            ', '.join('%s %.3f' % kv for kv in sorted(w['slots_ms'].items()))))
    text += ['', '## The device Gram\'s error on the tests\' planted matrices', '',
             'max |C_dev - C_np| / sqrt(C_ii C_jj); `tests/test_gpu_afa.py` asserts it below 1e-5, a hundredth of the 1e-3 margin that',
             '`tests/test_afa.py` asserts of every decision.', '', '| n x d | planting | seed | error |', '|---|---|---|---|']
    for e in errors:
        text.append('| %d x %d | %s | %d | %.3g |' % (e['n'], e['d'], e['kind'], e['seed'], e['error']))
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
    errors = gram_errors(eng, torch)
    stages = [stage(args, eng, torch, n) for n in (1000, 4000, 10000)]
    wholes = [whole(args, eng, torch, 1000, 1000000)]
    if not args.skip_large:
        wholes.append(whole(args, eng, torch, 4000, 10000000))
    if args.write:
        resources = open(args.resources).read() if args.resources else ''
        with open(args.write, 'w') as fh:
            fh.write(note(stages, wholes, errors, resources))


if __name__ == '__main__':
    main()
