"""Auror timing on one MI355X.  Every figure of a run comes from ONE process:

    python scripts/auror_timing.py --write profiles/auror_timing.md        # 1000 x 1e6, 4000 x 2.5e5 and 10,000 x 1e5, the note written
    python scripts/auror_timing.py --n 4000 --d 250000                     # one size

Per (n, d), on 0.1 x N(0, 1) rows of which the first fifth has +0.5 on every tenth column, alpha = 0.3, with device events, the
median of `--reps` calls after one warm-up call:
    votes       byz_auror_votes_dev beside byz_coordinate_median_dev on the same matrix (an iteration does about the work of one
                radix pass, the median makes four passes, a Gaussian column takes 15 .. 29 sweeps: several times the median's time
                is expected);
    whole       byz_auror_dev beside byz_auror_votes_dev + byz_scaled_rows_sum_dev with the same rows kept: what the selection
                adds (expected: under 1 %).
The sweeps' histogram is of the first 2000 columns, from the numpy restatement in tests/test_auror.py.  One JSON line per
measurement.  `--resources FILE`: the compiler's resource report of auror.hip (hipcc -Rpass-analysis=kernel-resource-usage),
quoted in the note."""
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


def planted(torch, device, n, d, seed):
    gen = torch.Generator(device=device).manual_seed(seed)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    for r0 in range(0, n, 50):
        g[r0:r0 + 50].normal_(generator=gen)
    g.mul_(0.1)
    g[:n // 5, ::10] += 0.5
    return g


def measure(args, eng, torch, n, d):
    import numpy as np
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    from tests.test_auror import restated_auror_votes
    device = 'cuda:%d' % eng.device
    g = planted(torch, device, n, d, n)
    out = torch.empty(d, dtype=torch.float32, device=device)
    votes = torch.empty(n, dtype=torch.int64, device=device)
    bad = torch.empty(n, dtype=torch.int32, device=device)
    counts = torch.empty(4, dtype=torch.int64, device=device)
    kept = torch.empty(n, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(g.device).cuda_stream
    params = _native.AurorParams(0.3, 0.5, 32, 0)
    weights = torch.ones(n, dtype=torch.float64, device=device)
    weights[:n // 5] = 0.0
    count = torch.tensor([float(n - n // 5)], dtype=torch.float64, device=device)

    def auror_votes():
        _check(eng.lib.byz_auror_votes_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), ctypes.byref(params), _vp(votes.data_ptr()),
                                           _vp(bad.data_ptr()), _vp(counts.data_ptr()), None, _vp(stream)))

    def median():
        _check(eng.lib.byz_coordinate_median_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), None, _vp(out.data_ptr()), _vp(stream)))

    def auror():
        _check(eng.lib.byz_auror_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), ctypes.byref(params), None, None, None,
                                     _vp(out.data_ptr()), _vp(kept.data_ptr()), None, _vp(stream)))

    def pieces():
        auror_votes()
        _check(eng.lib.byz_scaled_rows_sum_dev(eng.ctx, _vp(g.data_ptr()), n, d, g.stride(0), _vp(weights.data_ptr()),
                                               _vp(count.data_ptr()), _vp(out.data_ptr()), _vp(stream)))
    line = {'n': n, 'd': d, 'reps': args.reps}
    line['votes_ms'] = round(timed(torch, auror_votes, args.reps), 3)
    line['median_ms'] = round(timed(torch, median, args.reps), 3)
    line['votes_over_median'] = round(line['votes_ms'] / line['median_ms'], 3)
    line['auror_ms'] = round(timed(torch, auror, args.reps), 3)
    line['removed'], line['indicative'] = n - int(kept.sum().item()), int(counts[0].item())
    line['votes_and_sum_ms'] = round(timed(torch, pieces, args.reps), 3)
    line['auror_over_pieces'] = round(line['auror_ms'] / line['votes_and_sum_ms'], 4)
    sweeps = restated_auror_votes(g[:, :2000].cpu().numpy(), 0.3)['sweeps']
    line['sweeps_histogram'] = {int(k): int(v) for k, v in zip(*np.unique(sweeps, return_counts=True))}
    print(json.dumps(line), flush=True)
    del g, out
    torch.cuda.empty_cache()
    return line


def note(lines, resources):
    text = ['# Auror: the votes beside the coordinate-wise median, and the whole call', '',
            'Written by `scripts/auror_timing.py`: one process on one MI355X, device events, the median of the repetitions after a',
            'warm-up call.  0.1 x N(0, 1) rows, the first fifth with +0.5 on every tenth column, alpha = 0.3, max_iter = 32.',
            'Recorded, not gated.', '',
            '| n x d | votes ms | median ms | votes / median | auror ms | votes + sum ms | auror / pieces | selection adds | removed | indicative |',
            '|---|---|---|---|---|---|---|---|---|---|']
    for w in lines:
        text.append('| %d x %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.4f | %.2f %% | %d | %d |' % (
            w['n'], w['d'], w['votes_ms'], w['median_ms'], w['votes_over_median'], w['auror_ms'], w['votes_and_sum_ms'],
            w['auror_over_pieces'], 100.0 * (w['auror_over_pieces'] - 1.0), w['removed'], w['indicative']))
    text += ['', '## Sweeps a column (the first 2000 columns, `tests/test_auror.py`\'s restatement)', '']
    for w in lines:
        text.append('- %d rows: %s' % (w['n'], ', '.join('%d: %d' % kv for kv in sorted(w['sweeps_histogram'].items()))))
    text += ['', '## The compiler\'s resource report (gfx950)', '', '```', resources.strip() or 'not collected', '```', '']
    return '\n'.join(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=0)
    ap.add_argument('--d', type=int, default=0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--write', default='')
    ap.add_argument('--resources', default='')
    args = ap.parse_args()
    import torch
    from attacking_federate_learning_amd.engine import get_engine
    eng = get_engine()
    if args.n:
        measure(args, eng, torch, args.n, args.d)
        return
    lines = [measure(args, eng, torch, n, d) for n, d in ((1000, 1000000), (4000, 250000), (10000, 100000))]
    if args.write:
        resources = open(args.resources).read() if args.resources else ''
        with open(args.write, 'w') as fh:
            fh.write(note(lines, resources))


if __name__ == '__main__':
    main()
