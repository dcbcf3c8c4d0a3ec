"""FoolsGold timing on one MI355X.  Every figure of a run comes from ONE process:

    python scripts/foolsgold_timing.py --write profiles/foolsgold_timing.md     # everything below, the note written
    python scripts/foolsgold_timing.py --skip-large                             # without the 4000 x 1e7 matrix (160 GB)

Device events, the median of `--reps` calls after one warm-up call.
    rows_add    byz_rows_add_dev at 1000 x 1e6 and 4000 x 1e6, both operands 16-byte aligned and with the window one column into
                a matrix of one more column (the mixed path), beside a device-to-device copy (torch's contiguous copy_, a
                hipMemcpyAsync) of the same n x w floats.  It moves 3 bytes where the copy moves 2: 1.5 times the copy's time is
                expected, with 15 % over that for the second read stream.
    weights     byz_foolsgold_weights_dev (four launches) at n = 1000 / 4000 / 10,000 on the drift-attack Gram of
                scripts/afa_timing.py, beside byz_afa_select_dev on the same Gram.  Expected: below afa_select at 4000 and 10,000.
    whole       byz_foolsgold_dev with a full-width history at 1000 x 1e6 beside byz_rows_add_dev + byz_gram_dev (of the history)
                + byz_scaled_rows_sum_dev timed singly; at 4000 x 1e7 with a 1e6-column window, and byz_afa_dev beside it.
                Expected: within 5 % of the pieces' sum.
    logit       the worst |l_dev - l_ref| over the graded Grams of tests/test_gpu_foolsgold.py, in units of 2^-53.
One JSON line per measurement.  `--resources FILE`: the compiler's resource report of foolsgold.hip (hipcc
-Rpass-analysis=kernel-resource-usage), quoted in the note."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from afa_timing import drift_matrix, slots_of, timed      # noqa: E402  (the same matrix, the same clock)


def rows_add(args, eng, torch, n, w, misaligned):
    from attacking_federate_learning_amd.engine import _check, _vp
    device = 'cuda:%d' % eng.device
    d = w + 1 if misaligned else w
    g = torch.empty((n, d), dtype=torch.float32, device=device).normal_()
    h = torch.zeros((n, w), dtype=torch.float32, device=device)
    dst = torch.empty((n, w), dtype=torch.float32, device=device)
    src = g.reshape(-1)[:n * w].view(n, w)
    stream = torch.cuda.current_stream(g.device).cuda_stream
    start = 1 if misaligned else 0

    def add():
        _check(eng.lib.byz_rows_add_dev(eng.ctx, _vp(h.data_ptr()), w, _vp(g.data_ptr()), n, w, d, start, _vp(stream)))
    line = {'rows_add': True, 'n': n, 'w': w, 'misaligned': misaligned, 'reps': args.reps}
    line['rows_add_ms'] = round(timed(torch, add, args.reps), 4)
    line['copy_ms'] = round(timed(torch, lambda: dst.copy_(src), args.reps), 4)
    line['ratio'] = round(line['rows_add_ms'] / line['copy_ms'], 3)
    line['gbytes_per_s'] = round(3 * 4 * n * w / line['rows_add_ms'] / 1e6, 1)
    print(json.dumps(line), flush=True)
    del g, h, dst, src
    torch.cuda.empty_cache()
    return line


def weights_stage(args, eng, torch, n):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    device = 'cuda:%d' % eng.device
    g = drift_matrix(torch, device, n, 2048, n)
    gram = eng.gram(g)
    weights = torch.empty(n, dtype=torch.float64, device=device)
    flags = torch.empty(n, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(g.device).cuda_stream
    fg, afa = _native.FoolsgoldParams(1.0, 0), _native.AfaParams(2.0, 0.5, 0)
    total = _native.FoolsgoldParams(1.0, 1)

    def run(params=fg):
        _check(eng.lib.byz_foolsgold_weights_dev(eng.ctx, _vp(gram.data_ptr()), n, ctypes.byref(params), _vp(weights.data_ptr()), None,
                                                 None, _vp(stream)))

    def select():
        _check(eng.lib.byz_afa_select_dev(eng.ctx, _vp(gram.data_ptr()), n, None, ctypes.byref(afa), _vp(flags.data_ptr()), None, None,
                                          _vp(stream)))
    line = {'weights': True, 'n': n, 'reps': args.reps}
    line['weights_ms'] = round(timed(torch, run, args.reps), 4)
    info = eng.foolsgold_info()
    line.update(at_zero=info['at_zero'], at_one=info['at_one'], sybils_at_zero=int((weights[:n // 4] == 0).sum().item()))
    line['weights_sum_ms'] = round(timed(torch, lambda: run(total), args.reps), 4)
    line['afa_select_ms'] = round(timed(torch, select, args.reps), 4)
    line['weights_over_afa_select'] = round(line['weights_ms'] / line['afa_select_ms'], 3)
    line['slots_ms'] = {k: round(v, 4) for k, v in slots_of(eng, torch, run).items()}
    print(json.dumps(line), flush=True)
    return line


def whole(args, eng, torch, n, d, window):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    device = 'cuda:%d' % eng.device
    g = drift_matrix(torch, device, n, d, n + 1)
    w = window or d
    h = torch.zeros((n, w), dtype=torch.float32, device=device)
    out = torch.empty(d, dtype=torch.float32, device=device)
    gram = torch.empty((n, n), dtype=torch.float64, device=device)
    weights = torch.empty(n, dtype=torch.float64, device=device)
    flags = torch.empty(n, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(g.device).cuda_stream
    fg, afa = _native.FoolsgoldParams(1.0, 0), _native.AfaParams(2.0, 0.5, 0)
    G, H = _vp(g.data_ptr()), _vp(h.data_ptr())

    def foolsgold():
        _check(eng.lib.byz_foolsgold_dev(eng.ctx, G, n, d, g.stride(0), H, w, 0, w, ctypes.byref(fg), None, _vp(out.data_ptr()),
                                         _vp(weights.data_ptr()), _vp(stream)))
    line = {'whole': True, 'n': n, 'd': d, 'window': w, 'reps': args.reps}
    line['foolsgold_ms'] = round(timed(torch, foolsgold, args.reps), 3)
    info = eng.foolsgold_info()
    line.update(at_zero=info['at_zero'], at_one=info['at_one'], sybils_at_zero=int((weights[:n // 4] == 0).sum().item()))
    count = torch.tensor([float(n)], dtype=torch.float64, device=device)
    pieces = {
        'rows_add': lambda: _check(eng.lib.byz_rows_add_dev(eng.ctx, H, w, G, n, w, g.stride(0), 0, _vp(stream))),
        'gram': lambda: _check(eng.lib.byz_gram_dev(eng.ctx, H, n, w, w, _vp(gram.data_ptr()), _vp(stream))),
        'scaled_rows_sum': lambda: _check(eng.lib.byz_scaled_rows_sum_dev(eng.ctx, G, n, d, g.stride(0), _vp(weights.data_ptr()),
                                                                          _vp(count.data_ptr()), _vp(out.data_ptr()), _vp(stream))),
    }
    line['pieces_ms'] = {k: round(timed(torch, call, args.reps), 3) for k, call in pieces.items()}
    line['pieces_sum_ms'] = round(sum(line['pieces_ms'].values()), 3)
    line['foolsgold_over_pieces'] = round(line['foolsgold_ms'] / line['pieces_sum_ms'], 4)
    line['slots_ms'] = {k: round(v, 3) for k, v in slots_of(eng, torch, foolsgold).items()}
    if window:
        def run_afa():
            _check(eng.lib.byz_afa_dev(eng.ctx, G, n, d, g.stride(0), None, ctypes.byref(afa), None, _vp(out.data_ptr()),
                                       _vp(flags.data_ptr()), None, None, _vp(stream)))
        line['afa_ms'] = round(timed(torch, run_afa, args.reps), 3)
    print(json.dumps(line), flush=True)
    del g, h, out
    torch.cuda.empty_cache()
    return line


def logit_differences(eng):
    from tests.foolsgold_rule import graded_gram, restated_foolsgold_weights
    import numpy as np
    lines = []
    for n in (2, 3, 63, 64, 65, 257, 1000, 1023, 1024, 1025, 4097):
        c = graded_gram(n, 8 if n <= 257 else 12, 0)
        got, _ = eng.foolsgold_weights(c)
        want = restated_foolsgold_weights(c)['weights']
        lines.append({'logit': True, 'n': n, 'worst_in_2^-53': float(np.abs(got - want).max() * 2.0 ** 53),
                      'differing': int((got != want).sum())})
        print(json.dumps(lines[-1]), flush=True)
    return lines


def note(adds, stages, wholes, logits, resources):
    met = lambda ok: 'met' if ok else 'missed'     # noqa: E731
    text = ['# FoolsGold: the history update, the weights and the whole call', '',
            'Written by `scripts/foolsgold_timing.py`: one process on one MI355X, device events, the median of the repetitions after a',
            'warm-up call.  Recorded, not gated.', '',
            '## `rows_add` beside a device-to-device copy of the same n x w floats', '',
            'It moves 3 bytes where the copy moves 2.  Expected: 1.5 times the copy\'s time, with 15 % over that (1.725) for the second',
            'read stream.  "window one column in": G has w + 1 columns and the window starts at column 1, so G is read by dwords.', '',
            '| n x w | window | rows_add ms | copy ms | ratio | GB/s moved | within 1.725 |', '|---|---|---|---|---|---|---|']
    for a in adds:
        text.append('| %d x %d | %s | %.4f | %.4f | %.3f | %.1f | %s |' % (
            a['n'], a['w'], 'one column in' if a['misaligned'] else 'aligned', a['rows_add_ms'], a['copy_ms'], a['ratio'], a['gbytes_per_s'],
            met(a['ratio'] <= 1.725)))
    text += ['', '## The weights stage (four launches) on the drift-attack Gram (n // 4 copies of one vector), beside `afa_select`', '',
             'It reads the n x n matrix twice with no dependent loop.  Expected: below `afa_select` at 4000 and 10,000.', '',
             '| n | weights ms | with T = the sum ms | afa_select ms | weights / afa_select | below | copies at weight 0 | rows at 0 | rows at 1 '
             '| timers of one call (ms) |', '|---|---|---|---|---|---|---|---|---|---|']
    for s in stages:
        text.append('| %d | %.4f | %.4f | %.4f | %.3f | %s | %d of %d | %d | %d | %s |' % (
            s['n'], s['weights_ms'], s['weights_sum_ms'], s['afa_select_ms'], s['weights_over_afa_select'],
            met(s['weights_over_afa_select'] < 1.0) if s['n'] >= 4000 else 'no expectation', s['sybils_at_zero'], s['n'] // 4, s['at_zero'],
            s['at_one'], ', '.join('%s %.4f' % kv for kv in sorted(s['slots_ms'].items()))))
    text += ['', '## The whole call beside `rows_add` + `gram` (of the history) + `scaled_rows_sum`, each timed singly', '',
             'Expected: within 5 % of the pieces\' sum.', '',
             '| n x d | window | foolsgold ms | rows_add ms | gram ms | scaled_rows_sum ms | sum ms | foolsgold / sum | within 5 % | afa ms '
             '| timers of one call (ms) |', '|---|---|---|---|---|---|---|---|---|---|---|']
    for w in wholes:
        p = w['pieces_ms']
        text.append('| %d x %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.4f | %s | %s | %s |' % (
            w['n'], w['d'], w['window'], w['foolsgold_ms'], p['rows_add'], p['gram'], p['scaled_rows_sum'], w['pieces_sum_ms'],
            w['foolsgold_over_pieces'], met(w['foolsgold_over_pieces'] <= 1.05), '%.3f' % w['afa_ms'] if 'afa_ms' in w else '-',
            ', '.join('%s %.3f' % kv for kv in sorted(w['slots_ms'].items()))))
    text += ['', '## The final weight against numpy\'s: the two logs', '',
             '`tests/test_gpu_foolsgold.py` bounds |l_dev - l_ref| by kappa x 4 x 2^-53; m, a, top and the rescaled w are equal as bits.', '',
             '| n | worst difference (2^-53) | weights that differ |', '|---|---|---|']
    for l in logits:
        text.append('| %d | %.2f | %d |' % (l['n'], l['worst_in_2^-53'], l['differing']))
    text += ['', '## The compiler\'s resource report (gfx950)', '', '```', resources.strip() or 'not collected', '```', '']
    return '\n'.join(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--write', default='')
    ap.add_argument('--resources', default='')
    ap.add_argument('--skip-large', action='store_true')
    args = ap.parse_args()
    import torch
    from attacking_federate_learning_amd.engine import get_engine
    eng = get_engine()
    logits = logit_differences(eng)
    adds = [rows_add(args, eng, torch, n, 1000000, mis) for n in (1000, 4000) for mis in (False, True)]
    stages = [weights_stage(args, eng, torch, n) for n in (1000, 4000, 10000)]
    wholes = [whole(args, eng, torch, 1000, 1000000, 0)]
    if not args.skip_large:
        wholes.append(whole(args, eng, torch, 4000, 10000000, 1000000))
    if args.write:
        resources = open(args.resources).read() if args.resources else ''
        with open(args.write, 'w') as fh:
            fh.write(note(adds, stages, wholes, logits, resources))


if __name__ == '__main__':
    main()
