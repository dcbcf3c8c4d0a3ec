"""Timing of the Min-Max / Min-Sum attacks on one MI355X, each next to its yardstick.  Every figure of a run comes from ONE process:

    python scripts/minmax_timing.py                              # 1000 x 1e6 with m = 200, then 4000 x 1e7 with m = 800
    python scripts/minmax_timing.py --n 1000 --d 1000000 --m 200

Through the C ABI, device events round `--steps` calls back to back, the calls alternating, the median over `--rounds` rounds with
the lowest and highest beside it (sparsefed_timing.alternate):
  row_dots, row_moments       siblings on one kernel template: the same read of G, two fp64 sums a row each
  drift_stats                 byz_drift_attack_dev with write_back = 0: mu and sigma, what every attack starts from
  restore                     the m attacker rows copied back from a clone: every timed attack starts from the honest rows (an
                              attacked matrix holds m identical rows, which the Gram's duplicate-row search would treat
                              otherwise than the yardstick's fresh matrix); its time is taken off the attacks' (`*_net_ms`)
  minsum                      the whole byz_minmax_attack_dev, kind Min-Sum, std: against drift_stats + row_moments; what is left
                              over is the fill of the m attacker rows, the perturbation, c and the solve
  minsum_narrow               the same attack on the first 1024 columns with one attacker: launches and the one-workgroup solve
                              (Min-Sum's two sums in row order are one thread's loop over the r rows) with nothing else of size
  pairwise_distances, minmax  the whole Min-Max against pairwise_distances + drift_stats + row_moments (both wait where the Gram waits,
                              both on the restored rows)
One JSON line per shape.
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # the package, from a checkout that is not installed
from fang_timing import matrix  # noqa: E402
from geomed_timing import PEAK_HBM  # noqa: E402
from sparsefed_timing import alternate, summarise  # noqa: E402


def run(eng, torch, device, n, d, m, steps, warmup, rounds, with_minmax):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    g = matrix(torch, device, n, d)
    stream = torch.cuda.current_stream(device).cuda_stream
    mu, sigma, p = (torch.empty(d, dtype=torch.float32, device=device) for _ in range(3))
    a, b = (torch.empty(n, dtype=torch.float64, device=device) for _ in range(2))
    gp, ptr = _vp(g.data_ptr()), lambda t: _vp(t.data_ptr())
    _check(eng.lib.byz_drift_attack_dev(eng.ctx, gp, n, d, d, 0.0, None, ptr(mu), ptr(sigma), 0, _vp(stream)))
    p.copy_(-sigma)
    minsum, minmax = _native.MinmaxParams(1, 1, 0, 0), _native.MinmaxParams(0, 1, 0, 0)
    honest = g[:m].clone()

    def attack(params, dist_ptr):
        def call():
            g[:m].copy_(honest)
            _check(eng.lib.byz_minmax_attack_dev(eng.ctx, gp, n, d, d, m, ctypes.byref(params), None, dist_ptr, _vp(stream)))
        return call

    def narrow():
        g[:1, :1024].copy_(honest[:1, :1024])
        _check(eng.lib.byz_minmax_attack_dev(eng.ctx, gp, n, 1024, d, 1, ctypes.byref(minsum), None, None, _vp(stream)))
    calls = {
        'row_dots': lambda: _check(eng.lib.byz_row_dots_dev(eng.ctx, gp, n, d, d, ptr(p), ptr(a), ptr(b), _vp(stream))),
        'row_moments': lambda: _check(eng.lib.byz_row_moments_dev(eng.ctx, gp, n, d, d, ptr(mu), ptr(p), ptr(a), ptr(b), _vp(stream))),
        'drift_stats': lambda: _check(eng.lib.byz_drift_attack_dev(eng.ctx, gp, n, d, d, 0.0, None, ptr(mu), ptr(sigma), 0, _vp(stream))),
        'restore': lambda: g[:m].copy_(honest),
        'minsum': attack(minsum, None),
        'minsum_narrow': narrow,
    }
    if with_minmax:
        dist = torch.empty((n, n), dtype=torch.float32, device=device)
        def yardstick():          # on the honest rows as well: the Gram skips the duplicates an attacked matrix holds
            g[:m].copy_(honest)
            _check(eng.lib.byz_pairwise_distances_dev(eng.ctx, gp, n, d, d, ptr(dist), _vp(stream)))
        calls['pairwise_distances'] = yardstick
        calls['minmax'] = attack(minmax, ptr(dist))
    line = {'n': n, 'd': d, 'm': m, 'steps': steps, 'warmup': warmup, 'rounds': rounds}
    summarise(line, alternate(calls, steps, warmup, rounds), base='row_dots')
    for name in ('row_dots', 'row_moments'):
        line[name + '_hbm_frac'] = round(4.0 * n * d / (line[name + '_ms'] * 1e-3) / PEAK_HBM, 4)
    parts = line['drift_stats_ms'] + line['row_moments_ms']
    line['minsum_net_ms'] = round(line['minsum_ms'] - line['restore_ms'], 4)
    line['minsum_vs_parts'] = round(line['minsum_net_ms'] / parts, 3)
    line['minsum_fill_and_rest_ms'] = round(line['minsum_net_ms'] - parts, 4)
    if with_minmax:
        line['minmax_net_ms'] = round(line['minmax_ms'] - line['restore_ms'], 4)
        line['pairwise_distances_net_ms'] = round(line['pairwise_distances_ms'] - line['restore_ms'], 4)
        line['minmax_vs_parts'] = round(line['minmax_net_ms'] / (parts + line['pairwise_distances_net_ms']), 3)
    line['info'] = eng.minmax_info()
    del g
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int)
    ap.add_argument('--d', type=int)
    ap.add_argument('--m', type=int)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-minmax', action='store_true')
    args = ap.parse_args()
    import torch
    from attacking_federate_learning_amd.engine import get_engine
    eng = get_engine()
    device = 'cuda:%d' % eng.device
    shapes = [(args.n, args.d, args.m or max(1, args.n // 5))] if args.n else [(1000, 1000000, 200), (4000, 10000000, 800)]
    for n, d, m in shapes:
        print(json.dumps(run(eng, torch, device, n, d, m, args.steps, args.warmup, args.rounds, not args.no_minmax)), flush=True)


if __name__ == '__main__':
    main()
