"""FLTrust timing on one MI355X: the end-to-end call, its two passes alone, and the kernels they are held to.

    python scripts/fltrust_timing.py --n 4000 --d 10000000
    python scripts/fltrust_timing.py --n 1000 --d 1000000
    python scripts/fltrust_timing.py --mode dots ...       # one part alone (run under rocprofv3 --kernel-trace --stats)

scripts/geomed_timing.py's synthetic matrix and timing loop (device events); the root is the mean of the honest rows plus
noise, so that the honest rows are trusted and the repeated first row is whatever its cosine says.  One JSON line: ms per
call, and for every single pass its share of HBM, 4 * n * d bytes over the time against 8 TB/s.  `--mode all` also times
`rowsq` and `wmean`, the parent kernels of the two passes, on the same matrix in the same process (what
`scripts/geomed_timing.py --mode rowsq` / `--mode wmean` time): row_dots moves the bytes rowsq moves, scaled_rows_sum the
bytes wmean moves, each with one more fp64 multiply-add per value.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geomed_timing import PEAK_HBM, timed  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=1000)
    p.add_argument('--d', type=int, default=1_000_000)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--mode', default='all', choices=['all', 'e2e', 'dots', 'sum', 'rowsq', 'wmean'])
    p.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from attacking_federate_learning_amd.engine import _check, _vp, get_engine

    n, d = args.n, args.d
    f = int(n * 0.24)
    eng = get_engine()
    device = torch.device('cuda', eng.device)
    gen = torch.Generator(device=device).manual_seed(n + d)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    g.normal_(generator=gen)
    g.mul_(torch.linspace(1.0, 1.5, n, device=device)[torch.randperm(n, device=device, generator=gen)][:, None])
    if f:
        g[:f] = g[0]
    root = eng.no_defense(g[f:])
    root.add_(torch.empty_like(root).normal_(generator=gen), alpha=0.05)
    torch.cuda.synchronize()

    line = {'mode': args.mode, 'n': n, 'd': d, 'steps': args.steps, 'warmup': args.warmup,
            'package_root': os.path.abspath(args.package_root)}
    gbytes = 4.0 * n * d
    modes = ['rowsq', 'dots', 'wmean', 'sum', 'e2e'] if args.mode == 'all' else [args.mode]
    stream = torch.cuda.current_stream(device).cuda_stream
    out = torch.empty(d, dtype=torch.float32, device=device)
    w = torch.linspace(0.5, 1.5, n, device=device, dtype=torch.float64)
    total = w.sum().reshape(1)
    dot = torch.empty(n, dtype=torch.float64, device=device)
    sq = torch.empty(n, dtype=torch.float64, device=device)

    def single(name, call):
        ms = timed(call, args.steps, args.warmup)
        line[name + '_ms'], line[name + '_hbm_frac'] = round(ms, 4), round(gbytes / (ms * 1e-3) / PEAK_HBM, 4)

    # (the ABI entries alone: what the call enqueues, without the engine's output allocations)
    if 'rowsq' in modes:
        single('rowsq', lambda: _check(eng.lib.byz_row_sqdist_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(root.data_ptr()),
                                                                  _vp(sq.data_ptr()), _vp(stream))))
    if 'dots' in modes:
        single('row_dots', lambda: _check(eng.lib.byz_row_dots_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(root.data_ptr()),
                                                                   _vp(dot.data_ptr()), _vp(sq.data_ptr()), _vp(stream))))
    if 'wmean' in modes:
        single('wmean', lambda: _check(eng.lib.byz_weighted_mean_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(w.data_ptr()),
                                                                     _vp(out.data_ptr()), _vp(stream))))
    if 'sum' in modes:
        single('scaled_rows_sum', lambda: _check(eng.lib.byz_scaled_rows_sum_dev(eng.ctx, _vp(g.data_ptr()), n, d, d,
                                                                                 _vp(w.data_ptr()), _vp(total.data_ptr()),
                                                                                 _vp(out.data_ptr()), _vp(stream))))
    if 'e2e' in modes:
        line['e2e_ms'] = round(timed(lambda: _check(eng.lib.byz_fltrust_dev(eng.ctx, _vp(g.data_ptr()), n, d, d,
                                                                            _vp(root.data_ptr()), _vp(out.data_ptr()), None,
                                                                            None, _vp(stream))), args.steps, args.warmup), 4)
        trusted, excluded, ok, t = eng.fltrust_info()
        line['trusted_rows'], line['excluded_rows'], line['root_ok'], line['trust_sum'] = trusted, excluded, ok, round(t, 6)
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
