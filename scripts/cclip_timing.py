"""Centered clipping timing on one MI355X: the end-to-end call at iters 1 and 3, and clip_update alone.

    python scripts/cclip_timing.py --n 4000 --d 10000000
    python scripts/cclip_timing.py --n 1000 --d 1000000
    python scripts/cclip_timing.py --mode update ...       # one part alone (run under rocprofv3 --kernel-trace --stats)

scripts/geomed_timing.py's synthetic matrix and timing loop; tau is the median row norm, so that about half the rows are
clipped.  One JSON line: ms per call, and for the update its share of HBM, 4 * n * d bytes over the time against 8 TB/s.
Compare with `scripts/geomed_timing.py --mode rowsq` / `--mode wmean` at the same shape: an iteration is one rowsq and one
update, and the update moves the bytes wmean moves.
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
    p.add_argument('--mode', default='all', choices=['all', 'e2e', 'update'])
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
    torch.cuda.synchronize()
    zero = torch.zeros(d, dtype=torch.float32, device=device)
    tau = float(torch.sqrt(eng.row_sqdist(g, zero)).median().item())

    line = {'mode': args.mode, 'n': n, 'd': d, 'tau': tau, 'steps': args.steps, 'warmup': args.warmup,
            'package_root': os.path.abspath(args.package_root)}
    gbytes = 4.0 * n * d
    modes = ['e2e', 'update'] if args.mode == 'all' else [args.mode]
    for iters in ([1, 3] if 'e2e' in modes else []):
        ms = timed(lambda: eng.centered_clip(g, tau=tau, iters=iters), args.steps, args.warmup)
        line['e2e_iters%d_ms' % iters] = round(ms, 4)
    if 'e2e' in modes:
        _, info = eng.centered_clip(g, tau=tau, iters=3, return_info=True)
        line['clipped_rows'], line['excluded_rows'] = info['clipped_rows'], info['excluded_rows']
    if 'update' in modes:
        s = torch.linspace(0.5, 1.0, n, device=device, dtype=torch.float64)
        out = torch.empty(d, dtype=torch.float32, device=device)
        stream = torch.cuda.current_stream(device).cuda_stream

        def update():
            _check(eng.lib.byz_clip_update_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(zero.data_ptr()), _vp(s.data_ptr()),
                                               _vp(out.data_ptr()), _vp(stream)))
        ms = timed(update, args.steps, args.warmup)
        line['update_ms'], line['update_hbm_frac'] = round(ms, 4), round(gbytes / (ms * 1e-3) / PEAK_HBM, 4)
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
