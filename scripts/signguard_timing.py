"""SignGuard timing on one MI355X: the census beside row_dots (the kernel it is held to), the whole call beside no_defense,
DnC and FLTrust on the same matrix, and the selection's small kernels alone.

    python scripts/signguard_timing.py --n 1000 --d 1000000                  # every step, one child process each
    python scripts/signguard_timing.py --n 4000 --d 10000000 --mode signs    # one step alone (also the form to profile)
    python scripts/signguard_timing.py --mode select --n 10000               # the selection from synthetic counts, no matrix

`--mode all` never opens the GPU itself: it starts one child per step, each under its own time limit, and stops at the first
child that fails, so that nothing is started on a device that a step has left in doubt.  Every child prints one JSON line.
The matrix is scripts/geomed_timing.py's synthetic one (device events, the same timing loop) round a common direction, its
first 24 % of rows the reference's "A Little Is Enough" vector of those rows (Engine.drift_attack, z = 1).  A single pass
reports its share of HBM, 4 * n * d bytes over the time against 8 TB/s.  row_signs is to be compared with row_dots from the
same invocation, never with itself.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geomed_timing import PEAK_HBM, timed  # noqa: E402

STEPS = ['dots', 'signs', 'e2e', 'nodef', 'fltrust', 'dnc', 'select']


def run_children(args):
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), '--mode', step, '--n', str(args.n), '--d', str(args.d), '--steps',
               str(args.steps), '--warmup', str(args.warmup), '--package-root', args.package_root]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({'mode': step, 'error': 'time limit of %d s' % args.step_timeout}), flush=True)
            return 1
        if rc != 0:
            print(json.dumps({'mode': step, 'error': 'exit status %d' % rc}), flush=True)
            return 1
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=1000)
    p.add_argument('--d', type=int, default=1_000_000)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--mode', default='all', choices=['all'] + STEPS)
    p.add_argument('--step-timeout', type=int, default=240)
    p.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    if args.mode == 'all':
        sys.exit(run_children(args))
    sys.path.insert(0, os.path.abspath(args.package_root))
    import numpy as np
    import torch
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp, dnc_columns, get_engine, signguard_sample, signguard_window

    n, d = args.n, args.d
    f = int(n * 0.24)
    eng = get_engine()
    device = torch.device('cuda', eng.device)
    stream = torch.cuda.current_stream(device).cuda_stream
    line = {'mode': args.mode, 'n': n, 'd': d, 'steps': args.steps, 'warmup': args.warmup}
    sample = torch.from_numpy(signguard_sample(n, 50, 0)).to(device)

    if args.mode == 'select':
        # counts as an attacked matrix gives them: honest shares round a half, the attackers' tilted to the negative side
        m = max(1, d // 10)
        rng = np.random.default_rng(n)
        share = np.where(np.arange(n) < f, 0.42, 0.5) + 0.004 * rng.standard_normal(n)
        pos = np.clip((share * m).astype(np.int64), 0, m)
        counts = torch.from_numpy(np.stack([pos, np.zeros(n, dtype=np.int64), m - pos])).to(device)
        q = torch.from_numpy(1.0 + 0.01 * rng.standard_normal(n)).to(device)
        keep = torch.empty(n, dtype=torch.int32, device=device)
        params = _native.SignGuardParams(0, m, 0.1, 3.0, 0.0, int(sample.numel()))
        line['select_ms'] = round(timed(lambda: _check(eng.lib.byz_signguard_select_dev(
            eng.ctx, _vp(counts.data_ptr()), _vp(q.data_ptr()), n, ctypes.byref(params), _vp(sample.data_ptr()),
            _vp(keep.data_ptr()), None, None, None, _vp(stream))), args.steps, args.warmup), 4)
        line.update(eng.signguard_info())
        print(json.dumps(line), flush=True)
        return

    gen = torch.Generator(device=device).manual_seed(n + d)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    g.normal_(generator=gen)
    g.add_(torch.empty(d, dtype=torch.float32, device=device).normal_(generator=gen).mul_(0.5)[None, :])
    if f:
        eng.drift_attack(g[:f], 1.0, write_back=True)
    torch.cuda.synchronize()
    gbytes = 4.0 * n * d
    out = torch.empty(d, dtype=torch.float32, device=device)
    c0, m = signguard_window(d, 0.1, 0)

    def single(name, call):
        ms = timed(call, args.steps, args.warmup)
        line[name + '_ms'], line[name + '_hbm_frac'] = round(ms, 4), round(gbytes / (ms * 1e-3) / PEAK_HBM, 4)

    if args.mode == 'dots':
        root = torch.ones(d, dtype=torch.float32, device=device)
        dot = torch.empty(n, dtype=torch.float64, device=device)
        sq = torch.empty(n, dtype=torch.float64, device=device)
        single('row_dots', lambda: _check(eng.lib.byz_row_dots_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(root.data_ptr()),
                                                                   _vp(dot.data_ptr()), _vp(sq.data_ptr()), _vp(stream))))
    elif args.mode == 'signs':
        counts = torch.empty((3, n), dtype=torch.int64, device=device)
        q = torch.empty(n, dtype=torch.float64, device=device)
        single('row_signs', lambda: _check(eng.lib.byz_row_signs_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, c0, m,
                                                                     _vp(counts.data_ptr()), _vp(q.data_ptr()), _vp(stream))))
        line['window'] = [c0, m]
    elif args.mode == 'e2e':
        params = _native.SignGuardParams(c0, m, 0.1, 3.0, 0.0, int(sample.numel()))
        line['e2e_ms'] = round(timed(lambda: _check(eng.lib.byz_signguard_dev(
            eng.ctx, _vp(g.data_ptr()), n, d, d, ctypes.byref(params), _vp(sample.data_ptr()), _vp(out.data_ptr()), None, None,
            None, _vp(stream))), args.steps, args.warmup), 4)
        line.update(eng.signguard_info())
        line['attackers'] = f
    elif args.mode == 'nodef':
        single('no_defense', lambda: eng.no_defense(g))
    elif args.mode == 'fltrust':
        root = eng.no_defense(g[f:])
        line['fltrust_ms'] = round(timed(lambda: _check(eng.lib.byz_fltrust_dev(
            eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(root.data_ptr()), _vp(out.data_ptr()), None, None, _vp(stream))),
            args.steps, args.warmup), 4)
    elif args.mode == 'dnc':
        columns = dnc_columns(d, 10000, 1, 0)
        line['dnc_ms'] = round(timed(lambda: eng.dnc(g, f, columns), args.steps, args.warmup), 4)
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
