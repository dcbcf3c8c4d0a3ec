"""DnC timing on one MI355X, with Multi-Krum and Bulyan at the same shape from the same process beside it.

    python scripts/dnc_timing.py --n 1000 --d 1000000
    python scripts/dnc_timing.py --n 4000 --d 10000000 --others none      # DnC alone

Device-resident synthetic gradients (normal, row scales 1 .. 1.5, the first f = 0.24 n rows one vector as the attack leaves
them).  Every defence is timed over `--steps` calls after `--warmup` with device events on the current stream; a second pass
of `--steps` calls reads the library's own event timing, which splits DnC into its pre-mean work (`misc`: the gather, the
centring and the power iteration; `krum_argmin`: the ranking and the compaction) and the final row-list mean
(`column_stats`).  One JSON line.
"""
import argparse
import json
import os
import sys


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=1000)
    p.add_argument('--d', type=int, default=1_000_000)
    p.add_argument('--sub-dim', type=int, default=10000)
    p.add_argument('--niters', type=int, default=1)
    p.add_argument('--power-iters', type=int, default=32)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--others', default='multi_krum,bulyan', help="comma list of multi_krum, bulyan; 'none' for DnC alone")
    args = p.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from attacking_federate_learning_amd.engine import dnc_columns, get_engine

    n, d = args.n, args.d
    f = int(n * 0.24)
    eng = get_engine()
    device = torch.device('cuda', eng.device)
    gen = torch.Generator(device=device).manual_seed(n + d)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    for lo in range(0, n, 64):          # (in blocks of rows: the generator's scratch stays small next to a 160 GB matrix)
        g[lo:lo + 64].normal_(generator=gen)
    g.mul_(torch.linspace(1.0, 1.5, n, device=device)[torch.randperm(n, device=device, generator=gen)][:, None])
    if f:
        g[:f] = g[0]
    columns = torch.from_numpy(dnc_columns(d, args.sub_dim, args.niters, seed=0)).to(device)
    torch.cuda.synchronize()

    calls = {'dnc': lambda: eng.dnc(g, f, columns, power_iters=args.power_iters, validate_columns=False)}
    bf = (n - 3) // 4                   # Bulyan asserts n >= 4 f + 3
    if 'multi_krum' in args.others:
        calls['multi_krum'] = lambda: eng.multi_krum(g, n, f)
    if 'bulyan' in args.others:
        calls['bulyan'] = lambda: eng.bulyan(g, n, bf)
    line = {'n': n, 'd': d, 'f': f, 'bulyan_f': bf, 'sub_dim': int(columns.shape[1]), 'niters': args.niters,
            'power_iters': args.power_iters, 'steps': args.steps, 'warmup': args.warmup}
    for name, call in calls.items():
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.steps):
            call()
        stop.record()
        stop.synchronize()
        eng.timing(True)
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize()
        kernels = eng.timing_read()
        eng.timing(False)
        line[name] = {'ms_per_call': round(start.elapsed_time(stop) / args.steps, 4),
                      'kernels_ms_per_call': {k: round(v['total_ms'] / args.steps, 4) for k, v in kernels.items()}}
        if name == 'dnc':
            kept, inactive = eng.dnc_info()
            line[name]['kept_rows'] = kept
            line[name]['removed_are_the_attackers'] = bool(
                torch.equal(eng.dnc_select(g, f, columns, power_iters=args.power_iters, validate_columns=False).cpu(),
                            torch.arange(f, n, dtype=torch.int32)))
        print(json.dumps({name: line[name]}), flush=True)
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
