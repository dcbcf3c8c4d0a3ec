"""Bucketing timing on one MI355X: the one-launch bucket means next to the kernel they are held to, and next to the only
previous route.

    python scripts/bucketing_timing.py --n 1000 --d 1000000 --loop
    python scripts/bucketing_timing.py --n 4000 --d 10000000 --steps 5 --rounds 5

scripts/geomed_timing.py's synthetic matrix.  In one process, on one matrix, through the C ABI (what the call enqueues, without
the engine's output allocations): `byz_no_defense_dev`, the parent's kernel, then `byz_bucket_means_dev` with a seeded
permutation for every bucket size of `--s` (default 2 and 10).  The calls alternate: every round times `--steps` calls of each
back to back with device events, after `--warmup` calls of each; the figure is the median over `--rounds` rounds, with the
lowest and highest round beside it, so that a difference can be read against the spread of the same visit.  `--identity` adds
the same bucket sizes with a null `perm` (rows in storage order: what the shuffle itself costs); `--loop` adds the
route that existed before: one `byz_mean_rows_dev` launch per bucket of the first bucket size, into the rows of the same output.
One JSON line: ms per call, the algorithmic bytes (4 n d read; 4 ceil(n / s) d more written by bucketing), the share of HBM
those bytes make against 8 TB/s, and `per_byte_vs_no_defense`, the time per algorithmic byte over no_defense's: the bar is 1.10.
Before anything is timed the first bucket of every size is compared with no_defense's bits on that bucket's rows, and the loop's
output with the one launch's.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geomed_timing import PEAK_HBM, timed  # noqa: E402  (timed: events round `steps` calls after `warmup` calls)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=1000)
    p.add_argument('--d', type=int, default=1_000_000)
    p.add_argument('--s', type=int, nargs='+', default=[2, 10])
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--identity', action='store_true', help='also time every bucket size with a null perm (rows in order)')
    p.add_argument('--loop', action='store_true', help='also time one byz_mean_rows_dev launch per bucket (the first --s)')
    p.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from attacking_federate_learning_amd.engine import _check, _vp, bucketing_permutation, get_engine

    n, d = args.n, args.d
    eng = get_engine()
    device = torch.device('cuda', eng.device)
    gen = torch.Generator(device=device).manual_seed(n + d)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    g.normal_(generator=gen)
    g.mul_(torch.linspace(1.0, 1.5, n, device=device)[torch.randperm(n, device=device, generator=gen)][:, None])
    torch.cuda.synchronize()

    stream = torch.cuda.current_stream(device).cuda_stream
    perm_host = bucketing_permutation(n, seed=0)
    perm = torch.from_numpy(perm_host).to(device)
    mean = torch.empty(d, dtype=torch.float32, device=device)
    buckets = {s: -(-n // s) for s in args.s}
    y = torch.empty((max(buckets.values()), d), dtype=torch.float32, device=device)      # one output, reused by every size

    def bucket_call(s):
        return lambda: _check(eng.lib.byz_bucket_means_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(perm.data_ptr()), s,
                                                           _vp(y.data_ptr()), d, _vp(stream)))

    calls = {'no_defense': lambda: _check(eng.lib.byz_no_defense_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(mean.data_ptr()),
                                                                      _vp(stream)))}
    for s in args.s:
        calls['bucket_means_s%d' % s] = bucket_call(s)
    if args.identity:       # the same buckets over rows in storage order: what the shuffle itself costs
        for s in args.s:
            calls['bucket_means_identity_s%d' % s] = (lambda s=s: _check(eng.lib.byz_bucket_means_dev(
                eng.ctx, _vp(g.data_ptr()), n, d, d, None, s, _vp(y.data_ptr()), d, _vp(stream))))
    s0 = args.s[0]

    def loop_call():
        for b in range(buckets[s0]):
            count = min(s0, n - b * s0)
            _check(eng.lib.byz_mean_rows_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(perm.data_ptr() + 4 * b * s0), count,
                                             _vp(y.data_ptr() + 4 * b * d), _vp(stream)))
    if args.loop:
        calls['mean_rows_loop_s%d' % s0] = loop_call

    # the bits before the times: bucket 0 of every size is no_defense on its rows; the loop writes what the one launch writes
    for s in args.s:
        calls['bucket_means_s%d' % s]()
        rows = g[torch.from_numpy(perm_host[:s].astype('int64')).to(device)]
        _check(eng.lib.byz_no_defense_dev(eng.ctx, _vp(rows.data_ptr()), s, d, d, _vp(mean.data_ptr()), _vp(stream)))
        assert torch.equal(y[0].view(torch.int32), mean.view(torch.int32)), s
        del rows
    if args.loop:
        calls['bucket_means_s%d' % s0]()
        one_launch = y[:buckets[s0]].clone()
        y.zero_()
        loop_call()
        assert torch.equal(y[:buckets[s0]].view(torch.int32), one_launch.view(torch.int32))
        del one_launch

    samples = {name: [] for name in calls}
    for r in range(args.rounds):
        for name, call in calls.items():
            samples[name].append(timed(call, args.steps, args.warmup if r == 0 else 0))

    line = {'n': n, 'd': d, 's': args.s, 'steps': args.steps, 'warmup': args.warmup, 'rounds': args.rounds,
            'package_root': os.path.abspath(args.package_root)}
    read = 4.0 * n * d
    nbytes = {'no_defense': read}
    for s in args.s:
        nbytes['bucket_means_s%d' % s] = read + 4.0 * buckets[s] * d
    nbytes['mean_rows_loop_s%d' % s0] = read + 4.0 * buckets[s0] * d
    for s in args.s:
        nbytes['bucket_means_identity_s%d' % s] = nbytes['bucket_means_s%d' % s]
    base = statistics.median(samples['no_defense']) / nbytes['no_defense']
    for name, ms in samples.items():
        med = statistics.median(ms)
        line[name + '_ms'] = round(med, 4)
        line[name + '_ms_min_max'] = [round(min(ms), 4), round(max(ms), 4)]
        line[name + '_bytes'] = int(nbytes[name])
        line[name + '_hbm_frac'] = round(nbytes[name] / (med * 1e-3) / PEAK_HBM, 4)
        line[name + '_per_byte_vs_no_defense'] = round(med / nbytes[name] / base, 4)
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
