"""Robust learning rate timing on one MI355X: the sign vote alone and the fused call, next to the kernel they are held to.

    python scripts/robust_lr_timing.py --n 1000 --d 1000000
    python scripts/robust_lr_timing.py --n 4000 --d 10000000 --steps 5 --rounds 5

scripts/geomed_timing.py's synthetic matrix.  In one process, on one matrix, through the C ABI (what the call enqueues, without
the engine's output allocations): `byz_no_defense_dev`, the parent's kernel, then `byz_sign_votes_dev` and `byz_robust_lr_dev`
(theta = 0.24 n + 1, votes stored).  The three alternate: every round times `--steps` calls of each back to back with device
events, after `--warmup` calls of each; the figure is the median over `--rounds` rounds, with the lowest and highest round
beside it, so that a difference can be read against the spread of the same visit.  One JSON line: ms per call, the share of
HBM (4 * n * d bytes over the time against 8 TB/s), the ratio to no_defense, and the number of columns the fused call flipped.
The fused call's output is compared with no_defense's and the votes' bits before anything is timed.
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
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from attacking_federate_learning_amd.engine import _check, _vp, get_engine

    n, d = args.n, args.d
    f = int(n * 0.24)
    theta = f + 1
    eng = get_engine()
    device = torch.device('cuda', eng.device)
    gen = torch.Generator(device=device).manual_seed(n + d)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    g.normal_(generator=gen)
    g.mul_(torch.linspace(1.0, 1.5, n, device=device)[torch.randperm(n, device=device, generator=gen)][:, None])
    if f:
        g[:f] = g[0]
    torch.cuda.synchronize()

    stream = torch.cuda.current_stream(device).cuda_stream
    mean = torch.empty(d, dtype=torch.float32, device=device)
    out = torch.empty(d, dtype=torch.float32, device=device)
    votes = torch.empty(d, dtype=torch.int32, device=device)
    votes_fused = torch.empty(d, dtype=torch.int32, device=device)
    calls = {
        'no_defense': lambda: _check(eng.lib.byz_no_defense_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(mean.data_ptr()),
                                                                _vp(stream))),
        'sign_votes': lambda: _check(eng.lib.byz_sign_votes_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, _vp(votes.data_ptr()),
                                                                _vp(stream))),
        'robust_lr': lambda: _check(eng.lib.byz_robust_lr_dev(eng.ctx, _vp(g.data_ptr()), n, d, d, theta, _vp(out.data_ptr()),
                                                              _vp(votes_fused.data_ptr()), _vp(stream))),
    }
    for call in calls.values():
        call()
    flipped = eng.robust_lr_info()
    flip = votes.abs() < theta
    sign = torch.where(flip, torch.full_like(votes, -2 ** 31), torch.zeros_like(votes))
    assert torch.equal(votes, votes_fused) and int(flip.sum()) == flipped
    assert torch.equal(out.view(torch.int32), mean.view(torch.int32) ^ sign)
    del flip, sign

    samples = {name: [] for name in calls}
    for r in range(args.rounds):
        for name, call in calls.items():
            samples[name].append(timed(call, args.steps, args.warmup if r == 0 else 0))

    line = {'n': n, 'd': d, 'theta': theta, 'steps': args.steps, 'warmup': args.warmup, 'rounds': args.rounds,
            'flipped_cols': flipped, 'package_root': os.path.abspath(args.package_root)}
    gbytes = 4.0 * n * d
    base = statistics.median(samples['no_defense'])
    for name, ms in samples.items():
        med = statistics.median(ms)
        line[name + '_ms'] = round(med, 4)
        line[name + '_ms_min_max'] = [round(min(ms), 4), round(max(ms), 4)]
        line[name + '_hbm_frac'] = round(gbytes / (med * 1e-3) / PEAK_HBM, 4)
        line[name + '_vs_no_defense'] = round(med / base, 4)
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
