"""Two builds of libbyzagg against each other in ONE process on one MI355X: the kernels built on the row walk
(csrc/row_walk.hpp), bit for bit and in time.

    python scripts/row_walk_ab.py --old-lib OTHER/attacking_federate_learning_amd/libbyzagg.so --n 1000 --d 1000000
    python scripts/row_walk_ab.py --old-lib ... --n 4000 --d 10000000 --steps 5 --warmup 1

Both libraries are loaded side by side (ctypes, each with a context of its own) and work on the same device-resident matrix
(scripts/geomed_timing.py's synthetic gradients).  Bits: weighted_mean, clip_update, no_defense, mean_rows (the n - f honest
rows, ascending), column_chain (sum and squared deviations), the drift attack's statistics, geometric_median and centered_clip
end to end, old against new with torch.equal.  Time: per kernel old, new, old, new, ..., old (`--pairs` new timings, device
events over `--steps` calls after `--warmup`); neighbouring old timings are the parent against itself, the spread that a new
timing minus the mean of its two old neighbours is held to.  BYZ_ATTACK_RESIDENT=0 is set, so that the drift attack's
statistics run column_sequential_kernel<., 1> at every height (from 65 to 2560 rows the library otherwise takes the
register-resident kernel, which does not walk rows this way).  One JSON line per kernel, then one with the verdicts.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geomed_timing import timed  # noqa: E402


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = argparse.ArgumentParser()
    p.add_argument('--old-lib', required=True)
    p.add_argument('--new-lib', default=os.path.join(here, 'attacking_federate_learning_amd', 'libbyzagg.so'))
    p.add_argument('--n', type=int, default=1000)
    p.add_argument('--d', type=int, default=1_000_000)
    p.add_argument('--pairs', type=int, default=5)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    args = p.parse_args()
    sys.path.insert(0, here)
    os.environ['BYZ_ATTACK_RESIDENT'] = '0'
    import torch
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp

    _native._share_hip_runtime_with_torch()
    libs, ctxs = {}, {}
    for name, path in (('old', args.old_lib), ('new', args.new_lib)):
        lib = ctypes.CDLL(os.path.abspath(path))
        for fn_name, argtypes in _native._PROTOTYPES.items():
            fn = getattr(lib, fn_name)
            fn.argtypes, fn.restype = argtypes, _native._RESTYPES.get(fn_name, ctypes.c_int)
        ctx = ctypes.c_void_p()
        assert lib.byz_ctx_create(0, ctypes.byref(ctx)) == 0, lib.byz_last_error()
        libs[name], ctxs[name] = lib, ctx

    n, d = args.n, args.d
    f = int(n * 0.24)
    device = torch.device('cuda', 0)
    gen = torch.Generator(device=device).manual_seed(n + d)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    for lo in range(0, n, 64):          # (in blocks of rows: the generator's scratch stays small next to a 160 GB matrix)
        g[lo:lo + 64].normal_(generator=gen)
    g.mul_(torch.linspace(1.0, 1.5, n, device=device)[torch.randperm(n, device=device, generator=gen)][:, None])
    if f:
        g[:f] = g[0]
    w = torch.linspace(0.5, 1.5, n, device=device, dtype=torch.float64)
    w[::7] = 0.0                                                        # rows that are skipped
    v = torch.empty(d, dtype=torch.float32, device=device).normal_(generator=gen).mul_(0.1)
    rows = torch.arange(f, n, dtype=torch.int32, device=device)
    tau = float(g[f:f + 64].double().norm(dim=1).median().item())
    torch.cuda.synchronize()
    stream = _vp(torch.cuda.current_stream(device).cuda_stream)
    G = _vp(g.data_ptr())

    def vec():
        return torch.empty(d, dtype=torch.float32, device=device)

    def ok(which, rc):
        assert rc == 0, (which, rc, libs[which].byz_last_error())

    # every call: (library name, output tensors) -> None
    def weighted_mean(k, out):
        ok(k, libs[k].byz_weighted_mean_dev(ctxs[k], G, n, d, d, _vp(w.data_ptr()), _vp(out[0].data_ptr()), stream))

    def clip_update(k, out):
        ok(k, libs[k].byz_clip_update_dev(ctxs[k], G, n, d, d, _vp(v.data_ptr()), _vp(w.data_ptr()), _vp(out[0].data_ptr()), stream))

    def no_defense(k, out):
        ok(k, libs[k].byz_no_defense_dev(ctxs[k], G, n, d, d, _vp(out[0].data_ptr()), stream))

    def mean_rows(k, out):
        ok(k, libs[k].byz_mean_rows_dev(ctxs[k], G, n, d, d, _vp(rows.data_ptr()), n - f, _vp(out[0].data_ptr()), stream))

    def chain_sum(k, out):
        ok(k, libs[k].byz_column_chain_dev(ctxs[k], G, n, d, d, _vp(v.data_ptr()), None, _vp(out[0].data_ptr()), stream))

    def chain_squares(k, out):
        ok(k, libs[k].byz_column_chain_dev(ctxs[k], G, n, d, d, None, _vp(v.data_ptr()), _vp(out[0].data_ptr()), stream))

    def drift_stats(k, out):
        ok(k, libs[k].byz_drift_attack_dev(ctxs[k], G, n, d, d, 1.5, _vp(out[0].data_ptr()), _vp(out[1].data_ptr()),
                                           _vp(out[2].data_ptr()), 0, stream))

    def geometric_median(k, out):
        params = _native.GeomedParams(1e-6, 10, 1e-6)
        ok(k, libs[k].byz_geometric_median_dev(ctxs[k], G, n, d, d, ctypes.byref(params), _vp(out[0].data_ptr()), None, stream))

    def centered_clip(k, out):
        params = _native.CclipParams(tau, 3)
        ok(k, libs[k].byz_centered_clip_dev(ctxs[k], G, n, d, d, ctypes.byref(params), None, _vp(out[0].data_ptr()), None, stream))

    kernels = [(weighted_mean, 1, True), (clip_update, 1, True), (no_defense, 1, True), (mean_rows, 1, True), (chain_sum, 1, True),
               (chain_squares, 1, True), (drift_stats, 3, True), (geometric_median, 1, False), (centered_clip, 1, False)]
    verdicts = {}
    for call, n_out, time_it in kernels:
        outs = {k: [vec() for _ in range(n_out)] for k in ('old', 'new')}
        for k in ('old', 'new'):
            call(k, outs[k])
        torch.cuda.synchronize()
        equal = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs['old'], outs['new']))
        line = {'kernel': call.__name__, 'n': n, 'd': d, 'bits_equal': bool(equal)}
        if time_it:
            # old, new, old, new, ..., old: every new timing sits between two old ones, so position favours neither
            ms = [timed(lambda k=k: call(k, outs[k]), args.steps, args.warmup) for k in ['old', 'new'] * args.pairs + ['old']]
            olds, news = ms[0::2], ms[1::2]
            spread = max(abs(a - b) for a, b in zip(olds, olds[1:]))
            deltas = sorted(c - 0.5 * (a + b) for a, b, c in zip(olds, olds[1:], news))
            line.update(old_ms=[round(x, 4) for x in olds], new_ms=[round(x, 4) for x in news], spread_ms=round(spread, 4),
                        new_minus_old_ms=[round(x, 4) for x in deltas], median_delta_ms=round(deltas[len(deltas) // 2], 4),
                        inside_spread=bool(abs(deltas[len(deltas) // 2]) <= spread))
        verdicts[call.__name__] = {key: line[key] for key in line if key in ('bits_equal', 'inside_spread')}
        print(json.dumps(line), flush=True)
    print(json.dumps({'n': n, 'd': d, 'verdicts': verdicts}), flush=True)
    for k in ('old', 'new'):
        libs[k].byz_ctx_destroy(ctxs[k])
    if not all(vd['bits_equal'] for vd in verdicts.values()):
        sys.exit(1)


if __name__ == '__main__':
    main()
