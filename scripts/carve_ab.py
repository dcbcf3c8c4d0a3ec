"""Two builds of libbyzagg against each other in ONE process on one MI355X: the whole calls whose host side lays out a
workspace per call (csrc/carve.hpp), bit for bit and in time.  scripts/row_walk_ab.py's procedure on other calls.

    python scripts/carve_ab.py --old-lib OTHER/attacking_federate_learning_amd/libbyzagg.so --n 1000 --d 1000000
    python scripts/carve_ab.py --old-lib ... --n 100 --d 79510 --steps 200 --warmup 20
    python scripts/carve_ab.py --old-lib ... --n 9 --d 1025 --no-time

Both libraries are loaded side by side (ctypes, each with a context of its own) and work on the same device-resident matrix
(scripts/geomed_timing.py's synthetic gradients).  Calls: geometric_median, centered_clip, fltrust, signguard (a fixed sample,
the bandwidth estimated from it) and dnc (two iterations), each with every optional output.  Bits: old against new with
torch.equal on every output.  Up to 2^20 values the *_host entry points of the same calls are compared as well, on the host
copy of the matrix.  Time: per call old, new, old, new, ..., old (`--pairs` new timings, device events over `--steps` calls
after `--warmup`); neighbouring old timings are the parent against itself, the spread that a new timing minus the mean of its
two old neighbours is held to.  At 100 x 79,510 a call is tens of microseconds of kernels: what the host does per call shows
there if it grew.  One JSON line per call, then one with the verdicts; exit status 1 when any output differs.
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
    p.add_argument('--no-time', action='store_true')
    args = p.parse_args()
    sys.path.insert(0, here)
    import numpy as np
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
    for lo in range(0, n, 64):
        g[lo:lo + 64].normal_(generator=gen)
    g.mul_(torch.linspace(1.0, 1.5, n, device=device)[torch.randperm(n, device=device, generator=gen)][:, None])
    if f:
        g[:f] = g[0] + 0.5
    root = g[f:].mean(dim=0)
    tau = float(g[f:f + 64].double().norm(dim=1).median().item())
    sample = torch.arange(f, f + min(64, n - f), dtype=torch.int32, device=device)
    sub_dim = min(10_000, d // 2)
    columns = torch.cat([torch.randperm(d, device=device, generator=gen)[:sub_dim].sort().values for _ in range(2)]).to(torch.int64)
    geomed_params = _native.GeomedParams(1e-6, 10, 1e-6)
    cclip_params = _native.CclipParams(tau, 3)
    sg_params = _native.SignGuardParams(0, d, 0.1, 3.0, 0.0, int(sample.numel()))
    dnc_params = _native.DncParams(2, sub_dim, 8, max(1, f // 2))
    torch.cuda.synchronize()
    stream = _vp(torch.cuda.current_stream(device).cuda_stream)
    G = _vp(g.data_ptr())
    f32, f64, i32 = torch.float32, torch.float64, torch.int32

    def ok(which, rc):
        assert rc == 0, (which, rc, libs[which].byz_last_error())

    def ptrs(out):
        return [_vp(t.data_ptr()) for t in out]

    # every call: (library name, output tensors) -> None; its outputs: (length, dtype), the aggregate first
    def geometric_median(k, out):
        ok(k, libs[k].byz_geometric_median_dev(ctxs[k], G, n, d, d, ctypes.byref(geomed_params), *ptrs(out), stream))

    def centered_clip(k, out):
        ok(k, libs[k].byz_centered_clip_dev(ctxs[k], G, n, d, d, ctypes.byref(cclip_params), None, *ptrs(out), stream))

    def fltrust(k, out):
        ok(k, libs[k].byz_fltrust_dev(ctxs[k], G, n, d, d, _vp(root.data_ptr()), *ptrs(out), stream))

    def signguard(k, out):
        ok(k, libs[k].byz_signguard_dev(ctxs[k], G, n, d, d, ctypes.byref(sg_params), _vp(sample.data_ptr()), *ptrs(out), stream))

    def dnc(k, out):
        ok(k, libs[k].byz_dnc_dev(ctxs[k], G, n, d, d, ctypes.byref(dnc_params), _vp(columns.data_ptr()), *ptrs(out), stream))

    calls = [(geometric_median, [(d, f32), (n, f64)]), (centered_clip, [(d, f32), (n, f64)]),
             (fltrust, [(d, f32), (n, f64), (n, f64)]), (signguard, [(d, f32), (n, i32), (n, f64), (n, i32)]),
             (dnc, [(d, f32), (n, i32)])]

    def same_bits(a, b):
        return torch.equal(a.view(torch.uint8), b.view(torch.uint8))

    verdicts = {}
    for call, shapes in calls:
        outs = {k: [torch.zeros(length, dtype=dtype, device=device) for length, dtype in shapes] for k in ('old', 'new')}
        for k in ('old', 'new'):
            call(k, outs[k])
        torch.cuda.synchronize()
        line = {'call': call.__name__, 'n': n, 'd': d, 'bits_equal': all(same_bits(a, b) for a, b in zip(outs['old'], outs['new']))}
        if not args.no_time:
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

    if n * d <= 1 << 20:
        # the *_host entry points of the same calls on the host copy: outputs as numpy arrays, old against new
        gh = g.cpu().numpy()
        root_h, sample_h, columns_h = root.cpu().numpy(), sample.cpu().numpy(), columns.cpu().numpy()
        hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)     # noqa: E731
        kept = ctypes.c_int64()
        host_calls = {
            'geometric_median_host': lambda k, o: libs[k].byz_geometric_median_host(ctxs[k], hp(gh), n, d, ctypes.byref(geomed_params), *map(hp, o)),
            'centered_clip_host': lambda k, o: libs[k].byz_centered_clip_host(ctxs[k], hp(gh), n, d, ctypes.byref(cclip_params), hp(root_h), *map(hp, o)),
            'fltrust_host': lambda k, o: libs[k].byz_fltrust_host(ctxs[k], hp(gh), n, d, hp(root_h), *map(hp, o)),
            'signguard_host': lambda k, o: libs[k].byz_signguard_host(ctxs[k], hp(gh), n, d, ctypes.byref(sg_params), hp(sample_h), *map(hp, o)),
            'dnc_host': lambda k, o: libs[k].byz_dnc_host(ctxs[k], hp(gh), n, d, ctypes.byref(dnc_params), hp(columns_h), *map(hp, o), ctypes.byref(kept)),
        }
        np_of = {f32: np.float32, f64: np.float64, i32: np.int32}
        for (call, shapes), (name, host_call) in zip(calls, host_calls.items()):
            outs = {k: [np.zeros(length, dtype=np_of[dtype]) for length, dtype in shapes] for k in ('old', 'new')}
            for k in ('old', 'new'):
                ok(k, host_call(k, outs[k]))
            equal = all(a.tobytes() == b.tobytes() for a, b in zip(outs['old'], outs['new']))
            verdicts[name] = {'bits_equal': equal}
            print(json.dumps({'call': name, 'n': n, 'd': d, 'bits_equal': equal}), flush=True)

    print(json.dumps({'n': n, 'd': d, 'verdicts': verdicts}), flush=True)
    for k in ('old', 'new'):
        libs[k].byz_ctx_destroy(ctxs[k])
    if not all(vd['bits_equal'] for vd in verdicts.values()):
        sys.exit(1)


if __name__ == '__main__':
    main()
