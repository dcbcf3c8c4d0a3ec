"""Timing of the Fang et al. attacks on one MI355X, each next to its yardstick.  Every figure of a run comes from ONE process:

    python scripts/fang_timing.py                              # 1000 x 1e6 with c = 200, then 4000 x 1e7 with c = 800
    python scripts/fang_timing.py --n 1000 --d 1000000 --c 200 --mode trmean

trmean: through the C ABI, `byz_column_extremes_dev` beside `byz_no_defense_dev` on the same matrix (the same bytes, two more
outputs); `byz_fang_fill_dev` into the c attacker rows, full and partial, beside `byz_gaussian_noise_dev` in place on the same c x
d floats (the same generator, one block per four values; the noise reads what it writes and pays the Box-Muller transform), both
as ns per element written; the whole `byz_fang_trmean_attack_dev`.  The calls alternate: a round times `--steps` calls of each
back to back with device events, the figure is the median over `--rounds` rounds with the lowest and highest beside it.

krum: benign rows far from the origin, so that no lambda succeeds and the number of steps is the threshold's to choose:
`byz_fang_krum_attack_dev` at two thresholds, the difference of the two times over the difference of the step counts is ONE step
(the fill of the attackers' rows and columns, the library's Krum selection, the read of its index); beside it one
`byz_krum_select_dev` on the same n, and `byz_pairwise_distances_dev` + `byz_row_dots_dev` on the benign block, which is what the
attack cannot avoid.  Wall time of synchronous calls (the attack reads an index per step).  One JSON line per measurement.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geomed_timing import PEAK_HBM  # noqa: E402
from sparsefed_timing import alternate, summarise  # noqa: E402


def matrix(torch, device, n, d, shift=0.0):
    gen = torch.Generator(device=device).manual_seed(n + d)
    g = torch.empty((n, d), dtype=torch.float32, device=device)
    g.normal_(generator=gen)
    if shift:
        g.add_(shift)
    torch.cuda.synchronize()
    return g


def run_trmean(args, eng, torch, device, n, d, c, steps, warmup, rounds):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    g = matrix(torch, device, n, d)
    stream = torch.cuda.current_stream(device).cuda_stream
    mean, lo, hi, mu, sigma = (torch.empty(d, dtype=torch.float32, device=device) for _ in range(5))
    full, partial = _native.FangParams(2.0, 3.0, 4.0, 0, 2020, 3, 0), _native.FangParams(2.0, 3.0, 4.0, 1, 2020, 3, 0)
    noise = _native.NoiseParams(0.01, 2020, 3, 0)
    gp, ptr = _vp(g.data_ptr()), lambda t: _vp(t.data_ptr())
    _check(eng.lib.byz_column_extremes_dev(eng.ctx, gp, n, d, d, c, ptr(mean), ptr(lo), ptr(hi), _vp(stream)))
    _check(eng.lib.byz_drift_attack_dev(eng.ctx, gp, c, d, d, 0.0, None, ptr(mu), ptr(sigma), 0, _vp(stream)))
    agg = torch.empty(d, dtype=torch.float32, device=device)
    _check(eng.lib.byz_no_defense_dev(eng.ctx, gp, n, d, d, ptr(agg), _vp(stream)))
    assert torch.equal(agg.view(torch.int32), mean.view(torch.int32))             # the same chain: no_defense's bits
    calls = {
        'no_defense': lambda: _check(eng.lib.byz_no_defense_dev(eng.ctx, gp, n, d, d, ptr(agg), _vp(stream))),
        'column_extremes': lambda: _check(eng.lib.byz_column_extremes_dev(eng.ctx, gp, n, d, d, c, ptr(mean), ptr(lo), ptr(hi), _vp(stream))),
        'gaussian_noise': lambda: _check(eng.lib.byz_gaussian_noise_dev(eng.ctx, gp, c * d, ctypes.byref(noise), None, gp, _vp(stream))),
        'fill_full': lambda: _check(eng.lib.byz_fang_fill_dev(eng.ctx, gp, c, d, d, ctypes.byref(full), ptr(mean), ptr(lo), ptr(hi), _vp(stream))),
        'fill_partial': lambda: _check(eng.lib.byz_fang_fill_dev(eng.ctx, gp, c, d, d, ctypes.byref(partial), ptr(mu), ptr(sigma), None,
                                                                 _vp(stream))),
        'attack_full': lambda: _check(eng.lib.byz_fang_trmean_attack_dev(eng.ctx, gp, n, d, d, c, ctypes.byref(full), _vp(stream))),
        'attack_partial': lambda: _check(eng.lib.byz_fang_trmean_attack_dev(eng.ctx, gp, n, d, d, c, ctypes.byref(partial), _vp(stream))),
    }
    line = {'mode': 'trmean', 'n': n, 'd': d, 'c': c, 'steps': steps, 'warmup': warmup, 'rounds': rounds}
    summarise(line, alternate(calls, steps, warmup, rounds), base='no_defense')
    line['no_defense_hbm_frac'] = round(4.0 * n * d / (line['no_defense_ms'] * 1e-3) / PEAK_HBM, 4)
    line['column_extremes_hbm_frac'] = round(4.0 * n * d / (line['column_extremes_ms'] * 1e-3) / PEAK_HBM, 4)
    for name in ('gaussian_noise', 'fill_full', 'fill_partial'):
        line[name + '_ns_per_element'] = round(line[name + '_ms'] * 1e6 / (c * d), 5)
    line['fill_full_vs_noise'] = round(line['fill_full_ms'] / line['gaussian_noise_ms'], 3)
    line['fill_partial_vs_noise'] = round(line['fill_partial_ms'] / line['gaussian_noise_ms'], 3)
    del g
    torch.cuda.empty_cache()
    return line


def wall(call, sync, repeats):
    out = []
    for _ in range(repeats):
        sync()
        start = time.perf_counter()
        call()
        sync()
        out.append((time.perf_counter() - start) * 1e3)
    return out


def run_krum(args, eng, torch, device, n, d, c, repeats):
    from attacking_federate_learning_amd.engine import _check, _vp
    # |mu_j| = 3 against unit noise: far enough that no lambda succeeds, near enough that the benign rows are no "near-duplicate
    # pairs" of the distance kernel (d^2 = 2 d against (c_ii + c_jj) / 16 = 1.25 d), whose list would overflow
    g = matrix(torch, device, n, d, shift=3.0)
    honest = g[:c].clone()
    m = n - c
    stream = torch.cuda.current_stream(device).cuda_stream
    sync = torch.cuda.synchronize
    gp = _vp(g.data_ptr())
    dist = torch.empty((n, n), dtype=torch.float32, device=device)
    block = torch.empty((m, m), dtype=torch.float32, device=device)
    s = torch.ones(d, dtype=torch.float32, device=device)
    t, q = torch.empty(m, dtype=torch.float64, device=device), torch.empty(m, dtype=torch.float64, device=device)
    index = ctypes.c_int32(-2)

    def attack(threshold):
        th = ctypes.c_double(threshold)

        def call():
            g[:c].copy_(honest)
            _check(eng.lib.byz_fang_krum_attack_dev(eng.ctx, gp, n, d, d, c, ctypes.byref(th), _vp(dist.data_ptr()), None, None, _vp(stream)))
        return call

    def benign_work():
        _check(eng.lib.byz_pairwise_distances_dev(eng.ctx, _vp(g[c:].data_ptr()), m, d, d, _vp(block.data_ptr()), _vp(stream)))
        _check(eng.lib.byz_row_dots_dev(eng.ctx, _vp(g[c:].data_ptr()), m, d, d, _vp(s.data_ptr()), _vp(t.data_ptr()), _vp(q.data_ptr()),
                                        _vp(stream)))

    def select():
        _check(eng.lib.byz_krum_select_dev(eng.ctx, _vp(dist.data_ptr()), n, n, c, ctypes.byref(index), None, _vp(stream)))

    line = {'mode': 'krum', 'n': n, 'd': d, 'c': c, 'repeats': repeats}
    infos = {}
    for name, threshold in (('attack_few_steps', 1e-2), ('attack_many_steps', 1e-6)):
        call = attack(threshold)
        call()                                                                # warm: the workspaces grow here
        infos[name] = eng.fang_krum_info()
        ms = wall(call, sync, repeats)
        line[name + '_ms'], line[name + '_ms_min_max'] = round(statistics.median(ms), 4), [round(min(ms), 4), round(max(ms), 4)]
        line[name + '_steps'] = infos[name]['steps']
    assert not infos['attack_many_steps']['succeeded']
    for name, call in (('distances_and_row_dots', benign_work), ('krum_select', select)):
        call()
        ms = wall(call, sync, repeats)
        line[name + '_ms'], line[name + '_ms_min_max'] = round(statistics.median(ms), 4), [round(min(ms), 4), round(max(ms), 4)]
    more = line['attack_many_steps_steps'] - line['attack_few_steps_steps']
    line['step_ms'] = round((line['attack_many_steps_ms'] - line['attack_few_steps_ms']) / more, 4)
    line['step_vs_krum_select'] = round(line['step_ms'] / line['krum_select_ms'], 3)
    line['attack_few_steps_vs_distances_and_row_dots'] = round(line['attack_few_steps_ms'] / line['distances_and_row_dots_ms'], 3)
    line['lambda0'] = infos['attack_many_steps']['lambda0']
    del g, dist, block
    torch.cuda.empty_cache()
    return line


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', default='all', choices=['all', 'trmean', 'krum'])
    p.add_argument('--n', type=int, default=0, help='0: both of the recorded sizes')
    p.add_argument('--d', type=int, default=1_000_000)
    p.add_argument('--c', type=int, default=200)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from attacking_federate_learning_amd.engine import get_engine
    eng = get_engine()
    device = torch.device('cuda', eng.device)
    sizes = [(args.n, args.d, args.c, args.steps, args.warmup, args.rounds, 5)] if args.n else [
        (1000, 1_000_000, 200, args.steps, args.warmup, args.rounds, 5), (4000, 10_000_000, 800, 2, 1, 3, 3)]
    for n, d, c, steps, warmup, rounds, repeats in sizes:
        if args.mode in ('all', 'trmean'):
            print(json.dumps(run_trmean(args, eng, torch, device, n, d, c, steps, warmup, rounds)), flush=True)
        if args.mode in ('all', 'krum'):
            print(json.dumps(run_krum(args, eng, torch, device, n, d, c, repeats)), flush=True)


if __name__ == '__main__':
    main()
