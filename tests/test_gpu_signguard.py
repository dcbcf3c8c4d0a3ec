"""SignGuard on an MI355X, held to the numpy restatement of tests/test_signguard.py.

The bounds.  row_signs: the counts exactly; q the bits of row_dots' sq on the same view; two calls, and a strided view and its
dense copy, the same bits.  signguard_select from the device's own counts and q: labels, keep and the info counts exactly (every
input has margin >= 1e-9, asserted on the device's sums as a precondition of the inputs), M, h and w within rtol 1e-12 (the
project's tolerance for such scalars).  The sum from the device's own w and K: the bits of the sequential restatement.  The
whole call: rtol 1e-6, atol 1e-6 max|G| (tests/test_gpu_fltrust.py's tolerance).

The shapes cross every kernel boundary: one row, fewer rows than a wave's eight, one more than eight, one more than a block of
32, widths one short of a window of 1024, one past it and no multiple of four, more than 4096 rows, 20,000 x 64, one column;
600,000 columns take the four-wide second pass, and a view with an odd leading dimension the scalar loads of both passes.
The census windows start and end inside a chunk, span several chunks, are one whole chunk, and miss chunks entirely."""
import ctypes

import numpy as np
import pytest

from tests.test_signguard import (MARGIN, SHAPES, WIDE, alie, case, restated_census, restated_scaled_sum, restated_select,
                                  restated_signguard, sample_of)

pytestmark = pytest.mark.gpu

INFO_COUNTS = ('kept_rows', 'norm_failed_rows', 'outside_rows', 'clusters', 'seeds')
# (100, 5000) has five chunks of 1024 columns, (33, 2051) three, WIDE 59 of 10,240
WINDOWS = {(100, 5000): [(100, 300), (900, 2500), (1024, 1024), (4990, 10), (0, 5000), (0, 0), (5000, 0), (1023, 2)],
           (33, 2051): [(2047, 4), (0, 1), (2050, 1), (1000, 50)],
           WIDE: [(12000, 100), (15000, 40000), (599_990, 10)]}


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def close(got, want, g):
    scale = float(np.nanmax(np.abs(g[np.isfinite(g)]))) if np.isfinite(g).any() else 1.0
    return np.allclose(got, want, rtol=1e-6, atol=1e-6 * scale)


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:%d' % eng.device)


def odd_view(torch, dense):
    """The same values behind a leading dimension of d + 5, one float past an aligned start: scalar loads."""
    n, d = dense.shape
    view = torch.empty((n, d + 5), dtype=torch.float32, device=dense.device)[:, 1:d + 1]
    view.copy_(dense)
    return view


def host(v):
    if hasattr(v, 'cpu'):
        return v.cpu().numpy()
    return v.numpy() if hasattr(v, 'numpy') else np.asarray(v)


# ---- 1: the census ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', SHAPES + [WIDE])
def test_row_signs_counts_exactly_and_q_is_row_dots_sq(eng, torch, n, d):
    g, window, _, _, _, info = case(n, d)
    gt = on_gpu(torch, eng, g)
    rt = on_gpu(torch, eng, np.ones(d, dtype=np.float32))
    _, sq = eng.row_dots(gt, rt)
    view = odd_view(torch, gt)
    _, view_sq = eng.row_dots(view, rt)
    for c0, m in [window] + WINDOWS.get((n, d), []):
        pos, zero, neg, q = eng.row_signs(gt, c0, m)
        want = restated_census(g, c0, m)
        for got, ref in zip((pos, zero, neg), want[:3]):
            assert np.array_equal(host(got), ref), (c0, m)
        assert torch.equal(q, sq)                                               # the bits of row_dots' sq on the same view
        again = eng.row_signs(gt, c0, m)
        assert all(torch.equal(a, b) for a, b in zip(again, (pos, zero, neg, q)))               # two calls: equal bits
        strided = eng.row_signs(view, c0, m)
        assert all(torch.equal(a, b) for a, b in zip(strided, (pos, zero, neg, q)))             # the scalar loads: equal bits
        assert torch.equal(strided[3], view_sq)
    if n * d <= 1 << 20:
        staged = eng.row_signs(g, *window)                                      # a host matrix, staged
        assert all(np.array_equal(a, host(b)) for a, b in zip(staged, eng.row_signs(gt, *window)))


def test_row_signs_counts_special_values_on_their_bits(eng, torch):
    row = np.array([0.0, -0.0, 1e-45, -1e-45, np.inf, -np.inf, np.nan, -np.nan, 1.0, -2.0], dtype=np.float32)
    g = np.tile(row, (11, 300))                                                 # 3000 columns, three chunks
    gt = on_gpu(torch, eng, g)
    for c0, m in [(0, 3000), (2, 3), (1020, 10), (7, 2990)]:
        pos, zero, neg, _ = eng.row_signs(gt, c0, m)
        want = restated_census(g, c0, m)
        assert all(np.array_equal(host(a), b) for a, b in zip((pos, zero, neg), want[:3]))
    pos, zero, neg, _ = eng.row_signs(gt, 0, 10)
    assert (int(pos[0]), int(zero[0]), int(neg[0])) == (3, 2, 3)                # the two NaNs count nowhere


# ---- 2: the selection from the device's own counts and q ----------------------------------------------------------------
@pytest.mark.parametrize('n,d', SHAPES + [WIDE])
def test_the_selection_alone(eng, torch, n, d):
    g, window, sample, bandwidth, _, _ = case(n, d)
    gt = on_gpu(torch, eng, g)
    pos, zero, neg, q = eng.row_signs(gt, *window)
    want = restated_select(host(pos), host(zero), host(neg), host(q), window[1], bandwidth=bandwidth, sample=sample)
    assert want['margin'] >= MARGIN                              # a precondition of the inputs, not of the kernels
    sel = eng.signguard_select(pos, zero, neg, q, window[1], bandwidth=bandwidth, sample=sample)
    info = eng.signguard_info()
    print((n, d), 'h', info['bandwidth'], want['bandwidth'], 'M', info['median_norm'], want['median_norm'],
          {k: info[k] for k in INFO_COUNTS})
    assert np.array_equal(host(sel['labels']), want['labels'])
    assert np.array_equal(host(sel['keep']), want['keep'])
    assert {k: info[k] for k in INFO_COUNTS} == {k: want[k] for k in INFO_COUNTS}
    assert np.isclose(info['median_norm'], want['median_norm'], rtol=1e-12, atol=0.0)
    assert np.isclose(info['bandwidth'], want['bandwidth'], rtol=1e-12, atol=0.0)
    assert np.allclose(host(sel['weights']), want['weights'], rtol=1e-12, atol=0.0)
    mk = host(sel['mk'])
    assert mk[0] == info['median_norm'] and mk[1] == want['kept']
    # host vectors in: the same selection
    again = eng.signguard_select(host(pos), host(zero), host(neg), host(q), window[1], bandwidth=bandwidth, sample=sample)
    assert np.array_equal(host(again['labels']), host(sel['labels'])) and np.array_equal(host(again['weights']), host(sel['weights']))


# ---- 3: the sum from the device's own weights, and 4: the whole call -----------------------------------------------------
@pytest.mark.parametrize('n,d', SHAPES + [WIDE])
def test_matches_the_restatement(eng, torch, n, d):
    g, window, sample, bandwidth, want, winfo = case(n, d)
    gt = on_gpu(torch, eng, g)
    out, info = eng.signguard(gt, window=window, sample=sample, bandwidth=bandwidth, return_info=True)
    got = host(out)
    print((n, d), 'max |out - want|', float(np.abs(got - want).max()), {k: info[k] for k in INFO_COUNTS})
    assert not np.isnan(got).any() and close(got, want, g)
    assert np.array_equal(host(info['keep']), winfo['keep']) and np.array_equal(host(info['labels']), winfo['labels'])
    assert {k: info[k] for k in INFO_COUNTS} == {k: winfo[k] for k in INFO_COUNTS}
    assert info['window'] == tuple(window)
    # the sum from the device's own w and K: the bits of the sequential restatement
    w, K = host(info['weights']), float(info['kept_rows'])
    assert np.array_equal(got, restated_scaled_sum(g, w, K))
    assert torch.equal(eng.scaled_rows_sum(gt, info['weights'], K), out)
    assert torch.equal(eng.signguard(gt, window=window, sample=sample, bandwidth=bandwidth), out)          # two calls
    view, vinfo = eng.signguard(odd_view(torch, gt), window=window, sample=sample, bandwidth=bandwidth, return_info=True)
    assert torch.equal(view, out) and torch.equal(vinfo['weights'], info['weights'])         # ld > n_cols, odd: the scalar path
    assert torch.equal(vinfo['labels'], info['labels'])


# ---- 5: the other entry points -------------------------------------------------------------------------------------------
def test_host_inputs_defaults_and_bad_arguments(eng, torch):
    from attacking_federate_learning_amd import _native, defences
    from attacking_federate_learning_amd.engine import _vp, signguard_sample, signguard_window
    n, d = 100, 5000
    g, window, sample, _, _, _ = case(n, d)
    gt = on_gpu(torch, eng, g)
    want, winfo = eng.signguard(gt, window=window, sample=sample, return_info=True)
    got, hinfo = eng.signguard(g, window=window, sample=sample, return_info=True)             # the host entry point
    assert np.array_equal(got, host(want))
    for key in ('keep', 'weights', 'labels'):
        assert np.array_equal(hinfo[key], host(winfo[key])), key
    assert {k: hinfo[k] for k in INFO_COUNTS + ('bandwidth', 'median_norm')} == \
        {k: winfo[k] for k in INFO_COUNTS + ('bandwidth', 'median_norm')}
    # the defaults: the window and the sample drawn from the seed
    out7 = defences.signguard(gt, n, 24, seed=7)
    assert torch.equal(out7, eng.signguard(gt, window=signguard_window(d, 0.1, 7), sample=signguard_sample(n, 50, 7)))
    assert np.array_equal(defences.signguard(g, n, 24, seed=7), host(out7))
    _, dinfo = defences.signguard(gt, n, 24, seed=7, return_info=True)
    _, rinfo = restated_signguard(g, signguard_window(d, 0.1, 7), signguard_sample(n, 50, 7))
    assert rinfo['margin'] >= MARGIN
    assert dinfo['window'] == signguard_window(d, 0.1, 7) and np.array_equal(host(dinfo['keep']), rinfo['keep'])
    # frac = 1: the whole row is the window
    _, finfo = eng.signguard(gt, frac=1.0, seed=1, return_info=True)
    _, rinfo = restated_signguard(g, (0, d), signguard_sample(n, 50, 1))
    assert rinfo['margin'] >= MARGIN
    assert finfo['window'] == (0, d) and np.array_equal(host(finfo['keep']), rinfo['keep'])
    # the C ABI's refusals
    lib, ctx = eng.lib, eng.ctx
    out = eng.empty((d,), np.float32)
    dev_sample = eng.to_device(sample)

    def call(params, rows=n, ld=d, out_ptr=out.ptr, sample_ptr=dev_sample.ptr):
        return lib.byz_signguard_dev(ctx, _vp(gt.data_ptr()), rows, d, ld, ctypes.byref(params), _vp(sample_ptr), _vp(out_ptr),
                                     None, None, None, None)
    good = (window[0], window[1], 0.1, 3.0, 0.0, len(sample))
    assert call(_native.SignGuardParams(*good)) == 0
    for bad in [(-1, 10, 0.1, 3.0, 0.0, 50), (0, 0, 0.1, 3.0, 0.0, 50), (4995, 10, 0.1, 3.0, 0.0, 50), (0, 10, -0.1, 3.0, 0.0, 50),
                (0, 10, 3.0, 3.0, 0.0, 50), (0, 10, 0.1, float('nan'), 0.0, 50), (0, 10, 0.1, 3.0, -1.0, 50),
                (0, 10, 0.1, 3.0, float('nan'), 50), (0, 10, 0.1, 3.0, 0.0, 0), (0, 10, 0.1, 3.0, 0.0, 1025),
                (0, 10, 0.1, 3.0, 0.0, n + 1)]:
        assert call(_native.SignGuardParams(*bad)) == _native.E_INVALID, bad
    assert call(_native.SignGuardParams(*good), sample_ptr=None) == _native.E_INVALID
    assert call(_native.SignGuardParams(0, 10, 0.1, 3.0, 0.5, 0), sample_ptr=None) == 0          # a given bandwidth needs no sample
    assert call(_native.SignGuardParams(*good), out_ptr=gt.data_ptr() + 4000) == _native.E_INVALID
    assert 'overlaps' in _native.last_error()
    assert call(_native.SignGuardParams(*good), out_ptr=None) == _native.E_INVALID
    assert call(_native.SignGuardParams(*good), rows=0) == _native.E_INVALID
    assert call(_native.SignGuardParams(*good), ld=d - 1) == _native.E_INVALID
    assert lib.byz_signguard_dev(ctx, _vp(gt.data_ptr()), (1 << 20) + 1, 1, 1, ctypes.byref(_native.SignGuardParams(0, 1, 0.1, 3.0, 0.5, 0)),
                                 None, _vp(out.ptr), None, None, None, None) == _native.E_UNSUPPORTED
    eng.check()
    with pytest.raises(ValueError):
        eng.signguard(gt, window=(4995, 10))
    with pytest.raises(ValueError):
        eng.signguard(gt, sample=[1, 1, 2])
    with pytest.raises(ValueError):
        eng.signguard(g, sample=[n])


# ---- 6: the edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [120, 4200])
def test_non_finite_rows_are_never_kept(eng, torch, n):
    d = 1100
    g = alie(n, d, seed=35).copy()
    g[n - 5, 17], g[n - 40, 17], g[n - 77, 17] = np.nan, np.inf, -np.inf
    window, sample = (900, 150), sample_of(n, seed=35)
    want, winfo = restated_signguard(g, window, sample)
    assert winfo['margin'] >= MARGIN
    out, info = eng.signguard(on_gpu(torch, eng, g), window=window, sample=sample, return_info=True)
    assert torch.isfinite(out).all() and close(host(out), want, g)
    assert np.array_equal(host(info['keep']), winfo['keep']) and np.array_equal(host(info['labels']), winfo['labels'])
    assert host(info['keep'])[[n - 5, n - 40, n - 77]].tolist() == [0, 0, 0]
    assert host(info['weights'])[[n - 5, n - 40, n - 77]].tolist() == [0.0, 0.0, 0.0]
    assert info['norm_failed_rows'] == winfo['norm_failed_rows'] >= 3


def test_no_kept_row_identical_rows_and_a_scaled_row(eng, torch):
    zeros = np.zeros(300, dtype=np.float32)
    bad = np.full((6, 300), np.inf, dtype=np.float32)
    bad[::2] = np.nan
    for matrix in (bad, on_gpu(torch, eng, bad)):                               # nothing but non-finite rows: M is NaN
        out, info = eng.signguard(matrix, window=(0, 30), bandwidth=1.0, return_info=True)
        assert np.array_equal(host(out), zeros)
        assert (info['kept_rows'], info['norm_failed_rows']) == (0, 6) and np.isnan(info['median_norm'])
    g = alie(10, 300, seed=9, mal_prop=0.0)
    out, info = eng.signguard(on_gpu(torch, eng, g), window=(0, 30), lower=0.0, upper=1e-3, bandwidth=10.0, return_info=True)
    assert torch.equal(out, torch.zeros_like(out)) and (info['kept_rows'], info['norm_failed_rows']) == (0, 10)
    same = np.repeat(alie(1, 300, seed=6), 12, axis=0)                          # identical rows: h = 0, one cluster
    out, info = eng.signguard(on_gpu(torch, eng, same), window=(10, 30), sample=sample_of(12, seed=6), return_info=True)
    assert (info['bandwidth'], info['clusters'], info['seeds'], info['kept_rows']) == (0.0, 1, 0, 12)
    assert np.array_equal(host(out), same[0]) and (host(info['labels']) == 0).all()
    g = alie(30, 800, seed=4, mal_prop=0.0).copy()
    g[7] *= 10.0                                                                # ten times the median norm: filtered
    out, info = eng.signguard(on_gpu(torch, eng, g), window=(100, 80), bandwidth=10.0, return_info=True)
    assert host(info['keep'])[7] == 0 and (info['norm_failed_rows'], info['kept_rows']) == (1, 29)
    want, _ = restated_signguard(g, (100, 80), bandwidth=10.0)
    assert close(host(out), want, g)
    # open bounds and one cluster: the mean of the rows clipped to the median norm
    out, info = eng.signguard(on_gpu(torch, eng, g), window=(0, 800), lower=0.0, upper=np.inf, bandwidth=10.0, return_info=True)
    x = g.astype(np.float64)
    norm = np.sqrt((x * x).sum(axis=1))
    assert info['kept_rows'] == 30 and np.isclose(info['median_norm'], np.median(norm), rtol=1e-12)
    assert np.allclose(host(out), (x * np.minimum(1.0, np.median(norm) / norm)[:, None]).mean(axis=0), rtol=1e-6, atol=1e-6)


# ---- 7: the columns layout -----------------------------------------------------------------------------------------------
def test_sharded_aggregator_over_uneven_column_shards_matches_one_gpu(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator

    class LoopedKernels(HipKernels):
        """Every shard on this GPU: the counts and norms add the shards' parts, as the all-reduce over the ranks would."""

        def __init__(self, engine, bounds):
            super().__init__(engine)
            self.bounds = bounds

        def row_signs(self, g, window_start, window_len):
            total = None
            for lo, hi in self.bounds:
                a, b = max(window_start, lo), min(window_start + window_len, hi)
                part = self.engine.row_signs(g[:, lo:hi], a - lo if b > a else 0, max(0, b - a))
                total = part if total is None else tuple(x + y for x, y in zip(total, part))
            return total

        def scaled_rows_sum(self, g, weights, divisor):
            return torch.cat([self.engine.scaled_rows_sum(g[:, lo:hi], weights, divisor) for lo, hi in self.bounds])

    n, d = 100, 5000
    g, window, sample, _, _, _ = case(n, d)
    gt = on_gpu(torch, eng, g)
    want, winfo = eng.signguard(gt, window=window, sample=sample, return_info=True)
    for cuts in ([0, d], [0, d // 3 + 1, d], [0, window[0] + 7, window[0] + 9, d]):
        kern = LoopedKernels(eng, list(zip(cuts[:-1], cuts[1:])))
        got, info = ShardedAggregator(kern).signguard(gt, window=window, sample=sample, return_info=True)
        assert close(host(got), host(want), g)
        if len(cuts) == 2:
            assert torch.equal(got, want)                      # one shard: the same sums, the same result
        assert torch.equal(info['keep'], winfo['keep']) and torch.equal(info['labels'], winfo['labels'])
        assert np.allclose(host(info['weights']), host(winfo['weights']), rtol=1e-12, atol=0.0)
        assert {k: info[k] for k in INFO_COUNTS} == {k: winfo[k] for k in INFO_COUNTS}


# ---- 8: the server's round -----------------------------------------------------------------------------------------------
def test_device_server_draws_a_new_window_every_round(eng, torch):
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import signguard_window
    from attacking_federate_learning_amd.server import DeviceServer
    n, d = 50, 4000
    rng = np.random.default_rng(45)
    weights = rng.standard_normal(d).astype(np.float32)
    dev = 'cuda:%d' % eng.device
    server = DeviceServer(n, weights, 0.24, 0.1, 0.9, torch_device=dev, engine=eng)
    w, vel = on_gpu(torch, eng, weights), torch.zeros(d, dtype=torch.float32, device=dev)
    assert signguard_window(d, 0.1, 0) != signguard_window(d, 0.1, 1)           # the window moves between the rounds
    for round_no, seed in enumerate((46, 47)):
        g = alie(n, d, seed=seed)
        server.users_grads.data.copy_(on_gpu(torch, eng, g))
        agg = server.defend_signguard()
        assert server.signguard_round == round_no + 1
        want, info = defences.signguard(on_gpu(torch, eng, g), n, 12, seed=round_no, return_info=True)
        assert info['window'] == signguard_window(d, 0.1, round_no)
        assert torch.equal(agg, want)
        eng.server_update(w, vel, want, 0.9, 0.1)
        assert torch.equal(server.current_weights, w) and torch.equal(server.velocity, vel)
