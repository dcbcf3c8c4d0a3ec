"""The mean of the values nearest a given centre, Phocas and MeaMed on an MI355X (csrc/centre_window.hip), held to
the numpy restatement of tests/test_phocas.py: `radius` with its bits as integers, `out` within the bar |out - ref| <= 2^-23 |ref|
+ 2^-30 mabs + 2^-149 per element, where `ref` is the fp64 numpy mean of col[kept] (pairwise sums: its own error is (keep - 1)
2^-53 mabs at most, a thousandth of the bar's second term).  The kept rows are the restatement's: ties in |x - c| go to the
earlier LOGICAL row, and on the tie recipe the reversed order gives another answer in most columns, so a kernel that broke ties
any other way fails the bar there.  The heights straddle every edge of the dispatcher (256, 1024, 2304 and 4096 rows for the
register tiles, then the streamed kernel; 65,535 / 65,536 is where rank_select.hip's counters change and this kernel's do not);
nothing forces a kernel."""
import ctypes

import numpy as np
import pytest

from tests.test_phocas import (TIE_SHAPES, order_matters, restated_window, same_radius, tie_case, window_order,
                               window_within_bar)
from tests.test_rank_trim import negative_nan

pytestmark = pytest.mark.gpu

HEIGHTS = [1, 2, 3, 255, 256, 257, 1024, 1025, 2304, 2305, 4096, 4097, 65535, 65536]


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def on_device(eng, torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', eng.device))


def keeps(n):
    return sorted({k for k in (1, 2, n // 2, n - 1, n) if 1 <= k <= n})


def make(kind, n, d, seed):
    """(g, centre).  normal: normals around a centre of its own; tie: the tie recipe; attack: rows 0 .. 0.24 n are one
    vector (the drift attack's identical rows), the centre the column means."""
    rng = np.random.default_rng(seed)
    if kind == 'tie':
        return tie_case(n, d, seed)
    g = rng.standard_normal((n, d)).astype(np.float32)
    if kind == 'attack':
        g[:int(0.24 * n)] = (g.mean(axis=0) - np.float32(1.5) * g.std(axis=0)).astype(np.float32)
        return g, g.mean(axis=0).astype(np.float32)
    return g, (0.5 * rng.standard_normal(d)).astype(np.float32)


def check_window(eng, torch, g, c, ks, gt=None, ct=None):
    """window_mean on (g, c) for every keep of ks against the restatement; returns {keep: out}."""
    gt = on_device(eng, torch, g) if gt is None else gt
    ct = on_device(eng, torch, c) if ct is None else ct
    ordered = window_order(g, c)
    got = {}
    for keep in ks:
        out, radius = eng.window_mean(gt, ct, keep, return_radius=True)
        out, radius = out.cpu().numpy(), radius.cpu().numpy()
        want, want_radius, kept = restated_window(g, c, keep, ordered)
        assert same_radius(radius, want_radius), ('radius', g.shape, keep)
        assert window_within_bar(out, g, kept), ('out', g.shape, keep)
        got[keep] = out
    return got


# ---- heights, keeps, data ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', HEIGHTS)
@pytest.mark.parametrize('kind', ['normal', 'tie', 'attack'])
def test_every_height_either_side_of_the_dispatch_edges(eng, torch, n, kind):
    d = 259 if n <= 4096 else 256
    g, c = make(kind, n, d, seed=n + len(kind))
    check_window(eng, torch, g, c, keeps(n))


@pytest.mark.parametrize('n,keep', TIE_SHAPES)
def test_ties_go_to_the_earlier_row_not_the_later_one(eng, torch, n, keep):
    g, c = tie_case(n, 256, seed=n)
    fwd, rev, differ = order_matters(g, c, keep)
    assert np.count_nonzero(differ) >= 0.2 * 256          # the recipe discriminates here (the CPU file asserts it as well)
    out = check_window(eng, torch, g, c, [keep])[keep]    # within the bar of the forward choice in every column, so:
    assert not np.any(out[differ] == rev[differ])


@pytest.mark.parametrize('d', [1, 15, 17, 63, 65, 1000])
@pytest.mark.parametrize('n', [1000, 5000])
def test_column_counts_that_are_not_multiples_of_the_tile(eng, torch, n, d):
    g, c = make('normal', n, d, seed=n + d)
    g[:, ::2], c[::2] = tie_case(n, (d + 1) // 2, seed=d)
    check_window(eng, torch, g, c, [int(0.76 * n)])


@pytest.mark.parametrize('d', [1, 17, 2051])
@pytest.mark.parametrize('n', [300, 2305])
def test_sixteen_column_tiles_whose_count_is_no_multiple_of_eight(eng, torch, n, d):
    """Both heights take 16-column tiles, whose workgroups are regrouped by eights (column_select.hpp: column_tile): 1, 2 and
    129 tiles leave workgroups beyond the last tile and a last tile that is not full.  Without row_index and with one."""
    rng = np.random.default_rng(n + d)
    full, c = make('normal', n + 7, d, seed=n + d)
    full[:, ::2], c[::2] = tie_case(n + 7, (d + 1) // 2, seed=d)
    keep = int(0.76 * n)
    index = rng.permutation(n + 7)[:n]
    logical = np.ascontiguousarray(full[index])
    want = check_window(eng, torch, logical, c, [keep])[keep]
    ft, ct = on_device(eng, torch, full), on_device(eng, torch, c)
    idx = torch.from_numpy(index.astype(np.int32)).to(ft.device)
    got, radius = eng.window_mean(ft, ct, keep, row_index=idx, return_radius=True)
    want_radius, kept = restated_window(logical, c, keep)[1:]
    assert same_radius(radius.cpu().numpy(), want_radius)
    assert window_within_bar(got.cpu().numpy(), logical, kept)
    assert got.cpu().numpy().tobytes() == want.tobytes()


# ---- special columns ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [7, 1000, 2080, 4000, 6001])
def test_constant_and_two_valued_columns_are_exact(eng, torch, n):
    g = np.empty((n, 40), dtype=np.float32)
    g[:, :20] = np.float32(0.1) * np.arange(1, 21, dtype=np.float32)[None, :]      # constant columns: the value itself
    g[:, 20:] = np.where(np.arange(n)[:, None] % 3 == 0, np.float32(-1.75), np.float32(3.25))
    c = np.linspace(-2.0, 4.0, 40).astype(np.float32)                              # nearer to one value, then to the other
    c[20] = 0.75                                                                   # the same distance to both: all ties
    for keep, out in check_window(eng, torch, g, c, keeps(n)).items():
        assert np.array_equal(out[:20], g[0, :20]), (n, keep)
        kept = restated_window(g, c, keep)[2]
        exact = (np.take_along_axis(g, kept, axis=0).astype(np.float64).sum(axis=0) / keep).astype(np.float32)   # (exact sums)
        assert np.array_equal(out[20:], exact[20:]), (n, keep)


@pytest.mark.parametrize('n', [9, 300, 1500, 5000])
def test_non_finite_values_and_centres(eng, torch, n):
    rng = np.random.default_rng(n)
    keep = (2 * n) // 3
    g = rng.standard_normal((n, 16)).astype(np.float32)
    c = (0.1 * rng.standard_normal(16)).astype(np.float32)
    rows = rng.permutation(n)
    spare = n - keep
    g[rows[:spare], 0] = np.nan; g[rows[:spare:2], 0] = negative_nan()      # as many NaNs as are trimmed: none kept
    g[rows[:spare + 1], 1] = np.nan                                         # one more: a NaN is kept
    g[rows[:spare], 2] = np.inf                                             # trimmed
    g[rows[:spare + 1], 3] = np.inf                                         # one kept: +inf
    g[rows[:spare + 1], 4] = -np.inf                                        # one kept: -inf
    g[rows[:spare + 2], 5] = np.inf; g[np.sort(rows[:spare + 2])[:2], 5] = [-np.inf, np.inf]   # the two kept: -inf and +inf
    c[6] = np.nan                                                           # the first `keep` rows
    c[7] = np.inf; c[8] = -np.inf
    c[9] = np.inf; g[rows[:3], 9] = np.inf                                  # inf - inf: NaN distances behind the +inf ones
    g[:, 10] = np.nan; g[::2, 10] = negative_nan()                          # a column that is all NaN
    g[:, 11] = np.inf
    g[rows[:2], 12] = negative_nan()                                        # a negative NaN must not sort first
    with np.errstate(all='ignore'):
        got = check_window(eng, torch, g, c, [keep, 1, n])[keep]
    assert np.isfinite(got[0]) and np.isnan(got[1]) and np.isfinite(got[2]) and got[3] == np.inf and got[4] == -np.inf
    assert np.isnan(got[5]) and np.isfinite(got[6]) and np.isfinite(got[7]) and np.isfinite(got[12])
    assert got[6] == np.float32(g[:keep, 6].astype(np.float64).sum() / keep)


# ---- views and calls ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [300, 1000, 2080, 4000, 6000])
def test_row_index_strided_view_misaligned_base_and_host_matrix(eng, torch, n):
    rng = np.random.default_rng(n)
    full, c_full = tie_case(n + 50, 333, seed=n)
    keep = int(0.76 * n)
    ft = on_device(eng, torch, full)
    ct = on_device(eng, torch, c_full)
    for name, index in (('permutation', rng.permutation(n + 50)[:n]), ('subset', np.sort(rng.permutation(n + 50)[:n]))):
        logical = np.ascontiguousarray(full[index])
        # ties follow the LOGICAL order: the restatement on the rows as the index lists them
        want = check_window(eng, torch, logical, c_full, [keep])[keep]
        idx = torch.from_numpy(index.astype(np.int32)).to(ft.device)
        for row_index in (idx, index):                     # a device index and a host one
            got, rad = eng.window_mean(ft, ct, keep, row_index=row_index, return_radius=True)
            assert got.cpu().numpy().tobytes() == want.tobytes(), name
            assert same_radius(rad.cpu().numpy(), restated_window(logical, c_full, keep)[1])
        assert eng.phocas(ft, n // 4, row_index=idx).cpu().numpy().tobytes() == \
            eng.phocas(on_device(eng, torch, logical), n // 4).cpu().numpy().tobytes(), name
    logical, c = np.ascontiguousarray(full[:n, 11:210]), np.ascontiguousarray(c_full[11:210])
    want = check_window(eng, torch, logical, c, [keep])[keep]
    view = ft[:n, 11:210]                                  # a strided view whose base is 44 bytes into a row
    assert view.stride(0) == 333 and view.data_ptr() % 16 != 0
    assert eng.window_mean(view, ct[11:210].contiguous(), keep).cpu().numpy().tobytes() == want.tobytes()
    assert eng.window_mean(view, ct[11:210], keep).cpu().numpy().tobytes() == want.tobytes()      # a misaligned centre as well
    host, host_radius = eng.window_mean(logical, c, keep, return_radius=True)
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and host.tobytes() == want.tobytes()
    assert same_radius(host_radius, restated_window(logical, c, keep)[1])
    assert eng.window_mean(view, c, keep).cpu().numpy().tobytes() == want.tobytes()               # a host centre, device matrix
    assert eng.window_mean(logical, c, keep, row_index=np.arange(n)[::-1]).tobytes() == \
        eng.window_mean(np.ascontiguousarray(logical[::-1]), c, keep).tobytes()
    with pytest.raises(ValueError):
        eng.window_mean(ft, ct, keep, row_index=np.array([0, n + 50]))


def column_bounds(d):
    cuts = [0, d // 5, d // 5 + d // 2 + 1, d]
    return list(zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize('n', [200, 1000, 2080, 4000, 6000])
def test_two_calls_and_three_uneven_column_shards_give_the_same_bits(eng, torch, n):
    from attacking_federate_learning_amd.sharded import HipKernels
    kern = HipKernels(eng)
    d = 4099
    g, c = tie_case(n, d, seed=n)
    g[:, ::3] = np.random.default_rng(n).standard_normal((n, (d + 2) // 3)).astype(np.float32)
    keep, b = int(0.76 * n), int(0.24 * n)
    gt, ct = on_device(eng, torch, g), on_device(eng, torch, c)
    out = eng.window_mean(gt, ct, keep).cpu().numpy()
    ph = eng.phocas(gt, b).cpu().numpy()
    assert eng.window_mean(gt, ct, keep).cpu().numpy().tobytes() == out.tobytes()
    assert eng.phocas(gt, b).cpu().numpy().tobytes() == ph.tobytes()
    slices = [(gt[:, lo:hi], ct[lo:hi]) for lo, hi in column_bounds(d)]
    assert np.concatenate([kern.window_mean(v, cv, keep).cpu().numpy() for v, cv in slices]).tobytes() == out.tobytes()
    assert np.concatenate([kern.phocas(v, b).cpu().numpy() for v, _ in slices]).tobytes() == ph.tobytes()


def test_sharded_aggregator_at_world_size_one(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d, f = 150, 4099, 36
    g = np.random.default_rng(16).standard_normal((n, d)).astype(np.float32)
    g[9, 100] = np.nan
    gt = on_device(eng, torch, g)
    agg = ShardedAggregator(HipKernels(eng))
    ph = agg.phocas(gt, n, f, gather=True, total_columns=d).cpu().numpy()
    assert ph.tobytes() == eng.phocas(gt, f).cpu().numpy().tobytes()
    centre = eng.rank_trimmed_mean(gt, f)
    wm = agg.window_mean(gt, centre, n - f, gather=True, total_columns=d).cpu().numpy()
    assert wm.tobytes() == ph.tobytes() and np.isfinite(ph[100])
    with np.errstate(all='ignore'):
        kept = restated_window(g, centre.cpu().numpy(), n - f)[2]
        assert window_within_bar(ph, g, kept)
    with pytest.raises(AssertionError):
        agg.phocas(gt, n, 75)


# ---- Phocas is the composition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [11, 1000, 2305, 4097])
def test_phocas_is_the_window_around_the_rank_trimmed_means_bits(eng, torch, n):
    from attacking_federate_learning_amd.engine import _check, _vp
    d, b = 515, int(0.24 * n)
    g = tie_case(n, d, seed=n)[0]
    g[:, ::2] = np.random.default_rng(n).standard_normal((n, (d + 1) // 2)).astype(np.float32)
    gt = on_device(eng, torch, g)
    centre = eng.rank_trimmed_mean(gt, b)
    by_hand = eng.window_mean(gt, centre, n - b).cpu().numpy()
    ph = eng.phocas(gt, b).cpu().numpy()
    assert ph.tobytes() == by_hand.tobytes()
    with np.errstate(all='ignore'):
        kept = restated_window(g, centre.cpu().numpy(), n - b)[2]
    assert window_within_bar(ph, g, kept)
    # centre_out and radius of the one call, through the C interface
    out, centre_out, radius = (torch.empty(d, dtype=torch.float32, device=gt.device) for _ in range(3))
    _check(eng.lib.byz_phocas_dev(eng.ctx, _vp(gt.data_ptr()), n, d, d, None, b, _vp(out.data_ptr()), _vp(centre_out.data_ptr()),
                                  _vp(radius.data_ptr()), None))
    eng.synchronize()
    assert out.cpu().numpy().tobytes() == ph.tobytes()
    assert centre_out.cpu().numpy().tobytes() == centre.cpu().numpy().tobytes()
    assert same_radius(radius.cpu().numpy(), restated_window(g, centre.cpu().numpy(), n - b)[1])
    # and through _host: the host matrix in, numpy out
    host = eng.phocas(g, b)
    assert isinstance(host, np.ndarray) and host.tobytes() == ph.tobytes()
    assert eng.window_mean(g, eng.rank_trimmed_mean(g, b), n - b).tobytes() == ph.tobytes()
    h_out, h_centre, h_radius = (np.empty(d, dtype=np.float32) for _ in range(3))
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _check(eng.lib.byz_phocas_host(eng.ctx, hp(g), n, d, b, hp(h_out), hp(h_centre), hp(h_radius)))
    assert h_out.tobytes() == ph.tobytes() and h_centre.tobytes() == centre.cpu().numpy().tobytes()
    assert h_radius.tobytes() == radius.cpu().numpy().tobytes()


# ---- the reference's rule as a second oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [101, 1001, 5633])
@pytest.mark.parametrize('kind', ['uniform', 'tie'])
def test_around_the_median_it_keeps_what_the_references_trimmed_mean_keeps(eng, torch, n, kind):
    """window_mean(g, coordinate_median(g), n - f - 1) against trimmed_mean(g, n, f): the same kept set (the reference's
    sorted(key=abs) is stable: ties in row order), another finish -- the fp64 sum of x here, the reference's fp32
    mean(kept - med) + med there.  Absolute 2e-5: the 1e-5 the project holds trimmed_mean to, plus the fp32 pairwise mean's
    1.2e-6 for |d| <= 2 and k < 2^13, plus the bar."""
    d, f = 300, int(0.24 * n)
    if kind == 'uniform':
        g = np.random.default_rng(n).uniform(-1.0, 1.0, size=(n, d)).astype(np.float32)
    else:
        g = tie_case(n, d, seed=n, scale=0.1)[0]
    gt = on_device(eng, torch, g)
    ours = eng.window_mean(gt, eng.coordinate_median(gt), n - f - 1).cpu().numpy()
    theirs = eng.trimmed_mean(gt, n, f).cpu().numpy()
    worst = float(np.abs(ours.astype(np.float64) - theirs.astype(np.float64)).max())
    print('window_mean against trimmed_mean, n = %d, %s: max abs difference %.3g' % (n, kind, worst))
    assert worst <= 2e-5


# ---- large shapes -------------------------------------------------------------------------------------------------------------
def test_the_wide_case_needs_64_bit_column_arithmetic(eng, torch):
    n, d, keep = 1000, 600000, 760          # 2.4e9 bytes: element offsets beyond 2^31 / 4, byte offsets beyond 2^31
    device = torch.device('cuda', eng.device)
    gen = torch.Generator(device=device).manual_seed(5)
    gt = torch.empty((n, d), dtype=torch.float32, device=device)
    gt.normal_(generator=gen)
    ct = torch.empty(d, dtype=torch.float32, device=device)
    ct.normal_(generator=gen).mul_(0.25)
    out, radius = eng.window_mean(gt, ct, keep, return_radius=True)
    out, radius, c = out.cpu().numpy(), radius.cpu().numpy(), ct.cpu().numpy()
    for lo in (0, 275000, 575000):          # the first, a middle and the last block of columns
        block = gt[:, lo:lo + 25000].cpu().numpy()
        want, want_radius, kept = restated_window(block, c[lo:lo + 25000], keep)
        assert same_radius(radius[lo:lo + 25000], want_radius), lo
        assert window_within_bar(out[lo:lo + 25000], block, kept), lo


def test_the_drop_in_call_on_baseline_config_2(eng, torch):
    """BASELINE configs[2]: 1000 clients x 1e6 parameters, f = 240, through defences.phocas on a device-resident matrix,
    against the restatement on 512 sampled columns."""
    from attacking_federate_learning_amd import defences
    n, d, f = 1000, 1000000, 240
    device = torch.device('cuda', eng.device)
    gen = torch.Generator(device=device).manual_seed(6)
    gt = torch.empty((n, d), dtype=torch.float32, device=device)
    gt.normal_(generator=gen)
    gt[:f] = gt[:f].mean(dim=0) - 1.5 * gt[:f].std(dim=0)          # the attack's identical rows
    ph = defences.phocas(gt, n, f)
    cols = np.sort(np.random.default_rng(7).choice(d, size=512, replace=False))
    cols[0], cols[-1] = 0, d - 1
    pick = torch.from_numpy(cols).to(device)
    g = gt[:, pick].cpu().numpy()
    centre = eng.rank_trimmed_mean(gt, f)[pick].cpu().numpy()      # (held to its own restatement in test_gpu_rank_trim.py)
    del gt
    kept = restated_window(g, centre, n - f)[2]
    assert window_within_bar(ph[pick].cpu().numpy(), g, kept)


# ---- as a rule of the reference's signature ---------------------------------------------------------------------------------
def test_as_a_then_rule_and_through_the_device_server(eng, torch):
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.server import DeviceServer
    device = torch.device('cuda', eng.device)
    n, d, f, s = 40, 1031, 6, 2
    g = tie_case(n, d, seed=40)[0]
    g[:, ::2] = np.random.default_rng(40).standard_normal((n, (d + 1) // 2)).astype(np.float32)
    gt = on_device(eng, torch, g)
    bucketed = defences.bucketing(gt, n, f, s=s, seed=3)
    want = eng.window_mean(bucketed, eng.rank_trimmed_mean(bucketed, f), n // s - f)
    got = defences.bucketing(gt, n, f, s=s, seed=3, then=defences.phocas)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    host = defences.bucketing(g, n, f, s=s, seed=3, then=defences.phocas)
    assert isinstance(host, np.ndarray) and host.tobytes() == want.cpu().numpy().tobytes()
    # mean_around: 'trimmed' is Phocas, 'median' is the window around coordinate_median's bits, a vector is taken as it is
    assert torch.equal(defences.mean_around(gt, n, f, centre='trimmed').view(torch.int32), defences.phocas(gt, n, f).view(torch.int32))
    med = eng.coordinate_median(gt)
    meamed = defences.mean_around(gt, n, f)
    assert torch.equal(meamed.view(torch.int32), eng.window_mean(gt, med, n - f).view(torch.int32))
    assert torch.equal(defences.mean_around(gt, n, f, centre=med, keep=n - f - 1).view(torch.int32),
                       eng.window_mean(gt, med, n - f - 1).view(torch.int32))
    assert defences.mean_around(g, n, f).tobytes() == meamed.cpu().numpy().tobytes()
    # DeviceServer.defend takes the rule itself
    mal_prop = 0.15
    assert int(n * mal_prop) == f
    w0 = np.random.default_rng(3).standard_normal(d).astype(np.float32)
    server = DeviceServer(n, w0, mal_prop, 0.1, 0.9, torch_device=device, engine=eng)
    server.users_grads.data.copy_(gt)
    server.velocity.fill_(0.25)
    w, v = torch.from_numpy(w0).to(device), torch.full((d,), 0.25, dtype=torch.float32, device=device)
    expect = defences.phocas(gt, n, f)
    agg = server.defend(defences.phocas)
    assert torch.equal(agg.view(torch.int32), expect.view(torch.int32))
    eng.server_update(w, v, expect, 0.9, 0.1)
    assert torch.equal(server.current_weights.view(torch.int32), w.view(torch.int32))
    assert torch.equal(server.velocity.view(torch.int32), v.view(torch.int32))


# ---- argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import EngineError, _vp
    g = on_device(eng, torch, np.random.default_rng(1).standard_normal((10, 16)).astype(np.float32))
    c = torch.zeros(16, dtype=torch.float32, device=g.device)
    out = torch.full((16,), 7.0, dtype=torch.float32, device=g.device)
    lib, ctx = eng.lib, eng.ctx
    gp, cp, op = _vp(g.data_ptr()), _vp(c.data_ptr()), _vp(out.data_ptr())

    def wm(n_rows, n_cols, ld, keep, g_ptr=gp, c_ptr=cp, out_ptr=op):
        return lib.byz_window_mean_dev(ctx, g_ptr, n_rows, n_cols, ld, None, c_ptr, keep, out_ptr, None, None)

    def ph(n_rows, n_cols, ld, b, g_ptr=gp, out_ptr=op):
        return lib.byz_phocas_dev(ctx, g_ptr, n_rows, n_cols, ld, None, b, out_ptr, None, None, None)
    for call in (wm(10, 16, 16, 0), wm(10, 16, 16, 11), wm(10, 16, 16, -1), wm(0, 16, 16, 1), wm(10, 16, 15, 5),
                 wm(10, 16, 16, 5, g_ptr=None), wm(10, 16, 16, 5, c_ptr=None), wm(10, 16, 16, 5, out_ptr=None),
                 ph(10, 16, 16, 5), ph(10, 16, 16, -1), ph(0, 16, 16, 0), ph(10, 16, 15, 1), ph(10, 16, 16, 1, g_ptr=None),
                 ph(10, 16, 16, 1, out_ptr=None)):
        assert call == _native.E_INVALID
    # one row too many: refused before anything is read (the matrix behind the pointer has ten rows)
    too_many = (1 << 20) + 1
    assert wm(too_many, 16, 16, 5) == _native.E_UNSUPPORTED and ph(too_many, 16, 16, 1) == _native.E_UNSUPPORTED
    eng.synchronize()
    assert np.all(out.cpu().numpy() == 7.0)                # nothing was launched
    host, hc, hout = np.zeros((10, 16), dtype=np.float32), np.zeros(16, dtype=np.float32), np.zeros(16, dtype=np.float32)
    hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    assert lib.byz_window_mean_host(ctx, hp(host), too_many, 16, hp(hc), 5, hp(hout), None) == _native.E_UNSUPPORTED
    assert lib.byz_phocas_host(ctx, hp(host), too_many, 16, 1, hp(hout), None, None) == _native.E_UNSUPPORTED
    assert lib.byz_window_mean_host(ctx, hp(host), 10, 16, hp(hc), 0, hp(hout), None) == _native.E_INVALID
    assert lib.byz_window_mean_host(ctx, hp(host), 10, 16, hp(hc), 11, hp(hout), None) == _native.E_INVALID
    assert lib.byz_window_mean_host(ctx, hp(host), 10, 16, None, 5, hp(hout), None) == _native.E_INVALID
    assert lib.byz_window_mean_host(ctx, hp(host), 10, 16, hp(hc), 5, None, None) == _native.E_INVALID
    assert lib.byz_phocas_host(ctx, hp(host), 10, 16, 5, hp(hout), None, None) == _native.E_INVALID
    assert lib.byz_phocas_host(ctx, hp(host), 10, 16, 1, None, None, None) == _native.E_INVALID
    assert wm(10, 16, 16, 10) == _native.OK and ph(10, 16, 16, 4) == _native.OK
    eng.synchronize()
    for call in (lambda: eng.window_mean(g, c, 0), lambda: eng.window_mean(g, c, 11), lambda: eng.window_mean(g, c[:15], 5),
                 lambda: eng.window_mean(g, c, None), lambda: eng.phocas(g, 5), lambda: eng.phocas(g, -1),
                 lambda: eng.phocas(g, None), lambda: eng.window_mean(g, c, 5, row_index=np.array([], dtype=np.int64))):
        with pytest.raises(ValueError):
            call()
    assert issubclass(EngineError, RuntimeError)
