"""The coordinate-wise median and the rank-trimmed mean on an MI355X (csrc/rank_select.hip), held to the numpy
restatement of tests/test_rank_trim.py: the median with `==` and equal NaN positions, the rank-trimmed mean within the bar
|out - ref| <= 2^-23 |ref| + 2^-30 mabs + 2^-149 per element.  `ref` is the fp64 numpy mean of np.sort(col)[b : n - b] (pairwise
sums: its own error is (n - 1) 2^-53 mabs at most, a thousandth of the bar's second term); math.fsum over whole matrices would
take minutes, the CPU file checks the fp64 numpy mean against it.  The heights straddle every edge of the dispatcher (256, 1024,
2304 and 4096 rows for the register tiles, 65,535 for the packed counters of the streamed kernel); nothing forces a kernel."""
import ctypes

import numpy as np
import pytest

from tests.test_rank_trim import negative_nan, restated_median, same_median, within_bar

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
HEIGHTS = [1, 2, 3, 64, 65, 256, 257, 1000, 1024, 1025, 2080, 2304, 2305, 4000, 4096, 4097, 5633, 10000, 16385, 20001]


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def trims(n):
    """b = 0, 1, BASELINE's proportion and the largest legal one."""
    return sorted({b for b in (0, 1, int(0.24 * n), (n - 1) // 2) if 2 * b < n})


def make(kind, n, d, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d)).astype(np.float32)
    if kind == 'quarter':           # many ties across both rank edges, lo == hi included (few distinct values)
        g = (np.round(g * 4) / 4).astype(np.float32)
        g[:, ::7] = (np.round(g[:, ::7])).astype(np.float32)
    elif kind == 'cancel':          # the kept values cancel: centred data plus 1e-3
        g = (g - g.mean(axis=0, dtype=np.float64).astype(np.float32) + np.float32(1e-3)).astype(np.float32)
    elif kind == 'scaled':
        g *= np.exp(rng.uniform(-20, 20, size=d)).astype(np.float32)[None, :]
    return g


def on_device(eng, torch, g):
    return torch.from_numpy(np.ascontiguousarray(g)).to(torch.device('cuda', eng.device))


def check_both(eng, torch, g, bs=None, gt=None):
    """Both rules on g against the restatement; returns the device results for further comparisons."""
    n = g.shape[0]
    gt = on_device(eng, torch, g) if gt is None else gt
    results = {}
    med = eng.coordinate_median(gt).cpu().numpy()
    assert same_median(med, restated_median(g)), ('median', n)
    results['median'] = med
    s = np.sort(g, axis=0)
    for b in (trims(n) if bs is None else bs):
        out = eng.rank_trimmed_mean(gt, b).cpu().numpy()
        assert within_bar(out, s, b, presorted=True), ('rank_trimmed_mean', n, b)
        results[b] = out
    return results


@pytest.mark.parametrize('n', HEIGHTS)
@pytest.mark.parametrize('kind', ['normal', 'quarter', 'cancel'])
def test_every_height_either_side_of_the_dispatch_edges(eng, torch, n, kind):
    d = 515 if n <= 4097 else 131
    g = make(kind, n, d, seed=n + len(kind))
    res = check_both(eng, torch, g)
    if n % 2 == 1:      # NaN-free columns, odd n, b = (n - 1) / 2: the median exactly
        assert np.array_equal(res[(n - 1) // 2], res['median'])


@pytest.mark.parametrize('n', [65535, 65536, 70001])
def test_heights_either_side_of_the_packed_counters(eng, torch, n):
    g = make('normal', n, 67, seed=n)
    g[:, 3] = np.round(g[:, 3])
    g[:, 5] = 2.5
    check_both(eng, torch, g)


@pytest.mark.parametrize('d', [1, 63, 65, 2051])
@pytest.mark.parametrize('n', [300, 1000, 2080, 4000, 6000])
def test_column_counts_that_are_not_multiples_of_the_tile(eng, torch, n, d):
    check_both(eng, torch, make('scaled', n, d, seed=n + d), bs=[int(0.24 * n)])


def test_constant_and_two_valued_columns_are_exact(eng, torch):
    for n in (7, 1000, 1001, 2080, 4000, 6001):
        g = np.empty((n, 40), dtype=np.float32)
        g[:, :20] = np.float32(0.1) * np.arange(1, 21, dtype=np.float32)[None, :]      # constant columns: the value itself
        g[:, 20:] = np.where(np.arange(n)[:, None] % 3 == 0, np.float32(-1.7), np.float32(3.3))
        g[:, 39] = np.where(np.arange(n) % 2 == 0, np.float32(0.0), np.float32(-0.0))
        res = check_both(eng, torch, g)
        for key, out in res.items():
            assert np.array_equal(out[:20], g[0, :20]), (n, key)


def test_non_finite_values_trimmed_or_kept(eng, torch):
    for n in (50, 1000, 2081, 4000, 7000):
        b = n // 10
        rng = np.random.default_rng(n)
        g = rng.standard_normal((n, 70)).astype(np.float32)
        rows = rng.permutation(n)
        g[rows[:b], 0] = np.nan; g[rows[:b:2], 0] = negative_nan()          # b NaNs of both signs: all trimmed
        g[rows[:b + 1], 1] = np.nan; g[rows[0], 1] = negative_nan()         # one survives
        g[rows[:b], 2] = np.inf                                             # trimmed
        g[rows[:b + 1], 3] = np.inf                                         # one kept: +inf
        g[rows[:b + 1], 4] = -np.inf                                        # one kept: -inf
        g[rows[:b + 1], 5] = -np.inf; g[rows[b + 1:2 * b + 2], 5] = np.inf  # both kept: NaN
        g[rows[:b - 1], 6] = np.inf; g[rows[b - 1], 6] = np.nan             # NaN behind the infinities, all trimmed
        g[rows[:b], 7] = -np.inf                                            # trimmed
        g[:, 8] = np.nan; g[::2, 8] = negative_nan()                        # a column that is all NaN
        g[:, 9] = np.inf
        g[rows[:3], 10] = negative_nan()                                     # a negative NaN must not sort first
        with np.errstate(all='ignore'):
            check_both(eng, torch, g, bs=[b, 0, (n - 1) // 2])


def test_flt_max_in_an_even_height_median_overflows_as_numpys(eng, torch):
    for n in (4, 1000, 4000, 6000):
        g = np.zeros((n, 5), dtype=np.float32)
        g[:n // 2, 0] = -1.0; g[n // 2:, 0] = FLT_MAX            # the two middle values: -1 and FLT_MAX
        g[:n // 2 - 1, 1] = -1.0; g[n // 2 - 1:, 1] = FLT_MAX    # both FLT_MAX: the fp32 sum overflows
        g[:n // 2 - 1, 2] = 1.0; g[n // 2 - 1:, 2] = -FLT_MAX
        g[:, 3] = FLT_MAX
        g[:, 4] = np.where(np.arange(n) < n // 2, -FLT_MAX, FLT_MAX)
        gt = on_device(eng, torch, g)
        with np.errstate(all='ignore'):
            want = restated_median(g)
        got = eng.coordinate_median(gt).cpu().numpy()
        assert same_median(got, want)
        assert got[1] == np.inf and got[3] == np.inf and got[4] == 0.0


@pytest.mark.parametrize('n', [300, 1000, 2080, 4000, 6000])
def test_row_index_strided_view_and_host_matrix_give_the_contiguous_bits(eng, torch, n):
    rng = np.random.default_rng(n)
    full = make('quarter', n + 50, 333, seed=n)
    b = int(0.24 * n)
    ft = on_device(eng, torch, full)
    for name, index in (('permutation', rng.permutation(n + 50)[:n]), ('subset', np.sort(rng.permutation(n + 50)[:n])),
                        ('repeated', rng.integers(0, n + 50, size=n))):
        logical = np.ascontiguousarray(full[index])
        lt = on_device(eng, torch, logical)
        want_med = eng.coordinate_median(lt).cpu().numpy()
        want_rtm = eng.rank_trimmed_mean(lt, b).cpu().numpy()
        assert same_median(want_med, restated_median(logical)) and within_bar(want_rtm, logical, b)
        idx = torch.from_numpy(index.astype(np.int32)).to(ft.device)
        for row_index in (idx, index):                     # a device index and a host one
            got_med = eng.coordinate_median(ft, row_index=row_index).cpu().numpy()
            got_rtm = eng.rank_trimmed_mean(ft, b, row_index=row_index).cpu().numpy()
            assert got_med.tobytes() == want_med.tobytes(), name
            assert got_rtm.tobytes() == want_rtm.tobytes(), name
    logical = np.ascontiguousarray(full[:n, 10:210])
    lt = on_device(eng, torch, logical)
    view = ft[:n, 10:210]
    assert view.stride(0) == 333
    want_med, want_rtm = eng.coordinate_median(lt).cpu().numpy(), eng.rank_trimmed_mean(lt, b).cpu().numpy()
    assert eng.coordinate_median(view).cpu().numpy().tobytes() == want_med.tobytes()
    assert eng.rank_trimmed_mean(view, b).cpu().numpy().tobytes() == want_rtm.tobytes()
    host_med, host_rtm = eng.coordinate_median(logical), eng.rank_trimmed_mean(logical, b)
    assert isinstance(host_med, np.ndarray) and host_med.dtype == np.float32
    assert host_med.tobytes() == want_med.tobytes() and host_rtm.tobytes() == want_rtm.tobytes()
    with pytest.raises(ValueError):
        eng.coordinate_median(ft, row_index=np.array([0, n + 50]))


@pytest.mark.parametrize('n', [200, 1000, 2080, 4000, 6000, 66000])
def test_two_calls_and_other_widths_give_the_same_bits(eng, torch, n):
    wide = 4099 if n < 60000 else 300
    g = make('normal', n, wide, seed=n)
    b = int(0.24 * n)
    gt = on_device(eng, torch, g)
    med, rtm = eng.coordinate_median(gt).cpu().numpy(), eng.rank_trimmed_mean(gt, b).cpu().numpy()
    assert eng.coordinate_median(gt).cpu().numpy().tobytes() == med.tobytes()
    assert eng.rank_trimmed_mean(gt, b).cpu().numpy().tobytes() == rtm.tobytes()
    for lo, hi in ((0, 70), (64, 193), (wide - 130, wide)):      # the same columns inside narrower matrices: other grids
        part = on_device(eng, torch, g[:, lo:hi])
        assert eng.coordinate_median(part).cpu().numpy().tobytes() == med[lo:hi].tobytes()
        assert eng.rank_trimmed_mean(part, b).cpu().numpy().tobytes() == rtm[lo:hi].tobytes()


def test_argument_errors(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import EngineError, _vp
    g = on_device(eng, torch, make('normal', 10, 16, seed=1))
    out = torch.empty(16, dtype=torch.float32, device=g.device)
    lib, ctx = eng.lib, eng.ctx
    gp, op = _vp(g.data_ptr()), _vp(out.data_ptr())

    def rtm(n_rows, n_cols, ld, b, g_ptr=gp, out_ptr=op):
        return lib.byz_rank_trimmed_mean_dev(ctx, g_ptr, n_rows, n_cols, ld, None, b, out_ptr, None)

    def med(n_rows, n_cols, ld, g_ptr=gp, out_ptr=op):
        return lib.byz_coordinate_median_dev(ctx, g_ptr, n_rows, n_cols, ld, None, out_ptr, None)
    assert rtm(10, 16, 16, 4) == _native.OK and med(10, 16, 16) == _native.OK
    assert rtm(10, 16, 16, 5) == _native.E_INVALID          # 2 b >= n
    assert rtm(10, 16, 16, -1) == _native.E_INVALID
    assert rtm(0, 16, 16, 0) == _native.E_INVALID and med(0, 16, 16) == _native.E_INVALID
    assert rtm(10, 16, 15, 1) == _native.E_INVALID and med(10, 16, 15) == _native.E_INVALID
    assert rtm(10, 16, 16, 1, out_ptr=None) == _native.E_INVALID and med(10, 16, 16, out_ptr=None) == _native.E_INVALID
    assert rtm(10, 16, 16, 1, g_ptr=None) == _native.E_INVALID and med(10, 16, 16, g_ptr=None) == _native.E_INVALID
    # one row too many: refused before anything is read (the matrix behind the pointer has ten rows)
    too_many = (1 << 20) + 1
    assert rtm(too_many, 16, 16, 1) == _native.E_UNSUPPORTED and med(too_many, 16, 16) == _native.E_UNSUPPORTED
    host = np.zeros((10, 16), dtype=np.float32)
    hp, hout = host.ctypes.data_as(ctypes.c_void_p), np.zeros(16, dtype=np.float32)
    assert lib.byz_rank_trimmed_mean_host(ctx, hp, too_many, 16, 1, hout.ctypes.data_as(ctypes.c_void_p)) == _native.E_UNSUPPORTED
    assert lib.byz_coordinate_median_host(ctx, hp, too_many, 16, hout.ctypes.data_as(ctypes.c_void_p)) == _native.E_UNSUPPORTED
    assert lib.byz_rank_trimmed_mean_host(ctx, hp, 10, 16, 5, hout.ctypes.data_as(ctypes.c_void_p)) == _native.E_INVALID
    assert lib.byz_rank_trimmed_mean_host(ctx, hp, 10, 16, 1, None) == _native.E_INVALID
    eng.synchronize()
    for call in (lambda: eng.rank_trimmed_mean(g, 5), lambda: eng.rank_trimmed_mean(g, -1),
                 lambda: eng.rank_trimmed_mean(host, 5), lambda: eng.rank_trimmed_mean(g, None)):
        with pytest.raises(ValueError):
            call()
    assert issubclass(EngineError, RuntimeError)


def column_bounds(d, parts=3):
    cuts = [0, d // 5, d // 5 + d // 2 + 1, d][:parts + 1]
    return list(zip(cuts[:-1], cuts[1:]))


def test_hip_kernels_over_uneven_column_shards_match_one_gpu(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels
    kern = HipKernels(eng)
    for n in (1000, 6000):
        g = make('quarter', n, 10001, seed=n)
        b = int(0.24 * n)
        gt = on_device(eng, torch, g)
        med, rtm = eng.coordinate_median(gt).cpu().numpy(), eng.rank_trimmed_mean(gt, b).cpu().numpy()
        slices = [gt[:, lo:hi] for lo, hi in column_bounds(10001)]
        got_med = np.concatenate([kern.coordinate_median(v).cpu().numpy() for v in slices])
        got_rtm = np.concatenate([kern.rank_trimmed_mean(v, b).cpu().numpy() for v in slices])
        assert got_med.tobytes() == med.tobytes() and got_rtm.tobytes() == rtm.tobytes()


def test_sharded_aggregator_at_world_size_one(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d, f = 150, 4099, 36
    g = make('normal', n, d, seed=16)
    g[9, 100] = np.nan
    gt = on_device(eng, torch, g)
    agg = ShardedAggregator(HipKernels(eng))
    med = agg.coordinate_median(gt, n, f, gather=True, total_columns=d).cpu().numpy()
    rtm = agg.rank_trimmed_mean(gt, n, f, gather=True, total_columns=d).cpu().numpy()
    with np.errstate(all='ignore'):
        assert same_median(med, restated_median(g)) and np.isnan(med[100])
        assert within_bar(rtm, g, f) and np.isfinite(rtm[100])
    with pytest.raises(AssertionError):
        agg.rank_trimmed_mean(gt, n, 75)


def chunked_check(med, rtm, g, b, step=50000):
    """Both results against the restatement, a block of columns at a time (np.sort of a block, never of the whole matrix)."""
    for lo in range(0, g.shape[1], step):
        block = np.ascontiguousarray(g[:, lo:lo + step])
        assert same_median(med[lo:lo + step], restated_median(block)), lo
        assert within_bar(rtm[lo:lo + step], block, b), lo


def test_the_wide_case_needs_64_bit_column_arithmetic(eng, torch):
    n, d, b = 1000, 600000, 240          # 2.4e9 bytes: byte offsets beyond 2^31
    gen = torch.Generator(device=torch.device('cuda', eng.device)).manual_seed(5)
    gt = torch.empty((n, d), dtype=torch.float32, device=torch.device('cuda', eng.device))
    gt.normal_(generator=gen)
    med = eng.coordinate_median(gt).cpu().numpy()
    rtm = eng.rank_trimmed_mean(gt, b).cpu().numpy()
    g = gt.cpu().numpy()
    del gt
    for lo in (0, 250000, 550000):        # the first, a middle and the last block of columns
        block = np.ascontiguousarray(g[:, lo:lo + 50000])
        assert same_median(med[lo:lo + 50000], restated_median(block))
        assert within_bar(rtm[lo:lo + 50000], block, b)


def test_the_drop_in_call_on_baseline_config_2(eng, torch):
    """BASELINE configs[2]: 1000 clients x 1e6 parameters, f = 240, through defences.* on a device-resident matrix."""
    from attacking_federate_learning_amd import defences
    n, d, f = 1000, 1000000, 240
    device = torch.device('cuda', eng.device)
    gen = torch.Generator(device=device).manual_seed(6)
    gt = torch.empty((n, d), dtype=torch.float32, device=device)
    gt.normal_(generator=gen)
    gt[:f] = gt[:f].mean(dim=0) - 1.5 * gt[:f].std(dim=0)          # the attack's identical rows
    med = defences.coordinate_median(gt, n, f).cpu().numpy()
    rtm = defences.rank_trimmed_mean(gt, n, f).cpu().numpy()
    g = gt.cpu().numpy()
    del gt
    chunked_check(med, rtm, g, f, step=100000)
