"""Every *_host entry point against its _dev counterpart on an MI355X, bit for bit.

A *_host call stages the host matrix, carves its vectors and lists out of the context's staging area (csrc/carve.hpp, api.hip's
HostStage), runs the _dev call and copies the results back.  So for one matrix the two must give the same bits in every output:
here the _host call goes through raw ctypes on a numpy matrix, the _dev call on the same matrix uploaded by the test, once
with every optional output asked for and once with none.  The _dev paths themselves are held to the numpy restatements by the
tests of each defence, which is what makes them the reference here.

Shapes: 9 x 1025 and 33 x 2051.  An odd column count puts an fp32 vector of odd length in front of the fp64 and int64 arrays of
the staging area; 33 rows leave an int32 array per row off a 16-byte multiple in front of the next array.

What other tests already hold, and is not repeated: tests/test_gpu_robust_lr.py::test_raw_ctypes_host_call and
tests/test_gpu_bucketing.py (the permutation checks) compare byz_robust_lr_host (9 x 63) and byz_bucket_means_host with the numpy
restatement, not with the _dev call, and the engine's numpy paths reach the other *_host calls at other shapes against
restatements under tolerances; none of them asserts _host == _dev on the bits.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(9, 1025), (33, 2051)]
vp = ctypes.c_void_p


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


@pytest.fixture(scope='module')
def native():
    from attacking_federate_learning_amd import _native
    return _native


def matrix(n, d):
    rng = np.random.default_rng(1000 * n + d)
    g = rng.standard_normal((n, d)).astype(np.float32)
    g *= (1.0 + 0.5 * rng.permutation(n) / n).astype(np.float32)[:, None]
    g[: n // 4] += np.float32(0.75)            # a cluster of outliers: the selections have something to reject
    return g


def hp(a):
    return None if a is None else a.ctypes.data_as(vp)


def dp(t):
    return None if t is None else vp(t.data_ptr())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class Pair:
    """One output on both sides: a numpy array the _host call fills, a device tensor the _dev call fills."""

    def __init__(self, torch, device, shape, dtype, wanted=True):
        self.host = np.full(shape, -77, dtype=dtype) if wanted else None
        self.dev = torch.full(shape if isinstance(shape, tuple) else (shape,), -99, dtype=getattr(torch, np.dtype(dtype).name),
                              device=device) if wanted else None

    def same(self):
        return self.host is None or np.array_equal(bits(self.host), bits(self.dev.cpu().numpy()))


@pytest.fixture(scope='module', params=SHAPES, ids=lambda s: '%dx%d' % s)
def case(request, eng, torch):
    n, d = request.param
    device = 'cuda:%d' % eng.device
    g = matrix(n, d)
    gt = torch.from_numpy(g).to(device)
    f = (n - 3) // 4                            # Bulyan's n >= 4 f + 3: 1 of 9, 7 of 33
    return n, d, f, g, gt, device


def ok(eng, rc):
    assert rc == 0, (rc, eng.lib.byz_last_error())


def sync(eng, torch):
    torch.cuda.synchronize()
    ok(eng, eng.lib.byz_ctx_check(eng.ctx, None))


@pytest.mark.parametrize('wanted', [True, False], ids=['all', 'none'])
@pytest.mark.parametrize('name', [0, 1, 2, 3], ids=['no_defense', 'krum', 'trimmed_mean', 'bulyan'])
def test_defend(eng, torch, case, name, wanted):
    n, d, f, g, gt, device = case
    lib, ctx = eng.lib, eng.ctx
    theta = n - 2 * f
    out = Pair(torch, device, d, np.float32, wanted)
    # aux: Krum's index (asked for alone, too) and Bulyan's selection; the other two defences leave it alone
    aux = Pair(torch, device, theta if name == 3 else 1, np.int32, name == 1 or (name == 3 and wanted))
    ok(eng, lib.byz_defend_host(ctx, name, hp(g), n, d, n, f, 1, hp(out.host), hp(aux.host)))
    if name == 0 and wanted:
        ok(eng, lib.byz_no_defense_dev(ctx, dp(gt), n, d, d, dp(out.dev), None))
    if name == 1:
        index = ctypes.c_int32(-1)
        ok(eng, lib.byz_krum_dev(ctx, dp(gt), n, d, d, n, f, 1, dp(out.dev), ctypes.byref(index), None))
        aux.dev.fill_(index.value)
    if name == 2 and wanted:
        ok(eng, lib.byz_trimmed_mean_dev(ctx, dp(gt), n, d, d, None, f, dp(out.dev), None))
    if name == 3 and wanted:
        ok(eng, lib.byz_bulyan_dev(ctx, dp(gt), n, d, d, n, f, dp(out.dev), dp(aux.dev), None))
    sync(eng, torch)
    assert out.same() and aux.same()


@pytest.mark.parametrize('wanted', [(True, True, True), (False, True, False), (False, False, False)], ids=['all', 'mean', 'none'])
def test_drift_attack(eng, torch, case, wanted):
    n, d, f, g, gt, device = case
    outs = [Pair(torch, device, d, np.float32, w) for w in wanted]
    ok(eng, eng.lib.byz_drift_attack_host(eng.ctx, hp(g), n, d, 1.5, *[hp(o.host) for o in outs]))
    scratch = torch.empty(d, dtype=torch.float32, device=device)      # (the host entry point has the kernel write all three)
    ok(eng, eng.lib.byz_drift_attack_dev(eng.ctx, dp(gt), n, d, d, 1.5, *[dp(scratch if o.dev is None else o.dev) for o in outs], 0, None))
    sync(eng, torch)
    assert all(o.same() for o in outs)


@pytest.mark.parametrize('wanted', [(True, True), (True, False), (False, True)], ids=['all', 'out', 'selection'])
def test_multi_krum(eng, torch, case, wanted):
    n, d, f, g, gt, device = case
    m = n - f
    out, sel = Pair(torch, device, d, np.float32, wanted[0]), Pair(torch, device, m, np.int32, wanted[1])
    ok(eng, eng.lib.byz_multi_krum_host(eng.ctx, hp(g), n, d, n, f, m, hp(out.host), hp(sel.host)))
    scratch = torch.empty(d, dtype=torch.float32, device=device)                  # (the device call always writes the aggregate)
    ok(eng, eng.lib.byz_multi_krum_dev(eng.ctx, dp(gt), n, d, d, n, f, m, 1, dp(out.dev if wanted[0] else scratch), dp(sel.dev), None))
    sync(eng, torch)
    assert out.same() and sel.same()


@pytest.mark.parametrize('median', [True, False], ids=['coordinate_median', 'rank_trimmed_mean'])
def test_rank_rules(eng, torch, case, median):
    n, d, f, g, gt, device = case
    out = Pair(torch, device, d, np.float32)
    if median:
        ok(eng, eng.lib.byz_coordinate_median_host(eng.ctx, hp(g), n, d, hp(out.host)))
        ok(eng, eng.lib.byz_coordinate_median_dev(eng.ctx, dp(gt), n, d, d, None, dp(out.dev), None))
    else:
        ok(eng, eng.lib.byz_rank_trimmed_mean_host(eng.ctx, hp(g), n, d, f, hp(out.host)))
        ok(eng, eng.lib.byz_rank_trimmed_mean_dev(eng.ctx, dp(gt), n, d, d, None, f, dp(out.dev), None))
    sync(eng, torch)
    assert out.same()


@pytest.mark.parametrize('wanted', [True, False], ids=['all', 'none'])
def test_geometric_median(eng, torch, native, case, wanted):
    n, d, f, g, gt, device = case
    params = native.GeomedParams(1e-6, 10, 1e-6)
    out, weights = Pair(torch, device, d, np.float32), Pair(torch, device, n, np.float64, wanted)
    ok(eng, eng.lib.byz_geometric_median_host(eng.ctx, hp(g), n, d, ctypes.byref(params), hp(out.host), hp(weights.host)))
    ok(eng, eng.lib.byz_geometric_median_dev(eng.ctx, dp(gt), n, d, d, ctypes.byref(params), dp(out.dev), dp(weights.dev), None))
    sync(eng, torch)
    assert out.same() and weights.same()


@pytest.mark.parametrize('wanted', [True, False], ids=['all', 'none'])
@pytest.mark.parametrize('with_start', [True, False], ids=['start', 'no_start'])
def test_centered_clip(eng, torch, native, case, with_start, wanted):
    n, d, f, g, gt, device = case
    params = native.CclipParams(float(np.median(np.linalg.norm(g.astype(np.float64), axis=1))), 3)
    start = (0.1 * matrix(1, d)[0]).astype(np.float32) if with_start else None
    out, scales = Pair(torch, device, d, np.float32), Pair(torch, device, n, np.float64, wanted)
    ok(eng, eng.lib.byz_centered_clip_host(eng.ctx, hp(g), n, d, ctypes.byref(params), hp(start), hp(out.host), hp(scales.host)))
    if with_start:                              # in place on the start, as the host entry point runs it
        out.dev.copy_(torch.from_numpy(start))
    ok(eng, eng.lib.byz_centered_clip_dev(eng.ctx, dp(gt), n, d, d, ctypes.byref(params), dp(out.dev) if with_start else None,
                                          dp(out.dev), dp(scales.dev), None))
    sync(eng, torch)
    assert out.same() and scales.same()


@pytest.mark.parametrize('wanted', [True, False], ids=['all', 'none'])
def test_fltrust(eng, torch, case, wanted):
    n, d, f, g, gt, device = case
    root = g[n // 4:].mean(axis=0).astype(np.float32)
    out = Pair(torch, device, d, np.float32)
    trust, weights = Pair(torch, device, n, np.float64, wanted), Pair(torch, device, n, np.float64, wanted)
    ok(eng, eng.lib.byz_fltrust_host(eng.ctx, hp(g), n, d, hp(root), hp(out.host), hp(trust.host), hp(weights.host)))
    out.dev.copy_(torch.from_numpy(root))       # in place on the root, as the host entry point runs it
    ok(eng, eng.lib.byz_fltrust_dev(eng.ctx, dp(gt), n, d, d, dp(out.dev), dp(out.dev), dp(trust.dev), dp(weights.dev), None))
    sync(eng, torch)
    assert out.same() and trust.same() and weights.same()


@pytest.mark.parametrize('wanted', [True, False], ids=['all', 'none'])
@pytest.mark.parametrize('estimate', [False, True], ids=['bandwidth', 'sample5'])
def test_signguard(eng, torch, native, case, estimate, wanted):
    n, d, f, g, gt, device = case
    sample = np.array([0, 2, 4, 6, 8], dtype=np.int32) if estimate else None
    params = native.SignGuardParams(0, d, 0.1, 3.0, 0.0 if estimate else 0.05, 5 if estimate else 0)
    out = Pair(torch, device, d, np.float32)
    keep, labels = Pair(torch, device, n, np.int32, wanted), Pair(torch, device, n, np.int32, wanted)
    weights = Pair(torch, device, n, np.float64, wanted)
    ok(eng, eng.lib.byz_signguard_host(eng.ctx, hp(g), n, d, ctypes.byref(params), hp(sample), hp(out.host), hp(keep.host),
                                       hp(weights.host), hp(labels.host)))
    sample_dev = torch.from_numpy(sample).to(device) if estimate else None
    ok(eng, eng.lib.byz_signguard_dev(eng.ctx, dp(gt), n, d, d, ctypes.byref(params), dp(sample_dev), dp(out.dev), dp(keep.dev),
                                      dp(weights.dev), dp(labels.dev), None))
    sync(eng, torch)
    assert out.same() and keep.same() and weights.same() and labels.same()
    if wanted:
        assert 0 < int(keep.host.sum()) <= n    # (the parameters select something: the aggregate is no vector of zeros)


@pytest.mark.parametrize('wanted', [True, False], ids=['all', 'none'])
def test_nnm(eng, torch, case, wanted):
    n, d, f, g, gt, device = case
    k = n - f
    y, nbr = Pair(torch, device, (n, d), np.float32), Pair(torch, device, (n, k), np.int32, wanted)
    ok(eng, eng.lib.byz_nnm_host(eng.ctx, hp(g), n, d, n, f, hp(y.host), hp(nbr.host)))
    ok(eng, eng.lib.byz_nnm_dev(eng.ctx, dp(gt), n, d, d, n, f, dp(y.dev), d, dp(nbr.dev), None))
    sync(eng, torch)
    assert y.same() and nbr.same()


@pytest.mark.parametrize('wanted', [True, False], ids=['all', 'none'])
def test_robust_lr(eng, torch, case, wanted):
    n, d, f, g, gt, device = case
    out, votes = Pair(torch, device, d, np.float32), Pair(torch, device, d, np.int32, wanted)
    ok(eng, eng.lib.byz_robust_lr_host(eng.ctx, hp(g), n, d, f + 1, hp(out.host), hp(votes.host)))
    ok(eng, eng.lib.byz_robust_lr_dev(eng.ctx, dp(gt), n, d, d, f + 1, dp(out.dev), dp(votes.dev), None))
    sync(eng, torch)
    assert out.same() and votes.same()


@pytest.mark.parametrize('with_perm', [True, False], ids=['perm', 'identity'])
def test_bucket_means(eng, torch, case, with_perm):
    n, d, f, g, gt, device = case
    s = 2
    perm = np.random.default_rng(n).permutation(n).astype(np.int32) if with_perm else None
    y = Pair(torch, device, (-(-n // s), d), np.float32)
    ok(eng, eng.lib.byz_bucket_means_host(eng.ctx, hp(g), n, d, hp(perm), s, hp(y.host)))
    perm_dev = torch.from_numpy(perm).to(device) if with_perm else None
    ok(eng, eng.lib.byz_bucket_means_dev(eng.ctx, dp(gt), n, d, d, dp(perm_dev), s, dp(y.dev), d, None))
    sync(eng, torch)
    assert y.same()


@pytest.mark.parametrize('wanted', [True, False], ids=['all', 'none'])
def test_dnc(eng, torch, native, case, wanted):
    n, d, f, g, gt, device = case
    params = native.DncParams(2, 5, 8, max(1, f))              # two iterations of five columns
    columns = np.array([1, 64, 511, 1000, d - 1, 0, 3, 512, 513, d - 2], dtype=np.int64)
    out, good = Pair(torch, device, d, np.float32), Pair(torch, device, n, np.int32, wanted)
    kept = ctypes.c_int64(-1)
    ok(eng, eng.lib.byz_dnc_host(eng.ctx, hp(g), n, d, ctypes.byref(params), hp(columns), hp(out.host), hp(good.host),
                                 ctypes.byref(kept) if wanted else None))
    columns_dev = torch.from_numpy(columns).to(device)
    ok(eng, eng.lib.byz_dnc_dev(eng.ctx, dp(gt), n, d, d, ctypes.byref(params), dp(columns_dev), dp(out.dev), dp(good.dev), None))
    kept_dev = ctypes.c_int64(-1)
    ok(eng, eng.lib.byz_dnc_info(eng.ctx, ctypes.byref(kept_dev), None))
    sync(eng, torch)
    assert out.same() and good.same()
    if wanted:
        assert kept.value == kept_dev.value == int((good.host >= 0).sum())
