"""FLAME on an MI355X, held to the numpy restatements of tests/test_flame.py.

The clustering is compared EXACTLY: the admitted set, its count and w* as bits against restated_flame_select run on the very
matrix the device clustered (a crafted one, or the device's own cosine matrix downloaded), so no margin enters.  The cosine
matrix itself is held to fp64 numpy within 2 B + 2^-23, B = 4 sqrt(min(d, 2048)) 2^-24 being the bound
tests/test_gpu_views.py::test_gram derives for a Gram entry relative to |x_i| |x_j|: the entry g_ij contributes B, the two
diagonal entries B / 2 each through their square roots (times |cos| <= 1), and the one rounding to fp32 of a value of at most 2
contributes 2^-23.  Where two DIFFERENT device matrices must give the same set (a strided view, the host entry point's
staging), the case is first shown, on the CPU, to keep its restatement under 32 seeded symmetric perturbations of the fp64
matrix by +- that bound."""
import ctypes

import numpy as np
import pytest

from tests.test_flame import restated_core, restated_cosine, restated_flame_select

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:%d' % eng.device)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def cosine_bound(d):
    return 2.0 * 4.0 * np.sqrt(min(d, 2048)) * 2.0 ** -24 + 2.0 ** -23


def honest_and_opposite(n, d, seed):
    """An honest cluster round mu and a quarter of the clients pointing the other way (the first n // 4 rows)."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal(d)
    g = (mu + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    f = n // 4
    g[:f] = (-3.0 * mu + 0.3 * rng.standard_normal((f, d))).astype(np.float32)
    return g, f


def drift_shape(n, d, seed):
    """The reference's attack: a quarter of the clients are ONE vector, the honest mean minus one standard deviation."""
    rng = np.random.default_rng(seed)
    g = (0.5 * rng.standard_normal(d) + rng.standard_normal((n, d))).astype(np.float32)
    f = n // 4
    g[:f] = (g[f:].mean(0) - g[f:].std(0)).astype(np.float32)
    return g, f


def stable_under_the_bound(g, ms=1, trials=32):
    """The precondition of the placement tests, on the CPU: the restatement of the fp64 cosine matrix is unchanged under `trials`
    seeded symmetric perturbations by +- the cosine bound.  Returns (stable, mask)."""
    n, d = g.shape
    c = restated_cosine(g)
    m = n // 2 + 1
    mask, _ = restated_flame_select(c, m, ms)
    bound = cosine_bound(d)
    for seed in range(trials):
        sign = np.where(np.random.default_rng(1000 + seed).random((n, n)) < 0.5, -1.0, 1.0)
        sign = np.triu(sign, 1)
        e = (sign + sign.T) * bound
        if not np.array_equal(restated_flame_select(np.maximum(c + e, 0.0), m, ms)[0], mask):
            return False, mask
    return True, mask


# ---- the cosine matrix ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d,strided', [(5, 7, False), (63, 257, False), (65, 4097, False), (130, 1025, True)])
def test_cosine_matrix_against_fp64(eng, torch, n, d, strided):
    g = np.random.default_rng(n * 1000 + d).standard_normal((n, d)).astype(np.float32)
    g *= np.linspace(0.5, 3.0, n, dtype=np.float32)[:, None]
    zero_row, nan_row = 1, n - 2
    g[zero_row] = 0
    g[nan_row, d // 2] = np.nan
    if strided:      # a misaligned view: one float off a 16-byte boundary, rows 3 floats apart from dense
        flat = torch.full((n * (d + 3) + 1,), 7.0, dtype=torch.float32, device='cuda:%d' % eng.device)
        view = flat[1:1 + n * (d + 3)].view(n, d + 3)[:, :d]
        view.copy_(on_gpu(torch, eng, g))
        assert view.stride(0) == d + 3 and view.data_ptr() % 16 == 4
        got = eng.cosine_distances(view).numpy()
    else:
        got = eng.cosine_distances(on_gpu(torch, eng, g)).numpy()
    want = restated_cosine(g)
    assert got.dtype == np.float32 and got.shape == (n, n)
    assert np.array_equal(bits(got), bits(got.T))                                   # symmetric as bits
    assert np.array_equal(bits(np.diagonal(got)), np.full(n, bits(INF)[0]))         # diagonal +inf
    for r in (zero_row, nan_row):
        assert np.array_equal(bits(got[r]), np.full(n, bits(INF)[0])) and np.array_equal(bits(got[:, r]), np.full(n, bits(INF)[0]))
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite)                                 # nothing else moves
    assert finite.sum() == (n - 2) * (n - 3)
    worst = float(np.max(np.abs(got[finite].astype(np.float64) - want[finite])))
    print('cosine %dx%d%s: worst error %.3g, %.3f of the bound %.3g' % (n, d, ' strided' if strided else '', worst,
                                                                         worst / cosine_bound(d), cosine_bound(d)))
    assert worst <= cosine_bound(d)
    assert (got[finite] >= 0).all()
    # the second half alone, on the same Gram, gives the same bits
    dense = on_gpu(torch, eng, g)
    again = eng.cosine_from_gram(eng.gram(dense)).numpy()
    assert np.array_equal(bits(again), bits(eng.cosine_distances(dense).numpy()))


# ---- core distances ---------------------------------------------------------------------------------------------------------
def quarter_matrix(n, seed, levels=9):
    """A symmetric fp32 matrix of quarter-integers (many ties), diagonal +inf."""
    rng = np.random.default_rng(seed)
    c = np.triu(rng.integers(0, levels, size=(n, n)).astype(np.float32) / 4, 1)
    c = c + c.T
    np.fill_diagonal(c, INF)
    return c


@pytest.mark.parametrize('n', [2, 5, 64, 65, 1025])
def test_core_distances_are_np_sort(eng, n):
    c = quarter_matrix(n, n)
    if n >= 5:
        c[0, 1] = c[1, 0] = -0.0
        c[2, 3] = c[3, 2] = INF
    for ms in (0, 1, 2, 5, 32):
        if ms > n - 1:
            with pytest.raises(ValueError):
                eng.flame_core_distances(c, ms)
            continue
        got = eng.flame_core_distances(c, ms)
        want = restated_core(c, ms).astype(np.float32)
        assert np.array_equal(bits(got + np.float32(0)), bits(want + np.float32(0))), (n, ms)


# ---- the selection on crafted matrices --------------------------------------------------------------------------------------
def random_symmetric(n, seed):
    rng = np.random.default_rng(seed)
    c = np.triu(rng.random((n, n), dtype=np.float32) * 2, 1)
    c = c + c.T
    np.fill_diagonal(c, INF)
    return c


def zero_block(n, seed):
    """More than half of the rows duplicates of each other (distance 0), the rest random."""
    c = random_symmetric(n, seed)
    k = n // 2 + 1 if n > 3 else n - 1
    c[:k, :k] = 0
    np.fill_diagonal(c, INF)
    return c


def mostly_broken(n, seed):
    """More than n - m rows are +inf throughout: nobody can be admitted."""
    c = quarter_matrix(n, seed)
    k = n - (n // 2 + 1) + 1
    c[:k] = INF
    c[:, :k] = INF
    return c


FAMILIES = {'random': random_symmetric, 'quarters': lambda n, seed: quarter_matrix(n, seed, levels=4), 'zero_block': zero_block,
            'mostly_broken': mostly_broken}


def check_select(eng, c, m, ms):
    rows, info = eng.flame_select(c, min_samples=ms, min_cluster_size=m)
    mask, w_star = restated_flame_select(c, m, ms)
    assert np.array_equal(rows, np.flatnonzero(mask)), (c.shape[0], m, ms, len(rows), int(mask.sum()))
    assert info['admitted'] == int(mask.sum())
    assert np.array_equal(bits(np.float32(info['w_star'])), bits(np.float32(w_star))), (info['w_star'], w_star)
    return mask, info


@pytest.mark.parametrize('kind', sorted(FAMILIES))
@pytest.mark.parametrize('n', [2, 3, 5, 64, 65, 1023, 1025, 2049])
def test_select_equals_the_restatement(eng, n, kind):
    c = FAMILIES[kind](n, 7 * n + len(kind))
    m = n // 2 + 1
    for ms in (0, 1, 2):
        if ms > n - 1:
            continue
        mask, info = check_select(eng, c, m, ms)
        if kind == 'mostly_broken':
            assert not mask.any() and info['w_star'] == np.inf
            assert info['broken_rows'] == int((~np.isfinite(c)).all(axis=1).sum()) >= n - m + 1
        if kind == 'zero_block' and ms <= 1 and n > 3:
            assert mask[:m].all() and info['w_star'] == 0.0
    if n >= 5:
        check_select(eng, c, n - 1, 1)                  # a larger minimum cluster, up to everybody
        check_select(eng, c, n, min(3, n - 1))


def test_select_at_the_row_limit_admits_the_last_row(eng):
    """n = 16,384, the most one workgroup's registers and the LDS union-find hold: points on a line, a tight majority that
    includes row 16,383 and a spread-out rest."""
    n = 16384
    rng = np.random.default_rng(16384)
    x = np.where(rng.random(n) < 0.6, rng.random(n), 5.0 + 95.0 * rng.random(n)).astype(np.float32)
    x[n - 1] = np.float32(0.5)
    c = np.abs(x[:, None] - x[None, :])
    np.fill_diagonal(c, INF)
    mask, info = check_select(eng, c, n // 2 + 1, 1)
    assert mask[n - 1] and n // 2 + 1 <= info['admitted'] < n


def test_beyond_the_row_limit_is_refused_and_nothing_is_written(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    n = 16385
    flags = torch.full((64,), -7, dtype=torch.int32, device='cuda:%d' % eng.device)
    dist = torch.zeros(64, dtype=torch.float32, device='cuda:%d' % eng.device)        # (never read: refused on n alone)
    rc = eng.lib.byz_flame_select_dev(eng.ctx, _vp(dist.data_ptr()), n, n // 2 + 1, 1, _vp(flags.data_ptr()), None)
    assert rc == _native.E_UNSUPPORTED
    rc = eng.lib.byz_cosine_from_gram_dev(eng.ctx, _vp(dist.data_ptr()), n, _vp(flags.data_ptr()), None)
    assert rc == _native.E_UNSUPPORTED
    eng.synchronize()
    assert (flags == -7).all()


# ---- the selection on the device's own matrix, and the aggregate -------------------------------------------------------------
CASES = [(20, 64), (63, 300), (101, 1025)]


@pytest.mark.parametrize('shape', ['opposite', 'drift'])
@pytest.mark.parametrize('n,d', CASES)
def test_flame_admits_the_restatement_of_its_own_cosine_matrix_and_aggregates_them(eng, torch, n, d, shape):
    g, f = (honest_and_opposite if shape == 'opposite' else drift_shape)(n, d, seed=n + d)
    gt = on_gpu(torch, eng, g)
    lam, seed, rnd = 0.01, 5, 3
    out, info = eng.flame(gt, lam=lam, seed=seed, round=rnd, return_info=True)
    c = eng.cosine_distances(gt).numpy()
    m = n // 2 + 1
    mask, w_star = restated_flame_select(c, m, 1)
    assert np.array_equal(info['admitted_rows'], np.flatnonzero(mask))              # exact: the same matrix, no margin
    assert info['admitted'] == int(mask.sum()) >= m and info['broken_rows'] == 0
    assert np.array_equal(bits(np.float32(info['w_star'])), bits(np.float32(w_star)))
    if shape == 'opposite':
        assert not mask[:f].any()                                                   # no attacker is admitted
    else:
        assert mask[:f].all() or not mask[:f].any()                                 # identical rows: a block, in or out
    # the aggregate: the weighted sum of the admitted rows' clipped selves over their count, then the noise, from the pieces
    zero = torch.zeros(d, dtype=torch.float32, device=gt.device)
    scales, clip = eng.clip_scales(eng.row_sqdist(gt, zero), adaptive=True, return_clip=True)
    assert float(clip.item()) == info['clip']
    assert abs(info['clip'] / float(np.median(np.sqrt((g.astype(np.float64) ** 2).sum(1)))) - 1.0) < 1e-12
    weights = scales * on_gpu(torch, eng, mask.astype(np.float64))
    count = torch.tensor([float(mask.sum())], dtype=torch.float64, device=gt.device)
    mean = eng.scaled_rows_sum(gt, weights, count)
    want = eng.gaussian_noise(mean, lam, seed=seed, round=rnd, scale=clip)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    assert torch.equal(eng.flame(gt, lam=0.0).view(torch.int32), mean.view(torch.int32))      # lam = 0: the clipped mean's bits
    assert not torch.equal(out, mean)


def test_everybody_admitted_is_adaptive_weak_dp(eng, torch):
    n, d = 40, 3001
    g = np.random.default_rng(9).standard_normal((n, d)).astype(np.float32)
    g *= np.linspace(0.2, 4.0, n, dtype=np.float32)[:, None]
    gt = on_gpu(torch, eng, g)
    zeros = np.zeros((n, n), dtype=np.float32)
    np.fill_diagonal(zeros, INF)
    out, info = eng.flame(gt, lam=0.02, seed=11, round=2, distances=zeros, return_info=True)
    assert info['admitted'] == n and info['w_star'] == 0.0 and len(info['admitted_rows']) == n
    want = eng.weak_dp(gt, sigma=0.02, adaptive=True, seed=11, round=2)
    a = out.view(torch.int32).cpu().numpy().astype(np.int64)
    b = want.view(torch.int32).cpu().numpy().astype(np.int64)
    differing = int((a != b).sum())
    print('flame with everybody admitted against weak_dp(adaptive): %d of %d elements differ' % (differing, d))
    same_sign = (a < 0) == (b < 0)
    assert same_sign.all() and np.abs(a - b).max() <= 1                             # 1 fp32 ulp


def test_repeatability_host_entry_point_and_a_strided_view(eng, torch):
    n, d = 63, 300
    g, f = honest_and_opposite(n, d, seed=363)
    stable, mask = stable_under_the_bound(g)
    assert stable                                          # the precondition, computed on the CPU
    gt = on_gpu(torch, eng, g)
    a, ia = eng.flame(gt, lam=0.01, seed=2, round=1, return_info=True)
    b, ib = eng.flame(gt, lam=0.01, seed=2, round=1, return_info=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and np.array_equal(ia['admitted_rows'], ib['admitted_rows'])
    assert np.array_equal(ia['admitted_rows'], np.flatnonzero(mask))
    h, ih = eng.flame(g, lam=0.01, seed=2, round=1, return_info=True)               # numpy in -> numpy out
    assert isinstance(h, np.ndarray) and np.array_equal(ih['admitted_rows'], ia['admitted_rows'])
    assert np.array_equal(bits(h), bits(a.cpu().numpy()))                           # the host entry point is the device call
    flat = torch.full((n * (d + 5) + 3,), 3.0, dtype=torch.float32, device=gt.device)
    view = flat[3:3 + n * (d + 5)].view(n, d + 5)[:, :d]
    view.copy_(gt)
    v, iv = eng.flame(view, lam=0.01, seed=2, round=1, return_info=True)
    assert np.array_equal(iv['admitted_rows'], ia['admitted_rows'])
    assert np.allclose(v.cpu().numpy(), a.cpu().numpy(), rtol=0, atol=1e-5)
    from attacking_federate_learning_amd import defences
    assert torch.equal(defences.flame(gt, n, f, lam=0.01, seed=2, round=1).view(torch.int32), a.view(torch.int32))
    # `distances=` replaces the cosine stage: the Euclidean matrix is a legitimate input
    _, ie = eng.flame(gt, lam=0.01, distances=eng.pairwise_distances(gt), return_info=True)
    mask_e, _ = restated_flame_select(eng.pairwise_distances(gt).numpy(), n // 2 + 1, 1)
    assert np.array_equal(ie['admitted_rows'], np.flatnonzero(mask_e))


def test_nobody_admitted_gives_the_noise_alone(eng, torch):
    n, d = 9, 500
    g = np.random.default_rng(4).standard_normal((n, d)).astype(np.float32)
    g[:5] = 0                                               # five zero clients: four are left, m = 5
    gt = on_gpu(torch, eng, g)
    out, info = eng.flame(gt, lam=0.5, seed=8, return_info=True)
    assert info['admitted'] == 0 and info['broken_rows'] == 5 and info['w_star'] == np.inf and len(info['admitted_rows']) == 0
    assert info['clip'] == 0.0 and torch.isfinite(out).all()                        # the median of nine norms, five of them 0
    g[:5, 0] = np.nan                                       # five non-finite clients: the median is over the other four
    out, info = eng.flame(on_gpu(torch, eng, g), lam=0.5, seed=8, return_info=True)
    assert info['admitted'] == 0 and info['clip'] > 0
    zero = torch.zeros(d, dtype=torch.float32, device=gt.device)
    want = eng.gaussian_noise(zero, 0.5 * info['clip'], seed=8)
    assert np.abs(out.cpu().numpy() - want.cpu().numpy()).max() <= 1e-6 and float(out.abs().max()) > 0


def test_two_rounds_through_the_device_server(eng, torch):
    from attacking_federate_learning_amd.server import DeviceServer
    n, d = 20, 640
    g, f = honest_and_opposite(n, d, seed=77)
    weights = np.random.default_rng(51).standard_normal(d).astype(np.float32)
    dev = 'cuda:%d' % eng.device
    server = DeviceServer(n, weights, 0.25, 0.1, 0.9, torch_device=dev, engine=eng)
    assert server.flame_round == 0
    gt = on_gpu(torch, eng, g)
    steps = []
    for rnd in (0, 1):
        server.users_grads.data.copy_(gt)
        step = server.defend_flame(lam=0.01, seed=77)
        assert server.flame_round == rnd + 1
        want, info = eng.flame(gt, lam=0.01, seed=77, round=rnd, return_info=True)
        assert torch.equal(step.view(torch.int32), want.view(torch.int32))
        steps.append((step.clone(), info['admitted_rows']))
    assert np.array_equal(steps[0][1], steps[1][1]) and not (steps[0][1] < f).any()     # the same admitted set
    assert (steps[0][0] != steps[1][0]).float().mean() > 0.99                            # fresh noise


def test_invalid_arguments_are_refused_and_nothing_is_written(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    n, d = 20, 64
    g, _ = honest_and_opposite(n, d, seed=1)
    gt = on_gpu(torch, eng, g)
    out = torch.full((d,), -3.0, dtype=torch.float32, device=gt.device)
    flags = torch.full((n,), -7, dtype=torch.int32, device=gt.device)

    def call(lam=0.01, ms=1, m=0, out_ptr=None):
        params = _native.FlameParams(lam, ms, m, 0, 0, 0)
        return eng.lib.byz_flame_dev(eng.ctx, _vp(gt.data_ptr()), n, d, d, ctypes.byref(params), None,
                                     _vp(out.data_ptr() if out_ptr is None else out_ptr), _vp(flags.data_ptr()), None)
    assert call(m=10) == _native.E_INVALID                   # 2 m <= n
    assert call(m=21) == _native.E_INVALID
    assert call(ms=33) == _native.E_UNSUPPORTED
    assert call(ms=20) == _native.E_INVALID                  # beyond n - 1
    assert call(lam=-1.0) == _native.E_INVALID
    assert call(lam=float('nan')) == _native.E_INVALID
    assert call(out_ptr=gt.data_ptr() + 4 * (d - 1)) == _native.E_INVALID            # out overlaps G
    assert eng.lib.byz_flame_dev(eng.ctx, _vp(gt.data_ptr()), n, d, d, None, None, _vp(out.data_ptr()), None, None) == _native.E_INVALID
    eng.synchronize()
    assert (out == -3.0).all() and (flags == -7).all() and torch.equal(gt, on_gpu(torch, eng, g))
    with pytest.raises(ValueError):
        eng.flame(gt, min_cluster_size=10)
    with pytest.raises((ValueError, NotImplementedError)):
        eng.flame(gt, min_samples=33)
    with pytest.raises(ValueError):
        eng.flame(gt, lam=-0.5)
    with pytest.raises(ValueError):
        eng.flame_select(np.zeros((4, 5), dtype=np.float32))
    assert call() == _native.OK
    eng.synchronize()
    assert (flags != -7).all()
