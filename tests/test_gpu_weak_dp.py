"""Clip and noise on an MI355X, held to the numpy restatement of tests/test_weak_dp.py.

The raw words of the Philox stream equal the restatement's AS INTEGERS.  The noise is compared with the restatement, never with
the code under test: every element within 1 fp32 ulp and at most 1 element in 10^4 differing at all, pooled over a test's grid.
Why these numbers: the device's and libm's fp64 log, sin and cos differ by a few fp64 ulp, which can move the single final
rounding by at most one fp32 ulp and only next to a rounding boundary; perturbing the restatement's z by 4 fp64 ulp changed 0 of
2,000,000 fp32 results, so the reference alone stays far inside the cap and an fp32 transform would not.  The layouts
(misaligned, in place, sharded, guard-banded) are held to the aligned call's bits, the clipping piece to centered clipping's
scales bit for bit (fixed mode) and to np.median of the device's own norms bit for bit (adaptive mode)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import views_arena
from tests.test_centered_clip import median_tau
from tests.test_geometric_median import attacked
from tests.test_weak_dp import bits, restated_clip, restated_noise, restated_weak_dp, restated_words

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 3, 4, 5, 1023, 1024, 1025, 4099]
OFFSETS = [0, 1, 2, 3, 5, (1 << 34) - 2]          # the last one crosses the carry into counter word 1
SEEDS = [0, (1 << 63) + 12345]
ROUNDS = [0, 7]
GRID = [(n, off, seed, rnd) for n in NS for off in OFFSETS for seed in SEEDS for rnd in ROUNDS]


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:%d' % eng.device)


def ordered(a):
    """float32 -> int64, monotone in the value (both zeros at 0): the difference of two is their distance in ulps."""
    b = bits(a).astype(np.int64)
    return np.where(b & 0x80000000, -(b & 0x7fffffff), b)


class NoiseTally:
    """Pools the comparisons of one test: every element within 1 ulp at once, the rate of differing elements at the end."""

    def __init__(self):
        self.elements = self.differing = 0

    def add(self, got, want, what=''):
        got, want = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
        assert got.shape == want.shape
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        ulps = np.abs(ordered(got) - ordered(want))[~nan]
        assert ulps.max(initial=0) <= 1, (what, int(ulps.max()), np.flatnonzero(ulps > 1)[:8])
        self.elements += int(ulps.size)
        self.differing += int((ulps != 0).sum())

    def finish(self):
        print('noise against the restatement: %d of %d elements differ (by one ulp)' % (self.differing, self.elements))
        assert self.differing * 10 ** 4 <= self.elements


# ---- the raw words ------------------------------------------------------------------------------------------------------
def test_the_raw_words_are_the_restatements_integers(eng, torch):
    assert [hex(w) for w in eng.noise_words(4)] == ['0x6627e8d5', '0xe169c58d', '0xbc57ac4c', '0x9b00dbd8']
    like = torch.empty(1, device='cuda:%d' % eng.device)
    for n, off, seed, rnd in GRID:
        got = eng.noise_words(n, seed=seed, round=rnd, column_offset=off, like=like).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, restated_words(n, seed, rnd, off)), (n, off, seed, rnd)
    # without torch: a buffer of the engine's own, downloaded
    assert np.array_equal(eng.noise_words(1025, seed=3, round=1, column_offset=2), restated_words(1025, 3, 1, 2))


# ---- the noise against the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', [1.0, 1e-3])
@pytest.mark.parametrize('kind', ['zeros', 'normals'])
def test_the_noise_is_within_one_ulp_of_the_restatement(eng, torch, sigma, kind):
    tally = NoiseTally()
    base = (np.random.default_rng(17).standard_normal(max(NS)) * 100).astype(np.float32)
    for n, off, seed, rnd in GRID:
        x = np.zeros(n, dtype=np.float32) if kind == 'zeros' else base[:n]
        got = eng.gaussian_noise(on_gpu(torch, eng, x), sigma, seed=seed, round=rnd, column_offset=off).cpu().numpy()
        tally.add(got, restated_noise(x, sigma, seed, rnd, off), (n, off, seed, rnd))
    tally.finish()


def test_sigma_zero_returns_the_bits_of_x_and_nothing_is_sanitised(eng, torch):
    x = np.random.default_rng(18).standard_normal(1025).astype(np.float32)
    x.view(np.uint32)[:6] = [0x80000000, 0x7fc00001, 0xffc00123, 0x7f800000, 0xff800000, 0x00000001]
    xt = on_gpu(torch, eng, x)
    out = eng.gaussian_noise(xt, 0.0, seed=5)
    assert out.data_ptr() != xt.data_ptr() and views_arena.same_bits(out.cpu().numpy(), x)
    assert eng.gaussian_noise(xt, 0.0, out=xt) is xt and views_arena.same_bits(xt.cpu().numpy(), x)
    noisy = eng.gaussian_noise(xt, 0.5, seed=5).cpu().numpy()
    assert np.isnan(noisy[1]) and np.isnan(noisy[2]) and noisy[3] == np.inf and noisy[4] == -np.inf
    tally = NoiseTally()
    tally.add(noisy, restated_noise(x, 0.5, seed=5))
    assert tally.differing <= 1


# ---- the layouts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 5, 1025, 4099])
def test_misaligned_in_place_and_guard_banded_calls_give_the_aligned_bits(eng, torch, n):
    x = (np.random.default_rng(19).standard_normal(n) * 3).astype(np.float32)
    dev = 'cuda:%d' % eng.device
    for off in OFFSETS:
        want = eng.gaussian_noise(on_gpu(torch, eng, x), 0.25, seed=9, round=3, column_offset=off)
        assert want.data_ptr() % 16 == 0
        for shift_x, shift_out in ((1, 0), (0, 1), (1, 1), (3, 2), (0, 0)):
            (xv,), xflat = views_arena.arena(torch, x[None, :], n + 5, shift_x, device=dev)
            (ov,), oflat = views_arena.arena(torch, np.zeros((1, n), np.float32), n + 5, shift_out, device=dev)
            xbefore, obefore = xflat.clone(), oflat.clone()
            assert xv.data_ptr() % 16 == 4 * shift_x and ov.data_ptr() % 16 == 4 * shift_out
            eng.gaussian_noise(xv, 0.25, seed=9, round=3, column_offset=off, out=ov)
            assert torch.equal(ov.view(torch.int32), want.view(torch.int32)), (off, shift_x, shift_out)
            views_arena.untouched(torch, oflat, ov[None, :], obefore)
            assert torch.equal(xflat.view(torch.int32), xbefore.view(torch.int32))              # x is only read
            # in place on the misaligned view: the same bits, the guards either side untouched
            eng.gaussian_noise(xv, 0.25, seed=9, round=3, column_offset=off, out=xv)
            assert torch.equal(xv.view(torch.int32), want.view(torch.int32)), (off, shift_x)
            views_arena.untouched(torch, xflat, xv[None, :], xbefore)


def test_three_uneven_shards_concatenate_to_the_one_call(eng, torch):
    n = 4099
    x = on_gpu(torch, eng, (np.random.default_rng(20).standard_normal(n) * 3).astype(np.float32))
    for off in (0, 3, (1 << 34) - 2):
        whole = eng.gaussian_noise(x, 1.0, seed=21, round=2, column_offset=off)
        parts = [eng.gaussian_noise(x[lo:hi], 1.0, seed=21, round=2, column_offset=off + lo)
                 for lo, hi in ((0, 1), (1, 2050), (2050, 4099))]
        assert torch.equal(torch.cat(parts).view(torch.int32), whole.view(torch.int32))


def test_a_device_scale_equals_the_product_passed_as_sigma(eng, torch):
    x = on_gpu(torch, eng, (np.random.default_rng(22).standard_normal(4099) * 3).astype(np.float32))
    scale = torch.tensor([0.25], dtype=torch.float64, device=x.device)
    for off in (0, 1):
        want = eng.gaussian_noise(x, 0.5, seed=23, column_offset=off)
        got = eng.gaussian_noise(x, 2.0, seed=23, column_offset=off, scale=scale)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    zero = torch.zeros(1, dtype=torch.float64, device=x.device)              # a scale of zero: x + 0.0, no NaN
    assert torch.equal(eng.gaussian_noise(x, 2.0, seed=23, scale=zero), x)


def test_the_host_entry_point_gives_the_device_bits(eng, torch):
    from attacking_federate_learning_amd import defences
    for n in (1, 1025, 4099):
        x = (np.random.default_rng(24).standard_normal(n) * 3).astype(np.float32)
        want = eng.gaussian_noise(on_gpu(torch, eng, x), 0.5, seed=25, round=1, column_offset=3).cpu().numpy()
        got = defences.gaussian_noise(x, 0.5, seed=25, round=1, column_offset=3)
        assert isinstance(got, np.ndarray) and views_arena.same_bits(got, want)
        assert views_arena.same_bits(eng.gaussian_noise(x, 0.0), x)


# ---- the clipping piece -----------------------------------------------------------------------------------------------------
def clip_case(n, d, seed):
    g = attacked(n, d, seed=seed) if n >= 5 else np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    if n >= 7:
        g[1] *= np.float32(40.0)
        g[2, d // 2] = np.inf
        g[n - 2, 0] = np.nan
    return g


@pytest.mark.parametrize('n', [1, 2, 7, 8, 100])
def test_clip_scales_in_both_modes(eng, torch, n):
    d = 130
    g = clip_case(n, d, seed=30 + n)
    gt = on_gpu(torch, eng, g)
    sq = eng.row_sqdist(gt, torch.zeros(d, device=gt.device))
    q = sq.cpu().numpy()
    excluded = 2 if n >= 7 else 0
    # fixed: centered clipping's reported scales, bit for bit
    tau = median_tau(np.where(np.isfinite(g), g, 0).astype(np.float32))
    _, cinfo = eng.centered_clip(gt, tau=tau, iters=1, return_info=True)
    scales, used = eng.clip_scales(sq, clip=tau, return_clip=True)
    assert torch.equal(scales, cinfo['scales']) and float(used.item()) == tau
    info = eng.weak_dp_info()
    assert (info['clipped_rows'], info['excluded_rows'], info['clip']) == (cinfo['clipped_rows'], excluded, tau)
    want, _, clipped, _ = restated_clip(q, clip=tau)
    assert np.allclose(scales.cpu().numpy(), want, rtol=1e-12, atol=0.0) and clipped == info['clipped_rows']
    # adaptive: np.median of the device's own norms, bit for bit (sqrt and the median are exact operations)
    scales, used = eng.clip_scales(sq, adaptive=True, return_clip=True)
    want, wclip, clipped, wexcluded = restated_clip(q, adaptive=True)
    info = eng.weak_dp_info()
    print('n', n, 'clip', float(used.item()), 'want', wclip, info)
    assert float(used.item()) == wclip == info['clip'] and wclip > 0
    assert np.allclose(scales.cpu().numpy(), want, rtol=1e-12, atol=0.0)
    assert (info['clipped_rows'], info['excluded_rows']) == (clipped, wexcluded) == (clipped, excluded)
    # host norms in, numpy out: the same bits
    hs, hc = eng.clip_scales(q, adaptive=True, return_clip=True)
    assert isinstance(hs, np.ndarray) and np.array_equal(hs, scales.cpu().numpy()) and hc[0] == wclip


def test_an_all_non_finite_matrix_gives_scales_of_zero_and_the_zero_vector(eng, torch):
    g = np.full((9, 130), np.nan, dtype=np.float32)
    g[1] = np.inf
    gt = on_gpu(torch, eng, g)
    sq = eng.row_sqdist(gt, torch.zeros(130, device=gt.device))
    for adaptive in (False, True):
        scales, used = eng.clip_scales(sq, clip=2.0, adaptive=adaptive, return_clip=True)
        assert not scales.any() and float(used.item()) == (0.0 if adaptive else 2.0)
        out, info = eng.weak_dp(gt, clip=2.0, sigma=0.0, adaptive=adaptive, return_info=True)
        assert not out.view(torch.int32).any() and info['excluded_rows'] == 9 and info['clipped_rows'] == 0
    out = eng.weak_dp(gt, sigma=0.5, adaptive=True, seed=3)                    # the noise is scaled by a clip of zero
    assert not out.any() and not torch.isnan(out).any()
    out = eng.weak_dp(gt, clip=2.0, sigma=0.5, seed=3).cpu().numpy()            # fixed: noise on the zero vector
    tally = NoiseTally()
    tally.add(out, restated_noise(np.zeros(130, dtype=np.float32), 0.5, seed=3))
    assert tally.differing == 0


# ---- the whole defence ------------------------------------------------------------------------------------------------------
def weak_dp_case(name):
    if name == 'attack':
        g = attacked(60, 2051, seed=41)
    else:
        n, d = {'7x5': (7, 5), '8x1025': (8, 1025), '100x4099': (100, 4099), 'strided': (17, 1025)}[name]
        g = attacked(n, d, seed=40 + n) if n >= 8 else np.random.default_rng(40).standard_normal((n, d)).astype(np.float32)
    g[1] *= np.float32(40.0)                       # a row far outside the clipping norm
    if g.shape[0] >= 8:
        g[g.shape[0] - 2, g.shape[1] // 2] = np.nan      # an excluded row
    return g


@pytest.mark.parametrize('name', ['7x5', '8x1025', '100x4099', 'strided', 'attack'])
def test_weak_dp_against_centered_clipping_and_the_restatement(eng, torch, name):
    from attacking_federate_learning_amd import defences
    g = weak_dp_case(name)
    n, d = g.shape
    if name == 'strided':
        gt, flat = views_arena.arena(torch, g, d + 6, 1, device='cuda:%d' % eng.device)
        before = flat.clone()
    else:
        gt = on_gpu(torch, eng, g)
    clip = median_tau(np.where(np.isfinite(g), g, 0).astype(np.float32))
    excluded = 1 if n >= 8 else 0
    # before the noise: centered_clip(iters=1)'s bits
    mean, cinfo = eng.centered_clip(gt, tau=clip, iters=1, return_info=True)
    out, info = eng.weak_dp(gt, clip=clip, sigma=0.0, return_info=True)
    assert torch.equal(out.view(torch.int32), mean.view(torch.int32))
    assert (info['clipped_rows'], info['excluded_rows'], info['clip']) == (cinfo['clipped_rows'], excluded, clip)
    assert 0 < info['clipped_rows'] < n
    # with noise: the restatement, fixed and adaptive
    tally = NoiseTally()
    for adaptive, sigma in ((False, 0.05), (True, 0.01)):
        want, winfo = restated_weak_dp(g, clip=clip, sigma=sigma, adaptive=adaptive, seed=11, round=3, column_offset=5)
        got, info = eng.weak_dp(gt, clip=clip, sigma=sigma, adaptive=adaptive, seed=11, round=3, column_offset=5, return_info=True)
        tally.add(got.cpu().numpy(), want, (name, adaptive))
        assert (info['clipped_rows'], info['excluded_rows']) == (winfo['clipped_rows'], winfo['excluded_rows'])
        assert np.isclose(info['clip'], winfo['clip'], rtol=1e-12, atol=0.0)
        assert (np.abs(got.cpu().numpy() - winfo['mean']) > 0).mean() > 0.9          # the noise is there
    print(name, 'differing', tally.differing, 'of', tally.elements)
    assert tally.differing * 10 ** 4 <= max(tally.elements, 10 ** 4)       # (a case shorter than 10^4: one element at most)
    if name == 'strided':
        views_arena.untouched(torch, flat, gt, before)
    else:
        # the drop-in entry on a host matrix, and the host entry point: the device's bits
        got = eng.weak_dp(gt, clip=clip, sigma=0.05, seed=11, round=3)
        host = defences.weak_dp(g, n, 0, clip=clip, sigma=0.05, seed=11, round=3)
        assert isinstance(host, np.ndarray) and views_arena.same_bits(host, got.cpu().numpy())
        host, hinfo = defences.weak_dp(g, n, 0, sigma=0.01, adaptive=True, seed=11, round=3, return_info=True)
        got, ginfo = eng.weak_dp(gt, sigma=0.01, adaptive=True, seed=11, round=3, return_info=True)
        assert views_arena.same_bits(host, got.cpu().numpy()) and hinfo == ginfo


def test_then_supplies_the_aggregate(eng, torch):
    from attacking_federate_learning_amd import defences
    n, d = 21, 1500
    g = attacked(n, d, seed=50)
    gt = on_gpu(torch, eng, g)
    med = np.median(g, axis=0)
    assert np.array_equal(defences.coordinate_median(gt, n, 4).cpu().numpy(), med)
    tally = NoiseTally()
    got = defences.weak_dp(gt, n, 4, sigma=0.05, seed=6, round=2, then=defences.coordinate_median)
    tally.add(got.cpu().numpy(), restated_noise(med, 0.05, seed=6, round=2))
    host = defences.weak_dp(g, n, 4, sigma=0.05, seed=6, round=2, then=defences.coordinate_median)
    assert isinstance(host, np.ndarray) and views_arena.same_bits(host, got.cpu().numpy())
    assert tally.differing <= 1
    with pytest.raises(TypeError):
        defences.weak_dp(gt, n, 4, then='median')
    with pytest.raises(ValueError):
        defences.weak_dp(gt, n, 4, adaptive=True, then=defences.coordinate_median)


def test_two_rounds_through_the_device_server_draw_rounds_zero_and_one(eng, torch):
    from attacking_federate_learning_amd.server import DeviceServer
    n, d, clip, sigma = 30, 3000, 3.0, 0.05
    weights = np.random.default_rng(51).standard_normal(d).astype(np.float32)
    dev = 'cuda:%d' % eng.device
    server = DeviceServer(n, weights, 0.2, 0.1, 0.9, torch_device=dev, engine=eng)
    assert server.weak_dp_round == 0
    w, vel = on_gpu(torch, eng, weights), torch.zeros(d, dtype=torch.float32, device=dev)
    g = attacked(n, d, seed=53)
    g[1] *= np.float32(40.0)
    gt = on_gpu(torch, eng, g)
    tally, steps = NoiseTally(), []
    for rnd in (0, 1):
        server.users_grads.data.copy_(gt)
        step = server.defend_weak_dp(clip=clip, sigma=sigma, seed=77)
        assert server.weak_dp_round == rnd + 1
        assert torch.equal(step.view(torch.int32), eng.weak_dp(gt, clip=clip, sigma=sigma, seed=77, round=rnd).view(torch.int32))
        tally.add(step.cpu().numpy(), restated_weak_dp(g, clip=clip, sigma=sigma, seed=77, round=rnd)[0], rnd)
        eng.server_update(w, vel, step, 0.9, 0.1)
        assert torch.equal(server.current_weights, w) and torch.equal(server.velocity, vel)       # the momentum step ran
        steps.append(step.clone())
    assert tally.differing <= 1
    assert (steps[0] != steps[1]).float().mean() > 0.99                     # the same gradients, fresh noise
    step = server.defend_weak_dp(sigma=sigma, seed=77, then=lambda grads, users, mal: eng.coordinate_median(grads))
    assert server.weak_dp_round == 3
    want = eng.gaussian_noise(eng.coordinate_median(gt), sigma, seed=77, round=2)
    assert torch.equal(step.view(torch.int32), want.view(torch.int32))


# ---- the columns layout -----------------------------------------------------------------------------------------------------
def test_sharded_aggregator_over_uneven_column_shards_matches_one_gpu(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator

    class LoopedKernels(HipKernels):
        """Every shard on this GPU: row_sqdist sums the shards' parts, as the all-reduce over the ranks would; the update and
        the noise run per shard, the noise with the shard's global column offset."""

        def __init__(self, engine, bounds):
            super().__init__(engine)
            self.bounds = bounds

        def row_sqdist(self, g, z):
            return sum(self.engine.row_sqdist(g[:, lo:hi], z[lo:hi].contiguous()) for lo, hi in self.bounds)

        def clip_update(self, g, v, scales):
            return torch.cat([self.engine.clip_update(g[:, lo:hi], v[lo:hi].contiguous(), scales) for lo, hi in self.bounds])

        def gaussian_noise(self, x, sigma, seed=0, round=0, column_offset=0, scale=None):
            return torch.cat([self.engine.gaussian_noise(x[lo:hi].contiguous(), sigma, seed=seed, round=round,
                                                         column_offset=column_offset + lo, scale=scale) for lo, hi in self.bounds])

    n, d = 60, 4099
    g = attacked(n, d, seed=52)
    g[1] *= np.float32(40.0)
    g[9, 100] = np.nan
    gt = on_gpu(torch, eng, g)
    clip = median_tau(attacked(n, d, seed=52))
    for adaptive, sigma in ((False, 0.05), (True, 0.01)):
        want, winfo = eng.weak_dp(gt, clip=clip, sigma=sigma, adaptive=adaptive, seed=8, round=4, column_offset=3, return_info=True)
        mean = eng.weak_dp(gt, clip=clip, sigma=0.0, adaptive=adaptive)
        for cuts in ([0, d], [0, 1, 2050, d], [0, d // 3 + 1, d // 2 + 7, d]):
            kern = LoopedKernels(eng, list(zip(cuts[:-1], cuts[1:])))
            got, info = ShardedAggregator(kern).weak_dp(gt, n, 0, 3, clip=clip, sigma=sigma, adaptive=adaptive, seed=8, round=4,
                                                        return_info=True)
            assert (info['clipped_rows'], info['excluded_rows']) == (winfo['clipped_rows'], winfo['excluded_rows']) and info['excluded_rows'] == 1
            if len(cuts) == 2:           # one shard: the library call's launches, bit for bit
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and info['clip'] == winfo['clip']
            else:                        # the norms summed in another order: the clipped mean within centered clipping's tolerance,
                noise_w, noise_g = (want - mean).cpu().numpy(), (got - mean).cpu().numpy()      # the noise the same to fp32 rounding
                assert np.isclose(info['clip'], winfo['clip'], rtol=1e-12, atol=0.0)
                assert np.allclose(noise_g, noise_w, rtol=0, atol=4 * np.spacing(np.abs(want.cpu().numpy()).max()))


def test_sharded_aggregator_at_world_size_one_with_every_collective_issued(eng):
    """ShardedAggregator(HipKernels).weak_dp with BYZ_FORCE_COLLECTIVES=1: the all-reduce of the norms goes through RCCL although
    there is nobody else, and both modes equal the single-GPU call bit for bit.  Own process: torch.distributed state stays
    out of the test session."""
    env = dict(os.environ, BYZ_FORCE_COLLECTIVES='1', MASTER_ADDR='127.0.0.1', MASTER_PORT='29541', RANK='0', WORLD_SIZE='1',
               LOCAL_RANK='0', HSA_ENABLE_IPC_MODE_LEGACY='0')
    proc = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'weak_dp_rccl_worker.py')], env=env, capture_output=True,
                          text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    report = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith('{')][-1])
    assert report['ok'], report
    assert report['comm'].get('allreduce_weak_dp_norms', {}).get('calls', 0) == 2, report['comm']


# ---- refused calls ----------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_nothing_is_written(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    n, rows = 300, 9
    flat = on_gpu(torch, eng, np.random.default_rng(60).standard_normal(3 * n).astype(np.float32))
    gt = on_gpu(torch, eng, attacked(rows, n, seed=61))
    words = torch.zeros(n, dtype=torch.int32, device=flat.device)
    sq = eng.row_sqdist(gt, torch.zeros(n, device=gt.device))
    scales = torch.full((rows,), 7.0, dtype=torch.float64, device=flat.device)
    before, g_before = flat.clone(), gt.clone()
    x, out = flat[:n], flat[n:2 * n]

    def noise(sigma, offset, count, xp, op, seed=0):
        params = _native.NoiseParams(sigma, seed, 0, offset)
        return eng.lib.byz_gaussian_noise_dev(eng.ctx, _vp(xp.data_ptr()), count, ctypes.byref(params), None, _vp(op.data_ptr()), None)

    def weak_dp(clip, sigma, adaptive, offset, op):
        params = _native.WeakDpParams(clip, sigma, adaptive, 0, 0, offset)
        return eng.lib.byz_weak_dp_dev(eng.ctx, _vp(gt.data_ptr()), rows, n, n, ctypes.byref(params), _vp(op.data_ptr()), None)

    def clip_scales(clip, adaptive):
        params = _native.WeakDpParams(clip, 0.0, adaptive, 0, 0, 0)
        return eng.lib.byz_clip_scales_dev(eng.ctx, _vp(sq.data_ptr()), rows, ctypes.byref(params), _vp(scales.data_ptr()), None, None)

    for sigma in (float('nan'), -1.0, float('inf'), -0.0 - 1e-300):
        assert noise(sigma, 0, n, x, out) == _native.E_INVALID and 'sigma' in _native.last_error(), sigma
        assert weak_dp(1.0, sigma, 0, 0, out) == _native.E_INVALID, sigma
    assert noise(1.0, -1, n, x, out) == _native.E_INVALID and noise(1.0, 0, 0, x, out) == _native.E_INVALID
    assert noise(1.0, (1 << 62) - n + 1, n, x, out) == _native.E_INVALID           # past column 2^62
    assert noise(1.0, 0, n, x, flat[1:n + 1]) == _native.E_INVALID and 'overlaps' in _native.last_error()
    assert noise(1.0, 0, n, flat[n // 2:n // 2 + n], x) == _native.E_INVALID
    assert noise(0.0, 0, n, x, flat[1:n + 1]) == _native.E_INVALID                  # also where only a copy would run
    assert weak_dp(1.0, 1.0, 0, -1, out) == _native.E_INVALID
    for clip in (0.0, -1.0, float('nan')):
        assert weak_dp(clip, 1.0, 0, 0, out) == _native.E_INVALID, clip
        assert clip_scales(clip, 0) == _native.E_INVALID, clip
    assert weak_dp(1.0, 1.0, 0, 0, gt[rows - 1]) == _native.E_INVALID               # the output inside the matrix
    wparams = _native.NoiseParams(0.0, 0, 0, -1)
    assert eng.lib.byz_noise_words_dev(eng.ctx, ctypes.byref(wparams), n, _vp(words.data_ptr()), None) == _native.E_INVALID
    wparams = _native.NoiseParams(0.0, 0, 0, 0)
    assert eng.lib.byz_noise_words_dev(eng.ctx, ctypes.byref(wparams), 0, _vp(words.data_ptr()), None) == _native.E_INVALID
    eng.synchronize()
    assert torch.equal(flat.view(torch.int32), before.view(torch.int32)) and torch.equal(gt, g_before)
    assert not words.any() and bool((scales == 7.0).all())
    for bad in (float('nan'), -1.0, float('inf')):
        with pytest.raises(ValueError):
            eng.gaussian_noise(x, bad)
    with pytest.raises(ValueError):
        eng.gaussian_noise(x, 1.0, column_offset=-1)
    # what is accepted: a clip of +inf, the adaptive mode with any clip, out == x, the last column below 2^62
    assert weak_dp(float('inf'), 1.0, 0, 0, out) == 0 and weak_dp(-1.0, 1.0, 1, 0, out) == 0 and clip_scales(-1.0, 1) == 0
    assert noise(1.0, (1 << 62) - n, n, x, x) == 0
    eng.synchronize()
