"""SparseFed's global top-k on an MI355X, held to the numpy restatement of tests/test_sparsefed.py BIT FOR BIT:
out, residual, the threshold key and the tie counts; no tolerance appears for the selection.  The lengths cross every
boundary of the kernels: one column, either side of a wave and of a workgroup, several one-tile chunks, the first length at
which the kernels go four-wide and the first at which a chunk holds more than one tile (both computed from the CU count,
plus 3: a masked last vector, a ragged last chunk).  The clipped mean in front of it is held to its own tolerance by
tests/test_gpu_centered_clip.py, and top-k is discontinuous, so `sparsefed` is checked compositionally: its top-k against the
restatement applied to the GPU's own clipped mean, bit for bit, and that clipped mean against its restatement separately."""
import ctypes

import numpy as np
import pytest

from tests import views_arena
from tests.test_centered_clip import restated_centered_clip
from tests.test_geometric_median import attacked
from tests.test_gpu_centered_clip import close
from tests.test_sparsefed import NO_KEY, bits, planted, restated_topk

pytestmark = pytest.mark.gpu

SMALL = [1, 63, 64, 65, 255, 257, 1025]
INFO_KEYS = ('selected', 'threshold_key', 'ties', 'ties_taken')


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:%d' % eng.device)


def four_wide_length(torch, eng):
    """The first length at which topk.hip goes four-wide (4 * 256 columns per CU), plus 3: one tile per chunk, a masked last
    vector."""
    return 4 * 256 * torch.cuda.get_device_properties(eng.device).multi_processor_count + 3


def wide_length(torch, eng):
    """The first length past the four-wide threshold at which there are more tiles than chunks (8 per CU), plus 3: chunks of two
    tiles, a ragged last chunk, a masked last vector, and ties that fall into different chunks."""
    return 4 * 256 * 8 * torch.cuda.get_device_properties(eng.device).multi_processor_count + 3


def ks_of(n):
    return sorted({0, 1, n // 3, n - 1, n} - {-1})


def check_topk(eng, torch, x, k, add=None):
    """One device call against the restatement: out, residual and the info, bit for bit."""
    want_out, want_res, want = restated_topk(x, k, add=add, return_info=True)
    out, res, info = eng.topk_sparsify(on_gpu(torch, eng, x), k, add=None if add is None else on_gpu(torch, eng, add),
                                       return_info=True)
    out, res = out.cpu().numpy(), res.cpu().numpy()
    print('n', x.size, 'k', k, 'info', info, 'want', {key: want[key] for key in INFO_KEYS})
    assert np.array_equal(bits(out), bits(want_out)), np.flatnonzero(bits(out) != bits(want_out))[:8]
    assert np.array_equal(bits(res), bits(want_res)), np.flatnonzero(bits(res) != bits(want_res))[:8]
    assert {key: info[key] for key in INFO_KEYS} == {key: want[key] for key in INFO_KEYS}
    return out, res, info


def all_equal(n):
    x = np.full(n, 0.375, dtype=np.float32)
    x[::3] = -0.375
    return x


# ---- the selection ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SMALL)
def test_planted_normals_at_every_small_length_and_k(eng, torch, n):
    x = planted(n, seed=100 + n)
    for k in ks_of(n):
        _, _, info = check_topk(eng, torch, x, k)
        assert info['selected'] == k
    assert check_topk(eng, torch, x, 0)[2]['threshold_key'] == NO_KEY


@pytest.mark.parametrize('which', ['four_wide', 'wide'])
def test_planted_normals_at_the_computed_lengths(eng, torch, which):
    n = four_wide_length(torch, eng) if which == 'four_wide' else wide_length(torch, eng)
    x = planted(n, seed=7)
    for k in ks_of(n):
        check_topk(eng, torch, x, k)


@pytest.mark.parametrize('n', SMALL)
def test_an_all_equal_vector_of_mixed_signs_takes_its_first_k(eng, torch, n):
    x = all_equal(n)
    for k in ks_of(n):
        out, _, info = check_topk(eng, torch, x, k)
        assert np.array_equal(out != 0, np.arange(n) < k)
        assert info['ties'] == (n if k else 0) and info['ties_taken'] == k


@pytest.mark.parametrize('which', ['four_wide', 'wide'])
def test_an_all_equal_vector_at_the_computed_lengths(eng, torch, which):
    n = four_wide_length(torch, eng) if which == 'four_wide' else wide_length(torch, eng)
    x = all_equal(n)
    for k in ks_of(n) + [n // 2 + 1]:
        out, _, _ = check_topk(eng, torch, x, k)
        assert np.array_equal(out != 0, np.arange(n) < k)


def test_threshold_ties_at_both_ends_and_the_middle_give_the_first_two(eng, torch):
    for n in (65, 1025, four_wide_length(torch, eng), wide_length(torch, eng)):
        x = (np.random.default_rng(n).uniform(0.001, 0.5, n) * np.random.default_rng(n + 1).choice([-1.0, 1.0], n)).astype(np.float32)
        big = [5, n // 5, n - 7]
        x[big] = [3.0, -4.0, 5.0]
        ties = [0, n // 2, n - 1]
        x[ties] = [0.75, -0.75, 0.75]
        out, res, info = check_topk(eng, torch, x, len(big) + 2)
        assert info['ties'] == 3 and info['ties_taken'] == 2 and info['threshold_key'] == 0x3f400000
        assert out[0] == 0.75 and out[n // 2] == -0.75 and out[n - 1] == 0.0 and res[n - 1] == 0.75
        # the quota of one and of three: the first alone, all of them
        assert check_topk(eng, torch, x, len(big) + 1)[0][n // 2] == 0.0
        assert check_topk(eng, torch, x, len(big) + 3)[0][n - 1] == 0.75


def test_neighbours_that_differ_in_the_lowest_mantissa_bit_or_only_in_the_exponent(eng, torch):
    n = 1025
    base = np.random.default_rng(3).uniform(0.001, 0.01, n).astype(np.float32)
    # the last pass decides: 1.5 with the lowest mantissa bit set, clear, and one below, among ties of 1.5
    x = base.copy()
    at = np.array([3, 200, 201, 640, 1024])
    x.view(np.uint32)[at] = [0x3fc00000, 0x3fc00001, 0xbfc00000, 0x3fbfffff, 0x3fc00000]
    for k in (1, 2, 3, 4, 5):
        check_topk(eng, torch, x, k)
    out, _, info = check_topk(eng, torch, x, 3)
    assert info['threshold_key'] == 0x3fc00000 and info['ties'] == 3 and info['ties_taken'] == 2
    assert bits(out)[3] == 0x3fc00000 and bits(out)[201] == 0xbfc00000 and out[1024] == 0.0 and out[640] == 0.0
    # the first pass decides: the same mantissa at neighbouring exponents
    x = base.copy()
    x.view(np.uint32)[at] = [0x40400000, 0x40c00000, 0xc0400000, 0x3fc00000, 0x40400000]       # 3, 6, -3, 1.5, 3
    for k in (1, 2, 3, 4, 5):
        check_topk(eng, torch, x, k)


# ---- the fused addition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [5, 257, 1025])
def test_the_error_feedback_addition_is_one_fp32_addition(eng, torch, n):
    x = planted(n, seed=20 + n).copy()
    add = planted(n, seed=21 + n)[::-1].copy()
    x[:5] = [3e38, np.inf, 1.0, 2.0 ** -126, -3e38]
    add[:5] = [3e38, -np.inf, 2.0 ** -24, -2.0 ** -127, -3e38]           # overflow, inf - inf = NaN, absorbed, a denormal sum
    for k in ks_of(n):
        check_topk(eng, torch, x, k, add=add)
    if n == 5:
        out, _, _ = check_topk(eng, torch, x, 1, add=add)
        assert np.isnan(out[1]) and not out[[0, 2, 3, 4]].any()          # the NaN is selected first and shows in the step


def test_the_computed_lengths_with_an_addition(eng, torch):
    for n in (four_wide_length(torch, eng), wide_length(torch, eng)):
        check_topk(eng, torch, planted(n, seed=30), n // 3, add=planted(n, seed=31)[::-1].copy())


# ---- in place, refused, determinism -------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [65, 1025, 'four_wide'])
def test_in_place_gives_the_bits_of_the_out_of_place_call(eng, torch, n):
    n = four_wide_length(torch, eng) if n == 'four_wide' else n
    x, add = planted(n, seed=40), planted(n, seed=41)[::-1].copy()
    k = n // 3 + 1
    xt, at = on_gpu(torch, eng, x), on_gpu(torch, eng, add)
    want_out, want_res = eng.topk_sparsify(xt, k, add=at)
    assert views_arena.same_bits(xt.cpu().numpy(), x) and views_arena.same_bits(at.cpu().numpy(), add)      # inputs are only read
    out, res = eng.topk_sparsify(xt, k, add=at, out=at, residual=xt)
    assert out is at and res is xt
    assert torch.equal(at.view(torch.int32), want_out.view(torch.int32))
    assert torch.equal(xt.view(torch.int32), want_res.view(torch.int32))
    # without an addition: the memory split where it lies
    xt = on_gpu(torch, eng, x)
    o2, r2 = eng.topk_sparsify(on_gpu(torch, eng, x), k)
    out, res = eng.topk_sparsify(xt, k, residual=xt)
    assert torch.equal(out.view(torch.int32), o2.view(torch.int32)) and torch.equal(xt.view(torch.int32), r2.view(torch.int32))


def test_other_overlaps_and_a_k_outside_the_length_are_refused_and_nothing_is_written(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    n = 300
    flat = on_gpu(torch, eng, np.random.default_rng(50).standard_normal(4 * n).astype(np.float32))
    before = flat.clone()
    x, add, out, res = (flat[i * n:(i + 1) * n] for i in range(4))

    def call(x, add, k, out, res, n=n):
        return eng.lib.byz_topk_sparsify_dev(eng.ctx, _vp(x.data_ptr()), _vp(add.data_ptr()) if add is not None else None, n, k,
                                             _vp(out.data_ptr()), _vp(res.data_ptr()) if res is not None else None, None)
    # out is x; residual is add; out is residual; out across x and add; residual across add and out; out is x with no addition;
    # out across itself and residual
    for args in ((x, add, 10, x, res), (x, add, 10, out, add), (x, add, 10, out, out), (x, add, 10, flat[n // 2:n // 2 + n], res),
                 (x, add, 10, out, flat[n + 1:2 * n + 1]), (x, None, 10, x, None), (x, add, 10, flat[2 * n + 5:3 * n + 5], res)):
        assert call(*args) == _native.E_INVALID, [a if a is None or isinstance(a, int) else a.data_ptr() for a in args]
        assert 'overlaps' in _native.last_error()
    for k in (-1, n + 1):
        assert call(x, add, k, out, res) == _native.E_INVALID and 'outside 0..%d' % n in _native.last_error()
    assert call(x, add, 0, out, res, n=0) == _native.E_INVALID
    eng.synchronize()
    assert torch.equal(flat.view(torch.int32), before.view(torch.int32))
    for bad in (-1, n + 1, 2.5, True):
        with pytest.raises(ValueError):
            eng.topk_sparsify(x, bad)
    with pytest.raises(ValueError):
        eng.topk_sparsify(x, 3, out=np.empty(n, dtype=np.float32))
    assert call(x, add, 10, out, res) == 0                                # the four separate vectors are accepted
    eng.synchronize()


def test_two_calls_give_the_same_bits(eng, torch):
    n = wide_length(torch, eng)
    x = on_gpu(torch, eng, planted(n, seed=60))
    add = on_gpu(torch, eng, all_equal(n))
    a = eng.topk_sparsify(x, n // 7, add=add, return_info=True)
    b = eng.topk_sparsify(x, n // 7, add=add, return_info=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert a[2] == b[2]


# ---- a misaligned caller ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [257, 1025, 'four_wide'])
def test_views_into_a_guard_banded_arena_give_the_dense_bits_and_leave_the_guard(eng, torch, n):
    n = four_wide_length(torch, eng) if n == 'four_wide' else n
    x, add = planted(n, seed=70), planted(n, seed=71)[::-1].copy()
    k = n // 3
    want_out, want_res = eng.topk_sparsify(on_gpu(torch, eng, x), k, add=on_gpu(torch, eng, add))
    dev = 'cuda:%d' % eng.device
    for offs in ((1, 2, 3, 1), (0, 0, 0, 1), (1, 0, 0, 0)):       # every vector off a 16-byte boundary; one of them only
        views, flats = zip(*(views_arena.arena(torch, v[None, :], n + 5, off, device=dev)
                             for v, off in zip((x, add, np.zeros(n, np.float32), np.zeros(n, np.float32)), offs)))
        befores = [f.clone() for f in flats]
        xv, av, ov, rv = (v[0] for v in views)
        assert xv.is_contiguous() and xv.data_ptr() % 16 == 4 * (offs[0] % 4)
        out, res = eng.topk_sparsify(xv, k, add=av, out=ov, residual=rv)
        assert views_arena.same_bits(ov.cpu().numpy(), want_out.cpu().numpy())
        assert views_arena.same_bits(rv.cpu().numpy(), want_res.cpu().numpy())
        assert views_arena.same_bits(xv.cpu().numpy(), x) and views_arena.same_bits(av.cpu().numpy(), add)
        for view, flat, before in zip(views, flats, befores):
            views_arena.untouched(torch, flat, view, before)


# ---- sparsefed, compositionally -------------------------------------------------------------------------------------------
def sparsefed_case(n, d, seed):
    g = attacked(n, d, seed=seed)
    g[1] *= np.float32(40.0)                      # a row far outside the clipping norm
    g[n - 2, d // 2] = np.nan                     # an excluded row: one NaN
    memory = (0.05 * np.random.default_rng(seed + 1).standard_normal(d)).astype(np.float32)
    return g, memory


@pytest.mark.parametrize('n,d', [(7, 63), (17, 1025), (100, 5000)])
@pytest.mark.parametrize('clip', [2.0, np.inf])
def test_sparsefed_is_the_top_k_of_the_memory_plus_the_gpus_own_clipped_mean(eng, torch, n, d, clip):
    from attacking_federate_learning_amd import defences
    g, memory = sparsefed_case(n, d, seed=n + d)
    gt = on_gpu(torch, eng, g)
    k = max(1, d // 10)
    agg, cinfo = eng.centered_clip(gt, tau=clip, iters=1, return_info=True)
    agg = agg.cpu().numpy()
    want_agg, winfo = restated_centered_clip(g, tau=clip, iters=1, start=None)
    print('max |agg - restated|', float(np.nanmax(np.abs(agg - want_agg))))
    assert close(agg, want_agg, g)
    assert cinfo['excluded_rows'] == winfo['excluded_rows'] == 1
    assert (cinfo['clipped_rows'] >= 1) == np.isfinite(clip)
    for start in (None, memory):
        res_in = None if start is None else on_gpu(torch, eng, start)
        out, res, info = eng.sparsefed(gt, k, clip=clip, residual=res_in, return_info=True)
        assert res_in is None or res is res_in                     # the caller's memory, updated in place
        base = np.zeros(d, dtype=np.float32) if start is None else start
        want_out, want_res, want = restated_topk(base, k, add=agg, return_info=True)
        assert views_arena.same_bits(out.cpu().numpy(), want_out) and views_arena.same_bits(res.cpu().numpy(), want_res)
        assert {key: info[key] for key in INFO_KEYS} == {key: want[key] for key in INFO_KEYS}
        assert (info['clipped_rows'], info['excluded_rows']) == (cinfo['clipped_rows'], 1)
        # the drop-in entry and a host matrix: the same bits
        step, mem = defences.sparsefed(
            g, n, 0, k=k, clip=clip, residual=None if start is None else start.copy(), return_residual=True)
        assert views_arena.same_bits(step, want_out) and views_arena.same_bits(mem, want_res)


def test_sparsefed_refuses_overlaps_and_bad_parameters(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    n, d = 9, 200
    gt = on_gpu(torch, eng, attacked(n, d, seed=80))
    res, out = torch.zeros(d, device=gt.device), torch.zeros(d, device=gt.device)

    def call(clip, k, res_ptr, out_ptr):
        params = _native.SparsefedParams(clip, k)
        return eng.lib.byz_sparsefed_dev(eng.ctx, _vp(gt.data_ptr()), n, d, d, ctypes.byref(params), _vp(res_ptr), _vp(out_ptr), None)
    assert call(1.0, 5, res.data_ptr(), res.data_ptr()) == _native.E_INVALID
    assert call(1.0, 5, res.data_ptr(), gt.data_ptr() + 4 * d) == _native.E_INVALID
    assert call(1.0, 5, gt.data_ptr(), out.data_ptr()) == _native.E_INVALID
    for clip, k in ((0.0, 5), (-1.0, 5), (float('nan'), 5), (1.0, -1), (1.0, d + 1)):
        assert call(clip, k, res.data_ptr(), out.data_ptr()) == _native.E_INVALID, (clip, k)
    eng.synchronize()
    assert not res.any() and not out.any()
    with pytest.raises(ValueError):
        eng.sparsefed(gt, d + 1)
    with pytest.raises(ValueError):
        eng.sparsefed(gt, 5, residual=np.zeros(d, dtype=np.float32))


def test_then_supplies_the_aggregate(eng, torch):
    from attacking_federate_learning_amd import defences
    n, d, k = 21, 1500, 40
    g = attacked(n, d, seed=81)
    gt = on_gpu(torch, eng, g)
    memory = (0.05 * np.random.default_rng(82).standard_normal(d)).astype(np.float32)
    med = defences.coordinate_median(gt, n, 4).cpu().numpy()
    assert np.array_equal(med, np.median(g, axis=0))
    mt = on_gpu(torch, eng, memory)
    step, mem = defences.sparsefed(gt, n, 4, k=k, residual=mt, then=defences.coordinate_median, return_residual=True)
    want_out, want_res = restated_topk(memory, k, add=med)
    assert mem is mt and views_arena.same_bits(step.cpu().numpy(), want_out) and views_arena.same_bits(mt.cpu().numpy(), want_res)
    step = defences.sparsefed(g, n, 4, then=defences.coordinate_median)              # a host matrix, the default k, a zero memory
    assert views_arena.same_bits(step, restated_topk(med, max(1, d // 100))[0])
    with pytest.raises(TypeError):
        defences.sparsefed(gt, n, 4, then='median')


def test_three_rounds_through_the_device_server_carry_the_memory(eng, torch):
    from attacking_federate_learning_amd.server import DeviceServer
    n, d, k, clip = 30, 3000, 120, 3.0
    weights = np.random.default_rng(83).standard_normal(d).astype(np.float32)
    dev = 'cuda:%d' % eng.device
    server = DeviceServer(n, weights, 0.2, 0.1, 0.0, torch_device=dev, engine=eng)        # momentum 0: the paper's Algorithm 1
    assert torch.equal(server.sparse_residual, torch.zeros(d, dtype=torch.float32, device=dev))
    memory = np.zeros(d, dtype=np.float32)
    w, vel = on_gpu(torch, eng, weights), torch.zeros(d, dtype=torch.float32, device=dev)
    carried = 0
    for seed in (84, 85, 86):
        g, _ = sparsefed_case(n, d, seed)
        gt = on_gpu(torch, eng, g)
        server.users_grads.data.copy_(gt)
        before = server.current_weights.clone()
        step = server.defend_sparsefed(k=k, clip=clip)
        agg = eng.centered_clip(gt, tau=clip, iters=1).cpu().numpy()
        assert close(agg, restated_centered_clip(g, tau=clip, iters=1)[0], g)
        want_out, memory, want = restated_topk(memory, k, add=agg, return_info=True)
        assert views_arena.same_bits(step.cpu().numpy(), want_out)
        assert views_arena.same_bits(server.sparse_residual.cpu().numpy(), memory)
        # what round t left in the memory decides round t + 1: some selected coordinate is one the aggregate alone would not take
        carried += int((want['mask'] & ~restated_topk(agg, k, return_info=True)[2]['mask']).sum())
        eng.server_update(w, vel, step, 0.0, 0.1)
        assert torch.equal(server.current_weights, w) and torch.equal(server.velocity, vel)
        moved = (server.current_weights != before).cpu().numpy()
        assert not (moved & ~want['mask']).any() and moved.sum() > 0          # the weights move in selected coordinates only
    assert carried > 0


# ---- the host entry points ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 257, 5000])
def test_the_host_entry_points_give_the_device_bits(eng, torch, n):
    x, add = planted(n, seed=90), planted(n, seed=91)[::-1].copy()
    k = n // 3
    want_out, want_res, want = eng.topk_sparsify(on_gpu(torch, eng, x), k, add=on_gpu(torch, eng, add), return_info=True)
    out, res, info = eng.topk_sparsify(x, k, add=add, return_info=True)
    assert isinstance(out, np.ndarray) and views_arena.same_bits(out, want_out.cpu().numpy())
    assert views_arena.same_bits(res, want_res.cpu().numpy()) and info == want
    out, res = eng.topk_sparsify(x, k)                                           # no addition, and in place on the host
    xc = x.copy()
    o2, r2 = eng.topk_sparsify(xc, k, residual=xc)
    assert r2 is xc and views_arena.same_bits(o2, out) and views_arena.same_bits(xc, res)
    assert views_arena.same_bits(out, restated_topk(x, k)[0])
    if n >= 257:
        g, memory = sparsefed_case(9, n, seed=92)
        dev_out, dev_res = eng.sparsefed(on_gpu(torch, eng, g), k, clip=2.0, residual=on_gpu(torch, eng, memory))
        mem = memory.copy()
        host_out, host_res = eng.sparsefed(g, k, clip=2.0, residual=mem)
        assert host_res is mem and views_arena.same_bits(host_out, dev_out.cpu().numpy())
        assert views_arena.same_bits(mem, dev_res.cpu().numpy())
