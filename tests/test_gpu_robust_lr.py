"""The robust learning rate on the GPU against tests/test_robust_lr.py's numpy restatement.  Every comparison is exact: the
votes are integer counts, the flip is one bit, and the fused aggregate is no_defense's sequential fp32 chain.  No tolerance
appears anywhere: np.array_equal on int32 votes or on uint32 views of the floats."""
import ctypes

import numpy as np
import pytest

from tests.test_robust_lr import (bits, model_mean, restated_flip, restated_robust_lr, restated_votes, special_columns)
from tests.views_arena import arena, untouched

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


@pytest.fixture(scope='module')
def device(eng, torch):
    return torch.device('cuda', eng.device)


SPECIALS = np.array([2.5, -0.75, 0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-38, -1e-38, 3.4e38, -3.4e38,
                     1.0, -1.0], dtype=np.float32)


def theta_of(n):
    """A threshold inside the range with room either side where the height allows."""
    return max(1, n // 3)


def planted(n, d, seed):
    """Seeded normals; the special values in the first 16 columns (as many as the width has); behind them three columns whose
    abs(votes) is exactly theta - 1, theta and theta + 1 (v values of one sign, the rest zeros, which cast no vote)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d)).astype(np.float32)
    if n >= 4:
        block = special_columns(n)[0]
    else:       # too short for whole columns of one kind: every special value somewhere in the block
        block = np.stack([np.roll(SPECIALS, 3 * r) for r in range(n)])
    w = min(16, d)
    g[:, :w] = block[:, :w]
    theta = theta_of(n)
    for k, v in enumerate((theta - 1, theta, theta + 1)):
        c = 16 + k
        if c < d and 0 <= v <= n:
            g[:, c] = 0.0
            g[:v, c] = -3.0 if k == 1 else 3.0
    g.setflags(write=False)
    return g


def wide_width(torch, device):
    """The first width past walk_shape's four-wide threshold, plus 3: the dwordx4 path with a masked last vector."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return 4 * 256 * cus * 2 + 3


_WANT = {}


def reference(g, key):
    """(votes, mean) of the restatement for a matrix, computed once per key and never written to."""
    if key not in _WANT:
        votes, mean = restated_votes(g), model_mean(g)
        votes.setflags(write=False)
        mean.setflags(write=False)
        _WANT[key] = (votes, mean)
    return _WANT[key]


def check_fused_and_votes(eng, torch, device, n, d):
    g = planted(n, d, seed=1000 * n + d % 997)
    votes_want, mean = reference(g, (n, d))
    theta = theta_of(n)
    if d >= 19:
        flip = np.abs(votes_want) < theta
        assert flip.any() and (~flip).any()             # the restatement takes both branches
        if n >= 3:
            assert (np.abs(votes_want[16:19]) == np.array([theta - 1, theta, theta + 1])).all()
    gt = torch.from_numpy(g).to(device)
    got_votes = eng.sign_votes(gt)
    assert got_votes.dtype == torch.int32 and np.array_equal(got_votes.cpu().numpy(), votes_want)
    assert eng.robust_lr_info() == 0                  # the vote alone has no threshold
    plain = eng.no_defense(gt).cpu().numpy()
    assert np.array_equal(bits(plain), bits(mean))
    for th in sorted({0, theta, n}):
        out, votes = eng.robust_lr(gt, th, return_votes=True)
        want = restated_robust_lr(g, th, agg=mean)
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)), th
        assert np.array_equal(votes.cpu().numpy(), votes_want), th
        assert eng.robust_lr_info() == int((np.abs(votes_want) < th).sum()), th
        if th == 0:
            assert np.array_equal(bits(out.cpu().numpy()), bits(plain))
    out = eng.robust_lr(gt, theta)                     # without the votes: the pointer is null
    assert np.array_equal(bits(out.cpu().numpy()), bits(restated_robust_lr(g, theta, agg=mean)))


# heights around walk_rows' runs of 8; one column per thread: one column, under one wave, several workgroups and a ragged last
@pytest.mark.parametrize('d', [1, 63, 1025])
@pytest.mark.parametrize('n', [1, 7, 8, 9, 17, 100])
def test_fused_and_votes_are_the_restatement(eng, torch, device, n, d):
    check_fused_and_votes(eng, torch, device, n, d)


@pytest.mark.parametrize('n', [9, 17])
def test_four_wide_walk_with_a_masked_last_vector(eng, torch, device, n):
    check_fused_and_votes(eng, torch, device, n, wide_width(torch, device))


def test_out_of_range_theta_and_shapes_are_refused(eng, torch, device):
    gt = torch.zeros((5, 8), dtype=torch.float32, device=device)
    for bad in (-1, 6, 2.5):
        with pytest.raises(ValueError):
            eng.robust_lr(gt, bad)
        with pytest.raises(ValueError):
            eng.robust_lr(np.zeros((5, 8), dtype=np.float32), bad)
    out = torch.zeros(8, dtype=torch.float32, device=device)
    vp = ctypes.c_void_p
    from attacking_federate_learning_amd import _native
    rc = eng.lib.byz_robust_lr_dev(eng.ctx, vp(gt.data_ptr()), 5, 8, 8, 6, vp(out.data_ptr()), None, None)
    assert rc == _native.E_INVALID
    rc = eng.lib.byz_robust_lr_dev(eng.ctx, vp(gt.data_ptr()), 5, 8, 7, 1, vp(out.data_ptr()), None, None)      # ld < n_cols
    assert rc == _native.E_INVALID
    rc = eng.lib.byz_robust_lr_dev(eng.ctx, vp(gt.data_ptr()), 5, 8, 8, 1, None, None, None)
    assert rc == _native.E_INVALID
    rc = eng.lib.byz_sign_votes_dev(eng.ctx, vp(gt.data_ptr()), (1 << 20) + 1, 8, 8, vp(out.data_ptr()), None)
    assert rc == _native.E_UNSUPPORTED
    rc = eng.lib.byz_sign_flip_dev(eng.ctx, vp(out.data_ptr()), vp(out.data_ptr()), 8, -1, vp(out.data_ptr()), None)
    assert rc == _native.E_INVALID


# ---- wrapping another rule ----------------------------------------------------------------------------------------------------
COMPOSE = (33, 2051)


def compose_input():
    n, d = COMPOSE
    g = np.array(planted(n, d, seed=33))
    g[:, :16] = np.random.default_rng(34).standard_normal((n, 16)).astype(np.float32)       # (the rules sort: finite input)
    g.setflags(write=False)
    return g


@pytest.mark.parametrize('rule', ['trimmed_mean', 'coordinate_median', 'rank_trimmed_mean'])
def test_then_composition_flips_the_rules_own_aggregate(eng, torch, device, rule):
    from attacking_federate_learning_amd import defences
    n, d = COMPOSE
    f = 8
    g = compose_input()
    votes_want, _ = reference(g, ('compose',) + COMPOSE)
    then = getattr(defences, rule)
    gt = torch.from_numpy(g).to(device)
    agg = then(gt, n, f).cpu().numpy()
    for theta in (None, 0, n):
        th = f + 1 if theta is None else theta
        want = restated_flip(agg, votes_want, th)
        flip = np.abs(votes_want) < th
        if theta is None:
            assert flip.any() and (~flip).any()
        out, votes = defences.robust_lr(gt, n, f, theta=theta, then=then, return_votes=True)
        assert out.is_cuda and votes.is_cuda              # the matrix and the results stay on the device
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)), (rule, theta)
        assert np.array_equal(votes.cpu().numpy(), votes_want)
        assert eng.robust_lr_info() == int(flip.sum())
    # a host matrix: uploaded once, the same bits back as numpy
    got = defences.robust_lr(g, n, f, then=then)
    assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(restated_flip(agg, votes_want, f + 1)))


def test_host_path_gives_the_device_calls_bits_as_numpy(eng, torch, device):
    from attacking_federate_learning_amd import defences
    n, d, f = 17, 1025, 4
    g = planted(n, d, seed=1000 * n + d % 997)
    votes_want, mean = reference(g, (n, d))
    on_device = defences.robust_lr(torch.from_numpy(g).to(device), n, f)
    got, votes = defences.robust_lr(g, n, f, return_votes=True)
    assert isinstance(got, np.ndarray) and isinstance(votes, np.ndarray) and votes.dtype == np.int32
    assert np.array_equal(bits(got), bits(on_device.cpu().numpy()))
    assert np.array_equal(bits(got), bits(restated_robust_lr(g, f + 1, agg=mean)))
    assert np.array_equal(votes, votes_want)
    assert np.array_equal(eng.sign_votes(g), votes_want)
    flipped = eng.sign_flip(mean, votes_want, f + 1)
    assert isinstance(flipped, np.ndarray) and np.array_equal(bits(flipped), bits(got))
    # DeviceBuffers, for a host without torch
    buf = eng.to_device(g)
    out, votes_buf = eng.robust_lr(buf, f + 1, return_votes=True)
    assert np.array_equal(bits(out.numpy()), bits(got)) and np.array_equal(votes_buf.numpy(), votes_want)


def test_raw_ctypes_host_call(eng):
    n, d, theta = 9, 63, 3
    g = planted(n, d, seed=1000 * n + d % 997)
    votes_want, mean = reference(g, (n, d))
    out = np.empty(d, dtype=np.float32)
    votes = np.empty(d, dtype=np.int32)
    vp = ctypes.c_void_p
    rc = eng.lib.byz_robust_lr_host(eng.ctx, g.ctypes.data_as(vp), n, d, theta, out.ctypes.data_as(vp), votes.ctypes.data_as(vp))
    assert rc == 0
    assert np.array_equal(bits(out), bits(restated_robust_lr(g, theta, agg=mean))) and np.array_equal(votes, votes_want)
    flipped = ctypes.c_int64(-1)
    assert eng.lib.byz_robust_lr_info(eng.ctx, ctypes.byref(flipped)) == 0
    assert flipped.value == int((np.abs(votes_want) < theta).sum())
    rc = eng.lib.byz_robust_lr_host(eng.ctx, g.ctypes.data_as(vp), n, d, theta, out.ctypes.data_as(vp), None)
    assert rc == 0 and np.array_equal(bits(out), bits(restated_robust_lr(g, theta, agg=mean)))


# ---- views ------------------------------------------------------------------------------------------------------------------
def guarded_call(eng, torch, device, view, theta):
    """byz_robust_lr_dev on `view` with out and votes inside NaN / sentinel guard bands -> (out, votes) as numpy; asserts that
    the bands are untouched."""
    n, d = view.shape
    guard = 64
    out_flat = torch.full((d + 2 * guard,), float('nan'), dtype=torch.float32, device=device)
    votes_flat = torch.full((d + 2 * guard,), -123456789, dtype=torch.int32, device=device)
    out_before, votes_before = out_flat.clone(), votes_flat.clone()
    vp = ctypes.c_void_p
    stream = torch.cuda.current_stream(device).cuda_stream
    rc = eng.lib.byz_robust_lr_dev(eng.ctx, vp(view.data_ptr()), n, d, view.stride(0), theta,
                                   vp(out_flat.data_ptr() + 4 * guard), vp(votes_flat.data_ptr() + 4 * guard), vp(stream))
    assert rc == 0
    torch.cuda.synchronize(device)
    for flat, before in ((out_flat.view(torch.int32), out_before.view(torch.int32)), (votes_flat, votes_before)):
        assert torch.equal(flat[:guard], before[:guard]) and torch.equal(flat[guard + d:], before[guard + d:])
    return out_flat[guard:guard + d].cpu().numpy(), votes_flat[guard:guard + d].cpu().numpy()


def test_strided_view_inside_a_nan_arena(eng, torch, device):
    n, d = 17, 1025
    g = planted(n, d, seed=1000 * n + d % 997)
    votes_want, mean = reference(g, (n, d))
    theta = theta_of(n)
    view, flat = arena(torch, g, d + 13, 0, device=device)
    before = flat.clone()
    out, votes = guarded_call(eng, torch, device, view, theta)
    untouched(torch, flat, view, before)
    assert np.array_equal(bits(out), bits(restated_robust_lr(g, theta, agg=mean))) and np.array_equal(votes, votes_want)
    assert np.array_equal(eng.sign_votes(view).cpu().numpy(), votes_want)
    assert np.array_equal(bits(eng.robust_lr(view, theta).cpu().numpy()), bits(out))


def test_misaligned_base_takes_the_one_column_path_and_gives_the_same_bits(eng, torch, device):
    n, d = 9, wide_width(torch, device)
    g = planted(n, d, seed=1000 * n + d % 997)
    votes_want, mean = reference(g, (n, d))
    theta = theta_of(n)
    ld = (d // 4 + 1) * 4                                 # every row as misaligned as the base: 20 bytes off a 16-byte boundary
    view, flat = arena(torch, g, ld, 5, device=device)
    assert view.data_ptr() % 16 == 4 and (view.data_ptr() - 20) % 16 == 0 and ld % 4 == 0
    before = flat.clone()
    out, votes = guarded_call(eng, torch, device, view, theta)
    untouched(torch, flat, view, before)
    assert np.array_equal(bits(out), bits(restated_robust_lr(g, theta, agg=mean))) and np.array_equal(votes, votes_want)


def test_sign_flip_in_place_and_out_of_place(eng, torch, device):
    n, d = 17, 1025
    g = planted(n, d, seed=1000 * n + d % 997)
    votes_want, mean = reference(g, (n, d))
    theta = theta_of(n)
    want = restated_flip(mean, votes_want, theta)
    agg = torch.from_numpy(np.array(mean)).to(device)
    votes = torch.from_numpy(np.array(votes_want)).to(device)
    out = eng.sign_flip(agg, votes, theta)
    assert out.data_ptr() != agg.data_ptr() and np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert np.array_equal(bits(agg.cpu().numpy()), bits(mean))
    assert eng.robust_lr_info() == int((np.abs(votes_want) < theta).sum())
    same = eng.sign_flip(agg, votes, theta, out=agg)
    assert same is agg and np.array_equal(bits(agg.cpu().numpy()), bits(want))
    eng.sign_flip(agg, votes, theta, out=agg)            # an involution: twice is the aggregate again
    assert np.array_equal(bits(agg.cpu().numpy()), bits(mean))
    assert np.array_equal(bits(eng.sign_flip(agg, votes, 0).cpu().numpy()), bits(mean)) and eng.robust_lr_info() == 0


# ---- the columns layout -------------------------------------------------------------------------------------------------------
def test_three_uneven_column_panels_give_the_bits_of_the_one_call(eng, torch, device):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d, f = 17, 1025, 4
    g = planted(n, d, seed=1000 * n + d % 997)
    votes_want, mean = reference(g, (n, d))
    gt = torch.from_numpy(g).to(device)
    whole, whole_votes = eng.robust_lr(gt, f + 1, return_votes=True)
    parts, part_votes, flipped = [], [], 0
    for lo, hi in ((0, 300), (300, 301), (301, d)):
        out, votes = eng.robust_lr(gt[:, lo:hi], f + 1, return_votes=True)      # a panel: a strided view, ld = d
        flipped += eng.robust_lr_info()
        parts.append(out)
        part_votes.append(votes)
    assert torch.equal(torch.cat(parts).view(torch.int32), whole.view(torch.int32))
    assert torch.equal(torch.cat(part_votes), whole_votes)
    assert flipped == int((np.abs(votes_want) < f + 1).sum())
    agg = ShardedAggregator(HipKernels(eng))
    assert agg.world == 1
    sharded = agg.robust_lr(gt, n, f, gather=True, total_columns=d)
    assert torch.equal(sharded.view(torch.int32), whole.view(torch.int32))
    assert np.array_equal(bits(whole.cpu().numpy()), bits(restated_robust_lr(g, f + 1, agg=mean)))
    assert np.array_equal(HipKernels(eng).sign_votes(gt).cpu().numpy(), votes_want)


# ---- the server ---------------------------------------------------------------------------------------------------------------
def test_device_server_moves_the_weights_by_the_restated_vector(eng, torch, device):
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.server import DeviceServer
    n, d, mal_prop = 17, 1025, 0.24
    f = int(n * mal_prop)
    g = planted(n, d, seed=1000 * n + d % 997)
    votes_want, mean = reference(g, (n, d))
    w0 = np.random.default_rng(3).standard_normal(d).astype(np.float32)
    for then in (None, defences.coordinate_median):
        server = DeviceServer(n, w0, mal_prop, 0.1, 0.9, torch_device=device, engine=eng)
        server.users_grads.data.copy_(torch.from_numpy(g))
        server.velocity.fill_(0.25)
        if then is None:
            expect = restated_robust_lr(g, f + 1, agg=mean)
            agg = server.defend_robust_lr()
        else:
            finite = torch.from_numpy(np.nan_to_num(g, nan=0.0, posinf=9.0, neginf=-9.0)).to(device)
            server.users_grads.data.copy_(finite)
            expect = restated_flip(then(finite, n, f).cpu().numpy(), restated_votes(finite.cpu().numpy()), f + 1)
            agg = server.defend_robust_lr(then=then)
        assert np.array_equal(bits(agg.cpu().numpy()), bits(expect))
        w = torch.from_numpy(w0).to(device)
        v = torch.full_like(w, 0.25)
        eng.server_update(w, v, torch.from_numpy(np.array(expect)).to(device), 0.9, 0.1)
        assert torch.equal(server.current_weights.view(torch.int32), w.view(torch.int32))
        assert torch.equal(server.velocity.view(torch.int32), v.view(torch.int32))
    with pytest.raises(TypeError):
        server.defend_robust_lr(then='trimmed_mean')
