"""AFA on the device against tests/test_afa.py's restatement of include/byzagg.h's rule.  On a given Gram the integers (flags,
rounds of removal, the report's counts and branch) are equal and the doubles (scores, mean, med, sd, thr, divisor) are equal AS
BITS, at every wave and slot boundary of the one-workgroup loop.  The whole call is held to the restatement on the device's own
Gram (exact) and on numpy's (through the margins tests/test_afa.py asserts); its aggregate is byz_scaled_rows_sum_dev's bits."""
import numpy as np
import pytest

from tests import views_arena
from tests.test_afa import (REPORT_FIELDS, STAT_FIELDS, THIN_SIZES, gram64, planted, restated_afa_select, thin_case,
                            thin_gram)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:%d' % eng.device)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_decisions(info, want):
    """the integers: flags, rounds of removal, the report's counts"""
    assert np.array_equal(info['round_of'], want['round_of']), np.flatnonzero(info['round_of'] != want['round_of'])
    assert {k: info[k] for k in REPORT_FIELDS} == {k: want[k] for k in REPORT_FIELDS}, (info, want)


def same_bits(info, want):
    assert np.array_equal(bits64(info['score']), bits64(want['score'])), np.flatnonzero(info['score'] != want['score'])
    for k in STAT_FIELDS:
        assert bits64(info[k]) == bits64(want[k]), (k, info[k], want[k])


def check_select(eng, c, weights=None, **params):
    rows, info = eng.afa_select(c, weights=weights, **params)
    want = restated_afa_select(c, weights, params.get('xi', 2.0), params.get('delta_xi', 0.5), params.get('max_rounds') or 0)
    assert np.array_equal(rows, np.flatnonzero(want['kept_flags']))
    same_decisions(info, want)
    same_bits(info, want)
    return info, want


# ---- the selection on a given Gram --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', THIN_SIZES)
def test_select_equals_the_restatement(eng, n):
    rows, info = eng.afa_select(thin_gram(n))
    want = thin_case(n)
    assert np.array_equal(rows, np.flatnonzero(want['kept_flags']))
    same_decisions(info, want)
    same_bits(info, want)
    assert info['excluded'] == 0 and not info['degenerate']
    assert eng.afa_info() == {k: info[k] for k in REPORT_FIELDS + STAT_FIELDS}


@pytest.mark.parametrize('n', [64, 65])
def test_odd_and_even_medians(eng, n):
    """one excluded row turns an even count odd and an odd one even"""
    c = thin_gram(n).copy()
    c[17, 17] = 0.0
    info, want = check_select(eng, c)
    assert info['excluded'] == 1 and info['round_of'][17] == 0 and info['kept'] + info['removed'] == n - 1


def test_identical_rows_remove_nobody(eng):
    row = np.random.default_rng(5).standard_normal(32).astype(np.float32)
    for n in (2, 65, 1025):
        info, want = check_select(eng, gram64(np.tile(row, (n, 1))))
        assert info['rounds'] == 1 and info['kept'] == n and info['branch'] == 0
    two, _ = check_select(eng, thin_gram(2))                    # mean = med exactly: the upper branch, nobody removed
    assert two['mean'] == two['med'] and two['thr'] > two['med'] and two['kept'] == 2


def test_weights_with_zeros_and_a_nan(eng):
    n = 1025
    w = np.random.default_rng(9).uniform(0.25, 4.0, n)
    w[[3, 1024]] = 0.0
    w[500] = np.nan
    info, want = check_select(eng, thin_gram(n), w)
    assert info['excluded'] == 3 and (info['round_of'][[3, 500, 1024]] == 0).all() and info['removed'] > 0
    assert info['divisor'] == want['divisor'] and info['divisor'] != float(info['kept'])


def test_unusable_rows_are_excluded(eng):
    n = 65
    c = thin_gram(n).copy()
    c[5, 5] = 0.0
    c[9, :] = c[:, 9] = np.nan
    c[11, 11] = np.inf
    info, want = check_select(eng, c)
    assert info['excluded'] == 3 and (info['round_of'][[5, 9, 11]] == 0).all() and np.isfinite(info['score']).all()
    assert np.isfinite([info[k] for k in STAT_FIELDS]).all()


def test_max_rounds_stops_after_the_first_removal(eng):
    full, _ = check_select(eng, thin_gram(65))
    one, _ = check_select(eng, thin_gram(65), max_rounds=1)
    assert full['rounds'] == 3 and one['rounds'] == 1 and 0 < one['removed'] < full['removed']
    assert (one['round_of'] <= 1).all()


def test_a_matrix_of_zeros_excludes_everybody(eng, torch):
    """include/byzagg.h: not refused; everybody is excluded, no round runs and the aggregate is the zero vector"""
    n, d = 9, 300
    info, want = check_select(eng, np.zeros((n, n)))
    assert info['excluded'] == n and info['kept'] == 0 and info['rounds'] == 0 and info['divisor'] == 0.0
    out, oinfo = eng.afa(on_gpu(torch, eng, np.zeros((n, d), dtype=np.float32)), return_info=True)
    assert oinfo['kept_rows'].size == 0 and oinfo['excluded_rows'].size == n and bool((out == 0).all())
    nan = np.full((n, d), np.nan, dtype=np.float32)
    out, oinfo = eng.afa(on_gpu(torch, eng, nan), return_info=True)
    assert oinfo['kept'] == 0 and bool((out == 0).all())


# ---- the refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(eng, torch):
    import ctypes
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    dev = 'cuda:%d' % eng.device
    n, d = 20, 64
    gt = on_gpu(torch, eng, planted(n, d, 'noise', 1)[0])
    gram = on_gpu(torch, eng, thin_gram(63)[:n, :n])
    flags = torch.full((n,), -7, dtype=torch.int32, device=dev)
    round_of = torch.full((n,), -9, dtype=torch.int32, device=dev)
    score = torch.full((n,), -5.0, dtype=torch.float64, device=dev)
    out = torch.full((d,), -3.0, dtype=torch.float32, device=dev)
    good = _native.AfaParams(2.0, 0.5, 0)

    def select(rows=n, params=good, gram_ptr=gram.data_ptr(), flags_ptr=flags.data_ptr()):
        return eng.lib.byz_afa_select_dev(eng.ctx, _vp(gram_ptr), rows, None, ctypes.byref(params) if params else None,
                                          _vp(flags_ptr), _vp(round_of.data_ptr()), _vp(score.data_ptr()), None)

    def whole(rows=n, params=good, out_ptr=out.data_ptr()):
        return eng.lib.byz_afa_dev(eng.ctx, _vp(gt.data_ptr()), rows, d, d, None, ctypes.byref(params) if params else None, None,
                                   _vp(out_ptr), _vp(flags.data_ptr()), _vp(round_of.data_ptr()), _vp(score.data_ptr()), None)
    assert select(rows=16385) == _native.E_UNSUPPORTED          # (the matrix is never read: refused on n alone)
    assert whole(rows=16385) == _native.E_UNSUPPORTED
    assert select(rows=1) == _native.E_INVALID and whole(rows=1) == _native.E_INVALID
    for bad in (_native.AfaParams(-1.0, 0.5, 0), _native.AfaParams(2.0, -0.5, 0), _native.AfaParams(float('nan'), 0.5, 0),
                _native.AfaParams(2.0, float('inf'), 0), _native.AfaParams(2.0, 0.5, -1), None):
        assert select(params=bad) == _native.E_INVALID and whole(params=bad) == _native.E_INVALID
    assert select(gram_ptr=None) == _native.E_INVALID and select(flags_ptr=None) == _native.E_INVALID
    assert whole(out_ptr=None) == _native.E_INVALID
    assert whole(out_ptr=gt.data_ptr() + 4 * (d - 1)) == _native.E_INVALID           # out overlaps G
    eng.synchronize()
    assert (flags == -7).all() and (round_of == -9).all() and (score == -5.0).all() and (out == -3.0).all()
    with pytest.raises(ValueError):
        eng.afa_select(thin_gram(63)[:1, :1])
    with pytest.raises(NotImplementedError):
        eng.afa_select(np.broadcast_to(np.zeros(1), (16385, 16385)))          # (refused on the shape: never uploaded)
    with pytest.raises(ValueError):
        eng.afa_select(thin_gram(63)[:5, :4])
    with pytest.raises(ValueError):
        eng.afa(gt, gram=thin_gram(63))                         # 63 rows of Gram, 20 of gradients


# ---- the whole call -----------------------------------------------------------------------------------------------------------
WHOLE = [(65, 2000, 'drift', 0), (130, 777, 'drift', 1), (65, 2000, 'flip', 1), (130, 777, 'flip', 0)]


@pytest.mark.parametrize('n,d,kind,seed', WHOLE)
def test_the_whole_call_on_a_padded_misaligned_view(eng, torch, n, d, kind, seed):
    g, f = planted(n, d, kind, seed)
    view, flat = views_arena.arena_variant(torch, g, 'odd_ld_odd_base', device='cuda:%d' % eng.device)
    before = flat.clone()
    out, info = eng.afa(view, return_info=True)
    views_arena.untouched(torch, flat, view, before)
    c_dev = eng.gram(view).cpu().numpy()
    # the device's decisions are the restatement's on the device's OWN Gram: exact, and the doubles as bits
    own = restated_afa_select(c_dev)
    assert np.array_equal(info['kept_rows'], np.flatnonzero(own['kept_flags']))
    same_decisions(info, own)
    same_bits(info, own)
    # and the restatement's on numpy's fp64 Gram: the margins of tests/test_afa.py against the Gram's error, measured here
    c_np = gram64(g)
    norm = np.sqrt(np.diagonal(c_np))
    err = (np.abs(c_dev - c_np) / (norm[:, None] * norm[None, :])).max()
    print('afa %s %dx%d: Gram error max |C_dev - C_np| / sqrt(C_ii C_jj) = %.3g' % (kind, n, d, err))
    assert err < 1e-3 / 100
    same_decisions(info, restated_afa_select(c_np))
    assert not own['kept_flags'][:f].any()                      # no attacker is kept
    # the aggregate: scaled_rows_sum of the same flags, as bits (unit weights: the divisor is the kept count)
    kept = own['kept_flags']
    assert info['divisor'] == float(kept.sum())
    mask = on_gpu(torch, eng, kept.astype(np.float64))
    count = torch.tensor([float(kept.sum())], dtype=torch.float64, device=view.device)
    assert torch.equal(out.view(torch.int32), eng.scaled_rows_sum(view, mask, count).view(torch.int32))
    ref = g[kept].astype(np.float64).mean(axis=0)
    assert np.allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-6)


def test_a_given_gram_skips_the_stage_and_gives_the_same_bits(eng, torch):
    n, d = 65, 2000
    g, f = planted(n, d, 'drift', 2)
    gt = on_gpu(torch, eng, g)
    a, ia = eng.afa(gt, return_info=True)
    gram = eng.gram(gt)
    b, ib = eng.afa(gt, gram=gram, return_info=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and np.array_equal(ia['round_of'], ib['round_of'])
    assert np.array_equal(bits64(ia['score']), bits64(ib['score']))
    # the two calls made by hand
    flags, info = eng.afa_select(gram, on_device=True, like=gt)
    assert flags.dtype == torch.int32 and flags.device == gt.device and info['round_of'].dtype == torch.int32
    by_hand = eng.scaled_rows_sum(gt, flags.to(torch.float64), flags.sum().to(torch.float64).reshape(1))
    assert torch.equal(a.view(torch.int32), by_hand.view(torch.int32))
    # weights: the divisor is their sum over the kept rows, in the stated order, and the aggregate scaled_rows_sum's with it
    w = np.random.default_rng(3).uniform(0.5, 2.0, n)
    c, ic = eng.afa(gt, weights=w, gram=gram, return_info=True)
    want = restated_afa_select(gram.cpu().numpy(), w)
    same_decisions(ic, want)
    same_bits(ic, want)
    by_hand = eng.scaled_rows_sum(gt, on_gpu(torch, eng, want['weights']),
                                  torch.tensor([want['divisor']], dtype=torch.float64, device=gt.device))
    assert torch.equal(c.view(torch.int32), by_hand.view(torch.int32))
    # the host entry point: numpy in -> numpy out
    h, ih = eng.afa(g, return_info=True)
    assert isinstance(h, np.ndarray) and np.array_equal(ih['round_of'], ia['round_of'])
    assert np.array_equal(views_arena.bits(h), views_arena.bits(a.cpu().numpy()))
    hg = eng.afa(g, weights=w, gram=gram.cpu().numpy())
    assert np.array_equal(views_arena.bits(hg), views_arena.bits(c.cpu().numpy()))


def test_two_runs_and_a_side_stream_give_the_same_outputs(eng, torch):
    n, d = 130, 777
    gt = on_gpu(torch, eng, planted(n, d, 'flip', 2)[0])
    a, ia = eng.afa(gt, return_info=True)
    b, ib = eng.afa(gt, return_info=True)
    side = torch.cuda.Stream(device=gt.device)
    side.wait_stream(torch.cuda.current_stream(gt.device))
    with torch.cuda.stream(side):
        s, is_ = eng.afa(gt, return_info=True)
    side.synchronize()
    for out, info in ((b, ib), (s, is_)):
        assert torch.equal(a.view(torch.int32), out.view(torch.int32))
        assert np.array_equal(ia['round_of'], info['round_of']) and np.array_equal(bits64(ia['score']), bits64(info['score']))
        assert all(bits64(ia[k]) == bits64(info[k]) for k in STAT_FIELDS) and all(ia[k] == info[k] for k in REPORT_FIELDS)
    assert ia['rounds'] >= 3                                     # (a case that updates twice)


# ---- the layers above ---------------------------------------------------------------------------------------------------------
def test_the_sharded_layout_at_world_size_one(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d = 65, 2000
    g, f = planted(n, d, 'drift', 0)
    gt = on_gpu(torch, eng, g)
    want, winfo = eng.afa(gt, return_info=True)
    out, info = ShardedAggregator(HipKernels(eng)).afa(gt, n, f, return_info=True)
    assert np.array_equal(info['kept_rows'], winfo['kept_rows']) and torch.equal(out.view(torch.int32), want.view(torch.int32))
    w = np.random.default_rng(4).uniform(0.5, 2.0, n)
    want, winfo = eng.afa(gt, weights=w, return_info=True)
    out, info = ShardedAggregator(HipKernels(eng)).afa(gt, weights=w, return_info=True)
    assert np.array_equal(info['kept_rows'], winfo['kept_rows']) and torch.equal(out.view(torch.int32), want.view(torch.int32))


def test_defences_afa_and_as_the_rule_of_a_pre_aggregation(eng, torch):
    from attacking_federate_learning_amd import defences
    n, d = 65, 2000
    g, f = planted(n, d, 'drift', 1)
    gt = on_gpu(torch, eng, g)
    want = eng.afa(gt)
    assert torch.equal(defences.afa(gt, n, f).view(torch.int32), want.view(torch.int32))
    host = defences.afa(g, n, f)
    assert isinstance(host, np.ndarray) and np.array_equal(views_arena.bits(host), views_arena.bits(want.cpu().numpy()))
    mixed = defences.nnm(gt, n, f, then=defences.afa)
    assert mixed.shape == (d,) and bool(torch.isfinite(mixed).all())
    assert torch.equal(mixed.view(torch.int32), eng.afa(defences.nnm(gt, n, f)).view(torch.int32))
    for pre, kwargs in ((defences.bucketing, dict(s=2)), (defences.robust_lr, {}), (defences.sparsefed, dict(k=100)),
                        (defences.weak_dp, {})):
        got = pre(gt, n, f, then=defences.afa, **kwargs)
        assert got.shape == (d,) and bool(torch.isfinite(got).all()), pre.__name__


def test_the_server_keeps_the_reputations_across_rounds(eng, torch):
    """three rounds with the same attackers (the drift attack on the first f rows, new honest gradients every round): their beta
    grows by one a round and their weight falls 1/2 -> 3/7 -> 3/8 -> 3/9; an honest client's counts move by one a round"""
    from attacking_federate_learning_amd.defences import AfaReputation
    from attacking_federate_learning_amd.server import DeviceServer
    n, d = 65, 2000
    f = n // 5
    server = DeviceServer(n, np.zeros(d, dtype=np.float32), f / n, 0.1, 0.9, torch_device='cuda:%d' % eng.device, engine=eng)
    assert server.afa_reputation is None
    host = AfaReputation(n)                                     # the same three rounds by the restatement on numpy's Gram
    for rnd in range(1, 4):
        g, _ = planted(n, d, 'drift', 10 + rnd)
        want = restated_afa_select(gram64(g), host.weights())
        assert want['margin_thr'] > 1e-3 and want['margin_side'] > 1e-3
        host.update(np.flatnonzero(want['kept_flags']), np.flatnonzero(want['round_of'] == 0))
        server.users_grads.data.copy_(on_gpu(torch, eng, g))
        step = server.defend_afa()
        rep = server.afa_reputation
        assert step.shape == (d,) and bool(torch.isfinite(step).all())
        assert rep.alpha[:f].tolist() == [3] * f and rep.beta[:f].tolist() == [3 + rnd] * f
        assert np.array_equal(rep.weights()[:f], np.full(f, 3 / (6 + rnd)))
        assert np.array_equal(rep.alpha, host.alpha) and np.array_equal(rep.beta, host.beta)
        assert ((rep.alpha[f:] + rep.beta[f:]) == 6 + rnd).all()
    assert not rep.blocked.any()
    stateless = server.defend_afa(reputation=False)
    assert rep.beta[:f].tolist() == [6] * f and stateless.shape == (d,)       # (no reputation asked for: none touched)
