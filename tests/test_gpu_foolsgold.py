"""FoolsGold on the device against tests/foolsgold_rule.py's restatement of include/byzagg.h's rule.  On a given Gram the integers
(flags, counts) are equal and the doubles m, a, top and the rescaled w are equal AS BITS -- fp64 sqrt, /, *, - and max are correctly
rounded on both sides -- at every wave, workgroup and owner-slot edge.  The final weight l is held within kappa * 4 * 2^-53: the
device's log and numpy's are each within 1 ulp, not equal (two log errors of at most 2^-54 each on |log| < 0.5, two roundings of the
sum below 1); a weight within that bound of 0 or 1 may sit on either side of the clip, which the same bound covers.  rows_add is
numpy's float32 += as bits; the whole call is held to the device's own Gram of the device's own history, and its aggregate to
byz_scaled_rows_sum_dev's bits."""
import numpy as np
import pytest

from tests import views_arena
from tests.foolsgold_rule import (LOGIT_BOUND, PLANTED_HONEST, graded_gram, history_chain, planted_rounds, restated_foolsgold_weights,
                                  with_edge_cases)

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 63, 64, 65, 257, 1000, 1023, 1024, 1025, 4097]       # the wave, workgroup and owner-slot edges
COUNTS = ('usable', 'excluded', 'at_zero', 'at_one', 'degenerate')


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:%d' % eng.device)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def sequential_sum(values):
    total = 0.0
    for x in np.asarray(values, dtype=np.float64).tolist():
        total = total + x
    return total


def check_weights(eng, c, kappa=1.0):
    """foolsgold_weights on a host-made Gram against the restatement; returns the worst |l_dev - l_ref| / kappa"""
    weights, info = eng.foolsgold_weights(c, kappa=kappa)
    want = restated_foolsgold_weights(c, kappa)
    assert np.array_equal(info['usable_flags'], want['usable'].astype(np.int32))
    for key in ('maxcs', 'alpha', 'rescaled'):
        assert np.array_equal(bits64(info[key]), bits64(want[key])), (key, np.flatnonzero(bits64(info[key]) != bits64(want[key]))[:8])
    assert bits64(info['top']) == bits64(want['top']) and info['divisor'] == want['divisor'] == float(want['usable_rows'])
    assert (info['usable'], info['excluded'], info['degenerate']) == (want['usable_rows'], want['excluded_rows'], want['degenerate'])
    worst = float(np.abs(weights - want['weights']).max())
    assert worst <= kappa * LOGIT_BOUND, worst
    # the counts are the device's own weights'; they are the restatement's too unless a weight sits within the bound of a clip
    live = want['usable']
    assert (info['at_zero'], info['at_one']) == (int((weights[live] == 0.0).sum()), int((weights[live] == 1.0).sum()))
    edge = np.minimum(np.abs(want['weights']), np.abs(1.0 - want['weights']))
    if not ((edge > 0) & (edge <= kappa * LOGIT_BOUND)).any():
        assert (info['at_zero'], info['at_one']) == (want['at_zero'], want['at_one'])
    return worst / kappa


# ---- the weights on a given Gram ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_weights_equal_the_restatement(eng, n):
    worst = check_weights(eng, graded_gram(n, 8 if n <= 257 else 12, 0))
    print('foolsgold_weights n = %d: worst |l_dev - l_ref| = %.3g = %.2f x 2^-53' % (n, worst, worst * 2.0 ** 53))


@pytest.mark.parametrize('n', [65, 1025])
def test_the_planted_edge_cases(eng, n):
    c = with_edge_cases(graded_gram(n, 8 if n <= 257 else 12, 0))
    check_weights(eng, c)
    check_weights(eng, c, kappa=2.0)


def test_small_and_degenerate_grams(eng):
    for c in (np.array([[4.0]]), np.array([[np.nan]]), np.array([[1.0, 0.0], [0.0, 4.0]]), np.array([[1.0, 2.0], [2.0, 4.0]]),
              np.array([[1.0, 2.0], [2.0, -4.0]])):
        check_weights(eng, c)
    x = np.tile(np.random.default_rng(0).normal(size=8).astype(np.float32), (70, 1)).astype(np.float64)
    weights, info = eng.foolsgold_weights(x @ x.T)
    assert info['degenerate'] and not weights.any() and info['at_zero'] == 70 and info['top'] == 0.0     # zeros, not NaN
    c = graded_gram(64, 8, 1)
    c[5, 7] = c[7, 5] = np.inf
    check_weights(eng, c)


def test_weights_on_the_device_and_the_refusals(eng, torch):
    c = graded_gram(257, 8, 3)
    host, info = eng.foolsgold_weights(c)
    ct = on_gpu(torch, eng, c)
    dev, dinfo = eng.foolsgold_weights(ct, on_device=True, like=ct)
    assert dev.dtype == torch.float64 and dev.device == ct.device and dinfo['maxcs'].device == ct.device
    assert np.array_equal(bits64(dev.cpu().numpy()), bits64(host))
    assert np.array_equal(bits64(dinfo['alpha'].cpu().numpy()), bits64(info['alpha']))
    from attacking_federate_learning_amd.sharded import HipKernels
    again, ainfo = HipKernels(eng).foolsgold_weights(ct, ct, normalise='sum')
    assert torch.equal(again.view(torch.int64), dev.view(torch.int64)) and bits64(ainfo['divisor']) == bits64(sequential_sum(host))
    with pytest.raises(ValueError):
        eng.foolsgold_weights(c[:5])
    with pytest.raises(ValueError):
        eng.foolsgold_weights(c, kappa=0.0)


# ---- the history update ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w', [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1027])
def test_rows_add_is_numpys_float32_sum(eng, torch, w):
    n, guard = 3, 8
    rng = np.random.default_rng(w)
    device = 'cuda:%d' % eng.device
    for h_off in (0, 1):
        for col_start in (0, 1, 2, 3):
            for h_pad in (0, 1, 4):
                for g_pad in (0, 1, 4):
                    d = col_start + w + 2
                    ld_h, ld_g = w + h_pad, d + g_pad
                    h0 = rng.standard_normal((n, w)).astype(np.float32)
                    g = (rng.standard_normal((n, d)) * 3).astype(np.float32)
                    flat = torch.full((guard + h_off + n * ld_h + guard,), float('nan'), dtype=torch.float32, device=device)
                    view = flat.as_strided((n, w), (ld_h, 1), guard + h_off)
                    view.copy_(torch.from_numpy(h0))
                    gflat = torch.zeros(n * ld_g, dtype=torch.float32, device=device)
                    gview = gflat.as_strided((n, d), (ld_g, 1), 0)
                    gview.copy_(torch.from_numpy(g))
                    before, gbefore = flat.clone(), gflat.clone()
                    assert eng.rows_add(view, gview, columns=(col_start, col_start + w)) is view
                    want = h0.copy()
                    want += g[:, col_start:col_start + w]
                    case = (h_off, col_start, h_pad, g_pad)
                    assert views_arena.same_bits(view.cpu().numpy(), want), case
                    views_arena.untouched(torch, flat, view, before)                    # the NaN guard bands and the padding
                    assert torch.equal(gflat.view(torch.int32), gbefore.view(torch.int32)), case


def test_rows_add_refusals_and_a_device_buffer(eng, torch):
    g = views_arena.gaussian(5, 4, 20)
    h = eng.empty((4, 6), np.float32).upload(np.ones((4, 6), dtype=np.float32))
    eng.rows_add(h, on_gpu(torch, eng, g), columns=(7, 13))
    assert views_arena.same_bits(h.numpy(), np.ones((4, 6), dtype=np.float32) + g[:, 7:13])
    eng.rows_add(h, g, columns=(0, 6))                                                  # a host matrix is staged
    assert views_arena.same_bits(h.numpy(), np.ones((4, 6), dtype=np.float32) + g[:, 7:13] + g[:, :6])
    with pytest.raises(ValueError):
        eng.rows_add(h, g, columns=(0, 7))
    with pytest.raises(ValueError):
        eng.rows_add(np.zeros((4, 6), dtype=np.float32), g, columns=(0, 6))
    with pytest.raises(ValueError):
        eng.rows_add(h, g, columns=(15, 21))


# ---- the whole call -------------------------------------------------------------------------------------------------------------
def whole_rounds(n, d, seed):
    """three rounds with a sybil group in the last n // 8 rows, so that the weights differ"""
    rng = np.random.default_rng(seed)
    centre, shared = rng.normal(size=(n, d)), rng.normal(size=d)
    f = n // 8
    out = []
    for _ in range(3):
        g = centre + rng.normal(size=(n, d))
        g[n - f:] = shared + 0.3 * rng.normal(size=(f, d))
        out.append(g.astype(np.float32))
    return out


@pytest.mark.parametrize('layout', ['contiguous', 'odd_ld_odd_base'])
@pytest.mark.parametrize('window', ['whole', 'interior'])
@pytest.mark.parametrize('with_history', [True, False])
@pytest.mark.parametrize('n,d', [(65, 1031), (257, 515)])
def test_the_whole_call(eng, torch, n, d, with_history, window, layout):
    device = 'cuda:%d' % eng.device
    columns = None if window == 'whole' else (3, d - 6)
    a, b = (0, d) if columns is None else columns
    history = torch.zeros((n, b - a), dtype=torch.float32, device=device) if with_history else None
    chain = np.zeros((n, b - a), dtype=np.float32)
    for rnd, g in enumerate(whole_rounds(n, d, n + d)):
        normalise = 'sum' if rnd == 1 else 'count'
        if layout == 'contiguous':
            view, flat = on_gpu(torch, eng, g), None
        else:
            view, flat = views_arena.arena_variant(torch, g, layout, device=device)
            before = flat.clone()
        out, info = eng.foolsgold(view, n, 0, history=history, columns=columns, normalise=normalise, return_info=True)
        if flat is not None:
            views_arena.untouched(torch, flat, view, before)
        previous = chain.copy()
        chain += g[:, a:b]
        if with_history:
            assert views_arena.same_bits(history.cpu().numpy(), chain)                   # the numpy += chain
        # the weights: foolsgold_weights of the device's own Gram of the device's own history (or window), as bits
        gram = eng.gram(history if with_history else view[:, a:b])
        weights, winfo = eng.foolsgold_weights(gram, on_device=True, like=view)
        assert np.array_equal(bits64(info['weights']), bits64(weights.cpu().numpy()))
        assert all(info[k] == winfo[k] for k in COUNTS) and bits64(info['top']) == bits64(winfo['top'])
        lw = info['weights']
        assert ((lw > 0) & (lw < 1)).any() or ((lw == 0).any() and (lw == 1).any())
        # T, and the aggregate: scaled_rows_sum of those weights and T, as bits
        total = float(n) if normalise == 'count' else sequential_sum(lw)
        assert bits64(info['divisor']) == bits64(total)
        by_hand = eng.scaled_rows_sum(view, weights, torch.tensor([total], dtype=torch.float64, device=device))
        assert torch.equal(out.view(torch.int32), by_hand.view(torch.int32))
        ref = (lw[:, None] * g.astype(np.float64)).sum(axis=0) / total
        assert np.allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-6)
        # a given Gram replaces the stage (the history is still added to: undo that once to compare)
        if rnd == 2:
            if with_history:
                history.copy_(on_gpu(torch, eng, previous))
            again = eng.foolsgold(view, history=history, columns=columns, normalise=normalise, gram=gram)
            assert torch.equal(out.view(torch.int32), again.view(torch.int32))
            assert not with_history or views_arena.same_bits(history.cpu().numpy(), chain)


def test_a_second_run_and_the_host_entry_point_give_the_same_bits(eng, torch):
    n, d = 65, 1031
    g = whole_rounds(n, d, 7)[0]
    gt = on_gpu(torch, eng, g)
    a, ia = eng.foolsgold(gt, columns=(3, 900), kappa=2.0, normalise='sum', return_info=True)
    b, ib = eng.foolsgold(gt, columns=(3, 900), kappa=2.0, normalise='sum', return_info=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and np.array_equal(bits64(ia['weights']), bits64(ib['weights']))
    assert bits64(ia['divisor']) == bits64(ib['divisor']) and a.device == gt.device
    h, ih = eng.foolsgold(g, columns=(3, 900), kappa=2.0, normalise='sum', return_info=True)      # host in -> host out
    assert isinstance(h, np.ndarray) and views_arena.same_bits(h, a.cpu().numpy())
    assert np.array_equal(bits64(ih['weights']), bits64(ia['weights']))
    with pytest.raises(ValueError):
        eng.foolsgold(g, history=torch.zeros((n, d), dtype=torch.float32, device=gt.device))    # a history needs a device matrix
    with pytest.raises(ValueError):
        eng.foolsgold(gt, history=torch.zeros((n, d - 1), dtype=torch.float32, device=gt.device))
    with pytest.raises(ValueError):
        eng.foolsgold(gt, columns=(5, d + 1))
    with pytest.raises(ValueError):
        eng.foolsgold(gt, gram=np.eye(n - 1))


# ---- the layers above -----------------------------------------------------------------------------------------------------------
def test_planted_sybils_through_defences_and_the_server(eng, torch):
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.server import DeviceServer
    rounds = planted_rounds(0)
    n, d = rounds[0].shape
    history = defences.FoolsGoldHistory(n, d)
    assert history.rounds == 0 and history.columns is None and not history.numpy().any()
    server = DeviceServer(n, np.zeros(d, dtype=np.float32), 6 / n, 0.1, 0.9, torch_device='cuda:%d' % eng.device, engine=eng)
    assert server.foolsgold_history is None
    chain = history_chain(rounds)
    for rnd, g in enumerate(rounds):
        gt = on_gpu(torch, eng, g)
        out, info = defences.foolsgold(gt, n, 6, history=history, return_info=True)
        assert (info['weights'][PLANTED_HONEST:] == 0.0).all() and (info['weights'][:PLANTED_HONEST] == 1.0).all()
        assert (info['at_zero'], info['at_one'], info['divisor']) == (6, PLANTED_HONEST, float(n))
        assert history.rounds == rnd + 1 and history.columns == (0, d) and views_arena.same_bits(history.numpy(), chain[rnd])
        honest_sum = torch.zeros(n, dtype=torch.float64, device=gt.device)
        honest_sum[:PLANTED_HONEST] = 1.0
        want = eng.scaled_rows_sum(gt, honest_sum, torch.tensor([float(n)], dtype=torch.float64, device=gt.device))
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
        server.users_grads.data.copy_(gt)
        step = server.defend_foolsgold()
        assert torch.equal(step.view(torch.int32), want.view(torch.int32))
        assert server.foolsgold_history.rounds == rnd + 1
        assert views_arena.same_bits(server.foolsgold_history.numpy(), chain[rnd])
    host = defences.FoolsGoldHistory(n, d)                       # numpy in -> numpy out, the history still on the device
    got = defences.foolsgold(rounds[0], n, 6, history=host)
    assert isinstance(got, np.ndarray) and host.rounds == 1 and views_arena.same_bits(host.numpy(), chain[0])
    history.reset()
    assert history.rounds == 0 and not history.numpy().any()
    stateless = server.defend_foolsgold(history=False)
    assert stateless.shape == (d,) and server.foolsgold_history.rounds == len(rounds)
    with pytest.raises(ValueError):
        defences.foolsgold(on_gpu(torch, eng, rounds[0]), n, 6, history=host, columns=(0, d - 1))


def test_as_the_rule_of_bucketing(eng, torch):
    from attacking_federate_learning_amd import defences
    n, d = 65, 515
    g = whole_rounds(n, d, 3)[0]
    gt = on_gpu(torch, eng, g)
    want = eng.foolsgold(gt)
    assert torch.equal(defences.foolsgold(gt, n, 8).view(torch.int32), want.view(torch.int32))
    host = defences.foolsgold(g, n, 8)
    assert isinstance(host, np.ndarray) and views_arena.same_bits(host, want.cpu().numpy())
    got = defences.bucketing(gt, n, 8, s=2, then=defences.foolsgold)
    assert got.shape == (d,) and bool(torch.isfinite(got).all())
    assert torch.equal(got.view(torch.int32), eng.foolsgold(defences.bucketing(gt, n, 8, s=2)).view(torch.int32))


def test_the_sharded_layout_at_world_size_one(eng, torch):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d = 65, 1031
    rounds = whole_rounds(n, d, 11)
    agg = ShardedAggregator(HipKernels(eng))
    device = 'cuda:%d' % eng.device
    for columns in (None, (3, 900)):
        a, b = (0, d) if columns is None else columns
        mine = torch.zeros((n, b - a), dtype=torch.float32, device=device)
        single = torch.zeros((n, b - a), dtype=torch.float32, device=device)
        for rnd, g in enumerate(rounds):
            gt = on_gpu(torch, eng, g)
            normalise = 'sum' if rnd == 1 else 'count'
            want, winfo = eng.foolsgold(gt, history=single, columns=columns, normalise=normalise, return_info=True)
            out, info = agg.foolsgold(gt, n, 8, history=mine, columns=columns, normalise=normalise, return_info=True)
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and torch.equal(mine.view(torch.int32), single.view(torch.int32))
            assert np.array_equal(bits64(info['weights']), bits64(winfo['weights'])) and bits64(info['divisor']) == bits64(winfo['divisor'])
    stateless = agg.foolsgold(on_gpu(torch, eng, rounds[0]), columns=(3, 900))
    assert torch.equal(stateless.view(torch.int32), eng.foolsgold(on_gpu(torch, eng, rounds[0]), columns=(3, 900)).view(torch.int32))
    # a slice the window misses contributes a zero Gram: every row is a zero-history row, every weight 1, the mean
    missed = agg.foolsgold(on_gpu(torch, eng, rounds[0]), columns=(0, 10), column_offset=20, total_columns=d + 20)
    assert np.allclose(missed.cpu().numpy(), rounds[0].astype(np.float64).mean(axis=0), rtol=1e-5, atol=1e-6)
