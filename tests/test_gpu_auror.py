"""Auror on the device against tests/test_auror.py's restatement of include/byzagg.h's rule.

Integers (votes, bad flags, counts, kept flags) are compared exactly.  The device sums in its own order, and a sum of m fp32
values in fp64 is within m * 2^-53 * max|x| of exact in any order: the seeded inputs are ones for which every decision of the
restatement (min |x - t| over every sweep, min |gap - alpha|) has a margin above margin_bound = n * 2^-51 * max|x|, which each
test asserts before it compares, and `gap` is compared within that bound.  Quarter-integer data (k / 4, |k| <= 8) makes every
sum exact and puts values exactly on the thresholds: there everything, `gap` included, is compared as bits.

Heights at every edge of column_select.hpp's geometries, widths either side of a 16- and a 64-column tile and widths that give
a workgroup several tiles; misaligned, strided, guard-banded views; a side stream; accumulate; the aggregate as
scaled_rows_sum's bits; the columns layout looped over two shards."""
import functools

import numpy as np
import pytest

from tests import views_arena
from tests.test_auror import (margin_bound, planted_case, quarter_case, restated_auror, restated_auror_select,
                              restated_auror_votes)

pytestmark = pytest.mark.gpu

HEIGHTS = [1, 2, 3, 255, 256, 257, 1024, 1025, 2304, 2305, 4096, 4097, 16384]
WIDTHS = [1, 15, 17, 63, 65, 1025]


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:%d' % eng.device)


def host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else (x.numpy() if hasattr(x, 'numpy') else np.asarray(x))


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def mixed_case(n, d, seed=0):
    """0.1 x normals with planted attackers (n // 5 rows, +0.5 on a tenth of the columns, at least one)"""
    rng = np.random.default_rng(1000 * n + d + seed)
    g = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    if n >= 5:
        rows = rng.choice(n, n // 5, replace=False)
        cols = rng.choice(d, max(d // 10, 1), replace=False)
        g[np.ix_(rows, cols)] += np.float32(0.5)
    return g


@functools.lru_cache(maxsize=None)
def wanted(n, d, alpha, max_iter=32, seed=0):
    return restated_auror_votes(mixed_case(n, d, seed), alpha, max_iter)


def check_votes(eng, torch, g, alpha, max_iter=32, want=None, exact=False, gt=None):
    want = restated_auror_votes(g, alpha, max_iter) if want is None else want
    bound = margin_bound(g)
    print('auror %dx%d alpha %g: margins %.3g (t) %.3g (alpha) against %.3g; sweeps up to %d' % (
        g.shape[0], g.shape[1], alpha, want['margin_t'], want['margin_alpha'], bound, want['sweeps'].max(initial=0)))
    if not exact:
        assert min(want['margin_t'], want['margin_alpha']) > bound          # the condition under which the orders may differ
    gt = on_gpu(torch, eng, g) if gt is None else gt
    votes, bad, counts, gap = eng.auror_votes(gt, alpha, max_iter=max_iter, return_gap=True)
    votes, bad, counts, gap = host(votes), host(bad), host(counts), host(gap)
    assert votes.dtype == np.int64 and bad.dtype == np.int32 and counts.dtype == np.int64 and gap.dtype == np.float64
    assert np.array_equal(counts, want['counts']), (counts, want['counts'])
    assert np.array_equal(bad, want['bad'])
    assert np.array_equal(votes, want['votes']), np.flatnonzero(votes != want['votes'])[:8]
    if exact:
        assert np.array_equal(gap.view(np.int64), want['gap'].view(np.int64))
    else:
        assert (np.abs(gap - want['gap']) <= bound).all()
    return want


# ---- the votes at every geometry edge ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', HEIGHTS)
def test_votes_at_every_height(eng, torch, n):
    d = 70                                                       # two 64-column tiles, five 16-column ones, both ragged
    for alpha in (0.3, 0.12):                                    # the planted columns alone; every Gaussian column as well
        want = check_votes(eng, torch, mixed_case(n, d), alpha, want=wanted(n, d, alpha))
    if n >= 255:
        assert want['counts'][0] == d and want['votes'].max() > d // 4


@pytest.mark.parametrize('d', WIDTHS)
@pytest.mark.parametrize('n', [100, 300])                        # 64-column tiles; 16-column tiles
def test_votes_at_every_width(eng, torch, n, d):
    check_votes(eng, torch, mixed_case(n, d), 0.12, want=wanted(n, d, 0.12))


@pytest.mark.parametrize('n,d', [(64, 16500), (300, 4200)])
def test_a_workgroup_walks_several_tiles(eng, torch, n, d):
    """more tiles than workgroups (one a CU, 256 of them): 258 tiles of 64 columns, 263 of 16"""
    g = mixed_case(n, d)
    want = check_votes(eng, torch, g, 0.3, want=wanted(n, d, 0.3))
    assert want['counts'][0] >= d // 10


@pytest.mark.parametrize('n', [3, 257, 1025, 4097])
def test_quarter_integers_are_compared_as_bits(eng, torch, n):
    g = quarter_case(n, 130, seed=n)
    g[:, 14] = np.float32(1e-45) * (1 + np.arange(n) % 3)        # denormals: whole multiples of 2^-149, their sums exact too
    for alpha in (0.0, 1.0, 2.25):
        want = check_votes(eng, torch, g, alpha, exact=True)
    assert want['margin_t'] == 0.0                               # values did land on a threshold


@pytest.mark.parametrize('max_iter', [1, 2, 3])
def test_the_cap(eng, torch, max_iter):
    n, d = 300, 130
    want = check_votes(eng, torch, mixed_case(n, d), 0.12, max_iter=max_iter, want=wanted(n, d, 0.12, max_iter))
    full = wanted(n, d, 0.12)
    assert want['counts'][2] == int((full['sweeps'] > max_iter).sum()) > 0


def test_non_finite_values_constant_and_empty_columns(eng, torch):
    n, d = 300, 70
    g = mixed_case(n, d).copy()
    g[5, 3], g[17, 3], g[299, 69], g[0, 0] = np.nan, np.inf, -np.inf, np.nan
    g[:, 10] = np.float32(0.25)                                  # constant
    g[:, 11] = np.where(np.arange(n) % 2 == 0, np.float32(-0.0), np.float32(0.0))      # -0 against +0: constant
    g[:, 12] = np.nan                                            # nobody takes part: every row is bad
    g[1:, 13] = np.inf                                           # m = 1
    want = check_votes(eng, torch, g, 0.12)
    assert want['bad'].all() and want['counts'][1] == d - 4
    h = mixed_case(n, d).copy()
    h[5, 3], h[17, 40] = np.nan, -np.inf
    want = check_votes(eng, torch, h, 0.12)
    assert np.flatnonzero(want['bad']).tolist() == [5, 17]


# ---- views, streams, accumulate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', views_arena.VARIANTS)
@pytest.mark.parametrize('n', [100, 300, 4100])
def test_votes_on_misaligned_strided_guard_banded_views(eng, torch, n, variant):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    import ctypes
    d = 70
    g = mixed_case(n, d)
    want = wanted(n, d, 0.12)
    dev = 'cuda:%d' % eng.device
    view, flat = views_arena.arena_variant(torch, g, variant, device=dev)
    before = flat.clone()
    check_votes(eng, torch, g, 0.12, want=want, gt=view)
    views_arena.untouched(torch, flat, view, before)
    # the outputs inside guard bands of their own, through the library itself
    guard = 64
    v = torch.full((n + 2 * guard,), -7, dtype=torch.int64, device=dev)
    b = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device=dev)
    k = torch.full((4 + 2 * guard,), -7, dtype=torch.int64, device=dev)
    gap = torch.full((d + 2 * guard,), -7.0, dtype=torch.float64, device=dev)
    params = _native.AurorParams(0.12, 0.5, 32, 0)
    rc = eng.lib.byz_auror_votes_dev(eng.ctx, _vp(view.data_ptr()), n, d, view.stride(0), ctypes.byref(params),
                                     _vp(v[guard:].data_ptr()), _vp(b[guard:].data_ptr()), _vp(k[guard:].data_ptr()),
                                     _vp(gap[guard:].data_ptr()), None)
    assert rc == _native.OK
    eng.synchronize()
    assert np.array_equal(host(v[guard:guard + n]), want['votes']) and np.array_equal(host(k[guard:guard + 4]), want['counts'])
    assert np.array_equal(host(b[guard:guard + n]), want['bad'])
    for t, size in ((v, n), (b, n), (k, 4), (gap, d)):
        assert bool((t[:guard] == -7).all()) and bool((t[guard + size:] == -7).all())
    views_arena.untouched(torch, flat, view, before)


def test_a_side_stream_and_the_host_entry_point(eng, torch):
    n, d = 300, 130
    g = mixed_case(n, d)
    gt = on_gpu(torch, eng, g)
    a, ia = eng.auror(gt, alpha=0.12, return_info=True)
    side = torch.cuda.Stream(device=gt.device)
    side.wait_stream(torch.cuda.current_stream(gt.device))
    with torch.cuda.stream(side):
        s, is_ = eng.auror(gt, alpha=0.12, return_info=True)
        check_votes(eng, torch, g, 0.12, want=wanted(n, d, 0.12), gt=gt)
    side.synchronize()
    assert np.array_equal(is_['votes'], ia['votes']) and torch.equal(a.view(torch.int32), s.view(torch.int32))
    h, ih = eng.auror(g, alpha=0.12, return_info=True)
    assert isinstance(h, np.ndarray) and np.array_equal(ih['votes'], ia['votes']) and np.array_equal(ih['counts'], ia['counts'])
    assert np.array_equal(ih['kept_rows'], ia['kept_rows']) and np.array_equal(bits32(h), bits32(host(a)))
    assert np.array_equal(ih['gap'].view(np.int64), ia['gap'].view(np.int64))


def test_accumulate_adds_and_overwrite_overwrites(eng, torch):
    n, d = 300, 70
    a, b = mixed_case(n, d, seed=1).copy(), mixed_case(n, d, seed=2).copy()
    b[7, 7] = np.nan
    wa, wb = restated_auror_votes(a, 0.12), restated_auror_votes(b, 0.12)
    for w, g in ((wa, a), (wb, b)):
        assert min(w['margin_t'], w['margin_alpha']) > margin_bound(g)
    ta, tb = on_gpu(torch, eng, a), on_gpu(torch, eng, b)
    votes, bad, counts = eng.auror_votes(ta, 0.12)
    eng.auror_votes(tb, 0.12, votes=votes, bad=bad, counts=counts)             # in place
    assert np.array_equal(host(votes), wa['votes'] + wb['votes']) and np.array_equal(host(counts), wa['counts'] + wb['counts'])
    assert np.array_equal(host(bad), np.maximum(wa['bad'], wb['bad']))
    eng.auror_votes(ta, 0.12, votes=votes, bad=bad, counts=counts)             # a flag that is set stays set
    assert host(bad)[7] == 1 and np.array_equal(host(votes), 2 * wa['votes'] + wb['votes'])
    fresh = eng.auror_votes(ta, 0.12)
    assert np.array_equal(host(fresh[0]), wa['votes']) and not host(fresh[1]).any()
    with pytest.raises(ValueError):
        eng.auror_votes(ta, 0.12, votes=votes)                                 # all three or none


# ---- the selection and the aggregate ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', [(100, 4000), (1000, 2000), (4097, 500)])
def test_planted_attackers_on_the_device(eng, torch, n, d):
    g, attackers, columns = planted_case(n, d, 0)
    ref, kept, want = restated_auror(g, 0.3, 0.5)
    assert min(want['margin_t'], want['margin_alpha']) > margin_bound(g)
    gt = on_gpu(torch, eng, g)
    out, info = eng.auror(gt, n, n // 5, alpha=0.3, tau=0.5, return_info=True)
    assert np.array_equal(info['kept_rows'], np.flatnonzero(kept)) and np.array_equal(np.flatnonzero(~kept), attackers)
    assert np.array_equal(info['votes'], want['votes']) and np.array_equal(info['counts'], want['counts'])
    assert info['indicative'] == columns.size and info['removed'] == attackers.size and info['kept'] == n - attackers.size
    assert info['bad_rows'] == 0 and info['capped_cols'] == 0
    # the aggregate: scaled_rows_sum's bits with the flags as weights and the kept count as the divisor
    mask = on_gpu(torch, eng, kept.astype(np.float64))
    count = torch.tensor([float(kept.sum())], dtype=torch.float64, device=gt.device)
    assert torch.equal(out.view(torch.int32), eng.scaled_rows_sum(gt, mask, count).view(torch.int32))
    err = np.abs(host(out).astype(np.float64) - ref)
    assert (err <= 2.0 ** -23 * np.abs(ref) + 1e-30).all()


def test_select_tau_and_the_pieces_by_hand(eng, torch):
    n, d = 300, 130
    g = mixed_case(n, d)
    gt = on_gpu(torch, eng, g)
    want = wanted(n, d, 0.12)
    votes, bad, counts = eng.auror_votes(gt, 0.12)
    for tau in (0.0, 0.3, 0.5, 1.0):
        rows, info = eng.auror_select(votes, bad, counts, tau=tau)
        kept = restated_auror_select(want['votes'], want['bad'], want['counts'], tau)
        assert np.array_equal(rows, np.flatnonzero(kept)), tau
        assert info == dict(indicative=int(want['counts'][0]), removed=int((~kept).sum()), kept=int(kept.sum()), bad_rows=0,
                            capped_cols=int(want['counts'][2]))
        flags, _ = eng.auror_select(votes, bad, counts, tau=tau, on_device=True, like=gt)
        by_hand = eng.scaled_rows_sum(gt, flags.to(torch.float64), flags.sum().to(torch.float64).reshape(1))
        whole = eng.auror(gt, alpha=0.12, tau=tau)
        assert torch.equal(whole.view(torch.int32), by_hand.view(torch.int32))
    assert eng.auror_select(votes, bad, counts, tau=1.0)[0].size == n          # tau = 1: nobody goes for votes
    # no indicative column: nobody is removed for votes, whatever tau
    v0, b0, c0 = eng.auror_votes(gt, 5.0)
    assert host(c0)[0] == 0 and eng.auror_select(v0, b0, c0, tau=0.0)[0].size == n


def test_nobody_kept_gives_the_zero_vector(eng, torch):
    g = mixed_case(30, 70).copy()
    g[:, 5] = np.nan
    out, info = eng.auror(on_gpu(torch, eng, g), alpha=0.3, return_info=True)
    assert info['kept'] == 0 and info['removed'] == 30 and info['bad_rows'] == 30 and info['kept_rows'].size == 0
    assert bool((out == 0).all())


def test_refusals_write_nothing(eng, torch):
    import ctypes
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    dev = 'cuda:%d' % eng.device
    n, d = 20, 64
    gt = on_gpu(torch, eng, mixed_case(n, d))
    votes = torch.full((n,), -7, dtype=torch.int64, device=dev)
    bad = torch.full((n,), -7, dtype=torch.int32, device=dev)
    counts = torch.full((4,), -7, dtype=torch.int64, device=dev)
    kept = torch.full((n,), -7, dtype=torch.int32, device=dev)
    out = torch.full((d,), -3.0, dtype=torch.float32, device=dev)

    def votes_call(rows=n, alpha=0.3, tau=0.5, cap=32, acc=0, votes_ptr=votes.data_ptr()):
        p = _native.AurorParams(alpha, tau, cap, acc)
        return eng.lib.byz_auror_votes_dev(eng.ctx, _vp(gt.data_ptr()), rows, d, d, ctypes.byref(p), _vp(votes_ptr),
                                           _vp(bad.data_ptr()), _vp(counts.data_ptr()), None, None)

    def select_call(rows=n, tau=0.5, kept_ptr=kept.data_ptr()):
        p = _native.AurorParams(0.3, tau, 32, 0)
        return eng.lib.byz_auror_select_dev(eng.ctx, _vp(votes.data_ptr()), _vp(bad.data_ptr()), _vp(counts.data_ptr()), rows,
                                            ctypes.byref(p), _vp(kept_ptr), None)

    def whole(rows=n, acc=0, out_ptr=out.data_ptr(), votes_ptr=None):
        p = _native.AurorParams(0.3, 0.5, 32, acc)
        return eng.lib.byz_auror_dev(eng.ctx, _vp(gt.data_ptr()), rows, d, d, ctypes.byref(p), _vp(votes_ptr), None, None,
                                     _vp(out_ptr), _vp(kept.data_ptr()), None, None)
    assert votes_call(rows=16385) == _native.E_UNSUPPORTED                     # (the matrix is never read: refused on n alone)
    assert select_call(rows=16385) == _native.E_UNSUPPORTED and whole(rows=16385) == _native.E_UNSUPPORTED
    for kw in (dict(alpha=-1.0), dict(alpha=float('nan')), dict(alpha=float('inf')), dict(tau=-0.1), dict(tau=1.5),
               dict(tau=float('nan')), dict(cap=0), dict(acc=2), dict(rows=0), dict(votes_ptr=None)):
        assert votes_call(**kw) == _native.E_INVALID, kw
    assert select_call(tau=2.0) == _native.E_INVALID and select_call(kept_ptr=None) == _native.E_INVALID
    assert whole(out_ptr=None) == _native.E_INVALID and whole(acc=1) == _native.E_INVALID      # accumulate without a history
    assert whole(votes_ptr=votes.data_ptr()) == _native.E_INVALID              # votes without bad and counts
    assert whole(out_ptr=gt.data_ptr() + 4 * (d - 1)) == _native.E_INVALID     # out overlaps G
    eng.synchronize()
    for t in (votes, bad, counts, kept):
        assert bool((t == -7).all())
    assert bool((out == -3.0).all())
    with pytest.raises(ValueError):
        eng.auror(gt)                                                          # alpha has no default
    with pytest.raises(NotImplementedError):
        eng.auror_votes(torch.zeros((16385, 2), dtype=torch.float32, device=dev), 0.3)


def test_the_report_is_auror_s_own(eng, torch):
    from tests.test_faba import euclidean_f32, shifted_case
    gt = on_gpu(torch, eng, mixed_case(300, 130))
    _, want = eng.auror(gt, alpha=0.12, return_info=True)
    want = {k: want[k] for k in ('indicative', 'removed', 'kept', 'bad_rows', 'capped_cols')}
    _, faba = eng.faba_select(euclidean_f32(shifted_case(65, 200, seed=65)), 31)
    assert eng.auror_info() == want and eng.faba_info() == faba
    eng.auror(gt, alpha=0.3)
    assert eng.auror_info() != want and eng.faba_info() == faba


# ---- the layers above -------------------------------------------------------------------------------------------------------------
def test_the_history_over_two_rounds_and_reset(eng, torch):
    from attacking_federate_learning_amd import defences
    n, d = 300, 70
    a, b = mixed_case(n, d, seed=1), mixed_case(n, d, seed=2)
    wa, wb = restated_auror_votes(a, 0.12), restated_auror_votes(b, 0.12)
    for w, g in ((wa, a), (wb, b)):
        assert min(w['margin_t'], w['margin_alpha']) > margin_bound(g)
    ta, tb = on_gpu(torch, eng, a), on_gpu(torch, eng, b)
    history = defences.AurorHistory(n)
    first = defences.auror(ta, n, 0, 0.12, history=history)
    assert torch.equal(first.view(torch.int32), eng.auror(ta, alpha=0.12).view(torch.int32))
    second, info = defences.auror(tb, n, 0, 0.12, history=history, return_info=True)
    votes, bad, counts = history.numpy()
    assert history.rounds == 2 and np.array_equal(votes, wa['votes'] + wb['votes']) and np.array_equal(counts, wa['counts'] + wb['counts'])
    kept = restated_auror_select(votes, bad, counts, 0.5)                      # the selection read the sums
    assert np.array_equal(info['kept_rows'], np.flatnonzero(kept)) and info['indicative'] == counts[0]
    mask = on_gpu(torch, eng, kept.astype(np.float64))
    count = torch.tensor([float(kept.sum())], dtype=torch.float64, device=tb.device)
    assert torch.equal(second.view(torch.int32), eng.scaled_rows_sum(tb, mask, count).view(torch.int32))
    history.reset()
    votes, bad, counts = history.numpy()
    assert history.rounds == 0 and not votes.any() and not bad.any() and not counts.any()
    again = defences.auror(a, n, 0, 0.12, history=history)                     # a host matrix: numpy back
    assert isinstance(again, np.ndarray) and np.array_equal(bits32(again), bits32(host(first)))
    with pytest.raises(ValueError):
        defences.auror(ta[:10], 10, 0, 0.12, history=history)


def test_defences_auror_as_the_rule_of_a_pre_aggregation_and_the_server_step(eng, torch):
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.server import DeviceServer
    n, d, f = 40, 640, 8
    g, attackers, _ = planted_case(n, d, 5)
    gt = on_gpu(torch, eng, g)
    want = eng.auror(gt, alpha=0.3)
    assert torch.equal(defences.auror(gt, n, f, 0.3).view(torch.int32), want.view(torch.int32))
    back = defences.auror(g, n, f, alpha=0.3)
    assert isinstance(back, np.ndarray) and np.array_equal(bits32(back), bits32(host(want)))
    mixed = defences.nnm(gt, n, f, then=defences.auror, alpha=0.3)
    assert torch.equal(mixed.view(torch.int32), eng.auror(defences.nnm(gt, n, f), alpha=0.3).view(torch.int32))
    bucketed = defences.bucketing(gt, n, f, s=2, then=defences.auror, alpha=0.3, tau=0.25)
    assert bucketed.shape == (d,) and bool(torch.isfinite(bucketed).all())
    for pre in (defences.robust_lr, defences.sparsefed, defences.weak_dp):
        v = pre(gt, n, f, then=defences.auror, alpha=0.3)
        assert v.shape == (d,) and bool(torch.isfinite(v).all())
    with pytest.raises(TypeError):
        defences.nnm(gt, n, f, then=defences.auror)                            # alpha has no default
    server = DeviceServer(n, np.zeros(d, dtype=np.float32), f / n, 0.1, 0.9, torch_device='cuda:%d' % eng.device, engine=eng)
    server.users_grads.data.copy_(gt)
    step = server.defend_auror(0.3)
    assert torch.equal(step.view(torch.int32), want.view(torch.int32)) and server.auror_history.rounds == 1
    assert np.array_equal(np.flatnonzero(server.auror_history.numpy()[0] > 0.5 * (d // 10)), attackers)
    assert torch.equal(server.defend_auror(0.3, history=False).view(torch.int32), want.view(torch.int32))


def test_the_columns_layout_looped_over_two_shards(eng, torch):
    """ShardedAggregator.auror on two uneven column panels on ONE engine, its one all-reduce formed the way an all-reduce forms
    it: the first pass adds the panels' packed votes up, the second hands every panel the sum.  The votes are integers, so the
    selection is the single call's; a column's sum is local, so the panels' outputs concatenate to the single call's bits."""
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d = 300, 2000
    g, attackers, columns = planted_case(n, d, 6)
    gt = on_gpu(torch, eng, g)
    want, winfo = eng.auror(gt, alpha=0.3, return_info=True)
    assert np.array_equal(winfo['kept_rows'], np.setdiff1d(np.arange(n), attackers))
    one = ShardedAggregator(HipKernels(eng)).auror(gt, alpha=0.3, return_info=True)
    assert np.array_equal(one[1]['kept_rows'], winfo['kept_rows']) and torch.equal(one[0].view(torch.int32), want.view(torch.int32))
    panels = [gt[:, :777].contiguous(), gt[:, 777:].contiguous()]

    class Looped(ShardedAggregator):
        total, summing, seen = None, True, []

        def _collective(self):
            return True

        def _all_reduce(self, name, tensor):
            self.seen.append((name, tensor.dtype, tensor.numel()))
            if self.summing:
                Looped.total = tensor.clone() if Looped.total is None else Looped.total + tensor
            else:
                tensor.copy_(Looped.total)
            return tensor

    agg = Looped(HipKernels(eng))
    for panel in panels:
        agg.auror(panel, alpha=0.3)
    agg.summing, agg.seen = False, []
    outs = [agg.auror(panel, alpha=0.3, return_info=True) for panel in panels]
    assert agg.seen == [('allreduce_auror_votes', torch.int64, 2 * n + 4)] * 2          # one all-reduce a rank
    for _, info in outs:
        assert np.array_equal(info['kept_rows'], winfo['kept_rows']) and np.array_equal(info['votes'], winfo['votes'])
    joined = torch.cat([o for o, _ in outs])
    assert torch.equal(joined.view(torch.int32), want.view(torch.int32))
