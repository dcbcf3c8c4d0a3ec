"""FABA on the device against tests/test_faba.py's restatement of include/byzagg.h's rule: the kept flags and the removal order
equal as integers, on Euclidean, cosine and Manhattan handles, on dense matrices at every slot boundary of the one-workgroup
loop (1024 rows a slot), with both powers and every removal count that takes another way through the loop (none, one, half,
the full peeling).  The aggregate is byz_scaled_rows_sum_dev's bits; equivalent calls give the same bits.  The sharded layout
is looped on one engine: three column panels, their Grams added the way an all-reduce adds them."""
import functools

import numpy as np
import pytest

from tests.test_faba import euclidean_f32, random_symmetric, restated_faba_select, shifted_case

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:%d' % eng.device)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def counts_of(n):
    return sorted({0, 1, max(n // 2 - 1, 0), n - 1})


@functools.lru_cache(maxsize=None)
def dense_case(n):
    """small n: the Euclidean distances of a shifted cloud; from 1023 rows on a random symmetric matrix, uploaded as it is"""
    if n < 1000:
        return euclidean_f32(shifted_case(n, 200, seed=n))
    return random_symmetric(n, seed=n)


def check_select(eng, handle, c, r, power):
    rows, order, info = eng.faba_select(handle, r, power=power, return_order=True)
    kept, want_order, want = restated_faba_select(c, r, power=power, return_info=True)
    assert np.array_equal(rows, np.flatnonzero(kept)), (c.shape[0], r, power)
    assert np.array_equal(order, want_order), (c.shape[0], r, power)
    assert info == want, (info, want)              # the counts, and the last score and the divisor as values
    return kept, want_order, info


# ---- the selection ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('n', [2, 3, 63, 64, 65, 1023, 1024, 1025, 2049, 4097])
def test_select_equals_the_restatement(eng, n, power):
    c = dense_case(n)
    handle, _ = eng._as_distances(c)
    for r in counts_of(n):
        kept, order, info = check_select(eng, handle, c, r, power)
        assert info['removed'] == r and info['forced'] == 0 and kept.sum() == n - r


def test_the_flags_and_the_order_on_the_device(eng, torch):
    """on_device=True: the 0 / 1 flags and the order padded with -1, beside `like`"""
    n, r = 65, 31
    c = dense_case(n)
    like = torch.zeros(1, device='cuda:%d' % eng.device)
    flags, order, info = eng.faba_select(c, r, on_device=True, like=like, return_order=True)
    kept, want = restated_faba_select(c, r)
    assert flags.dtype == torch.int32 and order.dtype == torch.int32 and flags.device == like.device
    assert np.array_equal(flags.cpu().numpy(), kept.astype(np.int32))
    assert np.array_equal(order.cpu().numpy(), np.concatenate([want, np.full(n - r, -1)]).astype(np.int32))


@pytest.mark.parametrize('metric', ['pairwise_distances', 'cosine_distances', 'manhattan_distances'])
def test_select_on_the_library_s_own_handles(eng, torch, metric):
    n, d = 65, 2000
    gt = on_gpu(torch, eng, shifted_case(n, d, seed=3))
    handle = getattr(eng, metric)(gt)
    c = handle.numpy()
    assert np.array_equal(bits(c), bits(c.T))                  # symmetric as bits: row q of it is column q
    for power in ((2,) if metric == 'pairwise_distances' else (1, 2)):
        for r in (1, 31, 64):
            check_select(eng, handle, c, r, power)


def drift_rows(n, d, f, seed):
    """the drift attack's block: the first f rows are ONE vector, the honest mean shifted by a standard deviation"""
    g = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    g[:f] = g[f:].mean(axis=0) - 1.0 * g[f:].std(axis=0)
    return g


def test_the_drift_attack_s_identical_rows_tie_and_pass(eng, torch):
    n, d, f = 65, 2000, 13
    gt = on_gpu(torch, eng, drift_rows(n, d, f, seed=8))
    handle = eng.pairwise_distances(gt)
    c = handle.numpy()
    kept, order, _ = check_select(eng, handle, c, f, 2)
    assert kept[:f].all()                                       # inside the crowd: FABA removes honest rows instead
    kept, order, _ = check_select(eng, handle, c, n - 1, 2)     # the full peeling: where they go, they go lowest row first
    block = [q for q in order.tolist() if q < f]
    assert block == sorted(block)


@pytest.mark.parametrize('broken,r', [(3, 8), (8, 3)])
@pytest.mark.parametrize('value', [np.nan, np.inf])
def test_broken_rows_go_first(eng, torch, broken, r, value):
    n, d = 65, 500
    g = shifted_case(n, d, seed=12)
    rows = np.sort(np.random.default_rng(broken).choice(n, broken, replace=False))
    g[rows, 7] = value
    gt = on_gpu(torch, eng, g)
    handle = eng.pairwise_distances(gt)
    c = handle.numpy()
    assert not np.isfinite(c[rows]).any()                       # a broken gradient's row holds no finite entry
    kept, order, info = check_select(eng, handle, c, r, 2)
    assert order[:broken].tolist() == rows.tolist() and info['removed'] == max(broken, r) and info['forced'] == max(broken - r, 0)
    out, oinfo = eng.faba(gt, n, r, return_info=True)
    assert np.array_equal(oinfo['kept_rows'], np.flatnonzero(kept)) and bool(torch.isfinite(out).all())


def test_one_unusable_pair_in_a_dense_matrix_and_an_all_nan_matrix(eng):
    c = dense_case(1025).copy()
    c[100, 1024] = c[1024, 100] = INF
    kept, order, info = check_select(eng, c, c, 0, 2)
    assert order.size == 1 and order[0] in (100, 1024) and info['forced'] == 1
    check_select(eng, c, c, 5, 1)
    for n in (2, 70):
        nobody = np.full((n, n), np.nan, dtype=np.float32)
        kept, order, info = check_select(eng, nobody, nobody, 0, 2)
        assert not kept.any() and info['kept'] == 0 and info['divisor'] == 0.0


# ---- the refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    dev = 'cuda:%d' % eng.device
    n, d = 20, 64
    gt = on_gpu(torch, eng, shifted_case(n, d, seed=1))
    dist_host = np.ascontiguousarray(dense_case(63)[:n, :n])
    dist = on_gpu(torch, eng, dist_host)
    flags = torch.full((n,), -7, dtype=torch.int32, device=dev)
    order = torch.full((n,), -9, dtype=torch.int32, device=dev)
    out = torch.full((d,), -3.0, dtype=torch.float32, device=dev)

    def select(rows=n, r=3, power=2, dist_ptr=dist.data_ptr(), flags_ptr=flags.data_ptr()):
        return eng.lib.byz_faba_select_dev(eng.ctx, _vp(dist_ptr), rows, r, power, _vp(flags_ptr), _vp(order.data_ptr()), None)

    def whole(rows=n, r=3, out_ptr=out.data_ptr()):
        return eng.lib.byz_faba_dev(eng.ctx, _vp(gt.data_ptr()), rows, d, d, r, None, _vp(out_ptr), _vp(flags.data_ptr()),
                                    _vp(order.data_ptr()), None)
    assert select(rows=16385) == _native.E_UNSUPPORTED          # (the matrix is never read: refused on n alone)
    assert whole(rows=16385) == _native.E_UNSUPPORTED
    assert select(rows=1, r=0) == _native.E_INVALID
    assert select(r=-1) == _native.E_INVALID and select(r=n) == _native.E_INVALID
    assert select(power=0) == _native.E_INVALID and select(power=3) == _native.E_INVALID
    assert select(dist_ptr=None) == _native.E_INVALID and select(flags_ptr=None) == _native.E_INVALID
    assert whole(r=-1) == _native.E_INVALID and whole(r=n) == _native.E_INVALID
    assert whole(out_ptr=None) == _native.E_INVALID
    assert whole(out_ptr=gt.data_ptr() + 4 * (d - 1)) == _native.E_INVALID           # out overlaps G
    eng.synchronize()
    assert (flags == -7).all() and (order == -9).all() and (out == -3.0).all()
    for bad in (dict(remove_count=n), dict(remove_count=-1), dict(remove_count=3, power=3)):
        with pytest.raises(ValueError):
            eng.faba_select(dist_host, **bad)
    with pytest.raises(ValueError):
        eng.faba_select({0: {1: 1.0}, 1: {0: 1.0}}, 0)
    with pytest.raises(ValueError):
        eng.faba(gt, n, 3, distances=dense_case(63))            # 63 rows of distances, 20 of gradients


# ---- the aggregate ------------------------------------------------------------------------------------------------------------
def test_the_aggregate_is_scaled_rows_sum_and_the_mean_of_the_kept_rows(eng, torch):
    n, d, f = 65, 2000, 13
    g = shifted_case(n, d, seed=21)
    gt = on_gpu(torch, eng, g)
    out, info = eng.faba(gt, n, f, return_info=True)
    kept, order, want = restated_faba_select(eng.pairwise_distances(gt).numpy(), f, return_info=True)
    assert np.array_equal(info['kept_rows'], np.flatnonzero(kept)) and np.array_equal(info['order'], order)
    assert {k: info[k] for k in want} == want and eng.faba_info() == want
    mask = on_gpu(torch, eng, kept.astype(np.float64))
    count = torch.tensor([float(kept.sum())], dtype=torch.float64, device=gt.device)
    assert torch.equal(out.view(torch.int32), eng.scaled_rows_sum(gt, mask, count).view(torch.int32))
    ref = g[kept].astype(np.float64).mean(axis=0)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    print('faba %dx%d: worst error %.3g of |ref|' % (n, d, (err / np.abs(ref)).max()))
    assert (err <= 2.0 ** -23 * np.abs(ref)).all()


def test_equivalent_calls_give_the_same_bits(eng, torch):
    n, d, f = 65, 2000, 13
    g = shifted_case(n, d, seed=22)
    gt = on_gpu(torch, eng, g)
    a, ia = eng.faba(gt, n, f, return_info=True)
    # the two calls made by hand, and the matrix handed in
    handle = eng.pairwise_distances(gt)
    flags, _ = eng.faba_select(handle, f, on_device=True, like=gt)
    by_hand = eng.scaled_rows_sum(gt, flags.to(torch.float64), flags.sum().to(torch.float64).reshape(1))
    assert torch.equal(a.view(torch.int32), by_hand.view(torch.int32))
    b, ib = eng.faba(gt, n, f, distances=handle, return_info=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and np.array_equal(ia['order'], ib['order'])
    # a strided view, one float off a 16-byte boundary
    flat = torch.full((n * (d + 5) + 3,), 3.0, dtype=torch.float32, device=gt.device)
    view = flat[3:3 + n * (d + 5)].view(n, d + 5)[:, :d]
    view.copy_(gt)
    v, iv = eng.faba(view, n, f, return_info=True)
    assert np.array_equal(iv['order'], ia['order']) and torch.equal(a.view(torch.int32), v.view(torch.int32))
    # a side stream
    side = torch.cuda.Stream(device=gt.device)
    side.wait_stream(torch.cuda.current_stream(gt.device))
    with torch.cuda.stream(side):
        s, is_ = eng.faba(gt, n, f, return_info=True)
    side.synchronize()
    assert np.array_equal(is_['order'], ia['order']) and torch.equal(a.view(torch.int32), s.view(torch.int32))
    # the host entry point: numpy in -> numpy out
    h, ih = eng.faba(g, n, f, return_info=True)
    assert isinstance(h, np.ndarray) and np.array_equal(ih['order'], ia['order']) and np.array_equal(bits(h), bits(a.cpu().numpy()))
    hd = eng.faba(g, n, f, distances=handle.numpy())
    assert np.array_equal(bits(hd), bits(h))


def test_nobody_kept_gives_the_zero_vector(eng, torch):
    n, d = 9, 300
    g = np.full((n, d), np.nan, dtype=np.float32)
    out, info = eng.faba(on_gpu(torch, eng, g), n, 2, return_info=True)
    assert info['kept'] == 0 and info['removed'] == n and info['divisor'] == 0.0 and info['kept_rows'].size == 0
    assert bool((out == 0).all())


def test_the_report_is_faba_s_own(eng):
    """DESIGN.md 3.4's table: a FABA call writes the FABA report and no other; another defence's call leaves it alone"""
    c = dense_case(65)
    _, want = eng.faba_select(c, 31)
    _, flame = eng.flame_select(c)
    assert eng.faba_info() == want                              # FLAME's selection did not touch it
    _, again = eng.faba_select(c, 5, power=1)
    assert again != want and eng.faba_info() == again
    info = eng.flame_info()
    info.pop('clip')
    assert info == flame                                        # nor FABA FLAME's


# ---- the layers above ---------------------------------------------------------------------------------------------------------
def test_defences_faba_its_assertion_and_as_the_rule_of_a_pre_aggregation(eng, torch):
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.server import DeviceServer
    n, d, f = 21, 640, 4
    g = shifted_case(n, d, seed=31)
    gt = on_gpu(torch, eng, g)
    want = eng.faba(gt, n, f)
    assert torch.equal(defences.faba(gt, n, f).view(torch.int32), want.view(torch.int32))
    host = defences.faba(g, n, f)
    assert isinstance(host, np.ndarray) and np.array_equal(bits(host), bits(want.cpu().numpy()))
    with pytest.raises(AssertionError):
        defences.faba(gt, n, 11)                                # 21 < 2 * 11 + 1
    mixed = defences.nnm(gt, n, f, then=defences.faba)
    assert mixed.shape == (d,) and bool(torch.isfinite(mixed).all())
    assert torch.equal(mixed.view(torch.int32), eng.faba(defences.nnm(gt, n, f), n, f).view(torch.int32))
    bucketed = defences.bucketing(gt, n, f, s=2, then=defences.faba)      # 11 buckets, 4 of them removed
    assert bucketed.shape == (d,) and bool(torch.isfinite(bucketed).all())
    server = DeviceServer(n, np.zeros(d, dtype=np.float32), f / n, 0.1, 0.9, torch_device='cuda:%d' % eng.device, engine=eng)
    server.users_grads.data.copy_(gt)
    step = server.defend_faba()
    assert torch.equal(step.view(torch.int32), eng.faba(gt, n, int(n * (f / n))).view(torch.int32))


def test_the_sharded_layout_on_three_column_panels(eng, torch):
    """ShardedAggregator.faba looped over three uneven panels on ONE engine.  Its all-reduces are formed here the way
    tests/test_gpu_flame_sharded.py forms them: in pass p the all-reduces before the p-th are replaced by the sums of the
    earlier passes and the p-th is added up over the panels, until a pass replaces them all -- what every rank of a real
    all-reduce sees.  The planted rows are far apart from the crowd, so the sum of the panels' Grams, which is not the one
    call's Gram bit for bit, gives the same kept set; a column's sum then has the one call's bits."""
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d, f = 65, 2000, 13
    g = np.random.default_rng(41).standard_normal((n, d)).astype(np.float32)
    g[:f] += (3.0 + np.arange(f, dtype=np.float32))[:, None]    # separated: every planted row at its own distance
    gt = on_gpu(torch, eng, g)
    want, winfo = eng.faba(gt, n, f, return_info=True)
    assert np.array_equal(winfo['kept_rows'], np.arange(f, n))
    bounds = [0, 397, 1101, d]
    panels = [gt[:, lo:hi].contiguous() for lo, hi in zip(bounds[:-1], bounds[1:])]

    class Looped(ShardedAggregator):
        sums, replaced, index, seen = {}, 0, 0, []

        def _collective(self):
            return True

        def _all_reduce(self, name, tensor):
            k = self.index
            self.index += 1
            self.seen.append(name)
            if k < self.replaced:
                tensor.copy_(self.sums[k])
            elif k == self.replaced:
                self.sums[k] = tensor.clone() if k not in self.sums else self.sums[k] + tensor
            return tensor

    one = ShardedAggregator(HipKernels(eng)).faba(gt, n, f, return_info=True)        # one rank holding every column first
    assert np.array_equal(one[1]['kept_rows'], winfo['kept_rows']) and torch.equal(one[0].view(torch.int32), want.view(torch.int32))
    agg = Looped(HipKernels(eng))
    per_call = None
    for _ in range(4):
        outs, agg.seen = [], []
        for panel in panels:
            agg.index = 0
            outs.append(agg.faba(panel, n, f, return_info=True))
            per_call = agg.index
        if agg.replaced == per_call:
            break
        agg.replaced += 1
    assert agg.replaced == per_call and set(agg.seen) <= {'allreduce_gram', 'allreduce_near_pairs'} and 'allreduce_gram' in agg.seen
    for (out, info), lo, hi in zip(outs, bounds[:-1], bounds[1:]):
        assert np.array_equal(info['kept_rows'], winfo['kept_rows'])
        assert torch.equal(out.view(torch.int32), want[lo:hi].view(torch.int32))
    with pytest.raises(AssertionError):
        agg.faba(gt, n, 33)
