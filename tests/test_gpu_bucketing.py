"""s-bucketing on the GPU against tests/test_bucketing.py's numpy restatement.  Every comparison of bucket means is exact
(uint32 views of the floats): a bucket's mean is no_defense's sequential fp32 chain over the bucket's rows and one division.
Where NaNs are planted, the NaN positions are compared and the bits of everything else."""
import ctypes

import numpy as np
import pytest

from tests.test_bucketing import bits, restated_buckets
from tests.views_arena import arena, even_ld, odd_ld, untouched

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


@pytest.fixture(scope='module')
def device(eng, torch):
    return torch.device('cuda', eng.device)


def matrix(n, d):
    g = np.random.default_rng(7000 + 31 * n + d % 1009).standard_normal((n, d)).astype(np.float32)
    g.setflags(write=False)
    return g


def permutations(n):
    """name -> perm: the identity (a null pointer), the reversed order, a seeded shuffle."""
    from attacking_federate_learning_amd.engine import bucketing_permutation
    return {'identity': None, 'reversed': np.arange(n - 1, -1, -1, dtype=np.int32), 'seeded': bucketing_permutation(n, seed=n)}


_WANT = {}


def reference(key, g, s, perm):
    """The restatement's matrix for a case, computed once per key and never written to."""
    if key not in _WANT:
        want = restated_buckets(g, s, perm)
        want.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def same_bits_nan_aware(got, want):
    """NaN positions equal, the bits of every other element equal."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan])


def bucket_sizes(n):
    return sorted({s for s in (1, 2, 3, 8, 9, n) if s <= n})


def check_shape(eng, torch, device, n, d, sizes=None):
    g = matrix(n, d)
    gt = torch.from_numpy(g).to(device)
    for s in sizes or bucket_sizes(n):
        for name, perm in permutations(n).items():
            want = reference((n, d, s, name), g, s, perm)
            got = eng.bucket_means(gt, s, perm)
            assert got.is_cuda and tuple(got.shape) == want.shape
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (n, d, s, name)
    return g, gt


# ---- row structure: a short last bucket; buckets shorter than, equal to and longer than the walk's run of eight rows; a run
# plus a tail within one bucket.  257 columns: two workgroups, the second with one column
@pytest.mark.parametrize('n', [1, 2, 7, 8, 9, 17, 64, 100])
def test_buckets_are_the_restatement(eng, torch, device, n):
    g, gt = check_shape(eng, torch, device, n, 257)
    # one bucket with the identity is no_defense's vector; buckets of one are the permuted rows
    one = eng.bucket_means(gt, n).cpu().numpy()
    assert np.array_equal(bits(one[0]), bits(eng.no_defense(gt).cpu().numpy()))
    perm = permutations(n)['seeded']
    assert np.array_equal(bits(eng.bucket_means(gt, 1, perm).cpu().numpy()), bits(g[perm]))


# ---- few columns: one partial workgroup, and the buckets spread over gridDim.y
@pytest.mark.parametrize('d', [1, 3, 255, 256])
def test_few_columns(eng, torch, device, d):
    check_shape(eng, torch, device, 17, d)


def test_more_buckets_than_workgroup_rows_walks_several_buckets_in_one_walk(eng, torch, device):
    """Three columns and 20,000 rows: the grid's y dimension is capped at eight workgroups per CU, so a workgroup takes 10, 5, 4,
    2 and 2 consecutive buckets at s = 1, 2, 3, 8 and 9 and ends buckets inside a run of eight rows; s = 5000 is a long chain."""
    from attacking_federate_learning_amd.engine import bucketing_permutation
    n, d = 20000, 3
    g = matrix(n, d)
    gt = torch.from_numpy(g).to(device)
    perm = bucketing_permutation(n, seed=4)
    for s in (1, 2, 3, 8, 9, 5000):
        want = reference((n, d, s, 'seed4'), g, s, perm)
        assert np.array_equal(bits(eng.bucket_means(gt, s, perm).cpu().numpy()), bits(want)), s


# ---- the four-wide walk, and the same data through views that force one column per thread
def wide_width(torch, device):
    """The first width past walk_shape's four-wide threshold, plus 3: the dwordx4 path with a masked last vector."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return 4 * 256 * cus * 2 + 3


def raw_call(eng, torch, device, view, s, perm_dev, ldy=None, sentinel=None):
    """byz_bucket_means_dev on a view -> the B x d result as numpy; with ldy > d the padding must keep its sentinel bits."""
    n, d = view.shape
    buckets = -(-n // s)
    ldy = d if ldy is None else ldy
    y = torch.full((buckets, ldy), float('nan') if sentinel is None else sentinel, dtype=torch.float32, device=device)
    before = y.clone()
    stream = torch.cuda.current_stream(device).cuda_stream
    rc = eng.lib.byz_bucket_means_dev(eng.ctx, vp(view.data_ptr()), n, d, view.stride(0),
                                      vp(perm_dev.data_ptr()) if perm_dev is not None else None, s, vp(y.data_ptr()), ldy,
                                      vp(stream))
    assert rc == 0
    torch.cuda.synchronize(device)
    assert torch.equal(y[:, d:].view(torch.int32), before[:, d:].view(torch.int32))
    return y[:, :d].cpu().numpy()


def test_wide_path_aligned_misaligned_base_and_odd_leading_dimension(eng, torch, device):
    from attacking_federate_learning_amd.engine import bucketing_permutation
    n, s = 11, 4
    d = wide_width(torch, device)
    g = matrix(n, d)
    perm = bucketing_permutation(n, seed=11)
    want = reference((n, d, s, 'seed11'), g, s, perm)
    gt = torch.from_numpy(g).to(device)
    assert gt.data_ptr() % 16 == 0 and gt.stride(0) % 4 != 0      # (d is odd: a contiguous matrix is not the four-wide case)
    # aligned: a leading dimension that is a multiple of four, the base on a 16-byte boundary -> VEC = 4, the last vector masked
    view, flat = arena(torch, g, even_ld(d), 0, device=device)
    assert view.data_ptr() % 16 == 0 and view.stride(0) % 4 == 0
    before = flat.clone()
    got = eng.bucket_means(view, s, perm)
    untouched(torch, flat, view, before)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    del view, flat, before
    # the base one float off 16-byte alignment; a leading dimension that is no multiple of four: VEC = 1 at that width
    perm_dev = torch.from_numpy(perm).to(device)
    for ld, off in ((even_ld(d), 1), (odd_ld(d), 0)):
        view, flat = arena(torch, g, ld, off, device=device)
        assert (view.data_ptr() % 16 != 0) or (view.stride(0) % 4 != 0)
        before = flat.clone()
        got = raw_call(eng, torch, device, view, s, perm_dev)
        untouched(torch, flat, view, before)
        assert np.array_equal(bits(got), bits(want)), (ld, off)
        del view, flat, before
    assert np.array_equal(bits(eng.bucket_means(gt, s, perm).cpu().numpy()), bits(want))


# ---- output layout and column panels
def test_padded_output_keeps_its_sentinel(eng, torch, device):
    from attacking_federate_learning_amd.engine import bucketing_permutation
    n, d, s = 17, 257, 3
    g = matrix(n, d)
    perm = bucketing_permutation(n, seed=n)
    want = reference((n, d, s, 'seeded'), g, s, perm)
    gt = torch.from_numpy(g).to(device)
    got = raw_call(eng, torch, device, gt, s, torch.from_numpy(perm).to(device), ldy=d + 7, sentinel=-123.25)
    assert np.array_equal(bits(got), bits(want))


def test_three_uneven_column_panels_give_the_bits_of_the_one_call(eng, torch, device):
    from attacking_federate_learning_amd.engine import bucketing_permutation
    n, d, s = 17, 1025, 3
    g = matrix(n, d)
    perm = bucketing_permutation(n, seed=n)
    want = reference((n, d, s, 'seeded'), g, s, perm)
    gt = torch.from_numpy(g).to(device)
    perm_dev = torch.from_numpy(perm).to(device)
    whole = eng.bucket_means(gt, s, perm_dev)
    assert np.array_equal(bits(whole.cpu().numpy()), bits(want))
    buckets = -(-n // s)
    y = torch.full((buckets, d), float('nan'), dtype=torch.float32, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    for lo, hi in ((0, 300), (300, 301), (301, d)):      # G + c0, Y + c0, the same ld and ldy
        rc = eng.lib.byz_bucket_means_dev(eng.ctx, vp(gt.data_ptr() + 4 * lo), n, hi - lo, d, vp(perm_dev.data_ptr()), s,
                                          vp(y.data_ptr() + 4 * lo), d, vp(stream))
        assert rc == 0
    torch.cuda.synchronize(device)
    assert torch.equal(y.view(torch.int32), whole.view(torch.int32))


# ---- special values stay inside their bucket and column
def test_planted_special_values_stay_in_their_bucket_and_column(eng, torch, device):
    from attacking_federate_learning_amd.engine import bucketing_permutation
    n, d = 17, 257
    g = np.array(matrix(n, d))
    planted = {(2, 5): np.nan, (3, 9): np.inf, (5, 9): -np.inf, (7, 100): np.inf, (11, 256): -np.inf, (13, 0): 1e-45}
    for (r, c), v in planted.items():
        g[r, c] = v
    g[:, 17] = -0.0                             # a column of -0.0: every chain starts at +0.0
    g[4, 200], g[4, 201] = 1e-45, -1e-45        # denormals: kept (s = 1), halved to zero by round-to-even (s = 2)
    g.setflags(write=False)
    gt = torch.from_numpy(g).to(device)
    perm = bucketing_permutation(n, seed=21)
    position = np.empty(n, dtype=np.int64)
    position[perm] = np.arange(n)
    for s in (1, 2, 3, 17):
        want = restated_buckets(g, s, perm)
        got = eng.bucket_means(gt, s, perm).cpu().numpy()
        same_bits_nan_aware(got, want)
        # not finite exactly where a planted non-finite value's row and column meet (rows 3 and 5 in one bucket: inf - inf)
        touched = np.zeros(want.shape, dtype=bool)
        for (r, c), v in planted.items():
            if not np.isfinite(v):
                touched[position[r] // s, c] = True
        assert np.array_equal(~np.isfinite(got), touched), s
        assert not np.signbit(got[:, 17]).any() and (got[:, 17] == 0).all()
        if s == 1:
            assert np.array_equal(bits(got[position[4], 200:202]), bits(g[4, 200:202]))
            nan = np.isnan(g[perm])
            assert np.array_equal(bits(got)[~nan & (g[perm] != 0)], bits(g[perm])[~nan & (g[perm] != 0)])
    # the host entry point: the same bits as numpy
    host = eng.bucket_means(g, 3, perm)
    assert isinstance(host, np.ndarray)
    same_bits_nan_aware(host, restated_buckets(g, 3, perm))


# ---- arguments
def test_arguments(eng, torch, device):
    from attacking_federate_learning_amd import _native
    n, d = 9, 8
    g = matrix(n, d)
    gt = torch.from_numpy(g).to(device)
    y = torch.zeros((n, d), dtype=torch.float32, device=device)
    call = eng.lib.byz_bucket_means_dev
    assert call(eng.ctx, vp(gt.data_ptr()), n, d, d, None, 0, vp(y.data_ptr()), d, None) == _native.E_INVALID
    assert call(eng.ctx, vp(gt.data_ptr()), n, d, d, None, n + 1, vp(y.data_ptr()), d, None) == _native.E_INVALID
    assert call(eng.ctx, vp(gt.data_ptr()), n, d, d, None, 2, vp(gt.data_ptr() + 4 * d), d, None) == _native.E_INVALID   # Y inside G
    assert call(eng.ctx, vp(gt.data_ptr()), n, d, d, None, 2, vp(y.data_ptr()), d - 1, None) == _native.E_INVALID          # ldy < n_cols
    assert call(eng.ctx, vp(gt.data_ptr()), n, d, d, None, 2, None, d, None) == _native.E_INVALID
    # the row ceiling is decided on the arguments alone: nothing is dereferenced, whatever the pointers
    limit = ctypes.c_int64(0)
    assert eng.lib.byz_limits(ctypes.byref(limit), None) == 0
    assert call(eng.ctx, None, limit.value + 1, d, d, None, 2, None, d, None) == _native.E_UNSUPPORTED
    assert call(eng.ctx, vp(gt.data_ptr()), limit.value + 1, d, d, None, 2, vp(y.data_ptr()), d, None) == _native.E_UNSUPPORTED
    for bad in (0, n + 1, 2.5):
        with pytest.raises(ValueError):
            eng.bucket_means(gt, bad)
        with pytest.raises(ValueError):
            eng.bucket_means(g, bad)
    # the host entry point checks the permutation
    out = np.empty((5, d), dtype=np.float32)
    host = eng.lib.byz_bucket_means_host
    good = np.arange(n, dtype=np.int32)
    assert host(eng.ctx, g.ctypes.data_as(vp), n, d, good.ctypes.data_as(vp), 2, out.ctypes.data_as(vp)) == 0
    assert np.array_equal(bits(out), bits(restated_buckets(g, 2)))
    assert host(eng.ctx, g.ctypes.data_as(vp), n, d, None, 2, out.ctypes.data_as(vp)) == 0
    assert np.array_equal(bits(out), bits(restated_buckets(g, 2)))
    for i, v in ((3, 4), (0, -1), (8, n)):
        bad = good.copy()
        bad[i] = v
        assert host(eng.ctx, g.ctypes.data_as(vp), n, d, bad.ctypes.data_as(vp), 2, out.ctypes.data_as(vp)) == _native.E_INVALID
        with pytest.raises(ValueError):
            eng.bucket_means(gt, 2, bad)
        with pytest.raises(ValueError):
            eng.bucket_means(g, 2, bad)
    assert host(eng.ctx, g.ctypes.data_as(vp), n, d, good.ctypes.data_as(vp), 0, out.ctypes.data_as(vp)) == _native.E_INVALID


def test_out_of_range_entries_on_the_device_are_skipped_and_the_divisor_stays(eng, torch, device):
    """Defined behaviour on a valid launch: an entry outside [0, n) is never used as a row number."""
    from attacking_federate_learning_amd.engine import bucketing_permutation
    n, d = 17, 257
    g = matrix(n, d)
    gt = torch.from_numpy(g).to(device)
    for s in (1, 3, 9):
        perm = bucketing_permutation(n, seed=s)
        perm[4], perm[12] = n, -1
        want = []
        for b in range(-(-n // s)):
            rows = perm[b * s:(b + 1) * s]
            kept = rows[(rows >= 0) & (rows < n)]
            total = np.zeros(d, dtype=np.float32)
            for r in kept:
                total = total + g[r]
            want.append(total / np.float32(len(rows)))
        got = raw_call(eng, torch, device, gt, s, torch.from_numpy(perm).to(device))
        assert np.array_equal(bits(got), bits(np.stack(want))), s


# ---- composition ----------------------------------------------------------------------------------------------------------
COMPOSE = (40, 1000, 6, 2)


def compose_case():
    from attacking_federate_learning_amd.engine import bucketing_permutation
    n, d, f, s = COMPOSE
    rng = np.random.default_rng(40)
    g = rng.standard_normal((n, d)).astype(np.float32)
    g *= (1.0 + 0.5 * rng.permutation(n) / n).astype(np.float32)[:, None]
    g[:f] = (g[:f].mean(axis=0) - 1.5 * g[:f].std(axis=0)).astype(np.float32)
    g.setflags(write=False)
    perm = bucketing_permutation(n, seed=0)
    return g, perm, reference(('compose', 0), g, s, perm)


@pytest.mark.parametrize('rule', ['krum', 'trimmed_mean', 'coordinate_median', 'geometric_median', 'centered_clip'])
def test_a_rule_behind_the_bucketing_sees_the_restated_matrix(eng, torch, device, rule):
    """The bucketed matrix is the restatement's bit for bit, so the rule behind it gives the bits it gives on the restatement's
    matrix with (20, 6): stricter than the rule's own tolerance."""
    from attacking_federate_learning_amd import defences
    n, d, f, s = COMPOSE
    g, perm, want = compose_case()
    then = getattr(defences, rule)
    expect = then(torch.from_numpy(np.array(want)).to(device), 20, f).cpu().numpy()
    assert expect.shape == (d,) and np.isfinite(expect).all()
    gt = torch.from_numpy(g).to(device)
    on_device = defences.bucketing(gt, n, f, s=s, then=then)            # seed = 0
    assert on_device.is_cuda and np.array_equal(bits(on_device.cpu().numpy()), bits(expect))
    got = defences.bucketing(g, n, f, s=s, then=then, perm=perm)
    assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(expect))
    # then=None: the matrix itself, on the device or as numpy; perm overrides seed
    assert np.array_equal(bits(defences.bucketing(gt, n, f, s=s).cpu().numpy()), bits(want))
    host = defences.bucketing(g, n, f, s=s, perm=perm, seed=99)
    assert isinstance(host, np.ndarray) and np.array_equal(bits(host), bits(want))


def test_device_server_reshuffles_every_round_and_steps_as_defend_would(eng, torch, device):
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import bucketing_permutation
    from attacking_federate_learning_amd.server import DeviceServer
    n, d, f, s = COMPOSE
    g, perm0, want0 = compose_case()
    mal_prop = 0.15
    assert int(n * mal_prop) == f
    w0 = np.random.default_rng(3).standard_normal(d).astype(np.float32)
    server = DeviceServer(n, w0, mal_prop, 0.1, 0.9, torch_device=device, engine=eng)
    assert server.bucketing_round == 0
    server.users_grads.data.copy_(torch.from_numpy(g))
    server.velocity.fill_(0.25)
    w = torch.from_numpy(w0).to(device)
    v = torch.full_like(w, 0.25)
    aggregates = []
    for rnd in range(2):
        perm = bucketing_permutation(n, seed=rnd)
        want = want0 if rnd == 0 else reference(('compose', rnd), g, s, perm)
        expect = defences.coordinate_median(torch.from_numpy(np.array(want)).to(device), 20, f)
        agg = server.defend_bucketing(defences.coordinate_median, s=s)
        assert server.bucketing_round == rnd + 1
        assert torch.equal(agg.view(torch.int32), expect.view(torch.int32)), rnd
        eng.server_update(w, v, expect, 0.9, 0.1)              # defend's arithmetic on the same aggregate
        assert torch.equal(server.current_weights.view(torch.int32), w.view(torch.int32))
        assert torch.equal(server.velocity.view(torch.int32), v.view(torch.int32))
        aggregates.append(agg.cpu().numpy())
    assert not np.array_equal(bucketing_permutation(n, 0), bucketing_permutation(n, 1))
    assert not np.array_equal(bits(aggregates[0]), bits(aggregates[1]))        # the second round's shuffle is another one
    with pytest.raises(TypeError):
        server.defend_bucketing(None)
    assert server.bucketing_round == 2


# ---- the columns layout -----------------------------------------------------------------------------------------------------
def test_columns_layout_looped_over_three_uneven_shards_equals_one_gpu(eng, torch, device):
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    n, d, f, s = 17, 1025, 4, 3
    g = matrix(n, d)
    gt = torch.from_numpy(g).to(device)
    agg = ShardedAggregator(HipKernels(eng))
    assert agg.world == 1
    whole = agg.bucketing(gt, n, f, s=s, seed=n)
    from attacking_federate_learning_amd.engine import bucketing_permutation
    want = reference((n, d, s, 'seeded'), g, s, bucketing_permutation(n, seed=n))
    assert np.array_equal(bits(whole.cpu().numpy()), bits(want))
    slices = []
    for lo, hi in ((0, 342), (342, 343), (343, d)):
        local = torch.empty((n, -(-(hi - lo) // 4) * 4), dtype=torch.float32, device=device)[:, :hi - lo]
        local.copy_(gt[:, lo:hi])
        slices.append(agg.bucketing(local, n, f, s=s, seed=n))        # every rank the same seed; no collective
    assert torch.equal(torch.cat(slices, dim=1).view(torch.int32), whole.view(torch.int32))
