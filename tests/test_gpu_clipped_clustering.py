"""ClippedClustering and the linkage on an MI355X, held to the numpy restatement of tests/test_clipped_clustering.py.

The merges are compared EXACTLY -- pairs, sizes, and heights as bits -- against restated_linkage run on the very matrix the device
clustered, so no margin enters.  Past n = 257 the O(n^3) restatement is too slow and scipy is the yardstick: sorted heights
within 1e-12 relative (scipy merges in another order, so its roundings differ) and the two-way partition exact, on planted data
whose last two heights are far apart (asserted)."""
import ctypes

import numpy as np
import pytest

from tests.test_clipped_clustering import (METHODS, planted, restated_clip_scales, restated_clipped_clustering, restated_cut,
                                           restated_linkage, restated_select, restated_working_copy, same_partition)
from tests.test_flame import restated_cosine

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


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the matrices -----------------------------------------------------------------------------------------------------------
def random_cosine(n, seed):
    g = np.random.default_rng(seed).standard_normal((n, 24)) + 0.5
    return restated_cosine(g.astype(np.float32)).astype(np.float32)


def all_equal(n, seed):
    c = np.full((n, n), 0.75, dtype=np.float32)
    np.fill_diagonal(c, INF)
    return c


def duplicate_blocks(n, seed):
    """Blocks of identical rows: zero distances inside a block, every choice among them a tie broken by index."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((max(n // 4, 1), 16)) + 0.3
    g = base[rng.integers(0, base.shape[0], n)]
    x = ((g[:, None, :] - g[None, :, :]) ** 2).sum(-1).astype(np.float32)
    np.fill_diagonal(x, INF)
    return x


def star(n, seed):
    """Every row's nearest partner is row n // 2: the worst case for the rescan queue under average and complete linkage."""
    rng = np.random.default_rng(seed)
    c = (1.0 + rng.random((n, n))).astype(np.float32)
    c = np.minimum(c, c.T)
    hub = n // 2
    c[hub, :] = c[:, hub] = (0.1 + 0.01 * np.arange(n)).astype(np.float32)
    np.fill_diagonal(c, INF)
    return c


def damaged(n, seed):
    """Rows that are not usable, and entries between usable rows that are not finite, negative or -0.0."""
    rng = np.random.default_rng(seed)
    c = random_cosine(n, seed)
    if n >= 3:
        dead = rng.choice(n, size=max(1, n // 5), replace=False)
        c[dead, :] = INF
        c[:, dead] = rng.choice([INF, np.float32(np.nan), -INF], size=(n, len(dead)))
        c[dead, :] = c[:, dead].T
    if n >= 5:
        i, j = rng.integers(0, n, 12), rng.integers(0, n, 12)
        for k, (a, b) in enumerate(zip(i, j)):
            if a != b:
                c[a, b] = c[b, a] = (np.float32(np.nan), -INF, np.float32(-0.5), np.float32(-0.0), INF)[k % 5]
    np.fill_diagonal(c, INF)
    return c


FAMILIES = {'cosine': random_cosine, 'all_equal': all_equal, 'duplicates': duplicate_blocks, 'star': star, 'damaged': damaged}


# ---- the merges as bits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('n', [2, 3, 5, 63, 64, 65, 130, 257])
def test_merges_equal_the_restatement_bit_for_bit(eng, n, method):
    for kind, make in FAMILIES.items():
        c = make(n, 31 * n + len(kind))
        for fill in ((2.0, 0.125) if kind == 'damaged' else (2.0,)):
            pair, height, size, usable = eng.linkage_merges(c, method=method, fill=fill)
            rpair, rheight, rsize, rusable = restated_linkage(c, method, fill)
            assert np.array_equal(usable, rusable), (kind, n)
            assert np.array_equal(pair, rpair), (kind, n, method)
            assert np.array_equal(size, rsize), (kind, n, method)
            assert np.array_equal(bits64(height), bits64(rheight)), (kind, n, method)
            info = eng.linkage_info()
            assert info['merges'] == max(int(rusable.sum()) - 1, 0) and 0 <= info['max_rescans'] <= n
            if method == 'single':
                assert info['rescans'] == 0                 # min(W[a][k], W[b][k]) always repairs the cache in registers
            flags, sinfo = eng.clipped_clustering_select(c, method=method, fill=fill)
            assert np.array_equal(flags, np.flatnonzero(restated_select(c, method, fill))), (kind, n, method)
            assert sinfo['usable'] == int(rusable.sum()) and sinfo['admitted'] == len(flags)
            if len(rheight) >= 1:
                assert bits64(sinfo['top_height']) == bits64(rheight[-1])
            if len(rheight) >= 2:
                assert bits64(sinfo['second_height']) == bits64(rheight[-2])


def test_scipy_takes_the_linkage_matrix(eng):
    from scipy.cluster.hierarchy import fcluster, is_valid_linkage
    c = random_cosine(41, 5)
    c[[3, 17], :] = INF                                     # two rows that are not usable
    c[:, [3, 17]] = INF
    z, usable = eng.linkage(c, method='average')
    u = int(usable.sum())
    assert z.shape == (u - 1, 4) and is_valid_linkage(z) and z[-1, 3] == u
    pair, _, _, rusable = restated_linkage(c, 'average')
    labels, _ = restated_cut(pair, rusable, 3)
    assert same_partition(fcluster(z, 3, 'maxclust'), labels[usable])


# ---- the ownership boundaries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,methods', [(1023, METHODS), (1024, METHODS), (1025, METHODS), (2049, METHODS), (4097, ('average',)),
                                        (8193, ('average',))])
def test_ownership_boundaries_against_scipy(eng, torch, n, methods):
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    g, f = planted(n, 200, seed=n)
    c = eng.cosine_distances(on_gpu(torch, eng, g)).numpy()
    w, usable = restated_working_copy(c)
    assert usable.all()
    condensed = squareform(w, checks=False)
    for method in methods:
        pair, height, size, dev_usable = eng.linkage_merges(c, method=method)
        assert dev_usable.all() and len(height) == n - 1 and size[-1] == n
        assert (pair[:, 0] < pair[:, 1]).all() and len(set(pair[:, 1].tolist())) == n - 1     # every slot but 0 retires once
        z = linkage(condensed, method=method)
        rel = np.abs(np.sort(height) - z[:, 2]) / z[:, 2]
        print('n = %d %s: heights within %.3g relative of scipy' % (n, method, rel.max()))
        assert rel.max() <= 1e-12
        assert (z[-1, 2] - z[-2, 2]) / z[-1, 2] > 1e-3                                          # the planted gap
        labels, sizes = eng.linkage_cut(pair, dev_usable, 2)
        assert same_partition(labels, fcluster(z, 2, 'maxclust'))
        assert labels[0] == 0 and sizes.sum() == n
        flags, _ = eng.clipped_clustering_select(c, method=method)
        if method == 'average':
            assert np.array_equal(flags, np.arange(f, n))                                       # exactly the honest rows


# ---- the cut ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['cosine', 'damaged'])
def test_the_cut_against_fcluster_and_the_numbering(eng, kind):
    from scipy.cluster.hierarchy import fcluster
    n = 37
    c = FAMILIES[kind](n, 99)
    for method in METHODS:
        pair, height, size, usable = eng.linkage_merges(c, method=method)
        z, _ = eng.linkage(c, method=method)
        u = int(usable.sum())
        for count in (1, 2, 3, u):
            labels, sizes = eng.linkage_cut(pair, usable, count)
            rlabels, rsizes = restated_cut(pair, usable, count)
            assert np.array_equal(labels, rlabels) and np.array_equal(sizes, rsizes)
            assert (labels[~usable] == -1).all() and sorted(set(labels[usable].tolist())) == list(range(count))
            if kind == 'cosine':                             # (distinct heights: maxclust gives exactly `count` clusters)
                assert same_partition(labels[usable], fcluster(z, count, 'maxclust'))
            first = [int(np.flatnonzero(labels == k)[0]) for k in range(count)]
            assert first == sorted(first)                    # numbered by lowest row
            assert np.array_equal(sizes, np.bincount(labels[usable], minlength=count))
        assert np.array_equal(eng.linkage_cut(pair, usable, u)[0][usable], np.arange(u))
    from attacking_federate_learning_amd import defences
    assert np.array_equal(defences.linkage_labels(c, n_clusters=3, method='complete'),
                          restated_cut(restated_linkage(c, 'complete')[0], restated_linkage(c, 'complete')[3], 3)[0])


# ---- the whole call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', [(9, 33), (65, 257), (130, 1025)])
def test_the_whole_call_from_its_pieces(eng, torch, n, d):
    g, f = planted(n, d, seed=7 * n + d)
    gt = on_gpu(torch, eng, g)
    out, info = eng.clipped_clustering(gt, return_info=True)
    c = eng.cosine_distances(gt).numpy()
    mask = restated_select(c)
    assert np.array_equal(info['admitted_rows'], np.flatnonzero(mask))               # exact: the same matrix, no margin
    assert np.array_equal(info['admitted_rows'], np.arange(f, n)) and info['usable'] == n and info['admitted'] == n - f
    _, height, _, _ = restated_linkage(c)
    assert bits64(info['top_height']) == bits64(height[-1]) and bits64(info['second_height']) == bits64(height[-2])
    zero = torch.zeros(d, dtype=torch.float32, device=gt.device)
    sq = eng.row_sqdist(gt, zero)
    scales, clip = eng.clip_scales(sq, adaptive=True, return_clip=True)
    assert float(clip.item()) == info['clip']
    weights = scales * on_gpu(torch, eng, mask.astype(np.float64))
    count = torch.tensor([float(mask.sum())], dtype=torch.float64, device=gt.device)
    want = eng.scaled_rows_sum(gt, weights, count)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    ref, rmask, rclip = restated_clipped_clustering(g)
    assert np.array_equal(rmask, mask) and abs(info['clip'] / rclip - 1.0) < 1e-12
    assert np.abs(out.cpu().numpy() - ref).max() <= 1e-5
    # a caller's squared norms spare the pass and change nothing; a fixed clip
    again = eng.clipped_clustering(gt, sq=sq)
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))
    fixed, finfo = eng.clipped_clustering(gt, clip=0.5 * info['clip'], sq=sq, return_info=True)
    fscales = eng.clip_scales(sq, clip=0.5 * info['clip'])
    fwant = eng.scaled_rows_sum(gt, fscales * on_gpu(torch, eng, mask.astype(np.float64)), count)
    assert torch.equal(fixed.view(torch.int32), fwant.view(torch.int32)) and finfo['clip'] == 0.5 * info['clip']
    fref, _, _ = restated_clipped_clustering(g, clip=0.5 * info['clip'])
    assert np.abs(fixed.cpu().numpy() - fref).max() <= 1e-5


def test_host_entry_point_views_distances_and_a_second_run(eng, torch):
    from attacking_federate_learning_amd import defences
    n, d = 63, 300
    g, f = planted(n, d, seed=363)
    honest = np.arange(f, n)
    gt = on_gpu(torch, eng, g)
    a, ia = eng.clipped_clustering(gt, return_info=True)
    b, ib = eng.clipped_clustering(gt, return_info=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and np.array_equal(ia['admitted_rows'], ib['admitted_rows'])
    assert np.array_equal(ia['admitted_rows'], honest)
    h, ih = eng.clipped_clustering(g, return_info=True)                              # numpy in -> numpy out
    assert isinstance(h, np.ndarray) and np.array_equal(ih['admitted_rows'], honest)
    assert np.array_equal(bits(h), bits(a.cpu().numpy()))                            # the host entry point is the device call
    flat = torch.full((n * (d + 5) + 8,), 3.0, dtype=torch.float32, device=gt.device)
    padded = flat[4:4 + n * (d + 5)].view(n, d + 5)[:, :d]                           # a padded ld
    padded.copy_(gt)
    v, iv = eng.clipped_clustering(padded, return_info=True)
    assert np.array_equal(iv['admitted_rows'], honest) and np.allclose(v.cpu().numpy(), a.cpu().numpy(), rtol=0, atol=1e-5)
    odd = flat[3:3 + n * (d + 5)].view(n, d + 5)[:, :d]                              # and a base 4 bytes off 16
    odd.copy_(gt)
    v, iv = eng.clipped_clustering(odd, return_info=True)
    assert np.array_equal(iv['admitted_rows'], honest) and np.allclose(v.cpu().numpy(), a.cpu().numpy(), rtol=0, atol=1e-5)
    assert torch.equal(defences.clipped_clustering(gt, n, f).view(torch.int32), a.view(torch.int32))
    hv = defences.clipped_clustering(g, n, f)
    assert isinstance(hv, np.ndarray) and np.array_equal(bits(hv), bits(h))
    # `distances=` replaces the cosine stage: the library's own cosine matrix gives the call's bits, the others their own sets
    via, iva = eng.clipped_clustering(gt, distances=eng.cosine_distances(gt), return_info=True)
    assert torch.equal(via.view(torch.int32), a.view(torch.int32)) and np.array_equal(iva['admitted_rows'], honest)
    for handle in (defences._krum_create_distances(gt), defences.manhattan_distances(gt)):
        _, ie = eng.clipped_clustering(gt, distances=handle, return_info=True)
        assert np.array_equal(ie['admitted_rows'], np.flatnonzero(restated_select(handle.numpy())))
        assert np.array_equal(ie['admitted_rows'], honest)
    for method in ('complete', 'single'):
        _, im = eng.clipped_clustering(gt, method=method, return_info=True)
        assert np.array_equal(im['admitted_rows'], np.flatnonzero(restated_select(eng.cosine_distances(gt).numpy(), method)))


# ---- the modes and the edges ------------------------------------------------------------------------------------------------
def test_fixed_adaptive_and_history_modes(eng, torch):
    from attacking_federate_learning_amd import defences
    n, d = 40, 513
    g, f = planted(n, d, seed=40)
    g *= np.linspace(0.5, 3.0, n, dtype=np.float32)[:, None]
    gt = on_gpu(torch, eng, g)
    norms = np.sqrt((g.astype(np.float64) ** 2).sum(1))
    _, adaptive = defences.clipped_clustering(gt, n, f, return_info=True)
    assert abs(adaptive['clip'] / np.median(norms) - 1.0) < 1e-12
    _, fixed = defences.clipped_clustering(gt, n, f, clip=1.25, return_info=True)
    assert fixed['clip'] == 1.25 and np.array_equal(fixed['admitted_rows'], adaptive['admitted_rows'])
    history = [0.5] * 30                                    # an earlier round's norms
    first, one = defences.clipped_clustering(gt, n, f, norm_history=history, return_info=True)
    assert len(history) == 30 + n and np.allclose(history[30:], norms, rtol=1e-12, atol=0)
    assert one['clip'] == float(np.median(np.asarray(history)))
    want = eng.clipped_clustering(gt, clip=one['clip'])
    assert torch.equal(first.view(torch.int32), want.view(torch.int32))
    second, two = defences.clipped_clustering(g, n, f, norm_history=history, max_tau=0.75, return_info=True)
    assert len(history) == 30 + 2 * n and two['clip'] == 0.75 and isinstance(second, np.ndarray)
    ref, _, _ = restated_clipped_clustering(g, clip=0.75)
    assert np.abs(second - ref).max() <= 1e-5
    with pytest.raises(ValueError):
        defences.clipped_clustering(gt, n, f, clip=1.0, norm_history=history)


def test_nobody_or_one_usable_never_gives_nan(eng, torch):
    n, d = 9, 200
    g = np.zeros((n, d), dtype=np.float32)
    out, info = eng.clipped_clustering(on_gpu(torch, eng, g), return_info=True)      # u = 0: nobody
    assert info['admitted'] == 0 and info['usable'] == 0 and len(info['admitted_rows']) == 0
    assert not out.cpu().numpy().any() and info['top_height'] == 0.0
    g[4] = np.random.default_rng(1).standard_normal(d).astype(np.float32)
    out, info = eng.clipped_clustering(on_gpu(torch, eng, g), return_info=True)      # one non-zero row: its cosines need a partner
    assert info['usable'] == 0 and not out.cpu().numpy().any()
    # a finite entry makes BOTH its rows usable, so one usable row cannot be built; two usable rows are one against one, a tie
    # that goes to the lower row, and the call then admits exactly one row
    c = np.full((n, n), INF, dtype=np.float32)
    c[6, 2] = np.float32(0.25)
    flags, sinfo = eng.clipped_clustering_select(c)
    assert sinfo['usable'] == 2 and flags.tolist() == [2]                             # a tie of one against one: the lowest row
    g = np.random.default_rng(2).standard_normal((n, d)).astype(np.float32)
    g[3] = np.nan
    out, info = eng.clipped_clustering(on_gpu(torch, eng, g), distances=c, return_info=True)
    assert info['admitted'] == 1 and np.isfinite(out.cpu().numpy()).all()
    want, _, _ = restated_clipped_clustering(g, dist=c)
    assert np.abs(out.cpu().numpy() - want).max() <= 1e-5
    # L = 0 with usable rows cannot happen (the larger cluster is never empty); L = 0 through non-finite rows alone
    g[:] = np.nan
    out = eng.clipped_clustering(on_gpu(torch, eng, g))
    assert not out.cpu().numpy().any()


def test_refusals_write_nothing(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    n, d = 20, 64
    g, _ = planted(n, d, seed=1)
    gt = on_gpu(torch, eng, g)
    dev = gt.device
    guard = 16
    out = torch.full((d + 2 * guard,), -3.0, dtype=torch.float32, device=dev)
    flags = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device=dev)
    pair = torch.full((2 * n + 2 * guard,), -7, dtype=torch.int32, device=dev)
    height = torch.full((n + 2 * guard,), -3.0, dtype=torch.float64, device=dev)
    dist = on_gpu(torch, eng, restated_cosine(g).astype(np.float32))
    two = ctypes.c_double(2.0)

    def whole(clip=0.0, adaptive=1, method=0, fill=2.0, rows=n, out_ptr=None):
        params = _native.ClippedClusteringParams(clip, adaptive, method, fill)
        return eng.lib.byz_clipped_clustering_dev(eng.ctx, _vp(gt.data_ptr()), rows, d, d, ctypes.byref(params), None, None,
                                                  _vp(out.data_ptr() + 4 * guard if out_ptr is None else out_ptr),
                                                  _vp(flags.data_ptr() + 4 * guard), None)

    def link(rows=n, method=0, fill=two):
        return eng.lib.byz_linkage_dev(eng.ctx, _vp(dist.data_ptr()), rows, method, ctypes.byref(fill) if fill is not None else None,
                                       _vp(pair.data_ptr() + 4 * guard), _vp(height.data_ptr() + 8 * guard),
                                       _vp(flags.data_ptr() + 4 * guard), None, None)

    def select(rows=n, method=0, fill=two):
        return eng.lib.byz_clipped_clustering_select_dev(eng.ctx, _vp(dist.data_ptr()), rows, method, ctypes.byref(fill),
                                                         _vp(flags.data_ptr() + 4 * guard), None)
    assert whole(rows=1) == _native.E_INVALID
    assert whole(rows=16385) == _native.E_UNSUPPORTED
    assert whole(method=3) == _native.E_INVALID and whole(method=-1) == _native.E_INVALID
    assert whole(fill=-1.0) == _native.E_INVALID and whole(fill=float('nan')) == _native.E_INVALID
    assert whole(fill=float('inf')) == _native.E_INVALID
    assert whole(adaptive=0, clip=0.0) == _native.E_INVALID and whole(adaptive=0, clip=float('nan')) == _native.E_INVALID
    assert whole(out_ptr=gt.data_ptr() + 4 * (d - 1)) == _native.E_INVALID            # out overlaps G
    assert link(rows=1) == _native.E_INVALID and link(rows=16385) == _native.E_UNSUPPORTED
    assert link(method=7) == _native.E_INVALID and link(fill=ctypes.c_double(-0.5)) == _native.E_INVALID
    assert link(fill=ctypes.c_double(float('inf'))) == _native.E_INVALID and link(fill=None) == _native.E_INVALID
    assert select(rows=1) == _native.E_INVALID and select(rows=16385) == _native.E_UNSUPPORTED
    assert select(method=3) == _native.E_INVALID and select(fill=ctypes.c_double(float('nan'))) == _native.E_INVALID
    assert eng.lib.byz_linkage_cut_dev(eng.ctx, _vp(pair.data_ptr()), n, _vp(flags.data_ptr()), 0, _vp(flags.data_ptr() + 4 * guard),
                                       _vp(pair.data_ptr() + 4 * guard), None) == _native.E_INVALID
    assert eng.lib.byz_linkage_cut_dev(eng.ctx, _vp(pair.data_ptr()), n, _vp(flags.data_ptr()), n + 1,
                                       _vp(flags.data_ptr() + 4 * guard), _vp(pair.data_ptr() + 4 * guard), None) == _native.E_INVALID
    eng.synchronize()
    assert (out == -3.0).all() and (flags == -7).all() and (pair == -7).all() and (height == -3.0).all()
    assert torch.equal(gt, on_gpu(torch, eng, g))
    with pytest.raises(ValueError):
        eng.clipped_clustering(gt, method='ward')
    with pytest.raises(ValueError):
        eng.clipped_clustering(gt, clip=0.0)
    with pytest.raises(ValueError):
        eng.linkage(np.zeros((4, 5), dtype=np.float32))
    # the accepted call writes inside its arrays only
    assert whole() == _native.OK and link() == _native.OK
    eng.synchronize()
    assert (out[:guard] == -3.0).all() and (out[-guard:] == -3.0).all() and (out[guard:-guard] != -3.0).all()
    assert (flags[:guard] == -7).all() and (flags[guard + n:] == -7).all()
    assert (pair[:guard] == -7).all() and (pair[guard + 2 * (n - 1):] == -7).all() and (pair[guard:guard + 2 * (n - 1)] >= 0).all()
    assert (height[:guard] == -3.0).all() and (height[guard + n - 1:] == -3.0).all()


def test_three_rounds_through_the_device_server(eng, torch):
    from attacking_federate_learning_amd.server import DeviceServer
    n, d = 20, 640
    weights = np.random.default_rng(51).standard_normal(d).astype(np.float32)
    dev = 'cuda:%d' % eng.device
    server = DeviceServer(n, weights, 0.25, 0.1, 0.9, torch_device=dev, engine=eng)
    assert server.clipped_clustering_norms == []
    seen = []
    for rnd in range(3):
        g, f = planted(n, d, seed=100 + rnd)
        g *= np.float32(1.0 + rnd)
        gt = on_gpu(torch, eng, g)
        server.users_grads.data.copy_(gt)
        step = server.defend_clipped_clustering()
        seen.extend(np.sqrt((g.astype(np.float64) ** 2).sum(1)).tolist())
        assert len(server.clipped_clustering_norms) == n * (rnd + 1)                 # the history carries over
        assert np.allclose(server.clipped_clustering_norms, seen, rtol=1e-12, atol=0)
        clip = float(np.median(np.asarray(server.clipped_clustering_norms)))
        want, info = eng.clipped_clustering(gt, clip=clip, return_info=True)
        assert torch.equal(step.view(torch.int32), want.view(torch.int32))
        assert not (info['admitted_rows'] < f).any() and info['admitted'] == n - f    # the planted attackers are never admitted
