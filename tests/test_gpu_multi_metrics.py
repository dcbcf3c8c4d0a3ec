"""Multi-Metrics on an MI355X, held to the numpy restatement of tests/test_multi_metrics.py.

The Manhattan matrix is held to the fp64 sums within the bound the kernel's header derives, (K + 2) * 2^-24 with K =
BYZ_MANHATTAN_CHAIN -- never a measured number.  The features are held to numpy on the three device matrices read back (1e-12
relative: fp64 sums of the same float32 entries in another association).  The selection is compared EXACTLY with the restatement
run on the very features the device selected on (crafted ones, or the device's own read back), each case first shown on the CPU
to have a relative score gap above 1e-9 at the keep boundary; the scores within 1e-9 relative."""
import ctypes

import numpy as np
import pytest

from tests.test_flame import restated_flame_select
from tests.test_multi_metrics import (PLANTED_SHAPES, boundary_gap, planted, restated_aggregate, restated_features, restated_manhattan,
                                      restated_select, usable_from_cosine, usable_rows)

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
INF_BITS = np.float32(np.inf).view(np.uint32)


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:%d' % eng.device)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def manhattan_bound():
    from attacking_federate_learning_amd import _native
    return (_native.MANHATTAN_CHAIN + 2) * 2.0 ** -24


def offset_view(torch, eng, g, pad):
    """g behind a base pointer one float off a 16-byte boundary and rows `pad` floats apart from dense."""
    n, d = g.shape
    flat = torch.full((n * (d + pad) + 1,), 7.0, dtype=torch.float32, device='cuda:%d' % eng.device)
    view = flat[1:1 + n * (d + pad)].view(n, d + pad)[:, :d]
    view.copy_(on_gpu(torch, eng, g))
    assert view.stride(0) == d + pad and view.data_ptr() % 16 == 4
    return view


def check_manhattan(got, g):
    n = g.shape[0]
    exact = restated_manhattan(g, exact=True)
    assert got.dtype == np.float32 and got.shape == (n, n)
    assert np.array_equal(bits(got), bits(got.T))                                   # symmetric as bits
    assert np.array_equal(bits(np.diagonal(got)), np.full(n, INF_BITS))             # diagonal +inf
    finite = np.isfinite(exact)
    assert np.array_equal(np.isfinite(got), finite)
    assert np.array_equal(bits(got[~finite]), np.full(int((~finite).sum()), INF_BITS))
    if finite.any():
        err = np.abs(got[finite].astype(np.float64) - exact[finite])
        worst = float(np.max(err / np.maximum(exact[finite], 1e-300)))
        print('manhattan %dx%d: worst relative error %.3g, %.3f of the bound %.3g' % (n, g.shape[1], worst, worst / manhattan_bound(),
                                                                                    manhattan_bound()))
        assert (err <= manhattan_bound() * exact[finite]).all()
    return exact


# ---- the Manhattan matrix -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 7, 257, 4099])
@pytest.mark.parametrize('n', [2, 3, 33, 65, 130])
def test_manhattan_matrix_against_fp64(eng, torch, n, d):
    g = np.random.default_rng(n * 10000 + d).standard_normal((n, d)).astype(np.float32)
    g *= np.linspace(0.5, 3.0, n, dtype=np.float32)[:, None]
    check_manhattan(eng.manhattan_distances(on_gpu(torch, eng, g)).numpy(), g)


def test_manhattan_long_chains_and_several_column_chunks(eng, torch):
    g = np.random.default_rng(200003).standard_normal((8, 200003)).astype(np.float32)
    check_manhattan(eng.manhattan_distances(on_gpu(torch, eng, g)).numpy(), g)


def test_manhattan_broken_rows_are_inf_and_a_zero_row_is_finite(eng, torch):
    n, d = 37, 300
    g = np.random.default_rng(37).standard_normal((n, d)).astype(np.float32)
    g[1, 150] = np.nan
    g[4, 7] = np.inf
    g[9, 299] = -np.inf
    g[20] = 3e38
    g[21] = -3e38
    g[30] = 0.0
    got = eng.manhattan_distances(on_gpu(torch, eng, g)).numpy()
    check_manhattan(got, g)
    for r in (1, 4, 9, 20, 21):
        assert np.array_equal(bits(got[r]), np.full(n, INF_BITS)) and np.array_equal(bits(got[:, r]), np.full(n, INF_BITS))
    others = np.setdiff1d(np.arange(n), [1, 4, 9, 20, 21, 30])
    assert np.isfinite(got[30, others]).all() and np.isfinite(got[others, 30]).all()


@pytest.mark.parametrize('n,d', [(33, 257), (130, 4099), (8, 70001)])
def test_manhattan_views_and_reruns_give_the_same_bits(eng, torch, n, d):
    g = np.random.default_rng(n + d).standard_normal((n, d)).astype(np.float32)
    dense = on_gpu(torch, eng, g)
    want = eng.manhattan_distances(dense).numpy()
    assert np.array_equal(bits(eng.manhattan_distances(dense).numpy()), bits(want))                       # two runs
    assert np.array_equal(bits(eng.manhattan_distances(offset_view(torch, eng, g, 3)).numpy()), bits(want))     # ld > d, base + 1 float
    assert np.array_equal(bits(eng.manhattan_distances(offset_view(torch, eng, g, 0)).numpy()), bits(want))     # base + 1 float alone
    wide = torch.full((n, d + 5), 7.0, dtype=torch.float32, device=dense.device)
    wide[:, :d] = dense
    assert np.array_equal(bits(eng.manhattan_distances(wide[:, :d]).numpy()), bits(want))                 # ld > d alone
    assert np.array_equal(bits(eng.manhattan_distances(g).numpy()), bits(want))                            # a host matrix
    # the two halves, as the columns layout calls them
    again = eng.manhattan_from_sums(eng.manhattan_sums(dense)).numpy()
    assert np.array_equal(bits(again), bits(want))


def test_manhattan_beyond_the_row_limit_is_refused_and_nothing_is_written(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    n = 16385
    dev = 'cuda:%d' % eng.device
    g = torch.zeros((n, 1), dtype=torch.float32, device=dev)
    dist = torch.full((64,), -3.0, dtype=torch.float32, device=dev)
    sums = torch.full((64,), -3.0, dtype=torch.float64, device=dev)
    flags = torch.full((64,), -7, dtype=torch.int32, device=dev)
    assert eng.lib.byz_manhattan_distances_dev(eng.ctx, _vp(g.data_ptr()), n, 1, 1, _vp(dist.data_ptr()), None) == _native.E_UNSUPPORTED
    assert eng.lib.byz_manhattan_sums_dev(eng.ctx, _vp(g.data_ptr()), n, 1, 1, _vp(sums.data_ptr()), None) == _native.E_UNSUPPORTED
    assert eng.lib.byz_manhattan_from_sums_dev(eng.ctx, _vp(sums.data_ptr()), n, _vp(dist.data_ptr()), None) == _native.E_UNSUPPORTED
    assert eng.lib.byz_multi_metrics_features_dev(eng.ctx, _vp(dist.data_ptr()), _vp(dist.data_ptr()), _vp(dist.data_ptr()), n,
                                                  _vp(sums.data_ptr()), None) == _native.E_UNSUPPORTED
    assert eng.lib.byz_multi_metrics_select_dev(eng.ctx, _vp(sums.data_ptr()), n, 5, _vp(flags.data_ptr()), None, None) == _native.E_UNSUPPORTED
    assert eng.lib.byz_multi_metrics_dev(eng.ctx, _vp(g.data_ptr()), n, 1, 1, 5, _vp(dist.data_ptr()), _vp(flags.data_ptr()),
                                         None) == _native.E_UNSUPPORTED
    eng.synchronize()
    assert (dist == -3.0).all() and (sums == -3.0).all() and (flags == -7).all()
    with pytest.raises(NotImplementedError):
        eng.manhattan_distances(g)


# ---- as a `distances=` argument ---------------------------------------------------------------------------------------------
def restated_krum_index(dist, users_count, corrupted_count):
    """The reference's Krum on a dense matrix: the row whose users_count - corrupted_count smallest distances sum least."""
    n = dist.shape[0]
    scores = []
    for i in range(n):
        row = np.sort(np.delete(dist[i], i).astype(np.float64))
        scores.append(row[:users_count - corrupted_count].sum())
    return scores


def test_manhattan_as_the_distances_of_krum_and_flame(eng, torch):
    n, f, d = 33, 8, 1000
    g = planted(n, d, f, seed=3)
    gt = on_gpu(torch, eng, g)
    man = eng.manhattan_distances(gt)
    dense = man.numpy()
    idx = eng.krum(gt, n, f, distances=man, return_index=True)
    scores = restated_krum_index(dense, n, f)
    order = np.argsort(scores)
    assert scores[order[1]] - scores[order[0]] > 1e-5 * scores[order[0]]            # the winner is clear of the fp32 row sums
    assert idx == int(order[0]) and idx < n - f
    rows, info = eng.flame_select(man)
    mask, _ = restated_flame_select(dense, n // 2 + 1, 1)
    assert np.array_equal(rows, np.flatnonzero(mask)) and info['admitted'] == int(mask.sum())


# ---- the features -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', [(5, 40), (65, 513), (300, 64)])
def test_features_against_numpy_on_the_matrices_read_back(eng, torch, n, d):
    g = np.random.default_rng(n + 7 * d).standard_normal((n, d)).astype(np.float32)
    g[1] = 0.0
    g[n - 2, d // 2] = np.nan
    gt = on_gpu(torch, eng, g)
    man, euc, cos = eng.manhattan_distances(gt), eng.pairwise_distances(gt), eng.cosine_distances(gt)
    got = eng.multi_metrics_features(man, euc, cos)
    m, e, c = man.numpy(), euc.numpy(), cos.numpy()
    usable = usable_from_cosine(c)
    assert np.array_equal(usable, usable_rows(g)) and usable.sum() == n - 2
    want = restated_features(m, e, c, usable)
    assert got.dtype == np.float64 and got.shape == (n, 3)
    assert np.isinf(got[[1, n - 2]]).all() and np.array_equal(np.isfinite(got), np.isfinite(want))
    ok = np.isfinite(want)
    assert (np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok])).all()
    # dense matrices are taken as well as handles
    again = eng.multi_metrics_features(m, e, c)
    assert np.array_equal(again, got)
    with pytest.raises(ValueError):
        eng.multi_metrics_features(man, euc, {0: {1: 1.0}})


# ---- the selection on given features ------------------------------------------------------------------------------------------
def check_select(eng, x, keep, tie=False):
    flags, scores, info = restated_select(x, keep)
    gap = boundary_gap(scores, flags)
    assert (gap == 0.0) if tie else (gap > 1e-9), gap      # (a tie at the boundary is decided by the row index, exactly)
    rows, got_scores, got_info = eng.multi_metrics_select(x, keep, return_scores=True)
    assert np.array_equal(rows, np.flatnonzero(flags))
    usable = np.isfinite(scores)
    assert np.array_equal(np.isfinite(got_scores), usable) and not np.isnan(got_scores).any()
    assert (np.abs(got_scores[usable] - scores[usable]) <= 1e-9 * np.abs(scores[usable])).all()
    assert got_info['kept'] == info['kept'] and got_info['usable'] == info['usable'] and got_info['degenerate'] == info['degenerate']
    if not info['degenerate']:
        assert abs(got_info['det'] - info['det']) <= 1e-9 * abs(info['det'])
    return flags, scores, info


def correlated_features(n, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, 3)) @ np.array([[1.0, 0.6, 0.3], [0.0, 0.8, 0.4], [0.0, 0.0, 0.5]])
    return base * [300.0, 20.0, 0.05] + [5000.0, 400.0, 0.9]


@pytest.mark.parametrize('n,keep,seed', [(4, 1, 0), (33, 9, 1), (257, 77, 2), (1025, 1025, 3), (5000, 1500, 4)])
def test_select_equals_the_restatement(eng, n, keep, seed):
    x = correlated_features(n, seed)
    if n >= 33:
        x[[2, n - 1]] = np.inf
        x[5, 1] = np.nan
    _, _, info = check_select(eng, x, keep)
    assert info['degenerate'] == 0 and info['usable'] == (n - 3 if n >= 33 else n)


def test_select_degenerate_cases_and_ties(eng):
    few = np.full((6, 3), np.inf)
    few[[1, 3, 4]] = [[5.0, 1.0, 0.1], [2.0, 9.0, 0.9], [3.0, 0.5, 0.5]]
    flags, _, info = check_select(eng, few, 2)
    assert info['degenerate'] == 1 and np.array_equal(np.flatnonzero(flags), [3, 4])
    constant = correlated_features(12, 8)
    constant[:, 1] = 0.1
    _, _, info = check_select(eng, constant, 4)
    assert info['degenerate'] == 1
    identical = np.tile([[0.0, 0.0, 0.0]], (10, 1))
    flags, _, info = check_select(eng, identical, 3, tie=True)
    assert info['degenerate'] == 1 and np.array_equal(np.flatnonzero(flags), [0, 1, 2])
    a = np.random.default_rng(9).standard_normal(20)
    singular = np.stack([a, 2.0 * a + 1.0, np.random.default_rng(10).standard_normal(20)], axis=1)
    _, _, info = check_select(eng, singular, 5)
    assert info['degenerate'] == 1
    nobody = np.full((7, 3), np.inf)
    flags, _, info = check_select(eng, nobody, 3)
    assert info['usable'] == 0 and info['kept'] == 0 and not flags.any()
    tied = correlated_features(9, 11)
    tied[6] = tied[2]
    tied[7] = tied[2]
    _, scores, _ = restated_select(tied, 9)
    order = np.lexsort((np.arange(9), scores))
    position = int(np.flatnonzero(order == 2)[0])
    for keep in (position + 1, position + 2):              # the boundary falls inside the tie: the lower rows win it
        flags, _, _ = check_select(eng, tied, keep, tie=True)
        assert flags[2] == 1 and flags[7] == 0


def test_select_at_the_row_limit_chooses_the_last_row(eng):
    n = 16384
    x = correlated_features(n, 16384)
    scores = restated_select(x, n)[1]
    best = int(np.argmin(scores))
    x[[best, n - 1]] = x[[n - 1, best]]                    # the smallest score sits in the last row
    flags, _, info = check_select(eng, x, 4915)
    assert flags[n - 1] == 1 and info['kept'] == 4915 and info['degenerate'] == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def own_features(eng, gt, g):
    """The restatement's features from the device's OWN three matrices read back (what the whole call selects on)."""
    m, e, c = eng.manhattan_distances(gt).numpy(), eng.pairwise_distances(gt).numpy(), eng.cosine_distances(gt).numpy()
    return restated_features(m, e, c, usable_rows(g))


@pytest.mark.parametrize('n,d,f', PLANTED_SHAPES)
def test_multi_metrics_chooses_the_restatement_of_its_own_features_and_averages_them(eng, torch, n, d, f):
    g = planted(n, d, f, seed=n)
    gt = on_gpu(torch, eng, g)
    out, info = eng.multi_metrics(gt, p=0.3, return_info=True)
    x = own_features(eng, gt, g)
    flags, scores, want = restated_select(x, int(0.3 * n))
    assert boundary_gap(scores, flags) > 1e-9
    assert np.array_equal(info['chosen_rows'], np.flatnonzero(flags))
    assert info['kept'] == want['kept'] == int(0.3 * n) and info['usable'] == n and info['degenerate'] == 0
    assert not (info['chosen_rows'] >= n - f).any()                                  # no planted attacker is chosen
    assert np.array_equal(bits(out.cpu().numpy()), bits(np.mean(g[info['chosen_rows']], axis=0)))
    assert np.array_equal(bits(out.cpu().numpy()), bits(restated_aggregate(g, flags)))


def test_broken_rows_are_never_chosen_and_nobody_usable_gives_zeros(eng, torch):
    n, d = 20, 300
    g = planted(n, d, 4, seed=2)
    g[0] = 0.0
    g[5, 17] = np.nan
    g[9, 3] = -np.inf
    gt = on_gpu(torch, eng, g)
    out, info = eng.multi_metrics(gt, p=1.0, return_info=True)
    assert info['usable'] == 17 and info['kept'] == 17
    assert np.array_equal(info['chosen_rows'], np.setdiff1d(np.arange(n), [0, 5, 9]))
    assert np.array_equal(bits(out.cpu().numpy()), bits(np.mean(g[info['chosen_rows']], axis=0)))
    zeros = torch.zeros((6, 10), dtype=torch.float32, device=gt.device)
    out, info = eng.multi_metrics(zeros, p=0.5, return_info=True)
    assert info['usable'] == 0 and info['kept'] == 0 and len(info['chosen_rows']) == 0
    assert np.array_equal(bits(out.cpu().numpy()), np.zeros(10, dtype=np.uint32))
    lone = np.zeros((5, 12), dtype=np.float32)             # one usable row: it has nobody to be compared with and is the mean
    lone[3] = np.arange(12, dtype=np.float32) + 1.0
    out, info = eng.multi_metrics(on_gpu(torch, eng, lone), p=0.5, return_info=True)
    assert info['usable'] == 1 and info['kept'] == 1 and info['degenerate'] == 1 and np.array_equal(info['chosen_rows'], [3])
    assert np.array_equal(out.cpu().numpy(), lone[3])


def test_repeatability_host_entry_point_and_a_strided_view(eng, torch):
    from attacking_federate_learning_amd import defences
    n, d, f = 33, 1000, 8
    g = planted(n, d, f, seed=5)
    gt = on_gpu(torch, eng, g)
    want, winfo = eng.multi_metrics(gt, return_info=True)
    again, ainfo = eng.multi_metrics(gt, return_info=True)
    assert torch.equal(want.view(torch.int32), again.view(torch.int32)) and np.array_equal(winfo['chosen_rows'], ainfo['chosen_rows'])
    host, hinfo = eng.multi_metrics(g, return_info=True)                              # numpy in -> numpy out
    assert isinstance(host, np.ndarray) and np.array_equal(hinfo['chosen_rows'], winfo['chosen_rows'])
    assert np.array_equal(bits(host), bits(want.cpu().numpy()))
    view, vinfo = eng.multi_metrics(offset_view(torch, eng, g, 3), return_info=True)
    assert np.array_equal(vinfo['chosen_rows'], winfo['chosen_rows']) and np.array_equal(bits(view.cpu().numpy()), bits(want.cpu().numpy()))
    assert np.array_equal(bits(defences.multi_metrics(g, n, f)), bits(host))
    assert np.array_equal(bits(defences.manhattan_distances(g).numpy()), bits(eng.manhattan_distances(gt).numpy()))


def test_two_rounds_through_the_device_server(eng, torch):
    from attacking_federate_learning_amd.server import DeviceServer
    n, d, f = 33, 640, 8
    weights = np.random.default_rng(51).standard_normal(d).astype(np.float32)
    dev = 'cuda:%d' % eng.device
    server = DeviceServer(n, weights, 0.25, 0.1, 0.9, torch_device=dev, engine=eng)
    twin_weights, twin_velocity = server.current_weights.clone(), server.velocity.clone()
    for rnd in (0, 1):
        g = planted(n, d, f, seed=60 + rnd)
        gt = on_gpu(torch, eng, g)
        server.users_grads.data.copy_(gt)
        step = server.defend_multi_metrics(p=0.3)
        want, info = eng.multi_metrics(gt, p=0.3, return_info=True)
        assert torch.equal(step.view(torch.int32), want.view(torch.int32)) and not (info['chosen_rows'] >= n - f).any()
        eng.server_update(twin_weights, twin_velocity, want, 0.9, 0.1)                # the same momentum step on a twin
        assert torch.equal(server.current_weights.view(torch.int32), twin_weights.view(torch.int32))
    assert not torch.equal(server.current_weights.cpu(), torch.from_numpy(weights))


def test_invalid_arguments_are_refused_and_nothing_is_written(eng, torch):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _vp
    n, d = 20, 64
    g = planted(n, d, 4, seed=1)
    gt = on_gpu(torch, eng, g)
    out = torch.full((d,), -3.0, dtype=torch.float32, device=gt.device)
    flags = torch.full((n,), -7, dtype=torch.int32, device=gt.device)
    feat = torch.zeros((n, 3), dtype=torch.float64, device=gt.device)

    def call(keep=6, out_ptr=None, rows=n, ld=d, g_ptr=None):
        return eng.lib.byz_multi_metrics_dev(eng.ctx, _vp(gt.data_ptr() if g_ptr is None else g_ptr), rows, d, ld, keep,
                                             _vp(out.data_ptr() if out_ptr is None else out_ptr), _vp(flags.data_ptr()), None)
    assert call(keep=0) == _native.E_INVALID
    assert call(keep=21) == _native.E_INVALID
    assert call(keep=-1) == _native.E_INVALID
    assert call(ld=d - 1) == _native.E_INVALID
    assert call(rows=0) == _native.E_INVALID
    assert call(out_ptr=gt.data_ptr() + 4 * (d - 1)) == _native.E_INVALID            # out overlaps G
    assert eng.lib.byz_multi_metrics_dev(eng.ctx, _vp(gt.data_ptr()), n, d, d, 6, None, _vp(flags.data_ptr()), None) == _native.E_INVALID
    assert eng.lib.byz_multi_metrics_dev(eng.ctx, None, n, d, d, 6, _vp(out.data_ptr()), _vp(flags.data_ptr()), None) == _native.E_INVALID
    assert eng.lib.byz_multi_metrics_select_dev(eng.ctx, _vp(feat.data_ptr()), n, 0, _vp(flags.data_ptr()), None, None) == _native.E_INVALID
    assert eng.lib.byz_multi_metrics_select_dev(eng.ctx, _vp(feat.data_ptr()), n, n + 1, _vp(flags.data_ptr()), None, None) == _native.E_INVALID
    assert eng.lib.byz_multi_metrics_select_dev(eng.ctx, None, n, 3, _vp(flags.data_ptr()), None, None) == _native.E_INVALID
    assert eng.lib.byz_multi_metrics_select_dev(eng.ctx, _vp(feat.data_ptr()), n, 3, None, None, None) == _native.E_INVALID
    assert eng.lib.byz_manhattan_distances_dev(eng.ctx, _vp(gt.data_ptr()), n, d, d, None, None) == _native.E_INVALID
    eng.synchronize()
    assert (out == -3.0).all() and (flags == -7).all() and torch.equal(gt, on_gpu(torch, eng, g))
    for p in (1.5, 0.0, 0.01, float('nan')):
        with pytest.raises(ValueError):
            eng.multi_metrics(gt, p=p)
    with pytest.raises(ValueError):
        eng.multi_metrics_select(np.zeros((4, 2)), 1)
    with pytest.raises(ValueError):
        eng.multi_metrics_select(np.zeros((4, 3)), 5)
    assert call() == _native.OK
    eng.synchronize()
    assert (flags != -7).all() and int(flags.sum().item()) == 6
