"""The attacks of Fang et al. on an MI355X, held to the numpy restatement of tests/test_fang.py.

Every comparison is exact, bits as integers: the column means are no_defense's chain, the extremes a chain of comparisons, the
draw and the Krum attack's distances single IEEE operations in a stated order (fang.hip is built with -ffp-contract=off, and
fp64 sqrt and division are correctly rounded on the device as in numpy).  Two things are NOT the restatement's to state and are
taken from the device: row_dots' t and q (fp64 sums in the kernel's own order, held to numpy's at test_gpu_fltrust.py's bound
d 2^-53 sum |x| |s|) and the benign rows' distance block (pairwise_distances, held to its own tests); given those, the matrix of
every step, lambda_0, the sequence of lambdas, the step count and the index Krum chose are the restatement's."""
import functools

import numpy as np
import pytest

from tests import views_arena
from tests.test_fang import (bits, cpu_krum, krum_case, rank_trimmed_mean_f64, restated_column_extremes, restated_fang_krum,
                             restated_fang_trmean, restated_krum_matrix, restated_mean, restated_sign, seeded)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.array(a, order='C')).to('cuda:%d' % eng.device)          # (a copy: a cached case is read-only)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def attackers_for(n):
    return sorted({0, min(1, n), n - 1})


@functools.lru_cache(maxsize=None)
def walk_case(n, d):
    """A matrix with every kind of value the rule names (computed once, never written to): a NaN among the benign rows, a column
    whose benign rows hold no number, an infinity, and a -0.0."""
    g = views_arena.gaussian(21000 + 37 * n + d % 1013, n, d)
    if d >= 5:
        g[n - 1, 1] = np.nan
        g[:, 2] = np.nan
        g[n - 1, 3] = np.inf
        g[0, 4] = -0.0
    g.setflags(write=False)
    return g


def check_extremes(eng, torch, view, g, c, what):
    got = [v.cpu().numpy() for v in eng.column_extremes(view, c)]
    want = restated_column_extremes(g, c)
    for name, a, b in zip(('mean', 'lo', 'hi'), got, want):
        assert same(a, b), (what, name, c, np.flatnonzero(bits(a) != bits(b))[:8])


# ---- column_extremes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 7, 8, 9, 17])
@pytest.mark.parametrize('d', [1, 3, 5, 255, 257, 1025])
def test_column_extremes_are_numpys_bits(eng, torch, n, d):
    g = walk_case(n, d)
    gt = on_gpu(torch, eng, g)
    for c in attackers_for(n):
        check_extremes(eng, torch, gt, g, c, 'dense')
    assert same(eng.column_extremes(gt, 0)[0].cpu().numpy(), eng.no_defense(gt).cpu().numpy())


@pytest.mark.parametrize('variant', views_arena.VARIANTS)
@pytest.mark.parametrize('n, d', [(9, 257), (17, 1025), (8, 5)])
def test_column_extremes_on_padded_and_misaligned_views(eng, torch, variant, n, d):
    """ld > n_cols (a multiple of 4 and not), the base one float off 16-byte alignment: the guard bands stay as they were."""
    g = walk_case(n, d)
    view, flat = views_arena.arena_variant(torch, g, variant, device='cuda:%d' % eng.device)
    before = flat.clone()
    for c in attackers_for(n):
        check_extremes(eng, torch, view, g, c, variant)
    views_arena.untouched(torch, flat, view, before)
    assert torch.equal(flat.view(torch.int32), before.view(torch.int32))         # the matrix itself is only read


def test_column_extremes_four_wide_with_its_tail(eng, torch):
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    n, d = 9, 4 * 256 * cus * 2 + 5
    g = views_arena.gaussian(22001, n, d)
    g[5, d - 2] = np.nan
    gt = on_gpu(torch, eng, g)
    assert gt.data_ptr() % 16 == 0
    view, flat = views_arena.arena(torch, g, views_arena.even_ld(d), 0, device='cuda:%d' % eng.device)   # aligned, ld % 4 == 0, a ragged tail
    before = flat.clone()
    for c in (0, 1, n - 1):
        check_extremes(eng, torch, gt, g, c, 'wide')
    check_extremes(eng, torch, view, g, 2, 'wide, padded')
    views_arena.untouched(torch, flat, view, before)


# ---- the trimmed-mean attack ---------------------------------------------------------------------------------------------------
TRMEAN_SHAPES = [(9, 3, 1), (9, 3, 5), (20, 4, 64), (17, 16, 257), (12, 1, 1027)]


@pytest.mark.parametrize('partial', [False, True])
@pytest.mark.parametrize('n, c, d', TRMEAN_SHAPES)
def test_trmean_attack_is_the_restatement(eng, torch, partial, n, c, d):
    g = np.array(walk_case(n, d)) if d >= 5 else seeded(23000 + d, n, d)
    want = restated_fang_trmean(g, c, partial=partial, seed=(1 << 63) + 12345, round=7, column_offset=2)
    for variant in (None,) + views_arena.VARIANTS:
        if variant is None:
            view = flat = on_gpu(torch, eng, g)
            before = None
        else:
            view, flat = views_arena.arena_variant(torch, g, variant, device='cuda:%d' % eng.device)
            before = flat.clone()
        rows = eng.fang_trmean_attack(view, c, partial=partial, seed=(1 << 63) + 12345, round=7, column_offset=2)
        got = view.cpu().numpy()
        assert same(got[:c], want[:c]), (variant, np.argwhere(bits(got[:c]) != bits(want[:c]))[:8])
        assert same(got[c:], g[c:])                                              # the benign rows are untouched
        assert rows.data_ptr() == view.data_ptr() and tuple(rows.shape) == (c, d)
        if before is not None:
            before.as_strided((c, d), (view.stride(0), 1), view.storage_offset()).copy_(view[:c])
            assert torch.equal(flat.view(torch.int32), before.view(torch.int32))     # guard bands, padding and benign rows: as before
    # a host matrix: left alone, the attacked rows come back
    host = g.copy()
    assert same(eng.fang_trmean_attack(host, c, partial=partial, seed=(1 << 63) + 12345, round=7, column_offset=2), want[:c])
    assert same(host, g)


@pytest.mark.parametrize('partial', [False, True])
def test_trmean_attack_repeats_itself_and_moves_with_seed_and_round(eng, torch, partial):
    g, c = seeded(24001, 20, 1025), 4

    def run(**kw):
        gt = on_gpu(torch, eng, g)
        eng.fang_trmean_attack(gt, c, partial=partial, **kw)
        return gt.cpu().numpy()[:c]
    first = run(seed=5, round=9)
    assert same(first, run(seed=5, round=9))
    assert same(first, restated_fang_trmean(g, c, partial=partial, seed=5, round=9)[:c])
    assert (bits(first) != bits(run(seed=5, round=10))).mean() > 0.99
    assert (bits(first) != bits(run(seed=6, round=9))).mean() > 0.99
    assert len({first[i].tobytes() for i in range(c)}) == c                      # every attacker row its own draws


@pytest.mark.parametrize('partial', [False, True])
@pytest.mark.parametrize('k', [1, 2, 3, 5])
def test_a_column_slice_with_its_offset_is_the_slice_of_the_one_call(eng, torch, partial, k):
    g, c = seeded(24002, 12, 261), 3
    whole = on_gpu(torch, eng, g)
    eng.fang_trmean_attack(whole, c, partial=partial, seed=3, round=1, column_offset=8)
    part = on_gpu(torch, eng, g)[:, k:]
    eng.fang_trmean_attack(part, c, partial=partial, seed=3, round=1, column_offset=8 + k)
    assert same(part.cpu().numpy(), whole.cpu().numpy()[:, k:])
    assert same(whole.cpu().numpy(), restated_fang_trmean(g, c, partial=partial, seed=3, round=1, column_offset=8))


def test_trmean_attack_in_place_on_a_device_server(eng, torch):
    from attacking_federate_learning_amd.server import DeviceServer

    class User:
        def __init__(self, grads):
            self.grads = grads
    n, c, d = 20, 4, 300
    g = seeded(24003, n, d)
    server = DeviceServer(n, np.zeros(d, dtype=np.float32), 0.2, 0.1, 0.9, torch_device='cuda:%d' % eng.device, engine=eng)
    assert server.fang_round == 0 and server.attack_fang_trimmed_mean(0) is None and server.fang_round == 0
    for rnd, partial in ((0, False), (1, False), (2, True)):
        server.collect_gradients([User(row) for row in g])
        rows = server.attack_fang_trimmed_mean(c, partial=partial, seed=77)
        assert server.fang_round == rnd + 1
        assert rows.data_ptr() == server.users_grads.data.data_ptr()
        assert same(server.users_grads.data.cpu().numpy(), restated_fang_trmean(g, c, partial=partial, seed=77, round=rnd))


def test_the_trimmed_mean_of_the_devices_attacked_matrix_only_moves_the_attackers_way(eng, torch):
    """tests/test_fang.py's property, on what the device wrote, in fp64 on the host; no exception allowed."""
    n, c, d = 20, 4, 64
    for seed in range(20):
        g = seeded(200 + seed, n, d, shift=0.25 * ((seed % 5) - 2))
        gt = on_gpu(torch, eng, g)
        eng.fang_trmean_attack(gt, c, seed=seed, round=seed)
        down = restated_mean(g) > 0
        honest, attacked = rank_trimmed_mean_f64(g, c), rank_trimmed_mean_f64(gt.cpu().numpy(), c)
        assert np.all(attacked[down] <= honest[down]) and np.all(attacked[~down] >= honest[~down])


def test_trmean_attack_refuses_what_the_header_says(eng, torch):
    gt = on_gpu(torch, eng, seeded(24004, 6, 10))
    before = gt.clone()
    with pytest.raises(ValueError):
        eng.fang_trmean_attack(gt, 6)                        # full knowledge without a benign row
    with pytest.raises(ValueError):
        eng.fang_trmean_attack(gt, 7, partial=True)
    with pytest.raises(ValueError):
        eng.fang_trmean_attack(gt, 2, b=1.0)
    assert eng.fang_trmean_attack(gt, 0).shape[0] == 0 and torch.equal(gt, before)


# ---- the Krum attack -----------------------------------------------------------------------------------------------------------
def run_krum_attack(eng, torch, g, c, threshold=1e-5):
    """(attacked matrix, info, the restatement from the device's own t, q and benign block)."""
    n, d = g.shape
    gt = on_gpu(torch, eng, g)
    block = eng.pairwise_distances(gt[c:]).numpy()
    rows, info = eng.fang_krum_attack(gt, c, threshold=threshold, return_working=True)
    assert rows.data_ptr() == gt.data_ptr()
    t, q = info['t'].cpu().numpy(), info['q'].cpu().numpy()
    want = restated_fang_krum(block, q, t, n, c, d, threshold)
    return gt.cpu().numpy(), info, want, (block, q, t)


@pytest.mark.parametrize('seed, n, c, d', [(7001, 12, 2, 40), (7002, 64, 15, 1000)])
def test_krum_attack_on_the_well_separated_case(eng, torch, seed, n, c, d):
    from attacking_federate_learning_amd import defences
    g = krum_case(seed, n, c, d)
    s = restated_sign(restated_mean(g))
    # row_dots' t and q against numpy's fp64 sums, at the bound of tests/test_gpu_fltrust.py
    gt = on_gpu(torch, eng, g)
    p, q = (v.cpu().numpy() for v in eng.row_dots(gt[c:], on_gpu(torch, eng, s)))
    x = np.abs(g[c:].astype(np.float64))
    assert (np.abs(p - g[c:].astype(np.float64) @ s.astype(np.float64)) <= d * U * x.sum(axis=1)).all()
    assert (np.abs(q - (x * x).sum(axis=1)) <= d * U * (x * x).sum(axis=1)).all()
    attacked, info, want, (block, dq, dt) = run_krum_attack(eng, torch, g, c)
    assert np.array_equal(dt, p) and np.array_equal(dq, q)                      # the attack's t and q are row_dots' own
    # given those and the benign block: the last step's matrix, lambda_0, the lambdas, the steps and Krum's index
    got_dist = info['distances'].numpy()
    assert same(got_dist, want['dist']), np.argwhere(bits(got_dist) != bits(want['dist']))[:8]
    assert same(got_dist[c:, c:], block)
    assert info['lambda0'] == want['lambda0'] and info['lambda'] == want['lambda'] and info['steps'] == want['steps']
    assert info['lambda'] == info['lambda0'] / 2.0 ** (info['steps'] - 1)
    assert info['chosen'] == want['chosen'] and info['succeeded'] and want['succeeded'] and 0 <= info['chosen'] < c
    for lam in want['lambdas'][:-1]:                                             # ... and no earlier lambda would have done
        assert cpu_krum(restated_krum_matrix(block, dq, dt, lam, n, c, d), c) >= c
    # the rows: -lambda s in every attacker row, the benign rows untouched
    assert same(attacked[:c], np.tile(-np.float32(info['lambda']) * s, (c, 1))) and same(attacked[c:], g[c:])
    # the library's own Krum on the attacked matrix returns an attacker row
    picked = defences.krum(on_gpu(torch, eng, attacked), n, c)
    assert same(picked.cpu().numpy(), attacked[0])
    assert 0 <= defences.krum(on_gpu(torch, eng, attacked), n, c, return_index=True) < c
    assert eng.fang_krum_info() == {k: info[k] for k in ('lambda0', 'lambda', 'steps', 'chosen', 'succeeded')}


@pytest.mark.parametrize('kind', ['far', 'identical'])
def test_krum_attack_gives_up_below_the_threshold(eng, torch, kind):
    n, c, d = 12, 2, 40
    g = krum_case(7003, n, c, d, mu=20.0) if kind == 'far' else np.tile(krum_case(7004, 1, 0, d, mu=1.0), (n, 1))
    attacked, info, want, _ = run_krum_attack(eng, torch, g, c, threshold=1e-3)
    assert not info['succeeded'] and info['chosen'] >= c and info['chosen'] == want['chosen']
    assert info['lambda0'] == want['lambda0'] and info['steps'] == want['steps'] and info['lambda'] == want['lambda']
    assert info['lambda'] < 1e-3 <= 2.0 * info['lambda']
    assert same(info['distances'].numpy(), want['dist'])
    assert np.isfinite(attacked).all() and np.all(np.abs(attacked[:c]) == np.float32(info['lambda'])) and same(attacked[c:], g[c:])


def test_krum_attack_beyond_the_small_row_kernels(eng, torch):
    """More than 128 benign rows: the benign block comes from the Gram and every step's selection from the row sort."""
    n, c, d = 150, 20, 300
    g = krum_case(7006, n, c, d)
    attacked, info, want, _ = run_krum_attack(eng, torch, g, c)
    print('steps', info['steps'], 'lambda0', info['lambda0'], 'lambda', info['lambda'], 'chosen', info['chosen'])
    assert same(info['distances'].numpy(), want['dist'])
    assert (info['lambda0'], info['lambda'], info['steps'], info['chosen'], info['succeeded']) == (
        want['lambda0'], want['lambda'], want['steps'], want['chosen'], want['succeeded'])
    s = restated_sign(restated_mean(g))
    assert same(attacked[:c], np.tile(-np.float32(info['lambda']) * s, (c, 1))) and same(attacked[c:], g[c:])


def test_krum_attack_on_a_device_server_and_what_it_refuses(eng, torch):
    from attacking_federate_learning_amd.server import DeviceServer
    n, c, d = 12, 2, 40
    g = krum_case(7001, n, c, d)
    server = DeviceServer(n, np.zeros(d, dtype=np.float32), 0.2, 0.1, 0.9, torch_device='cuda:%d' % eng.device, engine=eng)
    server.users_grads.data.copy_(on_gpu(torch, eng, g))
    info = server.attack_fang_krum(c)
    attacked, _, want, _ = run_krum_attack(eng, torch, g, c)
    assert info['succeeded'] and info['lambda'] == want['lambda'] and same(server.users_grads.data.cpu().numpy(), attacked)
    # a host matrix: left alone, the rows come back
    host = g.copy()
    rows = eng.fang_krum_attack(host, c)
    assert same(rows, attacked[:c]) and same(host, g)
    gt = on_gpu(torch, eng, g[:5])
    before = gt.clone()
    with pytest.raises(ValueError):
        eng.fang_krum_attack(gt, 2)                          # n <= 2c + 1
    with pytest.raises(ValueError):
        eng.fang_krum_attack(gt, 0)
    with pytest.raises(ValueError):
        eng.fang_krum_attack(gt, 1, threshold=0.0)
    bad = on_gpu(torch, eng, g)
    bad[7, 3] = float('inf')
    kept = bad.clone()
    with pytest.raises(ValueError):
        eng.fang_krum_attack(bad, c)                         # lambda_0 is not finite: nothing is written
    assert torch.equal(gt, before) and torch.equal(bad, kept)
