"""The Min-Max / Min-Sum attacks on an MI355X, held to the numpy restatement of tests/minmax_rule.py.

What is compared as bits: a against row_sqdist, the moments of strided and misaligned views against the aligned call's, the
attacker rows against fl32(mu + gamma p) formed in numpy from the gamma the device reports, the benign rows against themselves.
What is compared within a bound: the moments against math.fsum (d 2^-52 a, and d 2^-52 sqrt(c a) for b), gamma against the
restatement fed the device's own mu, sigma and Dmax (64 d 2^-53 sqrt(T / c): the forward error of a root whose slack is at
least T / 8; Min-Sum's T is S / r, the bound a row), and feasibility in exact arithmetic.  Feasibility is evaluated on the fp64
vector mu + gamma p with the device's gamma, as tests/test_minmax.py does: the rows themselves are that vector rounded to fp32,
which moves a distance by 2^-24 relative, eight orders above eta."""
import ctypes
import math

import numpy as np
import pytest

from tests import minmax_rule as mr
from tests import views_arena

pytestmark = pytest.mark.gpu

SEEDED = [(case, r) for case in mr.CASES for r in mr.known_counts(case[0])]
IDS = ['%dx%d-r%d' % (case[0], case[1], r) for case, r in SEEDED]
COLS = (1, 3, 5, 255, 257, 1023, 1025, 4099)


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def on_gpu(torch, eng, a):
    return torch.from_numpy(np.array(a, order='C')).to('cuda:%d' % eng.device)


def bits(a):
    return views_arena.bits(a)


def f64bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def device_statistics(eng, torch, known):
    """mu, sigma as the attack takes them (drift_attack's bits) and the three perturbations formed from them in numpy; `unit`
    divides by the square root of row_sqdist's |mu|^2, one correctly rounded fp64 quotient a column as on the device"""
    _, mu, sigma = eng.drift_attack(on_gpu(torch, eng, known), 0.0)
    mu, sigma = mu.cpu().numpy(), sigma.cpu().numpy()
    nrm = math.sqrt(float(eng.row_sqdist(mu[None, :], np.zeros_like(mu))[0]))
    unit = np.zeros_like(mu) if nrm == 0.0 else (-mu.astype(np.float64) / nrm).astype(np.float32)
    return mu, sigma, {'unit': unit, 'std': mr.perturbation('std', mu, sigma), 'sign': mr.perturbation('sign', mu, sigma)}


@pytest.mark.parametrize('n', (1, 7, 8, 9, 32, 33))
def test_row_moments(eng, torch, n):
    for d in COLS:
        rng = np.random.default_rng(4100 + 53 * n + d)
        g = rng.standard_normal((n, d)).astype(np.float32)
        z = (0.3 * rng.standard_normal(d)).astype(np.float32)
        p = rng.standard_normal(d).astype(np.float32)
        gd, zd, pd = on_gpu(torch, eng, g), on_gpu(torch, eng, z), on_gpu(torch, eng, p)
        a, b = (v.cpu().numpy() for v in eng.row_moments(gd, zd, pd))
        a2, b2 = (v.cpu().numpy() for v in eng.row_moments(gd, zd, pd))
        assert np.array_equal(f64bits(a), f64bits(a2)) and np.array_equal(f64bits(b), f64bits(b2)), (n, d)
        assert np.array_equal(f64bits(a), f64bits(eng.row_sqdist(gd, zd).cpu().numpy())), (n, d)
        for variant in views_arena.VARIANTS[:3]:
            view, flat = views_arena.arena_variant(torch, g, variant, device='cuda:%d' % eng.device)
            before = flat.clone()
            av, bv = (v.cpu().numpy() for v in eng.row_moments(view, zd, pd))
            views_arena.untouched(torch, flat, view, before)
            assert np.array_equal(f64bits(a), f64bits(av)) and np.array_equal(f64bits(b), f64bits(bv)), (n, d, variant)
        ea, eb, ec = mr.exact_moments(g, z, p)
        assert (np.abs(a - ea) <= d * 2.0 ** -52 * ea).all(), (n, d, np.abs(a - ea).max())
        assert (np.abs(b - eb) <= d * 2.0 ** -52 * np.sqrt(ec * ea)).all(), (n, d, np.abs(b - eb).max())


@pytest.mark.parametrize('case,r', SEEDED, ids=IDS)
def test_attack_on_the_seeded_cases(eng, torch, case, r):
    n, d = case[0], case[1]
    g = mr.matrix(*case)
    partial = r < n
    m = r if partial else max(1, n // 5)
    known = g[:r]
    mu, sigma, perturbations = device_statistics(eng, torch, known)
    want_dmax = mr.dmax_of(known)
    eta = 8 * d * 2.0 ** -53
    for kind in mr.KINDS:
        for name in mr.PERTURBATIONS:
            p = perturbations[name]
            gd = on_gpu(torch, eng, g)
            rows, info = eng.minmax_attack(gd, m, kind=kind, perturbation=name, partial=partial, return_info=True)
            what = (case, r, kind, name, info)
            assert not info['broken'] and not info['degenerate'] and info['known_rows'] == r, what
            assert rows.data_ptr() == gd.data_ptr()
            dmax = None
            if kind == 'minmax':
                dmax = np.float32(math.sqrt(info['bound']))            # T = (double)Dmax^2 is exact, and so is its root
                assert float(dmax) ** 2 == info['bound'], what
                assert abs(float(dmax) - float(want_dmax)) <= 1e-5 * float(want_dmax), what
            res = mr.rule(known, kind, mu, sigma, p, dmax=dmax)
            per_row = info['bound'] if kind == 'minmax' else info['bound'] / r
            tol = 64 * d * 2.0 ** -53 * math.sqrt(per_row / info['c'])
            print(what, 'restated gamma', res['gamma'], 'difference', info['gamma'] - res['gamma'], 'allowed', tol)
            assert abs(info['c'] - res['c']) <= d * 2.0 ** -52 * res['c'], what
            assert abs(info['gamma'] - res['gamma']) <= tol, what
            if kind == 'minsum':
                assert abs(info['bound'] - res['bound']) <= d * 2.0 ** -52 * res['bound'], what
                top = np.sort(res['a'])[-2:]
                margin = top[1] - top[0] > d * 2.0 ** -51 * top[1]
            else:
                margin = r > 2                                            # the runner-up lies 3.6e-4 above (tests/test_minmax.py)
            if margin:
                assert info['binding_row'] == res['row'], what
            out = gd.cpu().numpy()
            want_row = mr.vector(mu, p, info['gamma'])
            for i in range(m):
                assert np.array_equal(bits(out[i]), bits(want_row)), (what, i)
            assert np.array_equal(bits(out[m:]), bits(g[m:])), what
            mal = mu.astype(np.float64) + info['gamma'] * p.astype(np.float64)
            sq = mr.exact_sqdists(np.concatenate([known[:m], out[m:r]]), mal)
            got = float(sq.max()) if kind == 'minmax' else math.fsum(sq)
            print(what, 'tightness', got / info['bound'] - 1, 'eta', eta)
            assert info['bound'] * (1 - eta) <= got <= info['bound'] * (1 + eta), what


def test_custom_perturbation_and_a_host_matrix(eng, torch):
    case = mr.CASES[2]
    g = mr.matrix(*case)
    n, d = g.shape
    m = 13
    mu, sigma, _ = device_statistics(eng, torch, g)
    p = np.random.default_rng(99).standard_normal(d).astype(np.float32)
    for kind in mr.KINDS:
        gd = on_gpu(torch, eng, g)
        _, info = eng.minmax_attack(gd, m, kind=kind, perturbation='custom', p=on_gpu(torch, eng, p), return_info=True)
        dmax = np.float32(math.sqrt(info['bound'])) if kind == 'minmax' else None
        res = mr.rule(g, kind, mu, sigma, p, dmax=dmax)
        per_row = info['bound'] if kind == 'minmax' else info['bound'] / n
        assert abs(info['gamma'] - res['gamma']) <= 64 * d * 2.0 ** -53 * math.sqrt(per_row / info['c'])
        out = gd.cpu().numpy()
        assert all(np.array_equal(bits(out[i]), bits(mr.vector(mu, p, info['gamma']))) for i in range(m))
        assert np.array_equal(bits(out[m:]), bits(g[m:]))
        # the host matrix is left alone and the one vector comes back, the same bits
        host = g.copy()
        vec, host_info = eng.minmax_attack(host, m, kind=kind, perturbation='custom', p=p, return_info=True)
        assert np.array_equal(bits(host), bits(g)) and host_info['gamma'] == info['gamma']
        assert np.array_equal(bits(vec), bits(out[0]))


def test_degenerate(eng, torch):
    # all-zero columns with `unit`: mu = 0, p = 0, c = 0
    g = np.zeros((9, 130), dtype=np.float32)
    for kind in mr.KINDS:
        gd = on_gpu(torch, eng, g)
        _, info = eng.minmax_attack(gd, 3, kind=kind, perturbation='unit', return_info=True)
        assert info['degenerate'] and not info['broken'] and info['gamma'] == 0.0 and info['c'] == 0.0 and info['binding_row'] == -1
        assert np.array_equal(bits(gd.cpu().numpy()), bits(g))
    # one known row: mu is that row, every attacker row becomes it
    g = views_arena.gaussian(515, 6, 77)
    for kind in mr.KINDS:
        for name in mr.PERTURBATIONS:
            gd = on_gpu(torch, eng, g)
            _, info = eng.minmax_attack(gd, 1, kind=kind, perturbation=name, partial=True, return_info=True)
            assert info['degenerate'] and not info['broken'] and info['gamma'] == 0.0 and info['known_rows'] == 1
            assert np.array_equal(bits(gd.cpu().numpy()), bits(g))


@pytest.mark.parametrize('poison', (np.nan, np.inf, -np.inf))
def test_broken_input_leaves_the_rows(eng, torch, poison):
    g = views_arena.gaussian(616, 12, 300).copy()
    g[7, 123] = poison
    for kind in mr.KINDS:
        for name in mr.PERTURBATIONS:
            gd = on_gpu(torch, eng, g)
            _, info = eng.minmax_attack(gd, 4, kind=kind, perturbation=name, return_info=True)
            assert info['broken'] and math.isnan(info['gamma']) and not info['degenerate'], (kind, name, info)
            assert np.array_equal(bits(gd.cpu().numpy()), bits(g)), (kind, name)
    # a custom direction that is not finite
    p = np.ones(300, dtype=np.float32)
    p[5] = poison
    clean = views_arena.gaussian(617, 12, 300)
    gd = on_gpu(torch, eng, clean)
    _, info = eng.minmax_attack(gd, 4, kind='minsum', perturbation='custom', p=on_gpu(torch, eng, p), return_info=True)
    assert info['broken'] and math.isnan(info['gamma'])
    assert np.array_equal(bits(gd.cpu().numpy()), bits(clean))


def test_partial_knowledge_reads_no_benign_row(eng, torch):
    g = mr.matrix(*mr.CASES[4])
    m = 8
    poisoned = g.copy()
    poisoned[m:] = np.nan
    for kind in mr.KINDS:
        for name in mr.PERTURBATIONS:
            a, b = on_gpu(torch, eng, g), on_gpu(torch, eng, poisoned)
            _, ia = eng.minmax_attack(a, m, kind=kind, perturbation=name, partial=True, return_info=True)
            _, ib = eng.minmax_attack(b, m, kind=kind, perturbation=name, partial=True, return_info=True)
            assert not ib['broken'] and ia == ib, (kind, name, ia, ib)
            assert np.array_equal(bits(a.cpu().numpy()[:m]), bits(b.cpu().numpy()[:m]))
            assert np.isnan(b.cpu().numpy()[m:]).all()


def test_column_split(eng, torch):
    """Two column halves: the moments add up, and a slice's call -- its statistics, perturbation and fill local to its columns,
    the moments through the all-reduce -- writes the slice of the one call's rows."""
    case = mr.CASES[1]
    g = mr.matrix(*case)
    n, d = g.shape
    m, h = 10, 437
    mu, sigma, perturbations = device_statistics(eng, torch, g)
    zeros = np.zeros(d, dtype=np.float32)
    for name in ('std', 'sign'):
        p = perturbations[name]
        gd = on_gpu(torch, eng, g)
        whole = [v.cpu().numpy() for v in eng.row_moments(gd, mu, p)] + [eng.row_sqdist(p[None, :], zeros)]
        parts = []
        for lo, hi in ((0, h), (h, d)):
            a, b = (v.cpu().numpy() for v in eng.row_moments(gd[:, lo:hi], mu[lo:hi].copy(), p[lo:hi].copy()))
            parts.append((a, b, eng.row_sqdist(p[None, lo:hi].copy(), zeros[lo:hi].copy())))
        a, b, c = (parts[0][k] + parts[1][k] for k in range(3))
        assert (np.abs(a - whole[0]) <= 4 * d * 2.0 ** -53 * whole[0]).all()
        assert (np.abs(b - whole[1]) <= 4 * d * 2.0 ** -53 * np.sqrt(whole[2][0] * whole[0])).all()
        assert abs(c[0] - whole[2][0]) <= 4 * d * 2.0 ** -53 * whole[2][0]
        _, info = eng.minmax_attack(gd, m, kind='minsum', perturbation=name, return_info=True)
        one_call = gd.cpu().numpy()
        abc = torch.from_numpy(np.concatenate([whole[0], whole[1], whole[2]])).to(gd.device)
        calls = []

        def all_reduce(t):       # the other rank's share arrives: the sums are the whole matrix's
            calls.append(t.numel())
            t.copy_(abc)
        for lo, hi in ((0, h), (h, d)):
            local = on_gpu(torch, eng, g)[:, lo:hi]
            _, part_info = eng.minmax_attack(local, m, kind='minsum', perturbation=name, all_reduce=all_reduce, return_info=True)
            assert part_info == info, (name, lo, part_info, info)
            assert np.array_equal(bits(local.cpu().numpy()), bits(one_call[:, lo:hi])), (name, lo)
        assert calls == [2 * n + 1, 2 * n + 1]


def test_attack_in_place_on_a_device_server(eng, torch):
    from attacking_federate_learning_amd.server import DeviceServer
    case = mr.CASES[0]
    g = mr.matrix(*case)
    n, d = g.shape
    server = DeviceServer(n, np.zeros(d, dtype=np.float32), 0.2, 0.1, 0.9, torch_device='cuda:%d' % eng.device, engine=eng)
    assert server.attack_minmax(0) is None
    for kind in mr.KINDS:
        server.users_grads.data.copy_(on_gpu(torch, eng, g))
        info = server.attack_minmax(4, kind=kind, perturbation='sign')
        gd = on_gpu(torch, eng, g)
        _, want = eng.minmax_attack(gd, 4, kind=kind, perturbation='sign', return_info=True)
        assert info == want and info['gamma'] > 0
        assert np.array_equal(bits(server.users_grads.data.cpu().numpy()), bits(gd.cpu().numpy()))


def test_what_the_header_refuses(eng, torch):
    from attacking_federate_learning_amd import _native
    g = on_gpu(torch, eng, views_arena.gaussian(3, 6, 40))
    p = on_gpu(torch, eng, np.ones(40, dtype=np.float32))
    before = g.clone()

    def call(kind, perturbation, partial, m, custom=None, params=True, matrix=g.data_ptr(), dist_given=0):
        prm = _native.MinmaxParams(kind, perturbation, partial, dist_given)
        return eng.lib.byz_minmax_attack_dev(eng.ctx, matrix, 6, 40, 40, m, ctypes.byref(prm) if params else None, custom, None, None)
    assert call(0, 1, 0, 0) == _native.OK                       # no attacker: nothing happens
    assert call(2, 1, 0, 2) == _native.E_INVALID                # the kind
    assert call(-1, 1, 0, 2) == _native.E_INVALID
    assert call(0, 4, 0, 2) == _native.E_INVALID                # the perturbation
    assert call(0, -1, 0, 2) == _native.E_INVALID
    assert call(0, 3, 0, 2) == _native.E_INVALID                # custom without its vector
    assert call(0, 1, 0, 2, custom=p.data_ptr()) == _native.E_INVALID     # a vector without custom
    assert call(0, 1, 1, 0) == _native.E_INVALID                # partial knowledge of nobody
    assert call(0, 1, 0, 7) == _native.E_INVALID                # more attackers than rows
    assert call(0, 1, 0, -1) == _native.E_INVALID
    assert call(0, 1, 0, 2, params=False) == _native.E_INVALID
    assert call(0, 1, 0, 2, matrix=None) == _native.E_INVALID
    assert call(0, 1, 0, 2, dist_given=1) == _native.E_INVALID  # a given matrix that is not there
    a = torch.empty(6, dtype=torch.float64, device=g.device)
    assert eng.lib.byz_row_moments_dev(eng.ctx, g.data_ptr(), 6, 40, 40, None, p.data_ptr(), a.data_ptr(), a.data_ptr(), None) == _native.E_INVALID
    assert eng.lib.byz_row_moments_dev(eng.ctx, g.data_ptr(), 6, 40, 40, p.data_ptr(), p.data_ptr(), None, a.data_ptr(), None) == _native.E_INVALID
    eng.synchronize()
    assert np.array_equal(bits(g.cpu().numpy()), bits(before.cpu().numpy()))
    # Min-Max with the caller's distance matrix: the same gamma, no Gram
    dist = eng.pairwise_distances(g)
    x, y = g.clone(), g.clone()
    _, computed = eng.minmax_attack(x, 2, return_info=True)
    _, given = eng.minmax_attack(y, 2, distances=dist, return_info=True)
    assert computed == given and np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy()))


def test_the_attack_moves_the_trimmed_mean_and_hides_from_krum(eng, torch):
    """One-sided sanity on (50, 1000) with 10 attackers under Min-Max: the library's trimmed mean moves from where it stood
    towards p, away from the benign mean, and Krum's scores do not rank an attacker row last."""
    g = mr.matrix(*mr.CASES[1])
    n, d = g.shape
    m = 10
    mu, sigma, perturbations = device_statistics(eng, torch, g)
    benign_mean = g[m:].astype(np.float64).mean(0)
    for name in mr.PERTURBATIONS:
        p = perturbations[name].astype(np.float64)
        gd = on_gpu(torch, eng, g)
        honest = eng.trimmed_mean(gd, n, m).cpu().numpy().astype(np.float64)
        eng.minmax_attack(gd, m, kind='minmax', perturbation=name)
        attacked = eng.trimmed_mean(gd, n, m).cpu().numpy().astype(np.float64)
        assert float((attacked - benign_mean) @ p) > float((honest - benign_mean) @ p), name
        dist = eng.pairwise_distances(gd).numpy().astype(np.float64)
        np.fill_diagonal(dist, np.inf)
        scores = np.sort(dist, axis=1)[:, :n - m].sum(1)
        assert int(np.argmax(scores)) >= m, (name, np.argmax(scores))


@pytest.mark.parametrize('kind,name', [('minsum', 'unit'), ('minmax', 'unit'), ('minmax', 'std')])
def test_column_split_with_the_norm_and_the_distances(eng, torch, kind, name):
    """The all-reduces test_column_split does not reach: `unit`'s one double (|mu|^2) in front of the moments, and Min-Max's
    Gram through the sharded distances.  The other rank's share arrives as the whole matrix's value, the one call runs on the
    distances of that Gram: a slice's call writes the slice of the one call's rows, as bits."""
    g = mr.matrix(*mr.CASES[1])
    n, d = g.shape
    m, h = 10, 437
    mu, sigma, perturbations = device_statistics(eng, torch, g)
    p = perturbations[name]
    zeros = np.zeros(d, dtype=np.float32)
    gd = on_gpu(torch, eng, g)
    a, b = (v.cpu().numpy() for v in eng.row_moments(gd, mu, p))
    whole = {2 * n + 1: np.concatenate([a, b, eng.row_sqdist(p[None, :], zeros)]),
             1: np.asarray(eng.row_sqdist(mu[None, :], zeros), dtype=np.float64)}
    gram = eng.gram(gd)
    whole[n * n] = gram.cpu().numpy().reshape(-1)
    whole = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gd.device) for k, v in whole.items()}
    distances = eng.distances_from_gram(gram, n) if kind == 'minmax' else None
    _, info = eng.minmax_attack(gd, m, kind=kind, perturbation=name, distances=distances, return_info=True)
    assert not info['broken'] and info['gamma'] > 0
    one_call = gd.cpu().numpy()
    expected = ([1] if name == 'unit' else []) + [2 * n + 1] + ([n * n] if kind == 'minmax' else [])
    for lo, hi in ((0, h), (h, d)):
        calls = []

        def all_reduce(t):
            calls.append(t.numel())
            t.copy_(whole[t.numel()].reshape(t.shape))
        local = on_gpu(torch, eng, g)[:, lo:hi]
        _, part_info = eng.minmax_attack(local, m, kind=kind, perturbation=name, all_reduce=all_reduce, return_info=True)
        assert calls == expected, (calls, expected)
        assert part_info == info, (lo, part_info, info)
        assert np.array_equal(bits(local.cpu().numpy()), bits(one_call[:, lo:hi])), lo


@pytest.mark.parametrize('variant', views_arena.VARIANTS)
def test_the_fill_stays_inside_a_padded_misaligned_view(eng, torch, variant):
    """The attack on a strided, misaligned, guard-banded view: the bits of the aligned call inside, and not a word outside the
    view changed -- neither the padding behind a row nor the guards either side.  Widths that end inside, on and past a block
    of four; one attacker and several."""
    for d in (1, 5, 255, 1028):
        g = views_arena.gaussian(7300 + d, 11, d)
        for kind in mr.KINDS:
            for m in (1, 4):
                want = on_gpu(torch, eng, g)
                _, info = eng.minmax_attack(want, m, kind=kind, perturbation='sign', return_info=True)
                view, flat = views_arena.arena_variant(torch, g, variant, device='cuda:%d' % eng.device)
                before = flat.clone()
                _, got = eng.minmax_attack(view, m, kind=kind, perturbation='sign', return_info=True)
                views_arena.untouched(torch, flat, view, before)
                assert got == info and not info['broken'], (d, kind, m, got, info)
                assert np.array_equal(bits(view.cpu().numpy()), bits(want.cpu().numpy())), (d, kind, m)
