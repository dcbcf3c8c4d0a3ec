"""The CPU oracle against the golden vectors minted from the reference (bit-exact)."""
import warnings

import numpy as np
import pytest

from oracle import faithful, ideal


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_no_defense(golden):
    c = golden['nodef_7x130']
    assert same(faithful.no_defense(c['G'], 7, 1), c['out'])


@pytest.mark.parametrize('case', ['krum_iid_10x257', 'krum_scaled_33x1000', 'krum_attacked_12x300',
                                  'krum_allsame_6x64', 'krum_f0_5x40'])
def test_krum(golden, case):
    c = golden[case]
    g, f = c['G'], int(c['f'])
    dist = faithful.distance_matrix(g)
    assert same(dist, c['dist'])
    assert faithful.krum(g, len(g), f, return_index=True) == int(c['index'])
    assert same(faithful.krum(g, len(g), f), c['out'])
    # the fp64 tier agrees on the index (these cases have margins far above fp32 noise or exact ties)
    assert ideal.krum_index(ideal.distance_matrix(g), len(g), f) == int(c['index'])


def test_krum_all_nan_keeps_minus_one(golden):
    c = golden['krum_allnan_4x8']
    assert faithful.krum(c['G'], 4, int(c['f']), return_index=True) == int(c['index']) == -1


@pytest.mark.parametrize('case', ['tm_odd_11x97', 'tm_even_10x97', 'tm_100x64', 'tm_attacked_20x50',
                                  'tm_c0_9x33', 'tm_edge_ties_c1', 'tm_edge_ties_c2',
                                  'tm_edge_ties_c3', 'tm_edge_ties_c4', 'tm_kzero_6x20', 'tm_kneg_6x20'])
def test_trimmed_mean(golden, case):
    c = golden[case]
    g, cc = c['G'], int(c['c'])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert same(faithful.trimmed_mean(g, len(g), cc), c['out'])
        fast = ideal.trimmed_mean(g, cc)
    assert np.allclose(fast, c['out'], rtol=1e-6, atol=1e-6, equal_nan=True)


@pytest.mark.parametrize('case', ['bulyan_iid_11x200', 'bulyan_boundary_15x120', 'bulyan_scaled_40x500',
                                  'bulyan_attacked_23x150', 'bulyan_f0_6x30'])
def test_bulyan(golden, case):
    c = golden[case]
    g, f = c['G'], int(c['f'])
    agg, picked = faithful.bulyan(g, len(g), f, return_selection=True)
    assert picked == c['selection'].tolist()
    assert same(agg, c['out'])
    agg64, picked64 = ideal.bulyan(g, len(g), f, return_selection=True)
    assert picked64 == c['selection'].tolist()
    assert np.allclose(agg64, c['out'], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('case', ['attack_5x300_z1.5', 'attack_24x100_z0.5', 'attack_3x64_z0'])
def test_attack(golden, case):
    c = golden[case]
    g, z = c['G'], float(c['z'])
    mean, stdev = faithful.attack_statistics(g)
    assert same(stdev, c['stored_stdev'])
    vec = faithful.drift_vector(g, z)
    if z == 0:
        assert vec is None and same(mean, c['stored_mean']) and same(c['user0'], g[0])
    else:
        # the reference overwrites attacker.grads_mean with the drifted vector (malicious.py:35)
        assert same(vec, c['stored_mean']) and same(vec, c['user0'])
        v64, _, s64 = ideal.drift_vector(g, z)
        assert np.allclose(v64, vec, rtol=1e-5, atol=1e-5)
        assert np.allclose(s64, stdev, rtol=1e-5, atol=1e-6)


# ---- the steps either side of the path ---------------------------------------------
BACKDOOR_CASES = ['backdoor_300_z1.5', 'backdoor_1000_z0.5_faded_lr', 'backdoor_64_z0']


@pytest.mark.parametrize('case', BACKDOOR_CASES)
def test_backdoor_hook(golden, case):
    c = golden[case]
    lr, z = float(c['lr']), float(c['z'])
    assert same(faithful.backdoor_initial_params(c['params'], lr, c['mean']), c['start'])
    out = faithful.backdoor_attack_grads(c['mean'], c['stdev'], c['params'], lr, z, c['mal'])
    assert out.dtype == np.float32 and same(out, c['out'])
    # the clip really binds in these cases (otherwise they would not pin it)
    band = np.float32(z) * c['stdev']
    assert np.any(out == c['mean'] - band) and np.any(out == c['mean'] + band)


def test_gradient_assembly(golden):
    c = golden['assemble_4x204']
    g = np.empty_like(c['G'])
    for u in range(4):
        faithful.assemble_row(g, u, [c['u%d_t%d' % (u, t)] for t in range(5)])
    assert same(g, c['G'])


def check_client_rows(rows, c, rtol=1e-5, atol=1e-7):
    rows = np.asarray(rows)
    n = rows.shape[0]
    w1 = rows[:, :78400].reshape(n, 100, 784)
    assert np.allclose(w1[:, (0, 57), :], c['fc1_weight_rows'], rtol=rtol, atol=atol)
    assert np.allclose(rows[:, 78400:], c['tail'], rtol=rtol, atol=atol)
    assert np.allclose(rows.astype(np.float64).sum(axis=1), c['row_sums'], rtol=1e-4, atol=1e-5)
    assert np.allclose(np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1)), c['row_norms'], rtol=1e-5)


def test_client_step(golden):
    """user.py:76-92 for three MnistNet clients (fp32 GEMMs: equal up to summation order, 1e-5)."""
    torch = pytest.importorskip('torch')
    from oracle import clients
    c = golden['clients_mnist_3x5']
    rows = clients.all_client_gradients(clients.MnistNet(), c['weights'], torch.from_numpy(c['data']),
                                        torch.from_numpy(c['target']))
    assert rows.shape == (3, 79510) and rows.dtype == np.float32
    check_client_rows(rows, c)


def test_batched_client_step_matches_on_cpu_tensors(golden):
    """The vmap form (host-side torch plumbing, device agnostic) against the same golden vectors."""
    torch = pytest.importorskip('torch')
    from oracle import clients
    from attacking_federate_learning_amd.clients import per_client_gradients
    c = golden['clients_mnist_3x5']
    data = torch.from_numpy(c['data']).view(3, 5, 784)
    grads = per_client_gradients(clients.MnistNet(), c['weights'], data, torch.from_numpy(c['target']))
    assert [tuple(g.shape) for g in grads] == [(3, 100, 784), (3, 100), (3, 10, 100), (3, 10)]
    check_client_rows(np.concatenate([g.reshape(3, -1).numpy() for g in grads], axis=1), c)


def test_the_loops_as_shipped_equal_the_vectorised_restatement():
    """oracle.shipped (dicts, sorted, sum, key=abs: what bench.py times as "reference as shipped") against
    oracle.faithful, bit for bit."""
    from oracle import shipped
    rng = np.random.default_rng(77)
    g = rng.standard_normal((19, 300)).astype(np.float32)
    g[:4] = g[0]
    n, f = 19, 4
    assert shipped.krum(g, n, f, return_index=True) == faithful.krum(g, n, f, return_index=True)
    assert np.array_equal(shipped.trimmed_mean(g, n, f), faithful.trimmed_mean(g, n, f))
    assert np.array_equal(shipped.bulyan(g, n, f), faithful.bulyan(g, n, f))
    d = shipped.dict_from_dense(faithful.distance_matrix(g))
    assert list(d.keys()) == faithful.visit_order(n)
    assert shipped.krum(g, n, f, distances=d, return_index=True) == faithful.krum(g, n, f, return_index=True)


def test_golden_dropin_rounds_are_the_oracle_rounds():
    """tests/golden/dropin_rounds.npz holds two rounds of the reference's own `Server.defend` (server.py:86-90, its own
    defences.py) on the matrices its unmodified main loop produced, for every defence (tests/golden/make_golden_dropin.py).
    The oracle, pinned bit for bit to the reference's defences, followed by the same momentum step, must land on those
    weights exactly; the GPU replays the same rounds through the drop-in modules (tests/test_gpu_parity.py)."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dropin_rounds.npz')
    z = np.load(path)
    aggregates = {'NoDefense': faithful.no_defense, 'Krum': faithful.krum, 'TrimmedMean': faithful.trimmed_mean,
                  'Bulyan': faithful.bulyan}
    assert sorted('%s/weights1' % name for name in aggregates) == sorted(k for k in z.files if k.endswith('/weights1'))
    mal_prop, momentum, learning_rate = float(z['mal_prop']), 0.9, 0.1
    for name, aggregate in aggregates.items():
        weights = z['weights_start'].copy()
        velocity = np.zeros_like(weights)
        for e, key in enumerate(('round0_grads', '%s/round1_grads' % name)):
            users_grads = z[key]
            n = len(users_grads)
            current_grads = aggregate(users_grads, n, int(n * mal_prop))        # server.py:87
            velocity = momentum * velocity - learning_rate * current_grads      # server.py:89
            weights += velocity                                                # server.py:90
            assert same(weights, z['%s/weights%d' % (name, e)]), (name, e)
