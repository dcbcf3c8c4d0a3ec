"""Randomised bit-for-bit checks of oracle.faithful against the reference itself.

The inputs are seeded and regenerated here; what the unmodified reference returned for each of them is stored in
tests/golden/oracle_vs_reference.npz (minted by tests/golden/make_golden_oracle_vs_reference.py from a checkout of
the reference, with exactly the cases and inputs of this module), so these checks need nothing outside the repository.
"""
import contextlib
import hashlib
import os

import numpy as np
import pytest

from oracle import faithful, ideal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'oracle_vs_reference.npz')

KINDS = ['iid', 'dup', 'quantised']
KRUM_CASES = [(2, 5, 0), (3, 17, 1), (9, 64, 2), (16, 33, 3), (31, 257, 7)]
TRIMMED_MEAN_CASES = [(4, 9, 1), (7, 40, 2), (10, 33, 2), (25, 19, 6), (64, 12, 15)]
BULYAN_CASES = [(3, 8, 0), (7, 30, 1), (11, 50, 2), (19, 21, 4), (27, 100, 6)]
ATTACK_CASES = [(1, 10, 1.5), (4, 77, 1.5), (13, 300, 0.3), (5, 20, 0.0)]
BACKDOOR_CASES = [(1, 1.5, 0.1), (257, 1.5, 0.1), (1000, 0.3, 0.1 * 10 / 13), (4096, 3.0, 0.01)]


class FakeUser:
    def __init__(self, grads):
        self.grads, self.original_params, self.learning_rate = grads, None, None


def matrices(seed, n, d, kind):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d)).astype(np.float32)
    if kind == 'dup':           # blocks of identical rows, like the drift attack produces
        g[: n // 3] = g[0]
    elif kind == 'quantised':   # many exact ties in every column
        g = np.round(g * 2).astype(np.float32) / 2
    return g


def attack_rows(m, d):
    return matrices(400 + m, m, d, 'iid') * 2 + 1


def backdoor_inputs(d):
    rng = np.random.default_rng(900 + d)
    mean = rng.standard_normal(d).astype(np.float32)
    stdev = np.abs(rng.standard_normal(d)).astype(np.float32)
    params = rng.standard_normal(d).astype(np.float32)
    mal = (params + rng.standard_normal(d)).astype(np.float32)
    return mean, stdev, params, mal


def client_step_inputs():
    rng = np.random.default_rng(7)
    weights = (0.1 * rng.standard_normal(79510)).astype(np.float32)
    data = rng.standard_normal((4, 9, 1, 28, 28)).astype(np.float32)
    target = rng.integers(0, 10, size=(4, 9))
    return weights, data, target


@contextlib.contextmanager
def one_torch_thread():
    """The client step's bits depend on how many threads torch splits its CPU reductions over; the record is minted on
    one, so the step is compared on one."""
    import torch
    saved = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(saved)


def torch_arithmetic_canary():
    """The client step's op mix (linear, relu, log-softmax, NLL loss, backward) through torch.nn.functional on other fixed
    inputs, as the SHA-256 of its gradients' bytes.  Recorded with the golden: a host that reproduces its bits rounds these
    torch CPU kernels as the minting host did, so there the client step must be the reference's bit for bit."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(11)
    params = [torch.tensor((0.05 * rng.standard_normal(shape)).astype(np.float32), requires_grad=True)
              for shape in ((100, 784), (100,), (10, 100), (10,))]
    x = torch.from_numpy(rng.standard_normal((9, 784)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, 10, size=9))
    w1, b1, w2, b2 = params
    F.nll_loss(F.log_softmax(F.linear(F.relu(F.linear(x, w1, b1)), w2, b2), dim=1), y).backward()
    return digest(np.concatenate([p.grad.numpy().ravel() for p in params]))


def client_step_sample():
    """Flat gradient positions recorded in full for the client step: fc1.bias, fc2.weight and fc2.bias whole (the last
    1,110), and a seeded 2,048 of fc1.weight's 78,400."""
    fc1 = np.sort(np.random.default_rng(12).choice(78400, 2048, replace=False))
    return np.concatenate([fc1, np.arange(78400, 79510)])


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case_key(*parts):
    return '/'.join(str(p) for p in parts)


@pytest.fixture(scope='module')
def reference_out():
    """`reference_out(prefix)` -> {field: what the reference returned} for one case of the golden record."""
    z = np.load(GOLDEN)
    record = {key: z[key] for key in z.files}

    def case(prefix):
        fields = {key[len(prefix) + 1:]: value for key, value in record.items() if key.startswith(prefix + '/')}
        assert fields, 'no golden case %s' % prefix
        return fields
    return case


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,d,f', KRUM_CASES)
def test_krum_and_distances(reference_out, kind, n, d, f):
    ref = reference_out(case_key('krum', kind, n, d, f))
    g = matrices(100 + n, n, d, kind)
    assert ref['keys'].tolist() == faithful.visit_order(n)
    dist = faithful.distance_matrix(g)
    assert ref['all_float32'] and dist.dtype == np.float32
    assert len(ref['pairs']) == n * (n - 1)
    for (i, j), v in zip(ref['pairs'].tolist(), ref['values']):
        assert dist[i, j] == v
    assert faithful.krum(g, n, f, return_index=True) == int(ref['index'])
    if n >= 2 * f + 1:
        assert np.array_equal(faithful.krum(g, n, f), ref['krum'])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,d,c', TRIMMED_MEAN_CASES)
def test_trimmed_mean(reference_out, kind, n, d, c):
    want = reference_out(case_key('trimmed_mean', kind, n, d, c))['out']
    g = matrices(200 + n, n, d, kind)
    assert np.array_equal(faithful.trimmed_mean(g, n, c), want)
    assert np.allclose(ideal.trimmed_mean(g, c), want, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,d,f', BULYAN_CASES)
def test_bulyan(reference_out, kind, n, d, f):
    ref = reference_out(case_key('bulyan', kind, n, d, f))
    g = matrices(300 + n, n, d, kind)
    agg, picked = faithful.bulyan(g, n, f, return_selection=True)
    assert picked == ref['selection'].tolist()
    assert np.array_equal(agg, ref['out'])


def test_assertions_match(reference_out):
    ref = reference_out('assertions')
    g = matrices(1, 6, 10, 'iid')
    assert ref['krum_raises'] and ref['bulyan_raises']     # the reference asserts on (6, 3) in both
    for fn in (faithful.krum, faithful.bulyan):
        with pytest.raises(AssertionError):
            fn(g, 6, 3)
    # the Krum assert is skipped when only the index is requested (defences.py:24)
    assert faithful.krum(g, 6, 3, return_index=True) == int(ref['krum_index'])


@pytest.mark.parametrize('m,d,z', ATTACK_CASES)
def test_attack(reference_out, m, d, z):
    ref = reference_out(case_key('attack', m, d, z))
    g = attack_rows(m, d)
    vec = faithful.drift_vector(g, z)
    if z == 0:
        assert vec is None and np.array_equal(ref['grads0'], g[0])
    else:
        assert np.array_equal(vec, ref['grads0'])
    assert np.array_equal(faithful.attack_statistics(g)[1], ref['stdev'])


@pytest.mark.parametrize('d,z,lr', BACKDOOR_CASES)
def test_backdoor_hook(reference_out, d, z, lr):
    ref = reference_out(case_key('backdoor', d, z, lr))
    mean, stdev, params, mal = backdoor_inputs(d)
    assert np.array_equal(ref['start'], faithful.backdoor_initial_params(params, lr, mean))
    assert np.array_equal(ref['grads'], faithful.backdoor_attack_grads(mean, stdev, params, lr, z, mal), equal_nan=True)


def test_client_step_against_user_step(reference_out):
    """oracle.clients against the reference's own User.step / MnistNet on the same weights and batches.  The record holds
    the SHA-256 of the reference's gradient bytes, a fixed sample of them (`client_step_sample`), and every client's fp64
    sum, norm and largest magnitude."""
    torch = pytest.importorskip('torch')
    from oracle import clients
    ref = reference_out('client_step')
    weights, data, target = client_step_inputs()
    with one_torch_thread():
        got = clients.all_client_gradients(clients.MnistNet(), weights, torch.from_numpy(data), torch.from_numpy(target))
        same_rounding = torch_arithmetic_canary() == str(ref['canary'])
    assert got.shape == tuple(ref['shape']) and got.dtype == np.float32
    if same_rounding:
        assert digest(got) == str(ref['sha256'])     # same torch ops in the same order: bit-identical
    else:
        # this host's torch CPU kernels round differently from the minting host's (the canary differs): the same ops
        # agree up to fp32 summation order -- a few ulps of each client's largest gradient (another thread count on one
        # host moves them by up to 8e-7 of it)
        sample = got[:, client_step_sample()]
        assert np.all(np.abs(sample - ref['sample']) <= 1e-5 * np.abs(ref['sample']) + 4e-6 * ref['row_max'][:, None])
        rows = got.astype(np.float64)
        assert np.allclose(rows.sum(axis=1), ref['row_sums'], rtol=1e-4, atol=1e-5)
        assert np.allclose(np.sqrt((rows ** 2).sum(axis=1)), ref['row_norms'], rtol=1e-5)
