#!/usr/bin/env python3
"""The reference's own `main.main` and `Server.defend`, unmodified, driven through this repo's drop-in modules -- and
the golden record of its rounds that the test suite replays.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dropin.py REFERENCE_CHECKOUT [--mint]

The claim "drops into main.py unchanged" (BASELINE.json north_star) needs the reference's driver files, which are not
part of this repository, so it is checked here, against a reference checkout, and what the suite needs of it is
recorded:

  check 1  the unmodified main.py / server.py / user.py run two rounds with `dropin/` first on sys.path.  Their
           `import defences`, `import malicious` bind this repo's modules; every call goes through the drop-in
           signatures, return types and the attacker's rebinding protocol.  Behind the modules sits the real engine
           when an MI355X is visible and otherwise a test double with the engine's method surface computing with the
           CPU oracle -- so what is under test on a CPU host is the boundary, bit for bit, not the kernels.  The same
           rounds with the reference's OWN defences/malicious give the trajectory to compare with.
  check 2  `Server.defend` alone (server.py:86-90) on a hand-made server object through the drop-in modules.
  record   tests/golden/dropin_rounds.npz: the matrices the unmodified main loop handed to `Server.defend`, cut to
           3000 columns, and what the reference's own `Server.defend` makes of them over two rounds with momentum.
           Checked against the committed file, or (re)written with --mint.  The suite replays it on the CPU oracle
           (tests/test_oracle_golden.py::test_golden_dropin_rounds_are_the_oracle_rounds) and through the drop-in
           modules on the MI355X (tests/test_gpu_parity.py::test_golden_dropin_rounds).
"""
import contextlib
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import reference_harness as harness  # noqa: E402
from oracle import faithful  # noqa: E402

GOLDEN = os.path.join(HERE, 'dropin_rounds.npz')
DEFENCES = ['NoDefense', 'Krum', 'TrimmedMean', 'Bulyan']


class OracleBackedEngine:
    """Test double with the method surface `defences.py` / `malicious.py` use of `engine.Engine`, computing with the CPU
    oracle.  Lets the drop-in boundary be exercised by the unmodified reference on a box without a GPU."""

    def no_defense(self, g, users_count=None, corrupted_count=None):
        return faithful.no_defense(np.asarray(g), users_count, corrupted_count)

    def pairwise_distances(self, g):
        return faithful.distance_matrix(np.asarray(g))

    def krum(self, g, users_count, corrupted_count, distances=None, return_index=False):
        out = faithful.krum(np.asarray(g), users_count, corrupted_count, distances=distances, return_index=return_index)
        return out        # a view of the caller's matrix, like the reference (and, since round 6, like the engine's host path)

    def trimmed_mean(self, g, users_count=None, corrupted_count=0):
        return faithful.trimmed_mean(np.asarray(g), users_count, corrupted_count)

    def bulyan(self, g, users_count, corrupted_count):
        return faithful.bulyan(np.asarray(g), users_count, corrupted_count)

    def drift_attack(self, rows, num_std, write_back=False):
        rows = np.asarray(rows, dtype=np.float32)
        mean, std = faithful.attack_statistics(rows)
        return mean - num_std * std, mean, std

    def drift_axpy_host(self, mean, std, num_std):
        out = np.array(mean, dtype=np.float32, copy=True)
        out[:] -= num_std * np.asarray(std)[:]
        return out


@contextlib.contextmanager
def engine_in_use():
    """The real engine when this host has an MI355X (then this IS the end-to-end drop-in run), else the double."""
    from attacking_federate_learning_amd import engine as engine_module
    saved = engine_module._default
    kind = 'hip'
    try:
        engine_module._default = None
        engine_module.get_engine()
    except Exception:
        engine_module._default = OracleBackedEngine()
        kind = 'oracle-double'
    try:
        yield kind
    finally:
        engine_module._default = saved


def check_reference_main_runs_unchanged_on_the_dropin_modules(engine_in_use, defense):
    with tempfile.TemporaryDirectory() as tmp:
        own = harness.run_reference_main(False, defense, os.path.join(tmp, 'own'))
        ours = harness.run_reference_main(True, defense, os.path.join(tmp, 'dropin'))
    # the unmodified driver files in both runs; only `defences` / `malicious` differ
    ref = os.path.realpath(harness.REFERENCE_DIR)
    assert own['modules']['main'] == ours['modules']['main'] == os.path.join(ref, 'main.py')
    assert own['modules']['server'] == ours['modules']['server'] == os.path.join(ref, 'server.py')
    assert own['modules']['defences'] == os.path.join(ref, 'defences.py')
    assert ours['modules']['defences'].endswith('attacking_federate_learning_amd/dropin/defences.py')
    assert ours['modules']['malicious'].endswith('attacking_federate_learning_amd/dropin/malicious.py')
    assert len(own['weights']) == len(ours['weights']) == 2
    for epoch in range(2):
        # same client gradients and the same attack went in ...
        if engine_in_use == 'oracle-double':
            assert np.array_equal(own['users_grads'][epoch], ours['users_grads'][epoch])
            assert np.array_equal(own['weights'][epoch], ours['weights'][epoch]), (defense, epoch)
        else:
            assert np.allclose(own['users_grads'][epoch], ours['users_grads'][epoch], rtol=1e-5, atol=1e-6)
            assert np.allclose(own['weights'][epoch], ours['weights'][epoch], rtol=1e-5, atol=1e-6), (defense, epoch)
    # the attack really happened: the malicious rows are one vector (malicious.py:26-27), the honest ones are not
    g = ours['users_grads'][1]
    assert np.array_equal(g[0], g[1]) and not np.array_equal(g[1], g[2])
    # and the rounds moved the weights
    assert not np.array_equal(own['weights'][0], own['weights'][1])


def check_server_defend_of_the_reference_calls_the_dropin_signature(engine_in_use):
    """`Server.defend` alone (server.py:86-90) on a hand-made server object: the exact call of server.py:87."""
    with harness.reference_imports(True):
        import server as ref_server
        import defences as bound
        srv = ref_server.Server.__new__(ref_server.Server)      # skip __init__ (data loaders): defend needs five fields
        rng = np.random.default_rng(3)
        n, d = 15, 400
        srv.users = [None] * n
        srv.mal_prop, srv.momentum, srv.learning_rate = 0.2, 0.9, 0.1
        srv.users_grads = rng.standard_normal((n, d)).astype(np.float32)
        for name in DEFENCES:
            srv.current_weights = rng.standard_normal(d).astype(np.float32)
            srv.velocity = rng.standard_normal(d).astype(np.float32)
            w0, v0, g0 = srv.current_weights.copy(), srv.velocity.copy(), srv.users_grads.copy()
            srv.defend(name, 0)
            agg = {'NoDefense': faithful.no_defense, 'Krum': faithful.krum, 'TrimmedMean': faithful.trimmed_mean,
                   'Bulyan': faithful.bulyan}[name](g0, n, int(n * 0.2))
            v1 = np.float32(0.9) * v0 - 0.1 * agg
            tol = dict(rtol=0, atol=0) if engine_in_use == 'oracle-double' else dict(rtol=1e-5, atol=1e-6)
            assert np.allclose(srv.velocity, v1, **tol) and np.allclose(srv.current_weights, w0 + v1, **tol)
            assert np.array_equal(srv.users_grads, g0)                      # the callee must not touch the matrix
        assert bound.defend is bound.defend and set(bound.defend) == set(DEFENCES)


def mint_or_check_the_golden_rounds(mint):
    """A compact record of the reference's rounds: the matrices the unmodified main loop handed to `Server.defend`
    (client gradients of the reference's own `User.step`, drifted by its own `DriftAttack`), cut to 3000 columns, and
    what the reference's own `Server.defend` (server.py:86-90, its own defences.py) makes of them over two rounds with
    momentum."""
    with tempfile.TemporaryDirectory() as tmp:
        runs = {d: harness.run_reference_main(False, d, os.path.join(tmp, d)) for d in DEFENCES}
    record = {}
    first = runs['NoDefense']['users_grads'][0]
    for d in DEFENCES:     # round 0 aggregates the same matrix whatever the defence (same seeds, same initial weights)
        assert np.array_equal(runs[d]['users_grads'][0], first)
    n = first.shape[0]
    cols = np.sort(np.random.default_rng(0).choice(first.shape[1], 3000, replace=False))
    record['round0_grads'] = np.ascontiguousarray(first[:, cols])
    rng = np.random.default_rng(1)
    record['weights_start'] = rng.standard_normal(len(cols)).astype(np.float32)
    record['mal_prop'] = np.float64(0.24)
    with harness.reference_imports(False):
        import server as ref_server
        for d in DEFENCES:
            record['%s/round1_grads' % d] = np.ascontiguousarray(runs[d]['users_grads'][1][:, cols])
            srv = ref_server.Server.__new__(ref_server.Server)
            srv.users, srv.mal_prop, srv.momentum, srv.learning_rate = [None] * n, 0.24, 0.9, 0.1
            srv.current_weights = record['weights_start'].copy()
            srv.velocity = np.zeros_like(srv.current_weights)
            for e, key in enumerate(('round0_grads', '%s/round1_grads' % d)):
                srv.users_grads = record[key].copy()
                srv.defend(d, e)
                record['%s/weights%d' % (d, e)] = srv.current_weights.copy()
    if mint or not os.path.exists(GOLDEN):
        np.savez_compressed(GOLDEN, **record)
    z = np.load(GOLDEN)
    assert sorted(z.files) == sorted(record)
    for key in record:
        assert np.array_equal(z[key], record[key]), key


def main(argv):
    if len(argv) not in (1, 2) or argv[1:] not in ([], ['--mint']):
        raise SystemExit('usage: make_golden_dropin.py REFERENCE_CHECKOUT [--mint]')
    harness.REFERENCE_DIR = os.path.realpath(argv[0])
    with engine_in_use() as kind:
        for defense in DEFENCES:
            check_reference_main_runs_unchanged_on_the_dropin_modules(kind, defense)
            print('main.py on the drop-in modules (%s): %s ok' % (kind, defense))
        check_server_defend_of_the_reference_calls_the_dropin_signature(kind)
        print('Server.defend on the drop-in modules (%s): ok' % kind)
    mint_or_check_the_golden_rounds('--mint' in argv)
    print('%s: %s' % (GOLDEN, 'written' if '--mint' in argv else 'matches the reference'))


if __name__ == '__main__':
    main(sys.argv[1:])
