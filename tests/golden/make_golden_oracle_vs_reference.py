#!/usr/bin/env python3
"""Mint tests/golden/oracle_vs_reference.npz by running the UNMODIFIED reference on the inputs of
tests/test_oracle_vs_reference.py, and tests/golden/reference_surface.json from the signatures of its drop-in surface.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_oracle_vs_reference.py REFERENCE_CHECKOUT

The reference's defences.py, malicious.py, backdoor.py, user.py and data_sets.py are imported from the checkout, never
copied; the packages they import that are not needed on the lines exercised (torchvision, and data_sets / user for
backdoor.py) are stubbed for the duration of the import.  The cases and inputs come from the test module itself, so
the record always answers exactly what the tests ask.  Recorded for every case: what the reference returned (its
distance dict as (pair, value) lists in its own order, Krum index and row, trimmed mean, Bulyan selection and aggregate,
the attack's rebound gradient and standard deviation, the backdoor hook's start parameters and gradient, four
clients' `User.step` gradients on one torch thread as their SHA-256, a fixed sample and per-client sums, norms and
largest magnitudes, with the canary that tells whether a host rounds torch's CPU kernels the same way) and whether it
raised where the tests expect an assertion.
"""
import importlib.util
import inspect
import json
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import test_oracle_vs_reference as T  # noqa: E402


def load(ref_dir, name, stubs=None):
    """The reference's `name`.py, with `stubs` in sys.modules for the duration of the import only."""
    saved = {k: sys.modules.get(k) for k in (stubs or {})}
    sys.modules.update(stubs or {})
    try:
        spec = importlib.util.spec_from_file_location('reference_' + name, os.path.join(ref_dir, name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, old in saved.items():
            if old is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = old
    return mod


def stub(name, **attrs):
    mod = types.ModuleType(name)
    mod.__dict__.update(attrs)
    return mod


def ref_selection(ref, g, n, f):
    dist = ref._krum_create_distances(g)
    picks = []
    while len(picks) < n - 2 * f:
        idx = ref.krum(g, n - len(picks), f, dist, True)
        picks.append(idx)
        dist.pop(idx)
        for r in dist:
            dist[r].pop(idx)
    return picks


def raises_assertion(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def record_cases(ref_d, ref_m, ref_backdoor, ref_data_sets, ref_user):
    import torch
    out = {}
    for kind in T.KINDS:
        for n, d, f in T.KRUM_CASES:
            key = T.case_key('krum', kind, n, d, f)
            g = T.matrices(100 + n, n, d, kind)
            dist = ref_d._krum_create_distances(g)
            pairs = [(i, j) for i in dist for j in dist[i]]
            values = [dist[i][j] for i, j in pairs]
            out[key + '/keys'] = np.array(list(dist.keys()), dtype=np.int64)
            out[key + '/pairs'] = np.array(pairs, dtype=np.int64).reshape(-1, 2)
            out[key + '/values'] = np.array(values, dtype=np.float32)
            out[key + '/all_float32'] = np.bool_(all(type(v) is np.float32 for v in values))
            out[key + '/index'] = np.int64(ref_d.krum(g, n, f, return_index=True))
            if n >= 2 * f + 1:
                out[key + '/krum'] = np.array(ref_d.krum(g, n, f))
        for n, d, c in T.TRIMMED_MEAN_CASES:
            g = T.matrices(200 + n, n, d, kind)
            out[T.case_key('trimmed_mean', kind, n, d, c) + '/out'] = ref_d.trimmed_mean(g, n, c)
        for n, d, f in T.BULYAN_CASES:
            key = T.case_key('bulyan', kind, n, d, f)
            g = T.matrices(300 + n, n, d, kind)
            out[key + '/selection'] = np.array(ref_selection(ref_d, g, n, f), dtype=np.int64)
            out[key + '/out'] = ref_d.bulyan(g, n, f)
    g = T.matrices(1, 6, 10, 'iid')
    out['assertions/krum_raises'] = np.bool_(raises_assertion(ref_d.krum, g, 6, 3))
    out['assertions/bulyan_raises'] = np.bool_(raises_assertion(ref_d.bulyan, g, 6, 3))
    out['assertions/krum_index'] = np.int64(ref_d.krum(g, 6, 3, return_index=True))
    for m, d, z in T.ATTACK_CASES:
        key = T.case_key('attack', m, d, z)
        users = [T.FakeUser(r.copy()) for r in T.attack_rows(m, d)]
        att = ref_m.DriftAttack(z)
        att.attack(users)
        out[key + '/grads0'] = np.array(users[0].grads)
        out[key + '/stdev'] = np.array(att.grads_stdev)
    for d, z, lr in T.BACKDOOR_CASES:
        key = T.case_key('backdoor', d, z, lr)
        mean, stdev, params, mal = T.backdoor_inputs(d)
        att = object.__new__(ref_backdoor.BackdoorAttack)     # the constructor builds data loaders
        att.num_std = z
        starts = []
        att.train_malicious_network = lambda start: (starts.append(start.copy()), mal)[1]
        out[key + '/grads'] = np.array(att._attack_grads(mean.copy(), stdev.copy(), params.copy(), lr))
        out[key + '/start'] = starts[0]
    weights, data, target = T.client_step_inputs()
    grads = []
    with T.one_torch_thread():
        for c in range(len(data)):
            usr = types.SimpleNamespace(user_id=c, is_malicious=False, momentum=0.9, data_set=ref_data_sets.MNIST,
                                        net=ref_data_sets.MnistNet(), criterion=torch.nn.NLLLoss(),
                                        train_iterator=iter([(torch.from_numpy(data[c]), torch.from_numpy(target[c]))]))
            usr.train = types.MethodType(ref_user.User.train, usr)
            ref_user.User.step(usr, weights, 0.1)
            grads.append(usr.grads)
        out['client_step/canary'] = np.str_(T.torch_arithmetic_canary())
    grads = np.stack(grads)
    rows = grads.astype(np.float64)
    out['client_step/shape'] = np.array(grads.shape, dtype=np.int64)
    out['client_step/sha256'] = np.str_(T.digest(grads))
    out['client_step/sample'] = grads[:, T.client_step_sample()]
    out['client_step/row_sums'] = rows.sum(axis=1)
    out['client_step/row_norms'] = np.sqrt((rows ** 2).sum(axis=1))
    out['client_step/row_max'] = np.abs(rows).max(axis=1)
    return out


def record_surface(ref_d, ref_m):
    sig = lambda fn: str(inspect.signature(fn))      # noqa: E731
    return {
        'defences': {name: sig(getattr(ref_d, name))
                     for name in ('no_defense', '_krum_create_distances', 'krum', 'trimmed_mean', 'bulyan')},
        'defend': list(ref_d.defend),
        'DefenseTypes': {attr: getattr(ref_d.DefenseTypes, attr) for attr in ('NoDefense', 'Krum', 'TrimmedMean', 'Bulyan')},
        'malicious': {'%s.%s' % (cls, meth): sig(getattr(getattr(ref_m, cls), meth))
                      for cls in ('Attack', 'DriftAttack') for meth in ('__init__', 'attack')},
        'DriftAttack._attack_grads': sig(ref_m.DriftAttack._attack_grads),
    }


def main(ref_dir):
    ref_d = load(ref_dir, 'defences')
    ref_m = load(ref_dir, 'malicious')
    ref_backdoor = load(ref_dir, 'backdoor', stubs={
        'malicious': ref_m, 'data_sets': stub('data_sets', MNIST='MNIST', CIFAR10='CIFAR10'),
        'user': stub('user', flatten_params=None, row_into_parameters=None, cycle=None)})
    tv = stub('torchvision', datasets=stub('torchvision.datasets'), transforms=stub('torchvision.transforms'))
    tv_stubs = {'torchvision': tv, 'torchvision.datasets': tv.datasets, 'torchvision.transforms': tv.transforms}
    ref_data_sets = load(ref_dir, 'data_sets', stubs=tv_stubs)
    ref_user = load(ref_dir, 'user', stubs=dict(tv_stubs, data_sets=ref_data_sets))

    out = record_cases(ref_d, ref_m, ref_backdoor, ref_data_sets, ref_user)
    path = os.path.join(HERE, 'oracle_vs_reference.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d arrays, %d bytes)' % (path, len(out), os.path.getsize(path)))
    path = os.path.join(HERE, 'reference_surface.json')
    with open(path, 'w') as fh:
        json.dump(record_surface(ref_d, ref_m), fh, indent=1)
        fh.write('\n')
    print('wrote %s' % path)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit('usage: make_golden_oracle_vs_reference.py REFERENCE_CHECKOUT')
    main(sys.argv[1])
