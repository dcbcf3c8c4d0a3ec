"""What the engine does with the FORM of an operand.  Every public method that takes a vector, an index list or a second
matrix beside the gradient matrix is run with the matrix as numpy, as a DeviceBuffer and as a torch CUDA tensor, and with
the other operands as numpy, DeviceBuffer (for a distance matrix: a `Distances` handle), torch CUDA and torch CPU.  During
the call `eng.lib` is a recording proxy: the test reads the ordered log of library calls and asserts

  1. the kind (numpy / DeviceBuffer / torch, and dtype) of everything returned, against CASES' hand-written table;
  2. that every form returns the all-torch form's bits;
  3. that the compute calls (everything but malloc, free, upload, download, stream_sync, ctx_check) with their integer and
     float arguments are those of tests/golden/engine_calls.json, minted by make_golden_engine_calls.py on the commit
     before the engine's marshalling was folded into one converter;
  4. that the all-torch form issues exactly the golden's calls, synchronisations included (the server's and benchmark's path);
  5. the lifetime rule: a device temporary the call itself allocated and uploaded is not freed while a kernel that was
     handed it may still run -- a synchronising call lies between the last such kernel and the free;
  6. that a wrong dtype, length or device is refused with the golden commit's exception type and text before any compute call.

A form a method does not take is part of the record too: the golden holds the exception's type, and it must not change.
REFUSALS holds the texts of the refusals as the golden commit worded them; they must not change either.
The shapes are the smallest that reach every branch of the marshalling: 11 rows (Bulyan needs 4 f + 3 with f = 2), 70
columns (more than one wavefront, no multiple of 4), a 7-row index list, two DnC lists of 16, a (3, 20) SignGuard window.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from attacking_federate_learning_amd import _native
from attacking_federate_learning_amd.engine import DeviceBuffer, Distances, dnc_columns

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'engine_calls.json')
N, F, D, K, S = 11, 2, 70, 7, 2
M_FORMS = ('torch', 'buffer', 'numpy')
A_FORMS = ('torch', 'buffer', 'numpy', 'cpu')
BOOKKEEPING = ('byz_malloc', 'byz_free', 'byz_upload', 'byz_download', 'byz_stream_sync', 'byz_ctx_check')
_OUT_TYPES = tuple(ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_uint32))


# ---- the recording proxy ----------------------------------------------------------------------------------------------
def _norm(a):
    """One argument of a library call, as plain data (after the call: byz_malloc's out-pointer is then filled in)."""
    if a is None:
        return 0
    if isinstance(a, (bool, int, np.integer)):
        return int(a)
    if isinstance(a, float):
        return a
    if isinstance(a, ctypes.c_void_p):
        return int(a.value or 0)
    if isinstance(a, ctypes.Array):
        return ['array', len(a)] if a._type_ is ctypes.c_void_p else ['array'] + [int(v) for v in a]
    obj = getattr(a, '_obj', None)                    # byref(...)
    if isinstance(obj, ctypes.c_void_p):
        return ['ref', int(obj.value or 0)]
    if isinstance(obj, ctypes.Structure):
        return ['struct'] + [getattr(obj, name) for name, _ in obj._fields_]
    if obj is not None:
        return 'out'
    raise TypeError('unrecorded argument %r' % (a,))


class Recorder:
    """Stands in for eng.lib: forwards every call and appends (name, args) to `log`."""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def forward(*args):
            rc = fn(*args)
            self.log.append((name, [_norm(a) for a in args]))
            return rc
        return forward


def compute_calls(log):
    """The ordered compute calls with what does not change from run to run: integers, floats, parameter structs, and for a
    pointer whether it was null."""
    out = []
    for name, args in log:
        if name in BOOKKEEPING or name == 'END':
            continue
        row = []
        for t, v in zip(_native._PROTOTYPES[name], args):
            row.append(('p' if v else 0) if t is ctypes.c_void_p else v)
        out.append([name, row])
    return out


def _synchronises(name, args):
    if name in ('byz_stream_sync', 'byz_ctx_check', 'byz_download'):
        return True
    return any(t in _OUT_TYPES and v == 'out' for t, v in zip(_native._PROTOTYPES.get(name, ()), args))


def lifetime_violations(log, result_ptrs=()):
    """Pointers the call allocated AND uploaded that were freed while a compute call that received them was not yet followed
    by a synchronising call.  Only what the engine call itself does counts: nothing after the END mark synchronises."""
    live, bad, ended = {}, [], False
    for name, args in log:
        if name == 'END':
            ended = True
        elif name == 'byz_malloc':
            live[args[2][1]] = {'uploaded': False, 'in_flight': None}
        elif name == 'byz_upload':
            if args[1] in live:
                live[args[1]]['uploaded'] = True
        elif name == 'byz_free':
            state = live.pop(args[1], None)
            if state and state['uploaded'] and state['in_flight'] and args[1] not in result_ptrs:
                bad.append(state['in_flight'])
        elif name not in BOOKKEEPING:
            for t, v in zip(_native._PROTOTYPES[name], args):
                if t is ctypes.c_void_p and v in live:
                    live[v]['in_flight'] = name
        if not ended and _synchronises(name, args):
            for state in live.values():
                state['in_flight'] = None
    return bad


# ---- operands ------------------------------------------------------------------------------------------------------------
def _host():
    rng = np.random.default_rng(20261019)
    h = {}
    g = rng.standard_normal((N, D)).astype(np.float32)
    g *= (1.0 + 0.5 * rng.permutation(N) / N).astype(np.float32)[:, None]
    h['g'] = g
    h['idx'] = np.array([9, 0, 4, 10, 2, 7, 5], dtype=np.int64)
    for name in ('z', 'root', 'start', 'x', 'add', 'mean', 'std', 'params', 'mal', 'velocity', 'memory'):
        h[name] = rng.standard_normal(D).astype(np.float32)
    h['std'] = np.abs(h['std'])
    h['w'] = rng.uniform(0.5, 2.0, N)
    h['scales'] = rng.uniform(0.1, 1.0, N)
    h['divisor'] = np.array([3.5])
    h['scale'] = np.array([1.25])
    h['perm'] = rng.permutation(N).astype(np.int32)
    h['cols2'] = dnc_columns(D, 16, 2, seed=5)
    h['cols1'] = h['cols2'][0].copy()
    h['sample'] = np.array([1, 4, 6, 8, 10], dtype=np.int32)
    h['votes'] = rng.integers(-N, N + 1, D).astype(np.int32)
    diff = g[:, None, :].astype(np.float64) - g[None, :, :].astype(np.float64)
    dist = np.sqrt((diff * diff).sum(-1)).astype(np.float32)
    np.fill_diagonal(dist, np.inf)
    h['dist'] = dist
    near = np.argsort(np.where(np.isinf(dist), -1.0, dist), axis=1, kind='stable')[:, :N - F]
    h['nbr'] = np.sort(near, axis=1).astype(np.int32)
    h['counts'] = np.full(N, N - F, dtype=np.int32)
    h['sq'] = (g.astype(np.float64) ** 2).sum(1)
    window = g[:, 3:23]
    h['pos'], h['zero'], h['neg'] = ((window > 0).sum(1), (window == 0).sum(1), (window < 0).sum(1))
    h['gram'] = g.astype(np.float64) @ g.astype(np.float64).T
    h['acc'] = np.zeros((K, K))
    return h


HOST = _host()
_DEVICE_DTYPE = {'idx': np.int32, 'cols1': np.int64, 'cols2': np.int64, 'pos': np.int64, 'zero': np.int64, 'neg': np.int64}


def in_form(eng, name, form):
    """A fresh copy of HOST[name] in one form (the in-place calls write their operands)."""
    a = HOST[name].copy()
    if form == 'numpy':
        return a
    import torch
    if form == 'cpu':
        return torch.from_numpy(a)
    a = a.astype(_DEVICE_DTYPE.get(name, a.dtype))
    if form == 'torch':
        return torch.from_numpy(a).to('cuda:%d' % eng.device)
    buf = eng.to_device(a)
    return Distances(buf, N) if name == 'dist' else buf


# ---- the cases: (matrix operand, the operands whose form varies, operands in the matrix's form, call, kinds) --------
def L(form, dtype):
    return {'numpy': 'numpy', 'cpu': 'torch', 'torch': 'torch', 'buffer': 'DeviceBuffer'}[form] + ':' + dtype


def mixed(m, a, dtype='float32'):
    """Same-length float32 vectors: torch beside any torch CUDA operand, else a DeviceBuffer beside any DeviceBuffer, else numpy."""
    return L('torch' if 'torch' in (m, a) else 'buffer' if 'buffer' in (m, a) else 'numpy', dtype)


def sel_kind(m):
    return 'torch:int32' if m == 'torch' else 'numpy:int32'


def dist_kind(a, dtype='int32'):
    return 'DeviceBuffer:' + dtype if a == 'buffer' else 'numpy:' + dtype


INT2 = {'clipped_rows': 'int', 'excluded_rows': 'int'}
SG = {'kept_rows': 'int', 'norm_failed_rows': 'int', 'outside_rows': 'int', 'clusters': 'int', 'seeds': 'int',
      'bandwidth': 'float', 'median_norm': 'float', 'window': ('int', 'int')}
FL = {'admitted': 'int', 'broken_rows': 'int', 'w_star': 'float'}

CASES = {
    # name: (matrix, varying, with the matrix, call(e, p, o), kinds(m, a))
    'no_defense': ('g', (), (), lambda e, p, o: e.no_defense(p), lambda m, a: L(m, 'float32')),
    'krum': ('g', (), (), lambda e, p, o: e.krum(p, N, F), lambda m, a: L(m, 'float32')),
    'krum_unchecked': ('g', (), (), lambda e, p, o: e.krum(p, N, F, check=False), lambda m, a: L(m, 'float32')),
    'krum_index': ('g', (), (), lambda e, p, o: e.krum(p, N, F, return_index=True), lambda m, a: 'int'),
    'trimmed_mean': ('g', (), (), lambda e, p, o: e.trimmed_mean(p, N, F), lambda m, a: L(m, 'float32')),
    'bulyan_selection': ('g', (), (), lambda e, p, o: e.bulyan(p, N, F, return_selection=True),
                         lambda m, a: (L(m, 'float32'), L(m, 'int32'))),
    'multi_krum_selection': ('g', (), (), lambda e, p, o: e.multi_krum(p, N, F, return_selection=True),
                             lambda m, a: (L(m, 'float32'), L(m, 'int32'))),
    'drift_attack': ('g', (), (), lambda e, p, o: e.drift_attack(p, 1.5), lambda m, a: (L(m, 'float32'),) * 3),
    'geometric_median_info': ('g', (), (), lambda e, p, o: e.geometric_median(p, return_info=True),
                              lambda m, a: (L(m, 'float32'), {'iterations': 'int', 'objective': 'float', 'excluded_rows': 'int',
                                                              'weights': L(m, 'float64')})),
    'robust_lr_votes': ('g', (), (), lambda e, p, o: e.robust_lr(p, 3, return_votes=True),
                        lambda m, a: (L(m, 'float32'), L(m, 'int32'))),
    'nnm_fused': ('g', (), (), lambda e, p, o: e.nnm(p, N, F, return_neighbours=True), lambda m, a: (L(m, 'float32'), L(m, 'int32'))),
    'sign_votes': ('g', (), (), lambda e, p, o: e.sign_votes(p), lambda m, a: L(m, 'int32')),
    'weak_dp_info': ('g', (), (), lambda e, p, o: e.weak_dp(p, clip=5.0, return_info=True),
                     lambda m, a: (L(m, 'float32'), dict(INT2, clip='float'))),
    'pairwise_distances': ('g', (), (), lambda e, p, o: e.pairwise_distances(p), lambda m, a: 'Distances'),
    'cosine_distances': ('g', (), (), lambda e, p, o: e.cosine_distances(p), lambda m, a: 'Distances'),
    'row_signs': ('g', (), (), lambda e, p, o: e.row_signs(p, 3, 20),
                  lambda m, a: (('torch:int64',) * 3 + ('torch:float64',) if m == 'torch' else
                                ('numpy:int64',) * 3 + (L(m, 'float64'),))),
    'trimmed_mean_rows': ('g', ('idx',), (), lambda e, p, o: e.trimmed_mean(p, N, F, row_index=o['idx']),
                          lambda m, a: L(m, 'float32')),
    'trimmed_mean_rows_vouched': ('g', ('idx',), (), lambda e, p, o: e.trimmed_mean(p, N, F, row_index=o['idx'], validate_index=False),
                                  lambda m, a: L(m, 'float32')),
    'coordinate_median_rows': ('g', ('idx',), (), lambda e, p, o: e.coordinate_median(p, row_index=o['idx']),
                               lambda m, a: L(m, 'float32')),
    'rank_trimmed_mean_rows': ('g', ('idx',), (), lambda e, p, o: e.rank_trimmed_mean(p, F, row_index=o['idx']),
                               lambda m, a: L(m, 'float32')),
    'mean_rows': ('g', ('idx',), (), lambda e, p, o: e.mean_rows(p, o['idx']), lambda m, a: L(m, 'float32')),
    'gram_share': ('g', ('idx',), (), lambda e, p, o: e.gram_share(p, o['idx'], 2, 0), lambda m, a: L(m, 'float64')),
    'gram_share_add': ('g', ('idx',), ('acc',), lambda e, p, o: e.gram_share_add(p, o['idx'], 2, 1, o['acc']),
                       lambda m, a: L(m, 'float64')),
    'row_sqdist': ('g', ('z',), (), lambda e, p, o: e.row_sqdist(p, o['z']), lambda m, a: L(m, 'float64')),
    'weighted_mean': ('g', ('w',), (), lambda e, p, o: e.weighted_mean(p, o['w']), lambda m, a: L(m, 'float32')),
    'weighted_mean_vouched': ('g', ('w',), (), lambda e, p, o: e.weighted_mean(p, o['w'], validate=False),
                              lambda m, a: L(m, 'float32')),
    'clip_update': ('g', ('z', 'scales'), (), lambda e, p, o: e.clip_update(p, o['z'], o['scales']), lambda m, a: L(m, 'float32')),
    'centered_clip_start': ('g', ('start',), (), lambda e, p, o: e.centered_clip(p, tau=4.0, start=o['start'], return_info=True),
                            lambda m, a: (L(m, 'float32'), dict(INT2, scales=L(m, 'float64')))),
    'row_dots': ('g', ('root',), (), lambda e, p, o: e.row_dots(p, o['root']), lambda m, a: (L(m, 'float64'),) * 2),
    'scaled_rows_sum': ('g', ('w', 'divisor'), (), lambda e, p, o: e.scaled_rows_sum(p, o['w'], o['divisor']),
                        lambda m, a: L(m, 'float32')),
    'fltrust': ('g', ('root',), (), lambda e, p, o: e.fltrust(p, o['root'], return_info=True),
                lambda m, a: (L(m, 'float32'), {'trusted_rows': 'int', 'excluded_rows': 'int', 'root_ok': 'bool', 'trust_sum': 'float',
                                                'trust': L(m, 'float64'), 'weights': L(m, 'float64')})),
    'signguard_select': ('sq', ('pos', 'zero', 'neg'), (),
                         lambda e, p, o: e.signguard_select(o['pos'], o['zero'], o['neg'], p, 20, sample=HOST['sample']),
                         lambda m, a: {k: ('torch:' if m == 'torch' else 'DeviceBuffer:') + t for k, t in
                                       (('keep', 'int32'), ('weights', 'float64'), ('labels', 'int32'), ('mk', 'float64'))}),
    'signguard': ('g', ('sample',), (), lambda e, p, o: e.signguard(p, window=(3, 20), sample=o['sample'], return_info=True),
                  lambda m, a: (L(m, 'float32'), dict(SG, keep=L(m, 'int32'), weights=L(m, 'float64'), labels=L(m, 'int32')))),
    'nnm_neighbours': (None, ('dist',), (), lambda e, p, o: e.nnm_neighbours(o['dist'], N - F), lambda m, a: (dist_kind(a),) * 2),
    'nnm_mix': ('g', ('nbr', 'counts'), (), lambda e, p, o: e.nnm_mix(p, o['nbr'], o['counts']), lambda m, a: L(m, 'float32')),
    'nnm_mix_no_counts': ('g', ('nbr',), (), lambda e, p, o: e.nnm_mix(p, o['nbr']), lambda m, a: L(m, 'float32')),
    'nnm_distances': ('g', ('dist',), (), lambda e, p, o: e.nnm(p, N, F, distances=o['dist'], return_neighbours=True),
                      lambda m, a: (L(m, 'float32'), L(m, 'int32'))),
    'sign_flip': ('x', ('votes',), (), lambda e, p, o: e.sign_flip(p, o['votes'], 4), lambda m, a: L(m, 'float32')),
    'bucket_means': ('g', ('perm',), (), lambda e, p, o: e.bucket_means(p, S, o['perm']), lambda m, a: L(m, 'float32')),
    'topk_sparsify_add': ('x', ('add',), (), lambda e, p, o: e.topk_sparsify(p, K, add=o['add'], return_info=True),
                          lambda m, a: ((L('numpy', 'float32') if m == 'numpy' else mixed(m, a),) * 2 +
                                        ({'selected': 'int', 'threshold_key': 'int', 'ties': 'int', 'ties_taken': 'int'},))),
    'topk_sparsify_in_place': ('memory', ('add',), (), lambda e, p, o: e.topk_sparsify(p, K, add=o['add'], out=o['add'], residual=p),
                               lambda m, a: (L(a, 'float32'), L(m, 'float32'))),
    'sparsefed_memory': ('g', ('memory',), (), lambda e, p, o: e.sparsefed(p, K, clip=5.0, residual=o['memory']),
                         lambda m, a: (L(m, 'float32'), L(a, 'float32'))),
    'sparsefed_fresh': ('g', (), (), lambda e, p, o: e.sparsefed(p, K, clip=5.0), lambda m, a: (L(m, 'float32'),) * 2),
    'gaussian_noise_scale': ('x', ('scale',), (), lambda e, p, o: e.gaussian_noise(p, 0.5, seed=3, round=2, scale=o['scale']),
                             lambda m, a: L(m, 'float32')),
    'gaussian_noise': ('x', (), (), lambda e, p, o: e.gaussian_noise(p, 0.5, seed=3, round=2), lambda m, a: L(m, 'float32')),
    'clip_scales': ('sq', (), (), lambda e, p, o: e.clip_scales(p, clip=8.0, return_clip=True), lambda m, a: (L(m, 'float64'),) * 2),
    'flame_distances': ('g', ('dist',), (), lambda e, p, o: e.flame(p, distances=o['dist'], seed=1, return_info=True),
                        lambda m, a: (L(m, 'float32'), dict(FL, clip='float', admitted_rows='numpy:int64'))),
    'flame_info': ('g', (), (), lambda e, p, o: e.flame(p, seed=1, return_info=True),
                   lambda m, a: (L(m, 'float32'), dict(FL, clip='float', admitted_rows='numpy:int64'))),
    'flame_select': (None, ('dist',), (), lambda e, p, o: e.flame_select(o['dist']), lambda m, a: ('numpy:int64', FL)),
    'flame_select_flags': (None, ('dist',), (), lambda e, p, o: e.flame_select(o['dist'], on_device=True),
                           lambda m, a: ('DeviceBuffer:int32', FL)),
    'flame_core_distances': (None, ('dist',), (), lambda e, p, o: e.flame_core_distances(o['dist'], 2), lambda m, a: 'numpy:float32'),
    'dnc_scores': ('g', ('cols1',), (), lambda e, p, o: e.dnc_scores(p, o['cols1']), lambda m, a: L(m, 'float64')),
    'dnc_select': ('g', ('cols2',), (), lambda e, p, o: e.dnc_select(p, F, o['cols2']), lambda m, a: sel_kind(m)),
    'dnc_selection': ('g', ('cols2',), (), lambda e, p, o: e.dnc(p, F, o['cols2'], return_selection=True),
                      lambda m, a: (L(m, 'float32'), sel_kind(m))),
    'dnc': ('g', ('cols2',), (), lambda e, p, o: e.dnc(p, F, o['cols2']), lambda m, a: L(m, 'float32')),
    'krum_select': (None, ('dist',), (), lambda e, p, o: e.krum_select(o['dist'], N, F), lambda m, a: 'int'),
    'bulyan_select': (None, ('dist',), (), lambda e, p, o: e.bulyan_select(o['dist'], N, F), lambda m, a: 'numpy:int32'),
    'bulyan_select_on_device': (None, ('dist',), (), lambda e, p, o: e.bulyan_select(o['dist'], N, F, on_device=True),
                                lambda m, a: 'DeviceBuffer:int32'),
    'krum_bulyan_select_on_device': (None, ('dist',), (), lambda e, p, o: e.krum_bulyan_select(o['dist'], N, F, on_device=True),
                                     lambda m, a: ('int', 'DeviceBuffer:int32')),
    'multi_krum_select': (None, ('dist',), (), lambda e, p, o: e.multi_krum_select(o['dist'], N, F), lambda m, a: 'numpy:int32'),
    'multi_krum_select_on_device': (None, ('dist',), (), lambda e, p, o: e.multi_krum_select(o['dist'], N, F, on_device=True),
                                    lambda m, a: 'DeviceBuffer:int32'),
    'krum_distances': ('g', ('dist',), (), lambda e, p, o: e.krum(p, N, F, distances=o['dist']),
                       lambda m, a: L('numpy' if m == 'buffer' else m, 'float32')),
    'multi_krum_distances': ('g', ('dist',), (), lambda e, p, o: e.multi_krum(p, N, F, distances=o['dist'], return_selection=True),
                             lambda m, a: (L(m, 'float32'), sel_kind(m))),
    'distances_from_gram': ('gram', (), (), lambda e, p, o: e.distances_from_gram(p, N), lambda m, a: 'Distances'),
    'cosine_from_gram': ('gram', (), (), lambda e, p, o: e.cosine_from_gram(p), lambda m, a: 'Distances'),
    'server_update': ('params', ('velocity',), ('mean',),
                      lambda e, p, o: (e.server_update(p, o['velocity'], o['mean'], 0.9, 0.1), p, o['velocity']),
                      lambda m, a: ('NoneType', L(m, 'float32'), L(a, 'float32'))),
    'backdoor_initial_params': ('params', ('mean',), (), lambda e, p, o: e.backdoor_initial_params(p, o['mean'], 0.1),
                                lambda m, a: mixed(m, a)),
    'backdoor_clip': ('mean', ('std', 'params'), ('mal',), lambda e, p, o: e.backdoor_clip(p, o['std'], o['params'], o['mal'], 0.1, 1.5),
                      lambda m, a: mixed(m, a)),
}


def forms_of(case):
    matrix, varying = CASES[case][0], CASES[case][1]
    a_forms = A_FORMS if varying else ('torch',)
    if case == 'server_update':
        a_forms = A_FORMS[:3]      # (it takes device pointers on the caller's word: a CPU tensor's would reach the kernel)
    return [(m, a) for m in (M_FORMS if matrix else ('torch',)) for a in a_forms]


def on_the_torch_path(case, m, a):
    """Everything the caller's own device-resident torch tensors (a distance matrix: the `Distances` handle)."""
    return m == 'torch' and (a == 'torch' or (a == 'buffer' and CASES[case][1] == ('dist',)))


def form_key(case, m, a):
    return '%s/%s/%s' % (case, m, a)


# ---- running one form ---------------------------------------------------------------------------------------------------
def kinds_of(r):
    if isinstance(r, tuple):
        return tuple(kinds_of(v) for v in r)
    if isinstance(r, dict):
        return {k: kinds_of(v) for k, v in r.items()}
    if isinstance(r, np.ndarray):
        return 'numpy:' + r.dtype.name
    if isinstance(r, DeviceBuffer):
        return 'DeviceBuffer:' + r.dtype.name
    if isinstance(r, Distances):
        return 'Distances'
    if type(r).__module__.split('.')[0] == 'torch':
        return 'torch:' + str(r.dtype).split('.')[-1]
    return type(r).__name__


def values_of(r):
    """The result as host data, flattened: arrays as (dtype, shape, bytes)."""
    if isinstance(r, (tuple, list)):
        return [values_of(v) for v in r]
    if isinstance(r, dict):
        return {k: values_of(v) for k, v in sorted(r.items())}
    if isinstance(r, (DeviceBuffer, Distances)):
        r = r.numpy()
    elif type(r).__module__.split('.')[0] == 'torch':
        r = r.detach().cpu().numpy()
    if isinstance(r, np.ndarray):
        return (r.dtype.name, r.shape, np.ascontiguousarray(r).tobytes())
    return r


def result_pointers(r):
    if isinstance(r, (tuple, list)):
        return set().union(*[result_pointers(v) for v in r]) if r else set()
    if isinstance(r, dict):
        return result_pointers(tuple(r.values()))
    if isinstance(r, (DeviceBuffer, Distances)):
        return {r.ptr}
    return set()


def run_form(eng, case, m, a):
    """-> {'raises': type name, 'log'} or {'kinds', 'values', 'log', 'violations'}."""
    matrix, varying, with_matrix, call, _ = CASES[case]
    primary = in_form(eng, matrix, m) if matrix else None
    others = {name: in_form(eng, name, a) for name in varying}
    others.update({name: in_form(eng, name, m) for name in with_matrix})
    eng.synchronize()
    real, rec = eng.lib, Recorder(eng.lib)
    eng.lib = rec
    try:
        try:
            result = call(eng, primary, others)
        except Exception as exc:      # noqa: BLE001  (a refusal is part of the record)
            return {'raises': type(exc).__name__, 'log': rec.log}
        rec.log.append(('END', []))
        out = {'kinds': kinds_of(result), 'values': values_of(result), 'pointers': result_pointers(result)}
        del result
        out['log'] = rec.log
        out['violations'] = lifetime_violations(rec.log, out.pop('pointers'))
        return out
    finally:
        eng.lib = real
        eng.check()


def names_of(log):
    return [name for name, _ in log if name != 'END']


def jsonable(x):
    return json.loads(json.dumps(x))


SYNCS = ('byz_stream_sync', 'byz_ctx_check')


def write_golden(path, commit, forms, lacks):
    """forms: key -> {'raises'} or {'compute', 'names'}.  Equal compute lists are stored once; the full list of names is kept
    for the forms on the torch path only (assertion 4), the others keep their number of synchronisations."""
    unique, packed = [], {}
    for key, rec in forms.items():
        case, rest = key.split('/', 1)
        if 'raises' in rec:
            entry = rec['raises']
        else:
            if rec['compute'] not in unique:
                unique.append(rec['compute'])
            entry = [unique.index(rec['compute']), len([n for n in rec['names'] if n in SYNCS])]
            if on_the_torch_path(*key.split('/')):
                entry.append(rec['names'])
        packed.setdefault(case, {})[rest] = entry
    with open(path, 'w') as fh:
        fh.write('{"commit": %s,\n "parent_lacks_sync": %s,\n "compute": [\n' % (json.dumps(commit), json.dumps(lacks)))
        fh.write(',\n'.join('  ' + json.dumps(c, separators=(',', ':')) for c in unique))
        fh.write('\n ],\n "forms": {\n')
        fh.write(',\n'.join('  %s: %s' % (json.dumps(c), json.dumps(v, separators=(',', ':'))) for c, v in packed.items()))
        fh.write('\n }}\n')


def load_golden():
    """-> {'commit', 'parent_lacks_sync', 'forms': key -> {'raises'} or {'compute', 'syncs', 'names' (torch path only)}}"""
    table = json.load(open(GOLDEN))
    forms = {}
    for case, by_form in table['forms'].items():
        for rest, entry in by_form.items():
            forms[case + '/' + rest] = {'raises': entry} if isinstance(entry, str) else dict(
                zip(('compute', 'syncs', 'names'), [table['compute'][entry[0]]] + entry[1:]))
    return dict(table, forms=forms)


# ---- the tests ----------------------------------------------------------------------------------------------------------
def test_the_golden_names_every_form_of_every_case():
    table = load_golden()
    assert len(table['commit']) >= 7
    for case in CASES:
        for m, a in forms_of(case):
            rec = table['forms'][form_key(case, m, a)]
            assert 'raises' in rec or (rec['compute'] and ('names' in rec) == on_the_torch_path(case, m, a))
        assert any('raises' not in table['forms'][form_key(case, m, a)] for m, a in forms_of(case) if on_the_torch_path(case, m, a))
    assert all(key in table['forms'] for key in table['parent_lacks_sync'])
    assert not any(on_the_torch_path(*key.split('/')) for key in table['parent_lacks_sync'])


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_every_form_of_the_operands(eng, case):
    table = load_golden()
    kinds, reference = CASES[case][4], None
    for m, a in forms_of(case):                      # (the torch forms come first)
        key = form_key(case, m, a)
        want, got = table['forms'][key], run_form(eng, case, m, a)
        print(key, got.get('raises') or names_of(got['log']), got.get('violations'))
        assert got.get('raises') == want.get('raises'), key
        if 'raises' in got:
            assert not compute_calls(got['log']), key          # refused before anything was launched
            continue
        assert jsonable(got['kinds']) == jsonable(kinds(m, a)), key                   # 1
        if reference is None:
            reference = got['values']
        assert got['values'] == reference, key                                        # 2
        assert jsonable(compute_calls(got['log'])) == want['compute'], key            # 3
        names = names_of(got['log'])
        if on_the_torch_path(case, m, a):
            assert names == want['names'], key                                        # 4
        if key not in table['parent_lacks_sync']:
            assert len([n for n in names if n in SYNCS]) <= want['syncs'], key
        assert not got['violations'], key                                             # 5


REFUSALS = {
    # name: (the golden commit's text, the call)
    # the fp32 vectors that are used where they are (a torch tensor of another dtype or layout is refused)
    'fp32 dtype': ('device vectors must be contiguous float32', lambda e, t: e.row_sqdist(t['g'], t['z'].double())),
    'fp32 layout': ('device vectors must be contiguous float32', lambda e, t: e.row_sqdist(t['g'], t['z'].repeat_interleave(2)[::2])),
    'fp32 length': ('z has 69 entries, the matrix 70 columns', lambda e, t: e.row_sqdist(t['g'], t['z'][:-1])),
    'fp32 lengths': ('vector lengths differ: 70 and 69', lambda e, t: e.backdoor_initial_params(t['z'], HOST['z'][:-1], 0.1)),
    'fp32 out device': ('out must be a device-resident float32 vector of 70 entries', lambda e, t: e.topk_sparsify(t['z'], K, out=t['z'].cpu())),
    'fp32 out length': ('out has 69 entries, expected 70', lambda e, t: e.gaussian_noise(t['z'], 0.5, out=t['z'][:-1])),
    # the fp64 vectors that are converted
    'fp64 dtype': ('a DeviceBuffer here must hold 11 float64 values', lambda e, t: e.weighted_mean(t['g'], e.to_device(HOST['w'].astype(np.float32)))),
    'fp64 length': ('expected 11 values, got 10', lambda e, t: e.weighted_mean(t['g'], t['w'][:-1])),
    'fp64 host length': ('expected 1 values, got 11', lambda e, t: e.scaled_rows_sum(t['g'], HOST['w'], HOST['w'])),
    # int32 vectors and lists
    'int32 dtype': ('votes must be integers, got float32', lambda e, t: e.sign_flip(t['z'], HOST['votes'].astype(np.float32), 4)),
    'int32 buffer dtype': ('a DeviceBuffer of perm entries must hold 11 int32 values', lambda e, t: e.bucket_means(t['g'], S, e.to_device(HOST['perm'].astype(np.int64)))),
    'int32 length': ('expected 70 votes, got 69', lambda e, t: e.sign_flip(t['z'], t['votes'][:-1], 4)),
    'lists dtype': ('neighbour lists must hold integers, got float32', lambda e, t: e.nnm_mix(t['g'], HOST['nbr'].astype(np.float32))),
    'lists shape': ('expected 11 lists, got shape (10, 9)', lambda e, t: e.nnm_mix(t['g'], t['nbr'][:-1])),
    'lists counts shape': ('expected 11 lengths, got shape (11, 9)', lambda e, t: e.nnm_mix(t['g'], t['nbr'], t['nbr'])),
    # row indices
    'rows dtype': ('row_index must hold integers, got float32', lambda e, t: e.mean_rows(t['g'], HOST['idx'].astype(np.float32))),
    'rows torch dtype': ('row_index must hold integers, got torch.float32', lambda e, t: e.mean_rows(t['g'], t['idx'].float())),
    'rows buffer dtype': ('a DeviceBuffer row_index must hold int32', lambda e, t: e.mean_rows(t['g'], e.to_device(HOST['idx']))),
    'rows device': ('row_index must live on the GPU of the matrix (cuda:', lambda e, t: e.mean_rows(t['g'], t['idx'].cpu())),
    'rows range': ('row_index out of range: [11, 21] for 11 rows', lambda e, t: e.mean_rows(t['g'], t['idx'] + N)),
    'rows host range': ('row_index out of range: [-1, 9] for 11 rows', lambda e, t: e.trimmed_mean(t['g'], N, F, row_index=HOST['idx'] - 1)),
    'rows empty': ('row_index selects no rows', lambda e, t: e.mean_rows(t['g'], t['idx'][:0])),
    # DnC's int64 lists
    'columns dtype': ('device column lists must be a non-empty 1-D or 2-D int64 tensor on cuda:', lambda e, t: e.dnc(t['g'], F, t['cols2'].int())),
    'columns host dtype': ('column lists must be a non-empty 1-D or 2-D integer array', lambda e, t: e.dnc(t['g'], F, HOST['cols2'].astype(np.float64))),
    'columns range': ('column lists must be in [0, 70) and strictly ascending', lambda e, t: e.dnc(t['g'], F, t['cols2'] + D)),
    'columns count': ('dnc_scores() takes one list of columns', lambda e, t: e.dnc_scores(t['g'], t['cols2'])),
    # the second matrix
    'accumulator dtype': ('the accumulator must be a contiguous float64 CUDA tensor', lambda e, t: e.gram_share_add(t['g'], t['idx'], 2, 0, t['acc'].float())),
    'accumulator device': ('the accumulator must be a contiguous float64 CUDA tensor', lambda e, t: e.gram_share_add(t['g'], t['idx'], 2, 0, t['acc'].cpu())),
    'accumulator shape': ('the accumulator must be 7 x 7', lambda e, t: e.gram_share_add(t['g'], t['idx'], 2, 0, t['gram'])),
    'out shape': ('out must be a device-resident 11 x 70 float32 matrix', lambda e, t: e.nnm_mix(t['g'], t['nbr'], out=t['g'][:-1])),
    'memory on the host': ('residual must be a device-resident float32 vector of 70 entries', lambda e, t: e.sparsefed(t['g'], K, residual=HOST['memory'])),
    'memory on the device': ('a host matrix takes a host memory', lambda e, t: e.sparsefed(HOST['g'], K, residual=t['memory'])),
    'matrix dtype': ('device matrices must be 2-D float32 with unit column stride', lambda e, t: e.no_defense(t['g'].double())),
    'matrix on the host': ('mean_rows() takes a device-resident matrix', lambda e, t: e.mean_rows(HOST['g'], HOST['idx'])),
    'rows beyond int32': ('row_index out of range: [4294967296, 4294967306] for 11 rows',
                          lambda e, t: e.mean_rows(t['g'], HOST['idx'] + 2 ** 32)),
    'flip out length': ('out must be a device-resident float32 vector of 70 entries',
                        lambda e, t: e.sign_flip(t['z'], t['votes'], 4, out=t['z'][:-1])),
    'accumulator on the host': ('the accumulator must be a torch CUDA tensor or a DeviceBuffer',
                                lambda e, t: e.gram_share_add(t['g'], t['idx'], 2, 0, HOST['acc'])),
    'accumulator buffer dtype': ('the accumulator must be float64',
                                 lambda e, t: e.gram_share_add(t['g'], t['idx'], 2, 0, e.to_device(HOST['acc'].astype(np.float32)))),
    'lists buffer dtype': ('a DeviceBuffer of neighbour lists must hold int32',
                           lambda e, t: e.nnm_mix(t['g'], e.to_device(HOST['nbr'].astype(np.int64)))),
    'fp32 buffer dtype': (AssertionError, lambda e, t: e.row_sqdist(t['g'], e.to_device(HOST['z'].astype(np.float64)))),
}


@pytest.mark.gpu
@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_a_wrong_operand_is_refused_before_anything_is_launched(eng, what):
    t = {name: in_form(eng, name, 'torch') for name in ('g', 'z', 'w', 'votes', 'nbr', 'idx', 'cols2', 'acc', 'gram', 'memory')}
    real, rec = eng.lib, Recorder(eng.lib)
    eng.lib = rec
    try:
        text, call = REFUSALS[what]
        with pytest.raises(*((text,) if isinstance(text, type) else (ValueError,)), match=None if isinstance(text, type) else re.escape(text)):
            call(eng, t)
    finally:
        eng.lib = real
    assert not compute_calls(rec.log)


@pytest.mark.gpu
def test_an_operand_on_another_gpu_is_refused(eng):
    import torch
    other = [i for i in range(torch.cuda.device_count()) if i != eng.device]
    if not other:
        pytest.skip('needs a second GPU: the refusals of an operand on another device are not exercised here')
    g = in_form(eng, 'g', 'torch')
    real, rec = eng.lib, Recorder(eng.lib)
    eng.lib = rec
    try:
        for dev in other[:1]:
            for call in (lambda: eng.weighted_mean(g, in_form(eng, 'w', 'torch').to('cuda:%d' % dev)),
                         lambda: eng.bucket_means(g, S, in_form(eng, 'perm', 'torch').to('cuda:%d' % dev)),
                         lambda: eng.nnm_mix(g, in_form(eng, 'nbr', 'torch').to('cuda:%d' % dev)),
                         lambda: eng.mean_rows(g, in_form(eng, 'idx', 'torch').to('cuda:%d' % dev)),
                         lambda: eng.dnc(g, F, in_form(eng, 'cols2', 'torch').to('cuda:%d' % dev)),
                         lambda: eng.no_defense(g.to('cuda:%d' % dev))):
                with pytest.raises(ValueError):
                    call()
    finally:
        eng.lib = real
    assert not compute_calls(rec.log)
