"""The robust learning rate (Ozdayi, Kantarcioglu and Gel, AAAI 2021) restated in numpy, and the CPU checks of its surface.

The restatement is the contract the GPU file (tests/test_gpu_robust_lr.py) holds the kernels to, bit for bit:

    votes[c] = #{r : g[r, c] > 0} - #{r : g[r, c] < 0}           int32
    flip[c]  = abs(votes[c]) < theta
    out[c]   = -agg[c] where flip[c] (the sign bit inverted), agg[c] verbatim elsewhere

Every quantity is an integer count or a sign bit: no tolerance appears anywhere."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('byz_sign_votes_dev', 'byz_sign_flip_dev', 'byz_robust_lr_dev', 'byz_robust_lr_info', 'byz_robust_lr_host')


# ---- the restatement ------------------------------------------------------------------------------------------------------
def restated_votes(g):
    g = np.asarray(g, dtype=np.float32)
    return (g > 0).sum(0, dtype=np.int32) - (g < 0).sum(0, dtype=np.int32)


def check_theta(theta, n):
    if isinstance(theta, bool) or int(theta) != theta or not 0 <= int(theta) <= n:
        raise ValueError('theta = %r outside 0..%d' % (theta, n))
    return int(theta)


def restated_flip(agg, votes, theta):
    """agg with its sign bit inverted where abs(votes) < theta: np.where(flip, -agg, agg), written on the bits so that the
    restatement says by itself that a zero becomes -0.0 and a NaN keeps its payload."""
    agg = np.ascontiguousarray(agg, dtype=np.float32)
    flip = np.abs(np.asarray(votes, dtype=np.int64)) < int(theta)
    return (agg.view(np.uint32) ^ np.where(flip, np.uint32(0x80000000), np.uint32(0))).view(np.float32)


def model_mean(g):
    """no_defense's vector by the model in column_stats.hip's header: a sequential fp32 chain from +0.0 in row order, then
    / float(n) (tests/test_oracle_golden.py pins the model to np.mean(g, axis=0) itself)."""
    g = np.asarray(g, dtype=np.float32)
    s = np.zeros(g.shape[1], dtype=np.float32)
    with np.errstate(all='ignore'):
        for row in g:
            s = s + row
        return s / np.float32(g.shape[0])


def restated_robust_lr(g, theta, agg=None):
    g = np.asarray(g, dtype=np.float32)
    theta = check_theta(theta, g.shape[0])
    return restated_flip(model_mean(g) if agg is None else agg, restated_votes(g), theta)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


DENORMAL = np.float32(1e-45)        # the smallest positive fp32 denormal


def special_columns(n):
    """(n x 16 matrix, its votes by hand) for n >= 4: all positive, all negative, exactly balanced, zeros, NaN, infinities
    and denormals."""
    assert n >= 4
    inf, nan, h = np.float32(np.inf), np.float32(np.nan), n // 2
    cols, want = [], []

    def add(values, votes):
        cols.append(np.asarray(values, dtype=np.float32))
        want.append(votes)

    add(np.full(n, 2.5), n)                                             # 0: all positive
    add(np.full(n, -0.75), -n)                                          # 1: all negative
    add([1.0] * h + [-1.0] * h + [0.0] * (n - 2 * h), 0)                # 2: exactly balanced
    add(np.zeros(n), 0)                                                 # 3: +0.0 casts no vote
    add(np.full(n, -0.0), 0)                                            # 4: nor does -0.0
    add(np.full(n, nan), 0)                                             # 5: nor NaN
    add(np.full(n, -nan), 0)                                            # 6: of either sign bit
    add(np.full(n, inf), n)                                             # 7: +inf votes by its sign
    add(np.full(n, -inf), -n)                                           # 8: and so does -inf
    add(np.full(n, DENORMAL), n)                                        # 9: denormals vote by their sign
    add(np.full(n, -DENORMAL), -n)                                      # 10
    add([nan, 3.0] + [0.0] * (n - 2), 1)                                # 11: a NaN next to one vote
    add([inf, inf] + [-DENORMAL] * (n - 2), 4 - n)                      # 12: two infinities are two votes, no more
    add([-0.0, 0.0, 5.0, -5.0] + [7.0] * (n - 4), n - 4)                # 13
    add([nan] * (n - 1) + [-1e-38], -1)                                 # 14: one negative denormal among NaN
    add([3.4e38, -3.4e38] + [1.0] * (n - 2), n - 2)                     # 15: the largest magnitudes, of both signs
    assert len(cols) == 16
    with np.errstate(all='ignore'):
        return np.stack(cols, axis=1).astype(np.float32), np.asarray(want, dtype=np.int32)


# ---- the restatement against the definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [4, 7, 20])
def test_votes_of_special_values(n):
    g, want = special_columns(n)
    assert g[0, 9] != 0 and g[0, 9] == DENORMAL and np.signbit(g[0, 4]) and np.signbit(g[0, 6])
    votes = restated_votes(g)
    assert votes.dtype == np.int32 and np.array_equal(votes, want)
    # the same decision on the bits alone, as the kernel takes it: sign bit, then magnitude in (0, 0x7f800000]
    u = g.view(np.uint32)
    mag = u & np.uint32(0x7fffffff)
    voting = (mag > 0) & (mag <= np.uint32(0x7f800000))
    by_bits = np.where(voting, np.where(u >> np.uint32(31) == 1, -1, 1), 0).sum(0, dtype=np.int32)
    assert np.array_equal(by_bits, want)
    # ... and in the kernel's own form: one unsigned compare of mag - 1 (0 wraps to the top), the vote (bits >> 31) | 1
    wrapped = (mag - np.uint32(1)) < np.uint32(0x7f800000)
    kernel_form = np.where(wrapped, (g.view(np.int32) >> 31) | 1, 0).sum(0, dtype=np.int32)
    assert np.array_equal(kernel_form, want)


def test_flip_inverts_the_sign_bit_and_nothing_else():
    agg = np.array([1.5, -2.0, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45], dtype=np.float32)
    agg.view(np.uint32)[6] = 0x7fc12345             # a NaN with a payload
    votes = np.zeros(8, dtype=np.int32)
    out = restated_flip(agg, votes, 1)
    assert np.array_equal(bits(out), bits(agg) ^ np.uint32(0x80000000))
    assert bits(out)[6] == 0xffc12345 and bits(out)[2] == 0x80000000 and bits(out)[3] == 0
    assert np.array_equal(bits(restated_flip(agg, votes, 0)), bits(agg))
    with np.errstate(all='ignore'):
        where = np.where(np.abs(votes) < 1, -agg, agg)
    assert np.array_equal(bits(out), bits(where))


def semantic_case():
    """n = 20, f = 4: the 16 honest rows agree in sign on columns A, split 8 / 8 on columns B, where the 4 attackers put one
    large positive value."""
    n, f, a, b = 20, 4, 12, 9
    rng = np.random.default_rng(20)
    g = np.empty((n, a + b), dtype=np.float32)
    signs = np.where(rng.random(a) < 0.5, -1.0, 1.0).astype(np.float32)
    g[:, :a] = signs * (0.5 + rng.random((n, a))).astype(np.float32)         # everybody agrees on A, the attackers included
    honest_b = (0.5 + rng.random((n - f, b))).astype(np.float32)
    honest_b[8:] *= -1
    g[f:, a:] = honest_b
    g[:f, a:] = 50.0
    return g, n, f, a


def test_semantic_case_the_backdoor_columns_are_negated():
    g, n, f, a = semantic_case()
    mean = model_mean(g)
    assert np.array_equal(bits(mean), bits(np.mean(g, axis=0)))
    assert (mean[a:] > 0).all()                          # the plain mean follows the attackers on all of B
    votes = restated_votes(g)
    assert (np.abs(votes[:a]) == n).all() and (votes[a:] == f).all()
    out = restated_robust_lr(g, f + 1)
    assert (out[a:] < 0).all()
    assert np.array_equal(bits(out[:a]), bits(mean[:a]))
    assert np.array_equal(bits(out[a:]), bits(-mean[a:]))
    assert np.array_equal(np.sign(votes[:a]), np.sign(mean[:a]).astype(np.int32))       # signSGD's majority vote, for free


def test_thresholds_and_ranges():
    g, n, f, a = semantic_case()
    g = np.concatenate([g, special_columns(n)[0]], axis=1)
    mean = model_mean(g)
    assert np.array_equal(bits(restated_robust_lr(g, 0)), bits(mean))
    votes = restated_votes(g)
    unanimous = np.abs(votes) == n
    assert unanimous.any() and (~unanimous).any()
    out = restated_robust_lr(g, n)
    assert np.array_equal(bits(out)[unanimous], bits(mean)[unanimous])
    assert np.array_equal(bits(out)[~unanimous], bits(mean)[~unanimous] ^ np.uint32(0x80000000))
    for bad in (-1, n + 1, 2.5, True):
        with pytest.raises(ValueError):
            restated_robust_lr(g, bad)
    agg = np.median(g[:, :a], axis=0).astype(np.float32)
    assert np.array_equal(bits(restated_robust_lr(g[:, :a], f + 1, agg=agg)), bits(agg))   # unanimous columns: verbatim


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def header_text():
    return open(os.path.join(ROOT, 'include', 'byzagg.h')).read()


def test_the_header_declares_the_new_entry_points_and_keeps_the_abi_version():
    text = header_text()
    assert '#define BYZ_ABI_VERSION 1\n' in text
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    assert not re.search(r'\bbyz_(robust_lr|sign_votes|sign_flip)\w*sharded', code)     # column-local: no sharded entry point
    assert 'columns layout' in text[text.index('robust learning rate'):text.index('byz_robust_lr_host')]


def test_the_ctypes_table_lists_them():
    import ctypes
    from attacking_federate_learning_amd import _native
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS, name
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    assert _native._PROTOTYPES['byz_robust_lr_dev'] == [vp, vp, i64, i64, i64, i64, vp, vp, vp]
    assert _native._PROTOTYPES['byz_sign_flip_dev'] == [vp, vp, vp, i64, i64, vp, vp]


def test_the_sources_are_on_every_build_list():
    from attacking_federate_learning_amd import build_native
    assert 'robust_lr.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['robust_lr.hip']


def test_python_surface():
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.robust_lr)) == (
        '(users_grads, users_count, corrupted_count, theta=None, then=None, return_votes=False, **then_kwargs)')
    assert 'robust_lr' not in defences.defend and defences.robust_lr not in defences.defend.values()
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert 'corrupted_count + 1' in defences.robust_lr.__doc__
    assert str(inspect.signature(Engine.sign_votes)) == '(self, g)'
    assert list(inspect.signature(Engine.sign_flip).parameters)[:4] == ['self', 'agg', 'votes', 'theta']
    assert str(inspect.signature(Engine.robust_lr)) == '(self, g, theta, return_votes=False)'
    assert str(inspect.signature(Engine.robust_lr_info)) == '(self)'
    assert str(inspect.signature(DeviceServer.defend_robust_lr)) == '(self, theta=None, then=None, **then_kwargs)'
    assert str(inspect.signature(ShardedAggregator.robust_lr)) == (
        '(self, g_local, users_count, corrupted_count, theta=None, gather=False, total_columns=None)')
    assert callable(HipKernels.sign_votes) and callable(HipKernels.robust_lr)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    from attacking_federate_learning_amd import defences
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_rlr', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.robust_lr is defences.robust_lr and 'robust_lr' not in mod.defend


def test_theta_is_checked_before_anything_reaches_a_kernel():
    from attacking_federate_learning_amd.engine import Engine
    assert Engine._theta(0, 5) == 0 and Engine._theta(5, 5) == 5 and Engine._theta(np.int64(3)) == 3
    for bad in (-1, 6, 2.5, True):
        with pytest.raises(ValueError):
            Engine._theta(bad, 5)


def test_the_documents_name_the_new_entry_points():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert name in integration, name
    assert '3.4h' in open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'robust_lr_timing.md' in open(os.path.join(ROOT, 'profiles', 'INDEX.md')).read()
