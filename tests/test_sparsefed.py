"""SparseFed without a GPU: the numpy restatement of the global top-k (include/byzagg.h) that
tests/test_gpu_sparsefed.py holds the kernels to bit for bit, its own properties, and the public surface (names and signatures
at every layer, not a `defend` key).

The restatement: w = x or fl32(x + add); key = bits(w) & 0x7fffffff; the first k entries of a STABLE descending sort of the
keys are selected (a stable sort breaks ties by the lower column); out and residual are np.where on w and a +0.0 vector."""
import inspect
import os
import re

import numpy as np
import pytest

from tests.test_centered_clip import restated_centered_clip
from tests.test_geometric_median import attacked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ('byz_topk_sparsify_dev', 'byz_topk_info', 'byz_topk_sparsify_host', 'byz_sparsefed_dev', 'byz_sparsefed_host',
               'byz_topk_sparsify_sharded_dev')
NO_KEY = 0xffffffff          # the threshold reported for k = 0: above every key

# the sixteen special values the GPU tests plant: +-0, +-NaN with two payloads, +-inf, +-1e-45, +-1e-38, +-3.4e38, +-1, 2.5, -0.75
SPECIAL_BITS = np.array([0x00000000, 0x80000000, 0x7fc00001, 0xffc00123, 0x7f800000, 0xff800000, 0x00000001, 0x80000001],
                        dtype=np.uint32)
SPECIALS = np.concatenate([SPECIAL_BITS.view(np.float32),
                           np.array([1e-38, -1e-38, 3.4e38, -3.4e38, 1.0, -1.0, 2.5, -0.75], dtype=np.float32)])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the restatement -------------------------------------------------------------------------------------------------
def restated_w(x, add=None):
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if add is None:
        return x.copy()
    with np.errstate(over='ignore', invalid='ignore'):
        return (x + np.ascontiguousarray(add, dtype=np.float32).reshape(-1)).astype(np.float32)


def restated_topk(x, k, add=None, return_info=False):
    """(out, residual) of the global top-k, w's bits verbatim; return_info=True adds {selected, threshold_key, ties,
    ties_taken, mask}."""
    w = restated_w(x, add)
    n = w.size
    if isinstance(k, (bool, np.bool_)) or int(k) != k or not 0 <= int(k) <= n:
        raise ValueError('k = %r outside 0..%d' % (k, n))
    k = int(k)
    key = bits(w) & np.uint32(0x7fffffff)
    order = np.argsort(-key.astype(np.int64), kind='stable')
    mask = np.zeros(n, dtype=bool)
    mask[order[:k]] = True
    zero = np.zeros(n, dtype=np.float32)
    out, residual = np.where(mask, w, zero), np.where(mask, zero, w)
    if not return_info:
        return out, residual
    if k == 0:
        info = {'selected': 0, 'threshold_key': NO_KEY, 'ties': 0, 'ties_taken': 0}
    else:
        t = int(key[order[k - 1]])
        info = {'selected': k, 'threshold_key': t, 'ties': int((key == t).sum()), 'ties_taken': k - int((key > t).sum())}
    info['mask'] = mask
    return out, residual, info


def restated_sparsefed(g, k, clip=10.0, residual=None):
    """(out, residual, aggregate): the norm-clipped mean (centered clipping from zero, one iteration), added to the memory,
    the top-k of the sum."""
    agg, _ = restated_centered_clip(g, tau=clip, iters=1, start=None)
    memory = np.zeros(agg.size, dtype=np.float32) if residual is None else residual
    out, res = restated_topk(memory, k, add=agg)
    return out, res, agg


def planted(n, seed):
    """Seeded normals with the sixteen special values planted as far as the length allows, spread over the vector."""
    x = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    m = min(n, len(SPECIALS))
    at = (np.arange(m) * n) // m if m else np.arange(0)
    x[at] = SPECIALS[:m]
    x.setflags(write=False)
    return x


# ---- the restatement's own properties -------------------------------------------------------------------------------
def test_tie_free_normals_agree_with_argpartition():
    x = np.random.default_rng(1).standard_normal(5100).astype(np.float32)
    x = x[np.unique(np.abs(x), return_index=True)[1][:5000]]      # 5000 normals of distinct magnitude, in a shuffled order
    x = x[np.random.default_rng(2).permutation(x.size)]
    assert len(np.unique(np.abs(x))) == x.size == 5000
    for k in (1, 50, 1666, 4999):
        _, _, info = restated_topk(x, k, return_info=True)
        want = np.zeros(x.size, dtype=bool)
        want[np.argpartition(-np.abs(x), k - 1)[:k]] = True
        assert np.array_equal(info['mask'], want)
        assert info['ties'] == info['ties_taken'] == 1 and info['selected'] == k


def test_an_all_equal_vector_selects_its_first_k():
    x = np.full(300, 1.5, dtype=np.float32)
    x[::3] = -1.5                                      # mixed signs: the sign is not part of the key
    for k in (0, 1, 100, 299, 300):
        out, res, info = restated_topk(x, k, return_info=True)
        assert np.array_equal(info['mask'], np.arange(300) < k)
        assert info['ties'] == (300 if k else 0) and info['ties_taken'] == k
        assert np.array_equal(bits(out[:k]), bits(x[:k])) and not bits(out[k:]).any()
        assert np.array_equal(bits(res[k:]), bits(x[k:])) and not bits(res[:k]).any()


def test_the_order_is_nan_then_infinities_then_finite_then_denormals_then_zeros():
    x = SPECIALS.copy()
    key = bits(x) & np.uint32(0x7fffffff)
    order = np.argsort(-key.astype(np.int64), kind='stable')
    ranked = bits(x)[order]
    # the larger NaN payload first, then the other NaN, +inf before -inf (the lower column), ..., +0.0 before -0.0
    assert list(ranked[:4]) == [0xffc00123, 0x7fc00001, 0x7f800000, 0xff800000]
    assert list(ranked[-4:]) == [0x00000001, 0x80000001, 0x00000000, 0x80000000]
    assert list(x[order][4:12]) == [np.float32(3.4e38), np.float32(-3.4e38), 2.5, 1.0, -1.0, -0.75, np.float32(1e-38),
                                    np.float32(-1e-38)]
    out, res, info = restated_topk(x, 3, return_info=True)
    assert info['threshold_key'] == 0x7f800000 and info['ties'] == 2 and info['ties_taken'] == 1
    assert bits(out)[3] == 0xffc00123 and bits(out)[2] == 0x7fc00001          # payloads and signs come back as they are
    assert bits(out)[4] == 0x7f800000 and bits(out)[5] == 0 and bits(res)[5] == 0xff800000


def test_out_and_residual_partition_w():
    for n in (1, 63, 1025):
        x = planted(n, seed=n)
        add = planted(n, seed=n + 1)[::-1]
        for a in (None, add):
            w = restated_w(x, a)
            for k in {0, 1, n // 3, n - 1, n}:
                out, res, info = restated_topk(x, k, add=a, return_info=True)
                m = info['mask']
                assert m.sum() == k
                assert np.array_equal(bits(out)[m], bits(w)[m]) and not bits(out)[~m].any()
                assert np.array_equal(bits(res)[~m], bits(w)[~m]) and not bits(res)[m].any()
    out, res = restated_topk(x, 0)
    assert not bits(out).any() and np.array_equal(bits(res), bits(x))
    out, res = restated_topk(x, x.size)
    assert not bits(res).any() and np.array_equal(bits(out), bits(x))


def test_the_addition_is_one_fp32_operation():
    x = np.array([3e38, np.inf, 1.0, 2.0 ** -126], dtype=np.float32)
    add = np.array([3e38, -np.inf, 2.0 ** -24, -2.0 ** -127], dtype=np.float32)
    w = restated_w(x, add)
    assert np.isinf(w[0]) and np.isnan(w[1]) and w[2] == 1.0 and bits(w)[3] == 0x00400000      # a denormal sum stays
    out, _, info = restated_topk(x, 2, add=add, return_info=True)
    assert list(info['mask']) == [True, True, False, False]                                  # the NaN and the overflow first


def test_two_rounds_of_error_feedback_carry_a_coordinate_into_the_next_selection():
    """Coordinate 3 is second every round and k = 1 never takes it on its own; the memory adds up and takes it in round 2."""
    n, d = 8, 6
    agg = np.array([1.0, 0.1, 0.1, 0.7, 0.1, 0.1], dtype=np.float32)
    g = np.tile(agg, (n, 1))
    memory = np.zeros(d, dtype=np.float32)
    out1, memory, a1 = restated_sparsefed(g, 1, clip=np.inf, residual=memory)
    assert np.array_equal(a1, agg) and np.flatnonzero(out1).tolist() == [0] and memory[0] == 0.0 and memory[3] == agg[3]
    out2, memory, _ = restated_sparsefed(g, 1, clip=np.inf, residual=memory)
    assert np.flatnonzero(out2).tolist() == [3] and out2[3] == np.float32(0.7) + np.float32(0.7)
    assert memory[3] == 0.0 and memory[0] == 1.0                  # ... and coordinate 0 waits in the memory meanwhile


def test_sparsefed_composes_the_clipped_mean_with_the_top_k():
    g = attacked(23, 400, seed=5)
    out, res, agg = restated_sparsefed(g, 40, clip=3.0)
    want, info = restated_centered_clip(g, tau=3.0, iters=1)
    assert np.array_equal(agg, want) and info['clipped_rows'] > 0
    assert np.array_equal(bits(out) | bits(res), bits(agg)) and np.count_nonzero(out) == 40
    assert np.abs(out[out != 0]).min() >= np.abs(res).max()


def test_k_is_checked():
    x = np.zeros(5, dtype=np.float32)
    for bad in (-1, 6, 2.5, True):
        with pytest.raises(ValueError):
            restated_topk(x, bad)
    from attacking_federate_learning_amd.engine import Engine
    assert Engine._topk_k(0, 5) == 0 and Engine._topk_k(5, 5) == 5 and Engine._topk_k(np.int64(3)) == 3
    for bad in (-1, 6, 2.5, True):
        with pytest.raises(ValueError):
            Engine._topk_k(bad, 5)


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_new_entry_points_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    assert '#define BYZ_ABI_VERSION 1\n' in text
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    assert 'byz_sparsefed_params' in code and not re.search(r'\bbyz_sparsefed_sharded', code)
    sharded = text[text.index('Top-k over the slices'):text.index('byz_topk_sparsify_sharded_dev(')]
    assert '2048, 1024, 1024 and rank_count' in sharded            # the all-reduce lengths are stated


def test_the_ctypes_table_lists_them():
    import ctypes
    from attacking_federate_learning_amd import _native
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS, name
    i64, vp, ci = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
    assert _native._PROTOTYPES['byz_topk_sparsify_dev'] == [vp, vp, vp, i64, i64, vp, vp, vp]
    assert _native._PROTOTYPES['byz_topk_sparsify_sharded_dev'] == [vp, vp, vp, i64, i64, i64, ci, ci, vp, vp, vp, vp, vp]
    assert [f[0] for f in _native.SparsefedParams._fields_] == ['clip', 'k']
    assert ctypes.sizeof(_native.SparsefedParams) == 16


def test_the_source_is_on_the_build_list():
    from attacking_federate_learning_amd import build_native
    assert 'topk.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['topk.hip']


def test_python_surface():
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.sparsefed)) == (
        '(users_grads, users_count, corrupted_count, k=None, clip=10.0, residual=None, then=None, return_residual=False, '
        '**then_kwargs)')
    assert 'sparsefed' not in defences.defend and defences.sparsefed not in defences.defend.values()
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert 'max(1, D // 100)' in defences.sparsefed.__doc__ and "package's choice" in defences.sparsefed.__doc__
    assert str(inspect.signature(Engine.topk_sparsify)) == '(self, x, k, add=None, out=None, residual=None, return_info=False)'
    assert str(inspect.signature(Engine.topk_info)) == '(self)'
    assert str(inspect.signature(Engine.sparsefed)) == '(self, g, k, clip=10.0, residual=None, return_info=False)'
    assert list(inspect.signature(Engine.topk_sparsify_sharded).parameters)[:8] == [
        'self', 'x_local', 'k', 'n_total', 'rank', 'world', 'add', 'all_reduce']
    assert str(inspect.signature(DeviceServer.defend_sparsefed)) == '(self, k=None, clip=10.0, then=None, **then_kwargs)'
    doc = DeviceServer.defend_sparsefed.__doc__
    assert 'Algorithm 1' in doc and 'BEFORE the memory' in doc and 'AFTER' in doc
    assert str(inspect.signature(ShardedAggregator.sparsefed)) == (
        '(self, g_local, users_count, corrupted_count, k, clip=10.0, residual_local=None, total_columns=None, gather=False)')
    assert callable(HipKernels.topk_sparsify_sharded)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    from attacking_federate_learning_amd import defences
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_sparsefed', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.sparsefed is defences.sparsefed and 'sparsefed' not in mod.defend


def test_the_documents_name_the_new_entry_points():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert name in integration, name
    assert 'byz_centered_clip_sharded_dev' in integration[integration.index('byz_topk_sparsify_sharded_dev') - 2000:]
    assert '3.4k' in open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'SparseFed' in open(os.path.join(ROOT, 'PAPERS.md')).read()
