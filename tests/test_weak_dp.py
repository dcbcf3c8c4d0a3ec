"""Clip and noise ("weak DP") without a GPU: the numpy restatement of the Philox4x32-10 stream, of the fp64 Box-Muller transform
and of the defence (include/byzagg.h) that tests/test_gpu_weak_dp.py holds the kernels to, the restatement's own
properties, csrc/philox.hpp on the host (tests/philox_check.cpp, compiled as plain C++17), and the public surface.

The restatement: Philox in uint64 arithmetic (a 32 x 32 product is exact there), the counter (low, high word of column >> 2,
low, high word of round), the key (low, high word of seed), word i of a block at column 4 b + i; normals in fp64 exactly as
the header states them; out = fl32((double)x + sigma_eff * z)."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_centered_clip import restated_centered_clip, restated_clip_update, restated_scales
from tests.test_geometric_median import attacked, restated_rowsq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, 'attacking_federate_learning_amd', 'csrc')

NEW_SYMBOLS = ('byz_gaussian_noise_dev', 'byz_noise_words_dev', 'byz_gaussian_noise_host', 'byz_clip_scales_dev',
               'byz_weak_dp_info', 'byz_weak_dp_dev', 'byz_weak_dp_host')

# Random123's known answers for philox4x32_10: (counter, key, output)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
LOW = np.uint64(0xffffffff)
S32 = np.uint64(32)
TWO_PI = np.array([0x401921FB54442D18], dtype=np.uint64).view(np.float64)[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the restatement -------------------------------------------------------------------------------------------------
def restated_philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counters (uint64 arrays holding 32-bit words) -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & LOW for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & LOW, np.uint64(k1) & LOW
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # exact: both factors are below 2^32
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LOW, (p0 >> S32) ^ c3 ^ k1, p0 & LOW
        k0, k1 = (k0 + W0) & LOW, (k1 + W1) & LOW
    return c0, c1, c2, c3


def restated_blocks(first_block, n_blocks, seed=0, round=0):
    """(n_blocks, 4) uint32: the words of the blocks first_block .. first_block + n_blocks - 1."""
    seed, round = int(seed) % (1 << 64), int(round) % (1 << 64)
    b = np.uint64(first_block) + np.arange(n_blocks, dtype=np.uint64)
    ones = np.ones(n_blocks, dtype=np.uint64)
    words = restated_philox(b & LOW, b >> S32, ones * np.uint64(round & 0xffffffff), ones * np.uint64(round >> 32),
                            seed & 0xffffffff, seed >> 32)
    return np.stack(words, axis=1).astype(np.uint32)


def _block_range(n, column_offset):
    first = int(column_offset) >> 2
    return first, ((int(column_offset) + int(n) + 3) >> 2) - first, int(column_offset) & 3


def restated_words(n, seed=0, round=0, column_offset=0):
    """The n raw words of the global columns column_offset .. column_offset + n - 1."""
    first, count, head = _block_range(n, column_offset)
    return restated_blocks(first, count, seed, round).reshape(-1)[head:head + n]


def restated_normals(n, seed=0, round=0, column_offset=0):
    """The n fp64 standard normals of the same columns: one Box-Muller pair per two words of a block."""
    first, count, head = _block_range(n, column_offset)
    x = restated_blocks(first, count, seed, round).astype(np.float64)
    z = np.empty((count, 4), dtype=np.float64)
    for p in (0, 1):
        u1 = (x[:, 2 * p] + 0.5) * 2.0 ** -32
        u2 = (x[:, 2 * p + 1] + 0.5) * 2.0 ** -32
        r = np.sqrt(-2.0 * np.log(u1))
        t = TWO_PI * u2
        z[:, 2 * p] = r * np.cos(t)
        z[:, 2 * p + 1] = r * np.sin(t)
    return z.reshape(-1)[head:head + n]


def restated_noise(x, sigma, seed=0, round=0, column_offset=0, scale=1.0):
    """fl32((double)x + sigma_eff * z), sigma_eff = sigma * scale; sigma = 0 with scale None: x's bits."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if sigma == 0 and scale is None:
        return x.copy()
    sigma_eff = float(sigma) * (1.0 if scale is None else float(scale))
    with np.errstate(invalid='ignore', over='ignore'):
        return (x.astype(np.float64) + sigma_eff * restated_normals(x.size, seed, round, column_offset)).astype(np.float32)


def restated_clip(q, clip=10.0, adaptive=False):
    """(scales, clip used, clipped, excluded) from the squared norms."""
    q = np.asarray(q, dtype=np.float64)
    if adaptive:
        finite = np.isfinite(q)
        clip = float(np.median(np.sqrt(q[finite]))) if finite.any() else 0.0
    s, clipped, excluded = restated_scales(q, clip)
    if clip == 0.0:
        s = np.zeros_like(s)
    return s, float(clip), clipped, excluded


def restated_weak_dp(g, clip=10.0, sigma=0.01, adaptive=False, seed=0, round=0, column_offset=0):
    """(out, info): the norm-clipped mean (centered clipping from zero, one iteration, with the mode's clip), then the noise
    (adaptive: sigma * clip).  info: clipped_rows, excluded_rows, clip, and the vector before the noise ('mean')."""
    g = np.asarray(g, dtype=np.float32)
    zero = np.zeros(g.shape[1], dtype=np.float32)
    if not adaptive:
        mean, cinfo = restated_centered_clip(g, tau=clip, iters=1, start=None)
        used, clipped, excluded = float(clip), cinfo['clipped_rows'], cinfo['excluded_rows']
    else:
        s, used, clipped, excluded = restated_clip(restated_rowsq(g, zero), adaptive=True)
        mean = restated_clip_update(g, zero, s)
    out = mean if sigma == 0 else restated_noise(mean, sigma, seed, round, column_offset, scale=used if adaptive else None)
    return out, {'clipped_rows': clipped, 'excluded_rows': excluded, 'clip': used, 'mean': mean}


# ---- csrc/philox.hpp on the host -------------------------------------------------------------------------------------
def _build_and_run(tmp_path, extra):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if compiler is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'philox_check')
    build = subprocess.run([compiler, '-std=c++17', '-O1', '-Wall', '-ffp-contract=off', '-I', CSRC] + extra +
                           [os.path.join(HERE, 'philox_check.cpp'), '-o', exe], capture_output=True, text=True)
    return build, exe


def test_philox_header_on_the_host(tmp_path):
    build, exe = _build_and_run(tmp_path, [])
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[0].startswith('philox ok'), run.stdout
    # the program prints the normals of the columns 0..7 of (seed 12345, round 7) as fp64 bit patterns: the header's transform
    # on this host's libm is the restatement's on numpy's, which call the same functions
    got = np.array([int(v, 16) for v in lines[1].split()], dtype=np.uint64).view(np.float64)
    want = restated_normals(8, seed=12345, round=7)
    assert np.allclose(got, want, rtol=1e-14, atol=0.0)


def test_philox_header_under_the_host_sanitizers(tmp_path):
    """The stand-alone program again with AddressSanitizer and UndefinedBehaviorSanitizer (a host build: nothing here is loaded
    into Python)."""
    build, exe = _build_and_run(tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    if build.returncode != 0:
        pytest.skip('the host compiler has no sanitizer runtime: ' + build.stderr[-200:])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith('philox ok'), run.stdout


# ---- the restatement: known answers and properties ---------------------------------------------------------------------
def test_the_restatement_reproduces_the_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        got = restated_philox(*[np.array([c], dtype=np.uint64) for c in counter], *key)
        assert tuple(int(w[0]) for w in got) == want
    assert [hex(w) for w in restated_words(4)] == ['0x6627e8d5', '0xe169c58d', '0xbc57ac4c', '0x9b00dbd8']
    # the third answer through the stream's own layout: block, round and seed are its counter and key
    block, rnd, seed = 0x85a308d3243f6a88, 0x0370734413198a2e, 0x299f31d0a4093822
    assert tuple(int(w) for w in restated_blocks(block, 1, seed, rnd)[0]) == KNOWN_ANSWERS[2][2]


def test_the_counter_layout():
    # block 2^32 is counter (0, 1, 0, 0); round 2^32 + 5 is counter words (5, 1)
    want = restated_philox(*[np.array([c], dtype=np.uint64) for c in (0, 1, 0, 0)], 0, 0)
    assert np.array_equal(restated_blocks(1 << 32, 1)[0], np.array([int(w[0]) for w in want], dtype=np.uint32))
    want = restated_philox(*[np.array([c], dtype=np.uint64) for c in (3, 0, 5, 1)], 9, 2)
    assert np.array_equal(restated_blocks(3, 1, seed=(2 << 32) + 9, round=(1 << 32) + 5)[0],
                          np.array([int(w[0]) for w in want], dtype=np.uint32))
    # the carry into counter word 1 inside one call
    w = restated_words(8, column_offset=(1 << 34) - 2)
    assert np.array_equal(w[:2], restated_blocks((1 << 32) - 1, 1)[0][2:]) and np.array_equal(w[2:6], restated_blocks(1 << 32, 1)[0])


def test_seed_and_round_name_the_vector():
    x = np.random.default_rng(3).standard_normal(1001).astype(np.float32)
    a = restated_noise(x, 0.5, seed=11, round=4)
    assert np.array_equal(bits(a), bits(restated_noise(x, 0.5, seed=11, round=4)))
    assert (bits(a) != bits(restated_noise(x, 0.5, seed=12, round=4))).mean() > 0.99
    assert (bits(a) != bits(restated_noise(x, 0.5, seed=11, round=5))).mean() > 0.99
    assert (bits(a) != bits(restated_noise(x, 0.5, seed=11 + (1 << 32), round=4))).mean() > 0.99      # the key's high word
    assert (bits(a) != bits(restated_noise(x, 0.5, seed=11, round=4 + (1 << 32)))).mean() > 0.99      # counter word 3
    assert np.array_equal(bits(restated_noise(x, 0.0, scale=None)), bits(x))


def test_any_split_into_shards_concatenates_to_the_one_call_vector():
    n = 4099
    x = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    for offset in (0, 3, (1 << 34) - 2):
        whole = restated_noise(x, 1.0, seed=7, round=2, column_offset=offset)
        words = restated_words(n, seed=7, round=2, column_offset=offset)
        for cuts in ((1, 2050), (4, 8), (1, 2, 3, 5, 4098), tuple(sorted(np.random.default_rng(6).choice(n - 1, 9, replace=False) + 1))):
            edges = (0,) + tuple(int(c) for c in cuts) + (n,)
            parts = [restated_noise(x[lo:hi], 1.0, seed=7, round=2, column_offset=offset + lo) for lo, hi in zip(edges, edges[1:])]
            assert np.array_equal(bits(np.concatenate(parts)), bits(whole))
            wparts = [restated_words(hi - lo, seed=7, round=2, column_offset=offset + lo) for lo, hi in zip(edges, edges[1:])]
            assert np.array_equal(np.concatenate(wparts), words)


def test_the_normals_have_mean_zero_and_variance_one():
    """2^20 normals at x = 0, sigma = 1: |mean| <= 6 standard errors = 6 * 2^-10, |var - 1| <= 6 sqrt(2 / 2^20) (the variance
    of a normal sample's variance is 2 / n): derived bounds, and seed 2019 is inside them."""
    n = 1 << 20
    z = restated_noise(np.zeros(n, dtype=np.float32), 1.0, seed=2019, round=0).astype(np.float64)
    assert abs(z.mean()) <= 6.0 * 2.0 ** -10
    assert abs(z.var() - 1.0) <= 6.0 * np.sqrt(2.0 / n)
    assert np.isfinite(z).all() and np.abs(z).max() <= 6.77          # u1 >= 2^-33 bounds every normal
    # the two members of a Box-Muller pair and neighbouring columns are uncorrelated to the same six standard errors
    assert abs(np.mean(z[0::2] * z[1::2])) <= 6.0 / np.sqrt(n / 2)
    assert abs(np.mean(z[:-1] * z[1:])) <= 6.0 / np.sqrt(n - 1)


def test_the_noise_is_one_rounding_of_an_fp64_sum():
    x = np.array([1.0, -0.0, 3e38, np.inf, np.nan, 2.0 ** -149], dtype=np.float32)
    z = restated_normals(6, seed=1)
    out = restated_noise(x, 1e-3, seed=1)
    assert np.array_equal(bits(out[:3]), bits((x[:3].astype(np.float64) + 1e-3 * z[:3]).astype(np.float32)))
    assert np.isinf(out[3]) and np.isnan(out[4])                        # nothing is sanitised
    assert out[5] == np.float32(1e-3 * z[5] + 2.0 ** -149)
    scaled = restated_noise(x, 2.0, seed=1, scale=0.25)
    assert np.array_equal(bits(scaled[:3]), bits(restated_noise(x, 0.5, seed=1)[:3]))


# ---- the clipping piece ---------------------------------------------------------------------------------------------------
def test_the_adaptive_clip_is_the_median_of_the_finite_norms():
    for n in (1, 2, 7, 8, 100):
        g = attacked(n, 33, seed=n) if n >= 4 else np.random.default_rng(n).standard_normal((n, 33)).astype(np.float32)
        q = restated_rowsq(g, np.zeros(33, dtype=np.float32))
        s, clip, clipped, excluded = restated_clip(q, adaptive=True)
        norms = np.sqrt(q)
        assert clip == float(np.median(norms)) and excluded == 0 and clipped == int((norms > clip).sum())
        assert np.array_equal(s, np.where(norms > clip, clip / norms, 1.0))
        assert clipped == n // 2                                        # half the rows lie above a median of distinct norms
    q = np.array([4.0, np.inf, 9.0, np.nan, 16.0, 25.0])
    s, clip, clipped, excluded = restated_clip(q, adaptive=True)
    assert clip == 3.5 and excluded == 2 and clipped == 2 and list(s) == [1.0, 0.0, 1.0, 0.0, 3.5 / 4.0, 3.5 / 5.0]


def test_the_fixed_mode_is_centered_clipping_from_zero():
    g = attacked(23, 130, seed=2)
    out, info = restated_weak_dp(g, clip=3.0, sigma=0.0)
    want, winfo = restated_centered_clip(g, tau=3.0, iters=1)
    assert np.array_equal(bits(out), bits(want)) and info['clipped_rows'] == winfo['clipped_rows'] > 0 and info['clip'] == 3.0
    noisy, ninfo = restated_weak_dp(g, clip=3.0, sigma=0.25, seed=4, round=9, column_offset=5)
    assert np.array_equal(bits(ninfo['mean']), bits(want))
    assert np.array_equal(bits(noisy), bits(restated_noise(want, 0.25, seed=4, round=9, column_offset=5)))
    # adaptive: the noise is lambda * the median norm
    out, info = restated_weak_dp(g, sigma=0.01, adaptive=True, seed=4)
    assert np.array_equal(bits(out), bits(restated_noise(info['mean'], 0.01 * info['clip'], seed=4)))


def test_a_non_finite_row_is_excluded_and_still_counted():
    g = np.random.default_rng(8).standard_normal((10, 40)).astype(np.float32)
    bad = g.copy()
    bad[3, 7], bad[6, 0] = np.nan, np.inf
    for adaptive in (False, True):
        out, info = restated_weak_dp(bad, clip=1e9, sigma=0.0, adaptive=adaptive)
        assert info['excluded_rows'] == 2 and np.isfinite(out).all()
        if not adaptive:            # nothing clipped: the sum of the eight finite rows over TEN
            want = (np.delete(g, [3, 6], axis=0).astype(np.float64).sum(axis=0) / 10.0).astype(np.float32)
            assert np.allclose(out, want, rtol=1e-6, atol=1e-7)
        else:
            assert info['clip'] == float(np.median(np.sqrt((np.delete(g, [3, 6], axis=0).astype(np.float64) ** 2).sum(axis=1))))


def test_no_finite_row_gives_the_zero_vector_and_no_nan():
    g = np.full((5, 12), np.nan, dtype=np.float32)
    g[1] = np.inf
    for adaptive in (False, True):
        out, info = restated_weak_dp(g, clip=2.0, sigma=0.0, adaptive=adaptive)
        assert not bits(out).any() and info['excluded_rows'] == 5 and info['clipped_rows'] == 0
    out, info = restated_weak_dp(g, sigma=0.5, adaptive=True, seed=3)
    assert info['clip'] == 0.0 and not out.any() and not np.isnan(out).any()      # the noise is scaled by a clip of 0
    out, _ = restated_weak_dp(g, clip=2.0, sigma=0.5, seed=3)                     # fixed: noise on the zero vector
    assert np.array_equal(bits(out), bits(restated_noise(np.zeros(12, dtype=np.float32), 0.5, seed=3)))


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_new_entry_points_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    assert '#define BYZ_ABI_VERSION 1\n' in text
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    assert 'byz_noise_params' in code and 'byz_weak_dp_params' in code
    assert not re.search(r'\bbyz_weak_dp_sharded|\bbyz_gaussian_noise_sharded', code)
    assert 'NO SHARDED ENTRY POINT' in text and 'byz_centered_clip_sharded_dev already makes' in text
    assert '0xD2511F53' in open(os.path.join(CSRC, 'philox.hpp')).read()


def test_the_ctypes_table_lists_them():
    import ctypes
    from attacking_federate_learning_amd import _native
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS, name
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    P = ctypes.POINTER
    assert _native._PROTOTYPES['byz_gaussian_noise_dev'] == [vp, vp, i64, P(_native.NoiseParams), vp, vp, vp]
    assert _native._PROTOTYPES['byz_weak_dp_dev'] == [vp, vp, i64, i64, i64, P(_native.WeakDpParams), vp, vp]
    assert [f[0] for f in _native.NoiseParams._fields_] == ['sigma', 'seed', 'round', 'column_offset']
    assert [f[0] for f in _native.WeakDpParams._fields_] == ['clip', 'sigma', 'adaptive', 'seed', 'round', 'column_offset']
    assert ctypes.sizeof(_native.NoiseParams) == 32 and ctypes.sizeof(_native.WeakDpParams) == 48


def test_the_source_is_on_the_build_list():
    from attacking_federate_learning_amd import build_native
    assert 'noise.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['noise.hip']


def test_python_surface():
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.weak_dp)) == (
        '(users_grads, users_count, corrupted_count, clip=10.0, sigma=0.01, adaptive=False, seed=0, round=0, then=None, '
        'return_info=False, **then_kwargs)')
    assert str(inspect.signature(defences.gaussian_noise)) == '(vector, sigma, seed=0, round=0, column_offset=0)'
    assert 'weak_dp' not in defences.defend and defences.weak_dp not in defences.defend.values()
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert "package's choice" in defences.weak_dp.__doc__ and 'tune both' in defences.weak_dp.__doc__
    for name in ('gaussian_noise', 'noise_words', 'clip_scales', 'weak_dp', 'weak_dp_info'):
        assert callable(getattr(Engine, name)), name
    assert str(inspect.signature(Engine.weak_dp)) == (
        '(self, g, clip=10.0, sigma=0.01, adaptive=False, seed=0, round=0, column_offset=0, return_info=False)')
    assert str(inspect.signature(DeviceServer.defend_weak_dp)) == (
        '(self, clip=10.0, sigma=0.01, adaptive=False, seed=0, then=None, **then_kwargs)')
    assert 'weak_dp_round' in DeviceServer.defend_weak_dp.__doc__
    assert list(inspect.signature(ShardedAggregator.weak_dp).parameters)[:5] == [
        'self', 'g_local', 'users_count', 'corrupted_count', 'column_offset']
    assert callable(HipKernels.gaussian_noise) and callable(HipKernels.clip_scales)
    with pytest.raises(ValueError):
        Engine._noise_params(float('nan'), 0, 0, 0)
    with pytest.raises(ValueError):
        Engine._noise_params(-1.0, 0, 0, 0)
    with pytest.raises(ValueError):
        Engine._noise_params(1.0, 0, 0, -4)
    p = Engine._noise_params(0.5, (1 << 63) + 12345, 7, (1 << 34) - 2)
    assert (p.sigma, p.seed, p.round, p.column_offset) == (0.5, (1 << 63) + 12345, 7, (1 << 34) - 2)


def test_the_dropin_shim_re_exports_it():
    import importlib.util
    from attacking_federate_learning_amd import defences
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_weak_dp', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.weak_dp is defences.weak_dp and mod.gaussian_noise is defences.gaussian_noise and 'weak_dp' not in mod.defend


def test_the_documents_name_the_new_entry_points():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert name in integration, name
    assert '3.4l' in open(os.path.join(ROOT, 'DESIGN.md')).read()
    papers = open(os.path.join(ROOT, 'PAPERS.md')).read()
    assert 'Sun, Kairouz' in papers and 'FLAME' in papers and 'Salmon' in papers
