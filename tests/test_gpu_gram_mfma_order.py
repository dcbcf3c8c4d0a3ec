"""The issue order of the MFMAs inside the f16x2 tile kernel's pinned steady state (csrc/gram_planes.hip, super8) is free as
long as every accumulator block still receives m h', then h m', then h h' of super-stage sp, then the same of sp + 1: MFMAs
into different registers commute.  So a change of that order must leave the Gram's BITS alone.  The fixture
tests/golden/gram_order_digests.json holds, per shape, the SHA-256 of the fp64 Gram's bytes and 256 sampled entries as the
library of the commit BEFORE the order changed computed them (tests/golden/make_golden_gram_order.py, on an MI355X).

The shapes are the smallest the long-K path takes that still reach every loop variant:
  N = 2817 x D = 16,416   two full chunks and a ragged 32-column tail; the last slab has one live row (mask "row block 0 only")
  N = 3329 x D = 24,600   diagonal units D1 and D2, full waves in the pinned steady state, a chain that is never flushed
"""
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gram_order_digests.json')
SHAPES = ((2817, 16416), (3329, 24600))
N_SAMPLES = 256


def shape_key(n, d):
    return '%dx%d' % (n, d)


def host_matrix(n, d):
    """Host-seeded input: normal entries, row scales in [1, 1.5)."""
    rng = np.random.default_rng(9100 + n + d)
    g = rng.standard_normal((n, d), dtype=np.float32)
    g *= (1.0 + 0.5 * rng.permutation(n) / n).astype(np.float32)[:, None]
    return g


def sample_index(n):
    """256 entries: the corners, the one-row last slab, entries of the diagonal blocks, the rest anywhere."""
    rng = np.random.default_rng(77 + n)
    rows = rng.integers(0, n, N_SAMPLES)
    cols = rng.integers(0, n, N_SAMPLES)
    fixed = [(0, 0), (n - 1, n - 1), (n - 1, 0), (0, n - 1), (n - 1, n - 2), (255, 255), (256 + 130, 256 + 200), (191, 128)]
    for k, (i, j) in enumerate(fixed):
        rows[k], cols[k] = i, j
    diag = slice(len(fixed), 64)                     # inside the 256-row diagonal blocks: the D1 / D2 units
    cols[diag] = (rows[diag] // 256) * 256 + cols[diag] % 256
    cols[diag] = np.minimum(cols[diag], n - 1)
    return rows, cols


def digest_of(gram):
    gram = np.ascontiguousarray(gram, dtype=np.float64)
    rows, cols = sample_index(gram.shape[0])
    return {'sha256': hashlib.sha256(gram.tobytes()).hexdigest(),
            'samples': [float(v).hex() for v in gram[rows, cols]]}


def gram_of(eng, n, d):
    buf = eng.to_device(host_matrix(n, d))
    out = eng.gram(buf)
    eng.check()
    return out.numpy()


def test_the_golden_file_parses_and_names_both_shapes():
    table = json.load(open(GOLDEN))
    assert len(table['commit']) >= 7
    for n, d in SHAPES:
        rec = table['shapes'][shape_key(n, d)]
        assert len(rec['sha256']) == 64 and int(rec['sha256'], 16) >= 0
        assert len(rec['samples']) == N_SAMPLES
        values = np.array([float.fromhex(s) for s in rec['samples']])
        assert np.all(np.isfinite(values))
        assert values[0] > 0.0 and values[1] > 0.0     # |g_0|^2 and |g_(n-1)|^2
        assert values[2] == values[3]                   # the Gram is symmetric as bits


@pytest.mark.gpu
@pytest.mark.parametrize('n,d', SHAPES)
def test_gram_is_bitwise_what_it_was_before_the_order_changed(eng, monkeypatch, n, d):
    for key in ('BYZ_GRAM_MODE', 'BYZ_GRAM_DEFER', 'BYZ_GRAM_BLOCK_SKIP', 'BYZ_GRAM_PLANE_MB', 'BYZ_GRAM_ROUND', 'BYZ_GRAM_PLANES'):
        monkeypatch.delenv(key, raising=False)
    want = json.load(open(GOLDEN))['shapes'][shape_key(n, d)]
    gram = gram_of(eng, n, d)
    got = digest_of(gram)
    rows, cols = sample_index(n)
    wrong = [(int(i), int(j), g, w) for i, j, g, w in zip(rows, cols, got['samples'], want['samples']) if g != w]
    assert not wrong, wrong[:4]
    assert got['sha256'] == want['sha256']
