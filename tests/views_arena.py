"""Strided, misaligned, guard-banded views of a gradient matrix, for the tests of the device entry points.

The engine hands `data_ptr()` and `stride(0)` of any 2-D float32 view with unit column stride to the kernels as `G` and
`ld`, and the kernels pick their load path from `ld % 4` and from the base address modulo 16.  `arena` places a matrix at a
chosen (ld, offset) INSIDE one allocation whose every other element is NaN: a kernel that reads past a row or past the matrix
gets a NaN into its result, one that writes there changes a word that `untouched` compares bit for bit.  Neither is a GPU fault:
the guards and the row padding belong to the allocation.

tests/test_gpu_views.py runs the original entry points on these views; its case lists, inputs and fp64 references live here,
so that tests/test_views_arena.py can check the helper, on CPU tensors, with the very matrices the GPU file runs.
"""
import numpy as np

GUARD = 4096        # floats either side of the matrix: four times a 1024-column window, 1024 times a 16-byte vector

# id -> (leading dimension, offset of the matrix behind the leading guard), both as functions of the width d
VARIANTS = ('odd_ld_odd_base', 'even_ld_even_base', 'even_ld_odd_base', 'odd_ld_even_base')


def odd_ld(d):
    """d + 5, moved on by one where that is a multiple of 4: never a multiple of 4."""
    ld = d + 5
    return ld + 1 if ld % 4 == 0 else ld


def even_ld(d):
    """The next multiple of 4 strictly greater than d: a padded row whose ragged tail lies next to NaN."""
    return (d // 4 + 1) * 4


def layout(variant, d):
    """(ld, off) of a variant for a matrix of d columns."""
    ld = odd_ld(d) if variant.startswith('odd_ld') else even_ld(d)
    off = 1 if variant.endswith('odd_base') else 0
    return ld, off


def arena(torch, g, ld, off, guard=GUARD, device='cuda'):
    """-> (view, flat).  `flat`: one 1-D float32 tensor of guard + off + n * ld + guard elements, all NaN; `view`: the n x d
    matrix `g` inside it, as_strided((n, d), (ld, 1), guard + off).  guard % 4 == 0, so the view's address modulo 16 is
    4 * (off % 4).  A test clones `flat` before the call it checks and hands the clone to `untouched` afterwards."""
    g = torch.as_tensor(np.ascontiguousarray(g)) if isinstance(g, np.ndarray) else g
    n, d = g.shape
    assert guard % 4 == 0 and guard >= 4 and ld >= d and off >= 0
    flat = torch.full((guard + off + n * ld + guard,), float('nan'), dtype=torch.float32, device=device)
    view = flat.as_strided((n, d), (ld, 1), guard + off)
    view.copy_(g)
    assert flat.data_ptr() % 16 == 0, 'the allocator hands out 16-byte aligned blocks'
    assert view.data_ptr() == flat.data_ptr() + 4 * (guard + off)
    assert view.data_ptr() % 16 == 4 * (off % 4) and view.stride(0) == ld and view.stride(1) == 1
    return view, flat


def arena_variant(torch, g, variant, guard=GUARD, device='cuda'):
    """`arena` at a variant's layout, with the alignment class the variant is named after asserted."""
    ld, off = layout(variant, g.shape[1])
    view, flat = arena(torch, g, ld, off, guard, device)
    assert (view.stride(0) % 4 == 0) == variant.startswith('even_ld')
    assert (view.data_ptr() % 16 == 0) == variant.endswith('even_base')
    return view, flat


def inside_mask(torch, flat, view):
    """bool, one per element of flat: True where the element belongs to the view."""
    mask = torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device)
    mask.as_strided(tuple(view.shape), tuple(view.stride()), view.storage_offset()).fill_(True)
    return mask


def untouched(torch, flat, view, before):
    """Assert that every element of `flat` outside `view` holds the BITS it holds in `before`, a clone of `flat` taken before
    the call under test.  Through int32: NaN != NaN as floats, and a NaN of another payload is a changed word."""
    assert before.shape == flat.shape and before.data_ptr() != flat.data_ptr()
    outside = ~inside_mask(torch, flat, view)
    changed = (flat.view(torch.int32) != before.view(torch.int32)) & outside
    if bool(changed.any()):
        where = torch.nonzero(changed).flatten()
        first, last = view.storage_offset(), view.storage_offset() + (view.shape[0] - 1) * view.stride(0) + view.shape[1]
        places = []
        for i in where[:8].tolist():
            if i < first:
                places.append('%d (leading guard, %d before the matrix)' % (i, first - i))
            elif i >= last:
                places.append('%d (trailing guard, %d past the matrix)' % (i, i - last + 1))
            else:
                r, c = divmod(i - first, view.stride(0))
                places.append('%d (padding: row %d, column %d of ld %d)' % (i, r, c, view.stride(0)))
        raise AssertionError('%d words outside the view changed: %s' % (int(where.numel()), ', '.join(places)))


def bits(a):
    """float32 array -> its int32 bits (bit-for-bit comparisons that treat NaN like any other value)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- inputs (the families of tests/test_gpu_parity.py) -----------------------------------------------------------------------
def gaussian(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def scaled(seed, n, d):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d)).astype(np.float32)
    return g * (1.0 + 0.5 * rng.permutation(n) / n).astype(np.float32)[:, None]


# ---- the cases: the smallest shapes that reach each dispatch branch --------------------------------------------------------
# column walks: the run of eight rows and its tail; one column, either side of a 256-thread workgroup, several workgroups
WALK_SHAPES = [(n, d) for n in (7, 8, 9, 17) for d in (1, 255, 257, 1027)]
WALK_WIDE = (9, 524291)      # the four-wide walk starts at 4 * 256 threads * 2 * 256 CUs = 524,288 columns (walk_shape, row_walk.hpp)


def walk_input(n, d):
    return gaussian(11000 + 31 * n + d % 1009, n, d)


def walk_row_list(n):
    """mean_rows' list: a shuffle of the rows with two repeats (a list is any sequence of valid rows)."""
    rng = np.random.default_rng(12000 + n)
    return np.concatenate([rng.permutation(n), rng.integers(0, n, size=2)]).astype(np.int32)


def walk_vectors(n, d):
    """(carry, mean) for column_chain."""
    rng = np.random.default_rng(13000 + n + d % 1009)
    return rng.standard_normal(d).astype(np.float32), (0.1 * rng.standard_normal(d)).astype(np.float32)


def mean_f64(g, rows=None):
    g = np.asarray(g, dtype=np.float64)
    return (g if rows is None else g[np.asarray(rows)]).mean(axis=0)


def chain_f64(g, carry=None, mean=None):
    g = np.asarray(g, dtype=np.float64)
    terms = g if mean is None else (g - np.asarray(mean, dtype=np.float64)[None, :]) ** 2
    return terms.sum(axis=0) + (0.0 if carry is None else np.asarray(carry, dtype=np.float64))


# drift attack: the resident kernel takes 64 < n_rows <= 2560 with four waves up to 640 rows, eight up to 1280, sixteen beyond,
# and at least kTileCols = 32 columns (column_pass, column_stats.hip); everything else is the sequential kernel
DRIFT_SHAPES = [(n, d) for n in (7, 64, 65, 641, 1281, 2561) for d in (31, 33, 1027)]
DRIFT_WRITE_WIDE = (7, 16387)     # broadcast_rows_kernel<4>: one whole piece of 16 x 256 x 4 = 16,384 columns and a ragged three
DRIFT_Z = 1.5


def drift_input(n, d):
    return gaussian(14000 + n + d % 1009, n, d) * 2 + np.float32(0.5)


# trimmed mean below the tall kernel: 64 rows per lane slot, the ring selection from 129 rows, the general kernel behind it
TRIM_SHAPES = [(n, d) for n in (10, 100, 1025, 2561) for d in (1, 33, 130)]


def trim_input(n, d):
    return gaussian(15000 + n * 7 + d, n, d)


# distances and Gram: the small-N kernels (N <= 128), exact mode with three K tiles, split mode (N > 256: four tiles of C)
DIST_SHAPES = [(10, 257), (128, 1000), (129, 4097), (300, 2051)]
DIST_TWINS = (5, 200)        # in the (300, 2051) case: two identical rows ...
DIST_NEAR = 77               # ... and one that nearly coincides with them


def dist_input(n, d):
    g = gaussian(16000 + n, n, d)
    if (n, d) == (300, 2051):
        a, b = DIST_TWINS
        g[b] = g[a]
        noise = np.random.default_rng(16001).standard_normal(d).astype(np.float32)
        g[DIST_NEAR] = g[a] + np.float32(1e-6) * np.abs(g[a]) * noise
    return g


def dist_reference(g):
    """oracle.ideal's fp64 distance matrix.  For a pair of rows that nearly coincide the Gram identity cancels even in fp64
    (d^2 of 1e-9 out of norms of 2e3 with 1e-16 relative error each: four digits), so those entries are the fp64 norm of the
    difference itself, as tests/test_gpu_parity.py::test_small_krum_path_next_to_the_general_path forms its reference."""
    from oracle import ideal
    want = ideal.distance_matrix(g)
    norms = np.sqrt((g.astype(np.float64) ** 2).sum(axis=1))
    near = np.argwhere(np.triu(want < 1e-3 * np.minimum(norms[:, None], norms[None, :]), 1))
    for i, j in near:
        diff = g[i].astype(np.float64) - g[j].astype(np.float64)
        want[i, j] = want[j, i] = np.sqrt((diff * diff).sum())
    return want


def gram_reference(g):
    g64 = np.asarray(g, dtype=np.float64)
    return g64 @ g64.T


# Krum, Multi-Krum, Bulyan end to end: the small-N kernels and the Gram path
SELECT_CASES = [(33, 1000, 8), (300, 2051, 70)]
SELECT_TAU = 16 * np.finfo(np.float32).eps      # the suite's bound on fp32 noise in a score (test_krum_end_to_end_margin_protocol)


SELECT_SEEDS = {33: 17033, 300: 25300}


def select_input(n, d):
    """The `scaled` family.  Among 300 rows some pair of scores always lies close; the seeds are ones at which every decision
    oracle.ideal takes (Krum's pick, every step of Multi-Krum's ranking, every pick of Bulyan's loop) has a relative margin
    above SELECT_TAU, so that an fp32 path must take the same ones (tests/test_views_arena.py asserts the margins)."""
    return scaled(SELECT_SEEDS[n], n, d)


def multi_krum_ideal(dist, users_count, corrupted_count, m, with_margin=False):
    """The m best rows by oracle.ideal's fp64 Krum scores, ranked by (score, visit position): Multi-Krum's selection order."""
    from oracle import ideal
    from oracle.faithful import visit_order
    n = dist.shape[0]
    scores = ideal.krum_scores(dist, np.ones(n, dtype=bool), users_count, corrupted_count)
    position = np.empty(n, dtype=np.int64)
    position[np.asarray(visit_order(n))] = np.arange(n)
    ranking = np.lexsort((position, scores))
    if not with_margin:
        return ranking[:m].tolist()
    ranked = scores[ranking[:m + 1]]
    gaps = np.diff(ranked) / np.abs(ranked[:-1])
    return ranking[:m].tolist(), float(gaps.min()) if gaps.size else np.inf


def bulyan_f(n, f):
    """Bulyan asserts n >= 4 f + 3 (defences.py:56), which (33, f = 8) does not meet: Krum and Multi-Krum run at the case's f,
    Bulyan at the most the reference admits below it (7 of 33; 70 of 300 as given)."""
    return min(f, (n - 3) // 4)


def select_reference(g, f):
    """What oracle.ideal selects on g, and the smallest relative margin of any of those decisions."""
    from oracle import ideal
    n = g.shape[0]
    dist = ideal.distance_matrix(g)
    krum, krum_margin, _ = ideal.krum_index(dist, n, f, with_margin=True)
    multi, multi_margin = multi_krum_ideal(dist, n, f, n - f, with_margin=True)
    bulyan, bulyan_margins = ideal.bulyan_selection(dist, n, bulyan_f(n, f), with_margins=True)
    return {'krum': krum, 'multi_krum': multi, 'bulyan': bulyan,
            'margin': min(float(krum_margin), multi_margin, float(np.min(bulyan_margins)))}


# assembly: the tensor lists of tests/test_gpu_parity.py::test_golden_gradient_assembly (golden['assemble_4x204'])
ASSEMBLE_CASE, ASSEMBLE_CLIENTS, ASSEMBLE_TENSORS, ASSEMBLE_COLS = 'assemble_4x204', 4, 5, 204


def assemble_lists(case):
    """[client][tensor] -> float32 array, as the golden file holds them."""
    return [[np.ascontiguousarray(case['u%d_t%d' % (u, t)], dtype=np.float32) for t in range(ASSEMBLE_TENSORS)]
            for u in range(ASSEMBLE_CLIENTS)]
