"""The original entry points on strided, misaligned, padded views (needs an MI355X).

The engine passes `data_ptr()` and `stride(0)` of a 2-D float32 view straight through as `G` and `ld`, and the kernels choose
their load path from `ld % 4` and from the base address modulo 16: walk_shape (row_walk.hpp), launch_gram_rows and
near_pair_partial_kernel (gram.hip), find_unique_rows (dedup.hip), launch_broadcast_rows (column_stats.hip), copy_span
(round_edges.hip); the resident attack kernel and the trimmed-mean kernels take `ld` and test no alignment.  Every test here
runs one entry point on the four views of tests/views_arena.py next to `dense = view.contiguous()` and asserts

  1. dense against the fp64 reference the suite already holds that operation to, at that operation's tolerance in
     tests/test_gpu_parity.py (indices exactly; aggregated vectors RTOL = ATOL = 1e-5; distances 1e-6 relative);
  2. view against dense.  BIT FOR BIT wherever the arithmetic does not depend on the load path: the column walks, the drift
     statistics, the trimmed mean, every selection, the rows written back, the assembled matrix.  Distances and the Gram are
     the exception (their tests say why) and are held to the reference's tolerance on every view;
  3. `untouched`: no word of the arena outside the view changed, and for a reader the view itself did not either.

The arena is NaN outside the view, so a read past a row or past the matrix surfaces as a NaN in the result (no reference
contains one) and a write there as a changed word -- never as a GPU fault.  tests/test_views_arena.py checks the helper and
the case lists on the CPU."""
import functools

import numpy as np
import pytest

from oracle import faithful, ideal
from tests import views_arena as va

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-5          # aggregated vectors (BASELINE.json north_star; tests/test_gpu_parity.py)


@pytest.fixture(scope='module')
def torch():
    return pytest.importorskip('torch')


def close(got, want):
    """No equal_nan: no input here holds a NaN, so a NaN in a result came from outside the matrix."""
    return np.allclose(np.asarray(got), np.asarray(want), rtol=RTOL, atol=ATOL)


def host(t):
    return t.cpu().numpy() if hasattr(t, 'cpu') else t.numpy()


def same(torch, a, b):
    """Two device results, bit for bit."""
    assert a.dtype == b.dtype and a.shape == b.shape
    word = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(word), b.contiguous().view(word))


def placed(torch, eng, g, variant):
    """-> (dense, view, (flat, before)): g on the GPU behind a variant's layout, its contiguous copy, and the arena with the
    clone of it that `untouched` compares against (taken here: no test writes outside its view itself)."""
    view, flat = va.arena_variant(torch, g, variant, device='cuda:%d' % eng.device)
    dense = view.contiguous()
    assert dense.stride(0) == g.shape[1] and dense.data_ptr() % 16 == 0
    return dense, view, (flat, flat.clone())


def read_only(torch, eng, flat, view, dense):
    """After a reader: nothing moved, inside the view or outside."""
    eng.check()
    torch.cuda.synchronize()
    va.untouched(torch, flat[0], view, flat[1])
    assert same(torch, view, dense), 'a reader changed the matrix'


# ---- the column walks ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk_case(n, d):
    g = va.walk_input(n, d)
    rows = va.walk_row_list(n)
    carry, mean = va.walk_vectors(n, d)
    chains = {(c, m): va.chain_f64(g, carry if c else None, mean if m else None) for c in (False, True) for m in (False, True)}
    return g, rows, carry, mean, va.mean_f64(g), va.mean_f64(g, rows), chains


def four_wide_reached(torch, eng, d):
    """walk_shape (row_walk.hpp) takes dwordx4 loads from 4 * 256 threads * 2 * CUs columns on."""
    return d >= 4 * 256 * 2 * torch.cuda.get_device_properties(eng.device).multi_processor_count


WALKS = va.WALK_SHAPES + [va.WALK_WIDE]


@pytest.mark.parametrize('variant', va.VARIANTS)
@pytest.mark.parametrize('n,d', WALKS)
def test_no_defense(eng, torch, n, d, variant):
    """column_sequential_kernel<VEC, 0>.  numpy's sequential fp32 sum in row order whatever the load width: bit for bit.  In
    the wide case even_ld_even_base is the one view that takes the four-wide walk; dense (ld = 524,291) and the rest are
    scalar."""
    g, _, _, _, want, _, _ = walk_case(n, d)
    dense, view, flat = placed(torch, eng, g, variant)
    if (n, d) == va.WALK_WIDE:
        assert four_wide_reached(torch, eng, d)
    got_d, got_v = eng.no_defense(dense), eng.no_defense(view)
    read_only(torch, eng, flat, view, dense)
    assert close(host(got_d), want)
    assert same(torch, got_v, got_d)


@pytest.mark.parametrize('variant', va.VARIANTS)
@pytest.mark.parametrize('n,d', WALKS)
def test_mean_rows(eng, torch, n, d, variant):
    """column_sequential_kernel<VEC, 2> over a shuffled row list with repeats: the list's order is the sum's order, on every
    load path: bit for bit."""
    g, rows, _, _, _, want, _ = walk_case(n, d)
    dense, view, flat = placed(torch, eng, g, variant)
    got_d, got_v = eng.mean_rows(dense, rows), eng.mean_rows(view, rows)
    read_only(torch, eng, flat, view, dense)
    assert close(host(got_d), want)
    assert same(torch, got_v, got_d)


@pytest.mark.parametrize('variant', va.VARIANTS)
@pytest.mark.parametrize('n,d', WALKS)
def test_column_chain(eng, torch, n, d, variant):
    """column_chain_kernel<VEC, SQUARES>, with and without `carry` and `mean`: one link of a sequential fp32 chain: bit for
    bit."""
    g, _, carry, mean, _, _, chains = walk_case(n, d)
    dense, view, flat = placed(torch, eng, g, variant)
    carry_t, mean_t = (torch.from_numpy(v).to(dense.device) for v in (carry, mean))
    for (with_carry, with_mean), want in chains.items():
        kw = {'carry': carry_t if with_carry else None, 'mean': mean_t if with_mean else None}
        got_d, got_v = eng.column_chain(dense, **kw), eng.column_chain(view, **kw)
        assert close(host(got_d), want), (with_carry, with_mean)
        assert same(torch, got_v, got_d), (with_carry, with_mean)
    read_only(torch, eng, flat, view, dense)


# ---- the drift attack ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def drift_case(n, d):
    g = va.drift_input(n, d)
    mean, std = faithful.attack_statistics(g)
    return g, mean, std, faithful.drift_vector(g.copy(), va.DRIFT_Z)


@pytest.mark.parametrize('variant', va.VARIANTS)
@pytest.mark.parametrize('n,d', va.DRIFT_SHAPES + [va.DRIFT_WRITE_WIDE])
def test_drift_attack(eng, torch, n, d, variant):
    """column_resident_kernel (64 < n <= 2560 rows and d >= 32: four, eight, sixteen waves) and column_sequential_kernel<VEC, 1>
    either side of it: numpy's bits (as tests/test_gpu_parity.py::test_drift_attack_statistics), so bit for bit between the
    views too.  Then write_back=True: broadcast_rows_kernel<4> stores 16-byte vectors only on even_ld_even_base (the drift
    vector is a fresh, aligned allocation), <1> elsewhere; every row of the view becomes the drift vector, bit for bit, and
    the padding between the rows stays NaN."""
    g, mean, std, drift = drift_case(n, d)
    dense, view, flat = placed(torch, eng, g, variant)
    got_d = eng.drift_attack(dense, va.DRIFT_Z)
    got_v = eng.drift_attack(view, va.DRIFT_Z)
    read_only(torch, eng, flat, view, dense)
    for got, want in zip(got_d, (drift, mean, std)):
        assert va.same_bits(host(got), want)
    assert all(same(torch, v, w) for v, w in zip(got_v, got_d))
    # the writer
    dense_w = dense.clone()
    wrote_d = eng.drift_attack(dense_w, va.DRIFT_Z, write_back=True)
    wrote_v = eng.drift_attack(view, va.DRIFT_Z, write_back=True)
    eng.check()
    torch.cuda.synchronize()
    va.untouched(torch, flat[0], view, flat[1])
    assert all(same(torch, v, w) for v, w in zip(wrote_v, got_d)) and all(same(torch, v, w) for v, w in zip(wrote_d, got_d))
    rows = got_d[0].reshape(1, d).expand(n, d)
    assert same(torch, dense_w, rows)
    assert same(torch, view, rows)


# ---- trimmed mean below the tall kernel ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trim_case(n, d):
    g = va.trim_input(n, d)
    return g, ideal.trimmed_mean(g, n // 4)


@pytest.mark.parametrize('variant', va.VARIANTS)
@pytest.mark.parametrize('n,d', va.TRIM_SHAPES)
def test_trimmed_mean(eng, torch, n, d, variant):
    """The register kernels (median_window.hip) up to 128 rows, the ring selection (window_lean.hip) with the general kernel
    behind it above.  They load 16 bytes at 4-byte alignment whatever `ld` is and select by rank: nothing depends on the
    layout: bit for bit."""
    g, want = trim_case(n, d)
    dense, view, flat = placed(torch, eng, g, variant)
    got_d, got_v = eng.trimmed_mean(dense, n, n // 4), eng.trimmed_mean(view, n, n // 4)
    read_only(torch, eng, flat, view, dense)
    assert close(host(got_d), want)
    assert same(torch, got_v, got_d)


# ---- distances and Gram -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dist_case(n, d):
    g = va.dist_input(n, d)
    return g, va.dist_reference(g), va.gram_reference(g)


def check_distances(got, want):
    n = len(want)
    off = ~np.eye(n, dtype=bool)
    assert np.array_equal(got, got.T) and np.all(np.isinf(np.diag(got)))
    zero = want == 0.0
    assert np.all(got[zero] == 0.0)                    # identical rows: exactly 0
    far = off & ~zero
    rel = np.abs(got[far] - want[far]) / want[far]
    assert rel.max() < 1e-6, rel.max()                 # (a NaN fails this comparison too)


@pytest.mark.parametrize('variant', va.VARIANTS)
@pytest.mark.parametrize('n,d', va.DIST_SHAPES)
def test_pairwise_distances(eng, torch, n, d, variant):
    """NOT bit for bit between the views, by design, so every view is held to the fp64 reference at the tolerance of
    tests/test_gpu_parity.py::test_distances_vs_fp64 (1e-6 relative, exact zeros, symmetric, infinite diagonal):
    launch_gram_rows (gram.hip, `const bool dma = (ld % 4 == 0) && (G % 16 == 0) && ...` and `split_mode = dma && ...` below
    it) takes the bf16 x 3 arithmetic only where the rows are 16-byte aligned -- (300, 2051) is split mode on
    even_ld_even_base and exact mode on the other three views and on dense (ld = 2051) -- and near_pair_partial_kernel
    (gram.hip, `const bool vec = (ld % 4 == 0) && (G % 16 == 0)`) sums a near-duplicate pair's squares four columns to a thread
    there and one column to a thread elsewhere.  (10, 257) and (128, 1000) are the small-N kernels, (129, 4097) exact mode
    with three K tiles; in (300, 2051) two rows are identical and a third nearly coincides with them, which puts the pair
    list, the re-computation on the difference and the folding of identical rows on the view."""
    g, want, _ = dist_case(n, d)
    dense, view, flat = placed(torch, eng, g, variant)
    got_d = eng.pairwise_distances(dense).numpy()
    got_v = eng.pairwise_distances(view).numpy()
    if (n, d) == (300, 2051):
        assert eng.near_pairs_count() >= 2              # the near-duplicate against either twin
    read_only(torch, eng, flat, view, dense)
    check_distances(got_d, want)
    check_distances(got_v, want)
    if (n, d) == (300, 2051):
        a, b = va.DIST_TWINS
        for got in (got_d, got_v):
            assert got[a, b] == 0.0 and got[b, a] == 0.0
            keep = np.ones(n, dtype=bool)
            keep[[a, b]] = False
            assert np.array_equal(got[a, keep], got[b, keep])     # identical rows, identical distance rows
            assert 0.0 < got[va.DIST_NEAR, a] < 1e-3


@pytest.mark.parametrize('variant', va.VARIANTS)
@pytest.mark.parametrize('n,d', va.DIST_SHAPES)
def test_gram(eng, torch, n, d, variant):
    """The fp64 Gram of the view.  Not bit for bit between the views for the reason test_pairwise_distances gives (split mode
    needs LDS-DMA, gram.hip: `split_mode = dma && ...`), so every view is held to fp64.  The bound: an entry is a sum of fp32
    chains of at most L = min(d, kFlushK = 2048) products, added up in fp32 (a few) and fp64; a chain's rounding errors are
    L steps of at most u = 2^-24 each, relative to partial sums bounded by |x_i| |x_j| (Cauchy-Schwarz), and add up like a
    random walk: sqrt(L) u |x_i| |x_j|, times 4 for the largest of n^2 entries.  That is 4e-6 .. 1.1e-5 of |x_i| |x_j| here,
    while ONE wrong or missing column moves an entry by about 1 / d of it (2.4e-4 at d = 4097): still caught.  (The suite's
    2e-7, tests/test_gpu_scale.py, is measured on the long-K schedule with fp64 slabs and does not carry over to d = 257.)"""
    g, _, want = dist_case(n, d)
    dense, view, flat = placed(torch, eng, g, variant)
    got_d, got_v = eng.gram(dense), eng.gram(view)
    read_only(torch, eng, flat, view, dense)
    norms = np.sqrt(np.diag(want))
    scale = norms[:, None] * norms[None, :]
    bound = 4.0 * np.sqrt(min(d, 2048)) * 2.0 ** -24
    for name, got in (('dense', host(got_d)), ('view', host(got_v))):
        worst = float(np.max(np.abs(got - want) / scale))
        print('gram %s %dx%d %s: worst %.3g of bound %.3g' % (name, n, d, variant, worst, bound))
        assert worst < bound, (name, worst, bound)      # (a NaN fails this comparison too)


@pytest.mark.parametrize('variant', va.VARIANTS)
def test_duplicate_finder_verifies_rows_of_a_view(eng, torch, variant):
    """find_unique_rows (dedup.hip: `const bool vec = (ld % 4 == 0) && (G % 16 == 0)`) runs from 512 rows on, so the
    (300, 2051) case does not reach it: 520 rows of which 131 are one vector (four tiles of unique rows instead of five) and
    one differs from them in a single column.  The Gram then runs over a row list of the view.  Same assertions and tolerance
    as test_pairwise_distances."""
    n, d = 520, 259
    g = va.gaussian(18000, n, d)
    group = np.arange(3, n, 4)[:131]
    g[group] = g[group[0]]
    odd_one = 6
    g[odd_one] = g[group[0]]
    g[odd_one, d - 2] += np.float32(1.0)
    want = va.dist_reference(g)
    dense, view, flat = placed(torch, eng, g, variant)
    got_d = eng.pairwise_distances(dense).numpy()
    got_v = eng.pairwise_distances(view).numpy()
    read_only(torch, eng, flat, view, dense)
    for got in (got_d, got_v):
        check_distances(got, want)
        sub = got[np.ix_(group, group)]
        assert np.all(sub[~np.eye(len(group), dtype=bool)] == 0.0)
        assert 0.9 < got[odd_one, group[0]] < 1.1


# ---- Krum, Multi-Krum, Bulyan end to end --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def select_case(n, d, f):
    g = va.select_input(n, d)
    want = va.select_reference(g, f)
    assert want['margin'] > va.SELECT_TAU
    return g, want


@pytest.mark.parametrize('variant', va.VARIANTS)
@pytest.mark.parametrize('n,d,f', va.SELECT_CASES)
def test_krum_multi_krum_bulyan(eng, torch, n, d, f, variant):
    """(33, 1000): the small-N kernels (krum_small.hip); (300, 2051): Gram, row sort, selection loop, then copy_row /
    column_sequential_kernel<VEC, 2> / the trimmed mean over a row list of the view.  The distances underneath may differ in
    their last bits between the views (test_pairwise_distances), the decisions may not: every one oracle.ideal takes on these
    inputs has a margin above 16 eps (select_input).  Indices and selections exactly; the aggregates against fp64 at
    RTOL = ATOL = 1e-5 and, the selection being the same, bit for bit between view and dense (a row copy, a sequential
    mean in ascending row order, a rank selection: none depends on the load path)."""
    g, want = select_case(n, d, f)
    fb = va.bulyan_f(n, f)          # (33, f = 8) is past Bulyan's precondition n >= 4 f + 3: Bulyan alone runs at 7 there
    dense, view, flat = placed(torch, eng, g, variant)
    out = {}
    for name, m in (('dense', dense), ('view', view)):
        idx = eng.krum(m, n, f, return_index=True)
        row = eng.krum(m, n, f)
        mk, mk_sel = eng.multi_krum(m, n, f, return_selection=True)
        bul, bul_sel = eng.bulyan(m, n, fb, return_selection=True)
        out[name] = (idx, row, mk, mk_sel, bul, bul_sel)
    read_only(torch, eng, flat, view, dense)
    for name, (idx, row, mk, mk_sel, bul, bul_sel) in out.items():
        assert idx == want['krum'], name
        assert va.same_bits(host(row), g[idx]), name
        assert host(mk_sel).tolist() == want['multi_krum'], name
        assert close(host(mk), va.mean_f64(g, np.sort(want['multi_krum']))), name
        assert host(bul_sel).tolist() == want['bulyan'], name
        assert close(host(bul), ideal.trimmed_mean(g[want['bulyan']], 2 * fb)), name
    for a, b in zip(out['view'][1:], out['dense'][1:]):
        assert same(torch, a, b)


# ---- assembly: writers into G with ld ------------------------------------------------------------------------------------------
def assemble_into(torch, eng, golden, variant):
    case = golden[va.ASSEMBLE_CASE]
    lists = va.assemble_lists(case)
    zeros = np.zeros((va.ASSEMBLE_CLIENTS, va.ASSEMBLE_COLS), dtype=np.float32)
    dense, view, flat = placed(torch, eng, zeros, variant)
    device = [[torch.from_numpy(t).to(dense.device) for t in tensors] for tensors in lists]
    return case['G'], lists, device, dense, view, flat


def assembled(torch, eng, want, dense, view, flat):
    eng.check()
    torch.cuda.synchronize()
    va.untouched(torch, flat[0], view, flat[1])
    assert va.same_bits(host(dense), want)
    assert same(torch, view, dense)


@pytest.mark.parametrize('variant', va.VARIANTS)
def test_assemble_row(eng, torch, golden, variant):
    """assemble_row_kernel (copy_span, round_edges.hip: 16-byte moves where source and destination agree modulo 16, one by
    one otherwise) from per-parameter device tensors, then byz_assemble_row_host from the flat host vector: copies, bit for
    bit, and nothing next to the row is written."""
    want, lists, device, dense, view, flat = assemble_into(torch, eng, golden, variant)
    for u in range(va.ASSEMBLE_CLIENTS):
        eng.assemble_row(dense, u, device[u])
        eng.assemble_row(view, u, device[u])
    assembled(torch, eng, want, dense, view, flat)
    dense.zero_()
    view.zero_()
    for u in range(va.ASSEMBLE_CLIENTS):
        flat_vector = np.concatenate([t.ravel() for t in lists[u]])
        eng.assemble_row(dense, u, flat_vector)
        eng.assemble_row(view, u, flat_vector)
    assembled(torch, eng, want, dense, view, flat)


@pytest.mark.parametrize('variant', va.VARIANTS)
def test_assemble_rows(eng, torch, golden, variant):
    """assemble_rows_kernel, all clients in one launch; the second call takes byz_assemble_rows_again_dev (the device table
    of the first).  First row 0, and rows 1 .. 2 of the matrix alone."""
    want, _, device, dense, view, flat = assemble_into(torch, eng, golden, variant)
    for _ in range(2):
        dense.zero_()
        view.zero_()
        eng.assemble_rows(dense, 0, device)
        eng.assemble_rows(view, 0, device)
        assembled(torch, eng, want, dense, view, flat)
    dense.zero_()
    view.zero_()
    eng.assemble_rows(dense, 1, device[2:4])
    eng.assemble_rows(view, 1, device[2:4])
    part = np.zeros_like(want)
    part[1:3] = want[2:4]
    assembled(torch, eng, part, dense, view, flat)


@pytest.mark.parametrize('variant', va.VARIANTS)
def test_assemble_columns(eng, torch, golden, variant):
    """assemble_columns_kernel from batched per-parameter gradients (n_clients, *shape)."""
    want, _, device, dense, view, flat = assemble_into(torch, eng, golden, variant)
    batched = [torch.stack([device[u][t] for u in range(va.ASSEMBLE_CLIENTS)]) for t in range(va.ASSEMBLE_TENSORS)]
    eng.assemble_columns(dense, batched)
    eng.assemble_columns(view, batched)
    assembled(torch, eng, want, dense, view, flat)
