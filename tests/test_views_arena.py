"""The arena helper of tests/views_arena.py on CPU tensors: a GPU test on a view is only as good as the helper.

Every variant has the stride, offset and alignment class it is named after; `untouched` accepts a write inside the view and
rejects one changed word in either guard or in the padding between two rows, a NaN of another payload included; and for every
case listed for the GPU, the matrix read back out of the view gives the reference that the matrix itself gives."""
import numpy as np
import pytest

from oracle import faithful, ideal
from tests import views_arena as va

torch = pytest.importorskip('torch')


def cpu_variant(g, variant, guard=va.GUARD):
    return va.arena_variant(torch, g, variant, guard, device='cpu')


def untouched(flat, view, before):
    va.untouched(torch, flat, view, before)


@pytest.mark.parametrize('variant', va.VARIANTS)
@pytest.mark.parametrize('d', [1, 3, 4, 255, 256, 1027])
def test_every_variant_has_the_layout_it_is_named_after(variant, d):
    n = 5
    g = va.gaussian(d, n, d)
    ld, off = va.layout(variant, d)
    view, flat = cpu_variant(g, variant)
    assert view.stride(0) == ld and view.stride(1) == 1 and tuple(view.shape) == (n, d) and ld > d
    assert view.storage_offset() == va.GUARD + off and view.storage_offset() % 4 == off
    assert flat.numel() == 2 * va.GUARD + off + n * ld
    want = {'odd_ld_odd_base': (False, 1), 'even_ld_even_base': (True, 0), 'even_ld_odd_base': (True, 1),
            'odd_ld_even_base': (False, 0)}[variant]
    assert (ld % 4 == 0, off) == want
    assert view.data_ptr() % 16 == 4 * off
    if want[0]:
        assert ld - d <= 4 and ld == (d // 4 + 1) * 4
    else:
        assert ld in (d + 5, d + 6)
        # whatever the base, rows 0 and 1 cannot both be 16-byte aligned: a kernel has to look at ld, not only at G
        assert (view.data_ptr() + 4 * ld) % 16 != view.data_ptr() % 16
    # the matrix is where the view says, NaN everywhere else
    assert np.array_equal(view.numpy(), g)
    inside = va.inside_mask(torch, flat, view)
    assert int(inside.sum()) == n * d and bool(torch.isnan(flat[~inside]).all()) and not bool(torch.isnan(flat[inside]).any())
    assert np.array_equal(flat.numpy()[va.GUARD + off + 2 * ld:va.GUARD + off + 2 * ld + d], g[2])


def test_arena_rejects_a_guard_that_moves_the_alignment():
    with pytest.raises(AssertionError):
        va.arena(torch, va.gaussian(0, 3, 5), 8, 0, guard=4098, device='cpu')


@pytest.mark.parametrize('variant', va.VARIANTS)
def test_untouched_accepts_writes_inside_the_view_only(variant):
    n, d = 6, 37
    view, flat = cpu_variant(va.gaussian(1, n, d), variant)
    ld = view.stride(0)
    before = flat.clone()
    untouched(flat, view, before)
    view.fill_(3.0)                                   # a writer's whole business
    view[n - 1, d - 1] = float('nan')
    untouched(flat, view, before)
    first = view.storage_offset()
    last = first + (n - 1) * ld + d                   # one past the last element of the matrix
    places = [('leading guard', first - 1), ('leading guard', 0), ('trailing guard', last),
              ('trailing guard', flat.numel() - 1), ('padding: row 0', first + d),
              ('padding: row %d' % (n - 2), first + (n - 1) * ld - 1)]
    for name, index in places:
        saved = flat[index].clone()
        flat[index] = 1.0
        with pytest.raises(AssertionError, match='1 words outside the view changed'):
            untouched(flat, view, before)
        flat[index] = saved
        untouched(flat, view, before)
        # a NaN replaced by a NaN of another payload: equal as floats to nothing, different as bits
        word = flat.view(torch.int32)
        assert int(word[index]) == 0x7fc00000
        word[index] = 0x7fc00001
        assert bool(torch.isnan(flat[index]))
        with pytest.raises(AssertionError, match=name):     # ... and the message says where
            untouched(flat, view, before)
        word[index] = 0x7fc00000
        untouched(flat, view, before)


def test_untouched_compares_with_the_clone_it_is_given():
    view, flat = cpu_variant(va.gaussian(2, 4, 9), 'even_ld_odd_base')
    first = flat.clone()
    flat[0] = 7.0                                     # a test's own preparation, before the call under test
    with pytest.raises(AssertionError, match='leading guard'):
        untouched(flat, view, first)
    before = flat.clone()
    view.mul_(2.0)
    untouched(flat, view, before)
    with pytest.raises(AssertionError):               # the tensor itself is no clone of it
        untouched(flat, view, flat)


def views_of(g):
    """The matrix read back out of every variant's view, through numpy."""
    for variant in va.VARIANTS:
        view, flat = cpu_variant(g, variant)
        yield variant, np.ascontiguousarray(flat.numpy()[va.inside_mask(torch, flat, view).numpy()].reshape(g.shape))


@pytest.mark.parametrize('n,d', va.WALK_SHAPES + [va.WALK_WIDE])
def test_walk_cases_give_their_references_from_the_views(n, d):
    g = va.walk_input(n, d)
    rows = va.walk_row_list(n)
    carry, mean = va.walk_vectors(n, d)
    assert rows.min() >= 0 and rows.max() < n and len(rows) == n + 2
    for variant, back in views_of(g):
        assert np.array_equal(va.mean_f64(back), va.mean_f64(g)), variant
        assert np.array_equal(va.mean_f64(back, rows), va.mean_f64(g, rows))
        assert np.array_equal(va.chain_f64(back, carry, mean), va.chain_f64(g, carry, mean))
        assert np.array_equal(va.chain_f64(back), va.chain_f64(g))


@pytest.mark.parametrize('n,d', va.DRIFT_SHAPES + [va.DRIFT_WRITE_WIDE])
def test_drift_cases_give_their_references_from_the_views(n, d):
    g = va.drift_input(n, d)
    want = faithful.drift_vector(g.copy(), va.DRIFT_Z)
    mean, std = faithful.attack_statistics(g)
    for variant, back in views_of(g):
        assert va.same_bits(faithful.drift_vector(back.copy(), va.DRIFT_Z), want), variant
        got_mean, got_std = faithful.attack_statistics(back)
        assert va.same_bits(got_mean, mean) and va.same_bits(got_std, std)


@pytest.mark.parametrize('n,d', va.TRIM_SHAPES)
def test_trimmed_mean_cases_give_their_references_from_the_views(n, d):
    g = va.trim_input(n, d)
    want = ideal.trimmed_mean(g, n // 4)
    for variant, back in views_of(g):
        assert va.same_bits(ideal.trimmed_mean(back, n // 4), want), variant


@pytest.mark.parametrize('n,d', va.DIST_SHAPES)
def test_distance_cases_give_their_references_from_the_views(n, d):
    g = va.dist_input(n, d)
    want, gram = va.dist_reference(g), va.gram_reference(g)
    assert np.array_equal(want, want.T) and np.all(np.isinf(np.diag(want)))
    if (n, d) == (300, 2051):
        a, b = va.DIST_TWINS
        assert np.array_equal(g[a], g[b]) and want[a, b] == 0.0
        assert not np.array_equal(g[va.DIST_NEAR], g[a])
        # the near-duplicate is a few ulps off in most columns, and its distance is the norm of that difference
        diff = g[va.DIST_NEAR].astype(np.float64) - g[a].astype(np.float64)
        assert 0.0 < want[va.DIST_NEAR, a] == np.sqrt((diff * diff).sum()) < 1e-3
        assert want[va.DIST_NEAR, a] == want[va.DIST_NEAR, b]
        assert int((want[np.triu_indices(n, 1)] < 1.0).sum()) == 3
    for variant, back in views_of(g):
        assert np.array_equal(va.dist_reference(back), want), variant
        assert np.array_equal(va.gram_reference(back), gram)


@pytest.mark.parametrize('n,d,f', va.SELECT_CASES)
def test_selection_cases_give_their_references_from_the_views(n, d, f):
    g = va.select_input(n, d)
    want = va.select_reference(g, f)
    fb = va.bulyan_f(n, f)          # the reference's precondition (defences.py:56) holds, and f is lowered no further than it asks
    assert n >= 4 * fb + 3 and (fb == f or n < 4 * (fb + 1) + 3)
    # every decision is wider than the fp32 noise the suite allows a score: an fp32 path has to take the same ones
    assert want['margin'] > va.SELECT_TAU, want['margin'] / va.SELECT_TAU
    assert len(want['multi_krum']) == n - f and len(want['bulyan']) == n - 2 * va.bulyan_f(n, f) and want['multi_krum'][0] == want['krum']
    for variant, back in views_of(g):
        got = va.select_reference(back, f)
        assert got == want, variant


def test_assembly_case_gives_its_reference_from_the_views(golden):
    case = golden[va.ASSEMBLE_CASE]
    lists = va.assemble_lists(case)
    want = np.empty((va.ASSEMBLE_CLIENTS, va.ASSEMBLE_COLS), dtype=np.float32)
    for u, tensors in enumerate(lists):
        faithful.assemble_row(want, u, tensors)
    assert np.array_equal(want, case['G'])
    for variant in va.VARIANTS:
        view, flat = cpu_variant(np.zeros_like(want), variant)
        before = flat.clone()
        for u, tensors in enumerate(lists):
            view[u].copy_(torch.from_numpy(np.concatenate([t.ravel() for t in tensors])))
        untouched(flat, view, before)
        assert np.array_equal(view.numpy(), want), variant
