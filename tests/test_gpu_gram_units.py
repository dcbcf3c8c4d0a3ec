"""The unit table of the long-K Gram's f16x2 tile kernel (csrc/gram_planes.hip, build_gram_units): the diagonal of the Gram is
computed by D1 units (the (bi, 2 bi) tile whose idle wave takes sub-tile (2, 2)) and D2 units (the (3, 2) and (3, 3) sub-tiles
of three 256-row blocks in one workgroup) instead of the quarter-full (bi, 2 bi + 1) tiles, and the chunks' level-1 sums are
indexed by slab.  Which wave of which workgroup holds a 32 x 32 block changes nothing about its MFMA chain or its fp64
additions: the Gram must be the bits of the (bi, tj) list with the in-kernel update (BYZ_GRAM_DEFER=0)."""
import ctypes

import numpy as np
import pytest

ROWS = (2817,    # t128 = 23, odd: the last 256-row block has one slab; 32 live rows in the last slab
        2944,    # 23 full slabs
        3072,    # 12 blocks: four D2 triples
        3200,    # 13 blocks, the last with one slab
        3329)    # 14 blocks, the last with one slab and one live row: 13 join D2 units, four triples and a single
COLS = (16416,   # two full chunks and one ragged stage pair
        24600)   # the last MFMA chain is not flushed: ragged_sums


def unit_table(n_rows):
    from attacking_federate_learning_amd import _native
    lib = _native.load()
    count = ctypes.c_int64(0)
    assert lib.byz_gram_unit_table(n_rows, None, 0, ctypes.byref(count)) == 0
    table = np.zeros((count.value, 36), dtype=np.int32)
    assert lib.byz_gram_unit_table(n_rows, table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), count.value,
                                   ctypes.byref(count)) == 0
    assert count.value == len(table)
    return table


def blocks_of(table):
    """[(row block, column block, unit, wave)] of every live 32 x 32 block, read the way the kernel reads a unit; checks
    that the wave's operands in LDS are those blocks."""
    out = []
    for u, unit in enumerate(table):
        rb = unit[:12]
        for wave in range(8):
            where = int(np.uint32(unit[12 + 3 * wave]))
            a_slot, b_slot, mask = where & 255, (where >> 8) & 255, (where >> 16) & 255
            row64, col64 = (where >> 24) & 1, (where >> 25) & 1
            assert mask in (0, 1, 3, 13, 15)          # the k_loop instantiations
            if mask == 0:
                continue
            assert a_slot + 1 < 12 and b_slot + 1 < 12
            slab = int(unit[14 + 3 * wave])
            ti, tj = slab & 0xffff, slab >> 16
            assert unit[13 + 3 * wave] == ti * (ti + 1) // 2 + tj
            for m in range(2):
                for n in range(2):
                    if (mask >> (2 * m + n)) & 1:
                        rblk, cblk = ti * 4 + row64 * 2 + m, tj * 4 + col64 * 2 + n
                        assert rb[a_slot + m] == rblk and rb[b_slot + n] == cblk, (u, wave)
                        out.append((rblk, cblk, u, wave))
    return out


def test_every_live_block_is_in_exactly_one_wave_of_one_unit():
    """Host arithmetic only, t128 = 1 .. 80 with a full, a one-row and a three-block last slab."""
    for t128 in range(1, 81):
        for n_rows in (128 * t128, 128 * t128 - 127, 128 * t128 - 40):
            table = unit_table(n_rows)
            pad32 = -(-t128 // 2) * 8
            assert table[:, :12].min() >= 0 and table[:, :12].max() < pad32     # every DMA piece inside the planes
            live = blocks_of(table)
            n_blocks32 = -(-n_rows // 32)
            want = {(r, c) for r in range(n_blocks32) for c in range(r + 1)}
            assert len(live) == len(want), n_rows                                 # nobody twice
            assert {(r, c) for r, c, _, _ in live} == want, n_rows                # nobody missing, nobody extra


def test_the_unit_counts_and_the_three_simds_of_a_d2():
    # 272 -> 262 units per chunk at N = 4000, 1640 -> 1613 at N = 10,000 (t128 = 79: the last block joins no D2)
    assert len(unit_table(4000)) == 262
    assert len(unit_table(10000)) == 1613
    table = unit_table(3072)
    assert len(table) == 12 * 13 - 12 + 4
    d2 = [unit for unit in table if len(set(unit[:12].tolist())) == 12 and unit[4] - unit[3] != 1]
    assert len(d2) == 4
    for unit in d2:
        full = [w for w in range(8) if (int(np.uint32(unit[12 + 3 * w])) >> 16) & 255 == 15]
        assert len(full) == 3 and len({w % 4 for w in full}) == 3


def planted(torch, n, d):
    gen = torch.Generator(device='cuda').manual_seed(7300 + n + d)
    g = torch.randn((n, d), generator=gen, device='cuda', dtype=torch.float32)
    g *= (1.0 + 0.5 * torch.rand((n, 1), generator=gen, device='cuda'))
    return g


def against_the_tile_list(eng, monkeypatch, call, env=None):
    """call() on the production path (with `env`) and under BYZ_GRAM_DEFER=0: equal as bits."""
    torch = pytest.importorskip('torch')
    for key in ('BYZ_GRAM_MODE', 'BYZ_GRAM_DEFER', 'BYZ_GRAM_BLOCK_SKIP', 'BYZ_GRAM_PLANE_MB', 'BYZ_GRAM_ROUND'):
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv('BYZ_GRAM_PLANES', '1')
    for key, value in (env or {}).items():
        monkeypatch.setenv(key, value)
    got = call().clone()
    eng.check()
    for key in (env or {}):
        monkeypatch.delenv(key)
    monkeypatch.setenv('BYZ_GRAM_DEFER', '0')
    want = call().clone()
    eng.check()
    monkeypatch.delenv('BYZ_GRAM_DEFER')
    assert torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(got, got.T)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('d', COLS)
@pytest.mark.parametrize('n', ROWS)
def test_gram_by_units_is_bitwise_the_tile_list_gram(eng, monkeypatch, n, d):
    torch = pytest.importorskip('torch')
    g = planted(torch, n, d)
    got = against_the_tile_list(eng, monkeypatch, lambda: eng.gram(g))
    # and it is the Gram: the diagonal blocks that moved, against fp64
    rows = torch.tensor([0, 127, 128, 191, 192, 255, 256 + 130, 256 + 200, n - 33, n - 1], device='cuda')
    want = g[rows].double() @ g.double().T
    scale = (g.double() ** 2).sum(1).sqrt()
    assert float(((got[rows] - want).abs() / (scale[rows][:, None] * scale[None, :])).max()) < 1e-6


@pytest.mark.gpu
def test_gram_by_units_with_repeated_rows_behind_a_row_index(eng, monkeypatch):
    torch = pytest.importorskip('torch')
    n, d = 3200, 16416
    g = planted(torch, 2000, d)
    gen = torch.Generator(device='cuda').manual_seed(11)
    index = torch.randint(0, 2000, (n,), generator=gen, device='cuda', dtype=torch.int32)   # every row about 1.6 times
    against_the_tile_list(eng, monkeypatch, lambda: eng.gram_share(g, index, 1, 0))


@pytest.mark.gpu
def test_gram_by_units_over_several_super_chunks(eng, monkeypatch):
    torch = pytest.importorskip('torch')
    g = planted(torch, 3329, 24600)
    # 3584 padded rows x 2 planes x 2 bytes x 8192 columns = 112 MiB per chunk: one chunk per super-chunk, four launches
    against_the_tile_list(eng, monkeypatch, lambda: eng.gram(g), {'BYZ_GRAM_PLANE_MB': '120'})


@pytest.mark.gpu
def test_gram_by_units_against_the_slab_granular_rule(eng, monkeypatch):
    """BYZ_GRAM_BLOCK_SKIP=0 multiplies every block of a live slab: no wave of a diagonal tile is idle, so it keeps the (bi, tj)
    list.  The production Gram is its bits, with the deferred update and with the in-kernel one."""
    torch = pytest.importorskip('torch')
    g = planted(torch, 2817, 24600)
    skip_off = against_the_tile_list(eng, monkeypatch, lambda: eng.gram(g), {'BYZ_GRAM_BLOCK_SKIP': '0'})
    assert torch.equal(eng.gram(g), skip_off)
