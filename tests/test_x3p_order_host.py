"""CPU (no GPU): the ITEM LIST of a mapped 3x3 dgrad on the persistent kernel (include/aod_hip.h aod_conv2d_ws_map_order), read through
aod_conv2d_x3p_item_order -- the ranking is tile_order_kernel's (csrc/conv.hip, TileOrderArgs.items), the deal of list positions to
workgroups the kernel's (csrc/conv_x3p.h x3p_item_slot / x3p_slot_block); the entry applies both to a host copy of the map.

An item is one 128-row x 128-column tile, tile_m * tiles_n + tile_n; it is live when one of the (at most two) 64-row blocks of its rows is set.
Properties, on hand-made maps (all dead, all live, one live row tile, live counts that are no multiple of the grid, below and above it):
  * the list is a permutation of all items;
  * every live item stands ahead of every dead one;
  * (block, round) is a bijection onto the items, and a workgroup's rounds are consecutive from 0;
  * the live items per workgroup differ by at most one, and a workgroup's dead items come after its live ones;
  * the column tiles of one row tile fall into the same blockIdx % 8 class.
A ragged last row tile (rows not a multiple of 128) is decided by its own blocks."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd import _C
    return _C.lib


def _order(lib, rows, tiles_n, grid, m):
    n = (rows + 127) // 128 * tiles_n
    keep = np.ascontiguousarray(m, np.uint8)
    item, block, rnd = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_int32 * n)()
    assert lib.aod_conv2d_x3p_item_order(rows, tiles_n, grid, keep.ctypes.data, item, block, rnd) == 0
    return np.array(item[:], np.int64), np.array(block[:], np.int64), np.array(rnd[:], np.int64)


def _live(rows, tiles_n, m, item):
    """the definition, written out"""
    out = np.zeros(len(item), bool)
    for k, e in enumerate(item):
        r0 = (e // tiles_n) * 128
        r1 = min(r0 + 128, rows)
        out[k] = bool(m[r0 // 64:(r1 - 1) // 64 + 1].any())
    return out


def _check(lib, rows, tiles_n, grid, m):
    n = (rows + 127) // 128 * tiles_n
    item, block, rnd = _order(lib, rows, tiles_n, grid, m)
    assert sorted(item.tolist()) == list(range(n))                                  # a permutation
    live = _live(rows, tiles_n, m, item)
    nlive = int(live.sum())
    assert live[:nlive].all() and not live[nlive:].any()                            # live ahead of dead
    assert ((0 <= block) & (block < grid)).all()
    assert len(set(zip(block.tolist(), rnd.tolist()))) == n                         # no two items in one place
    per = np.zeros(grid, np.int64)
    for b in range(grid):
        mine = np.nonzero(block == b)[0]                                            # (list positions ascend: the order in which b runs them)
        assert rnd[mine].tolist() == list(range(len(mine))), b                      # rounds 0, 1, ... without a gap
        lv = live[mine]
        per[b] = lv.sum()
        assert lv[:per[b]].all() and not lv[per[b]:].any(), b                       # its dead items after its live ones
    assert per.sum() == nlive and per.max() - per.min() <= 1, per                   # ceil(live / G) or one fewer
    assert per.max() == -(-nlive // grid)
    cls = {}
    for k, e in enumerate(item):
        cls.setdefault(int(e) // tiles_n, set()).add(int(block[k]) % 8)
    assert all(len(s) == 1 for s in cls.values())                                   # a row tile's column tiles share an XCD class
    if nlive >= 8 * tiles_n:                                                        # and the live row tiles spread over all eight
        assert {int(b) % 8 for b in block[:nlive]} == set(range(8))
    return item, block, rnd, live


def _rows_map(rows, live_tiles):
    m = np.zeros((rows + 63) // 64, np.uint8)
    for t in live_tiles:
        m[2 * t] = 1                                                                # (the tile's first block; its second stays 0)
    return m


# 682 row tiles x 2 columns on 256 workgroups is the bench's launch; (21, 2, 32) the GPU test's; tiles_n = 1 and 4 are N = 128 and 512
SHAPES = [(682, 2, 256), (21, 2, 32), (21, 2, 16), (40, 1, 8), (40, 1, 40), (30, 4, 96), (9, 2, 16)]


@pytest.mark.parametrize('tiles_m,tiles_n,grid', SHAPES)
def test_hand_made_maps(lib, tiles_m, tiles_n, grid):
    rows = tiles_m * 128
    per_round = grid // tiles_n                                                     # row tiles that fill the grid once
    counts = {0, 1, tiles_m, min(per_round - 1, tiles_m), min(per_round, tiles_m), min(per_round + 1, tiles_m),
              min(2 * per_round + 3, tiles_m), tiles_m - 1}
    rng = np.random.default_rng(5)
    for c in sorted(counts):
        picks = [list(range(c)), list(range(tiles_m - c, tiles_m)), sorted(rng.choice(tiles_m, c, replace=False).tolist())]
        for lt in picks:
            m = _rows_map(rows, lt)
            item, _, _, live = _check(lib, rows, tiles_n, grid, m)
            want = [t * tiles_n + n for t in lt for n in range(tiles_n)]
            assert item[:len(want)].tolist() == want                                # ranked by (row tile, column tile)
            assert int(live.sum()) == c * tiles_n


def test_second_block_and_ragged_last_tile(lib):
    rows = 128 * 20 + 70                                                            # the last row tile has one whole block and six rows of a second
    nblk = (rows + 63) // 64
    assert nblk == 42
    for b in (1, 39, 40, 41):
        m = np.zeros(nblk, np.uint8)
        m[b] = 1
        item, _, _, live = _check(lib, rows, 2, 32, m)
        assert item[:2].tolist() == [2 * (b // 2), 2 * (b // 2) + 1] and int(live.sum()) == 2
    m = np.ones(nblk, np.uint8)
    item, _, _, live = _check(lib, rows, 2, 32, m)
    assert live.all() and item.tolist() == list(range(42))


def test_slot_rule_is_the_documented_deal(lib):
    """position pos of the list: round pos // G, slot pos % G; slot s belongs to row-tile group u = s // tiles_n, which sits in class u % 8"""
    rows, tiles_n, grid = 128 * 64, 2, 32
    _, block, rnd = _order(lib, rows, tiles_n, grid, np.ones(rows // 64, np.uint8))
    for pos in range(len(block)):
        s = pos % grid
        u, tn = s // tiles_n, s % tiles_n
        assert rnd[pos] == pos // grid
        assert block[pos] == (u % 8) + 8 * ((u // 8) * tiles_n + tn)


def test_grid_rule_and_refused_arguments(lib):
    assert lib.aod_conv2d_x3p_mapped_grid(682 * 128, 2, 256) == 256
    assert lib.aod_conv2d_x3p_mapped_grid(21 * 128, 2, 256) == 32                   # 42 items: the largest multiple of 16
    assert lib.aod_conv2d_x3p_mapped_grid(7 * 128, 2, 256) == 0                     # 14 items: too few for the deal, the launch stays as planned
    assert lib.aod_conv2d_x3p_mapped_grid(682 * 128, 2, 304) == 304
    assert lib.aod_conv2d_x3p_mapped_grid(682 * 128, 4, 300) == 288
    one = (C.c_int32 * 64)()
    m = np.ones(8, np.uint8)
    assert lib.aod_conv2d_x3p_item_order(0, 2, 16, m.ctypes.data, one, one, one) == -1
    assert lib.aod_conv2d_x3p_item_order(512, 2, 12, m.ctypes.data, one, one, one) == -1      # not a multiple of 8 * tiles_n
    assert lib.aod_conv2d_x3p_item_order(512, 2, 16, m.ctypes.data, one, one, one) == -1      # more workgroups than items
    assert lib.aod_conv2d_x3p_item_order(1024, 2, 16, None, one, one, one) == -1
    assert lib.aod_conv2d_x3p_item_order(1024, 2, 16, m.ctypes.data, None, one, one) == -1
