"""CPU (no GPU): the block order of a mapped grouped conv launch as the LIST that the device builds from the row-activity maps, read through
aod_conv2d_tile_order (host copies of the maps; the entry, tile_order_kernel and the conv kernel share conv_tile_live / conv_tile_order_slot
of csrc/conv.hip).

Four properties, for 2 and 3 members of 1, 5, 8, 9 and 341 tiles under four map patterns:
  * the list is a permutation of all (member, tile) pairs;
  * every live entry (a member without a map: all of its tiles) comes before every dead one;
  * the live tiles of the blockIdx % 8 classes are level to within one;
  * inside a class the live tiles of one member follow each other (an XCD finishes one member's filter before the next).
A ragged last tile (rows not a multiple of 256) is decided by its single partial block."""
import ctypes as C

import numpy as np
import pytest

NGROUPS = (2, 3)
TILES = (1, 5, 8, 9, 341)
PATTERNS = ('zero', 'ones', 'first', 'last')


@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd import _C
    return _C.lib


def _map(pattern, rows):
    nblk = (rows + 63) // 64
    m = np.zeros(nblk, np.uint8)
    if pattern == 'ones':
        m[:] = 1
    elif pattern == 'first':
        m[0] = 1
    elif pattern == 'last':
        m[-1] = 1
    return m


def _order(lib, rows, maps, tiles_n=1):
    ng, nwg = len(maps), (rows + 255) // 256 * tiles_n
    n = ng * nwg
    keep = [np.ascontiguousarray(m) if m is not None else None for m in maps]
    ptrs = (C.c_void_p * ng)(*[(m.ctypes.data if m is not None else None) for m in keep])
    tile, group = (C.c_int32 * n)(), (C.c_int32 * n)()
    assert lib.aod_conv2d_tile_order(rows, tiles_n, ng, ptrs, tile, group) == 0
    return np.array(tile[:], np.int64), np.array(group[:], np.int64)


def _live(rows, maps, tile, group, tiles_n=1):
    """the definition, written out: a tile is live when its member has no map or some 64-row block of the tile's rows is set"""
    out = np.zeros(len(tile), bool)
    for b, (t, g) in enumerate(zip(tile, group)):
        m = maps[g]
        r0 = (t // tiles_n) * 256
        r1 = min(r0 + 256, rows)
        out[b] = True if m is None else bool(m[r0 // 64:(r1 - 1) // 64 + 1].any())
    return out


def _check(rows, maps, tile, group, tiles_n=1):
    ng, nwg = len(maps), (rows + 255) // 256 * tiles_n
    n = ng * nwg
    assert ((0 <= tile) & (tile < nwg) & (0 <= group) & (group < ng)).all()
    assert len(set(zip(tile.tolist(), group.tolist()))) == n                       # a permutation
    live = _live(rows, maps, tile, group, tiles_n)
    nlive = int(live.sum())
    assert live[:nlive].all() and not live[nlive:].any()                          # live before dead
    per = np.array([live[c::8].sum() for c in range(8)])
    assert per.max() - per.min() <= 1, per                                        # level over the classes
    for c in range(8):
        members = group[c::8][live[c::8]].tolist()
        runs = [g for i, g in enumerate(members) if i == 0 or members[i - 1] != g]
        assert len(runs) == len(set(runs)), (c, members)                          # one member's live tiles are consecutive
    return nlive


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('ntiles', TILES)
@pytest.mark.parametrize('ng', NGROUPS)
def test_list_properties(lib, ng, ntiles, pattern):
    rows = ntiles * 256
    maps = [None] + [_map(pattern, rows) for _ in range(ng - 1)]                   # member 0 has no map: all of its tiles are live
    tile, group = _order(lib, rows, maps)
    nlive = _check(rows, maps, tile, group)
    per_member = {'zero': 0, 'ones': ntiles, 'first': 1, 'last': 1}[pattern]
    assert nlive == ntiles + (ng - 1) * per_member


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('ntiles', TILES)
@pytest.mark.parametrize('ng', NGROUPS)
def test_ragged_last_tile_is_decided_by_its_partial_block(lib, ng, ntiles, pattern):
    rows = ntiles * 256 - 200                                                     # the last tile: 56 rows, one (partial) block
    maps = [None] + [_map(pattern, rows) for _ in range(ng - 1)]
    tile, group = _order(lib, rows, maps)
    nlive = _check(rows, maps, tile, group)
    per_member = {'zero': 0, 'ones': ntiles, 'first': 1, 'last': 1}[pattern]
    assert nlive == ntiles + (ng - 1) * per_member
    if pattern == 'last':                                                         # ... and it is the LAST tile that the last block keeps alive
        live = _live(rows, maps, tile, group)
        assert sorted(tile[live & (group > 0)].tolist()) == [ntiles - 1] * (ng - 1)


@pytest.mark.parametrize('ng', NGROUPS)
def test_every_member_mapped_and_different_maps(lib, ng):
    rows = 341 * 256
    rng = np.random.default_rng(5)
    maps = [(rng.random((rows + 63) // 64) < p).astype(np.uint8) for p in (0.02, 0.3, 0.0)[:ng]]
    tile, group = _order(lib, rows, maps)
    _check(rows, maps, tile, group)


def test_bench_shape_live_entries_follow_the_xcd_ranges(lib):
    """3 x 341 tiles, the mapped members live on the last 85 tiles: 511 live entries, 63 or 64 per class; class 0 holds tiles 0 .. 63 of the
    dense member in this order, and the dead entries follow member-major"""
    rows, nwg = 341 * 256, 341
    m = np.zeros((rows + 63) // 64, np.uint8)
    m[(nwg - 85) * 4:] = 1
    maps = [None, m, m]
    tile, group = _order(lib, rows, maps)
    assert _check(rows, maps, tile, group) == 511
    assert tile[0:512:8].tolist() == list(range(64)) and set(group[0:512:8].tolist()) == {0}
    dead_t, dead_g = tile[511:], group[511:]
    assert dead_g.tolist() == [1] * 256 + [2] * 256 and dead_t.tolist() == list(range(256)) * 2


def test_two_column_tiles_share_their_row_tile(lib):
    rows = 9 * 256
    maps = [None, _map('last', rows)]
    tile, group = _order(lib, rows, maps, tiles_n=2)
    assert _check(rows, maps, tile, group, tiles_n=2) == 18 + 2


def test_entry_refuses_bad_arguments(lib):
    one = (C.c_int32 * 8)()
    ptrs = (C.c_void_p * 4)()
    assert lib.aod_conv2d_tile_order(0, 1, 2, ptrs, one, one) == -1
    assert lib.aod_conv2d_tile_order(256, 1, 5, ptrs, one, one) == -1
    assert lib.aod_conv2d_tile_order(256, 1, 2, None, one, one) == -1
    assert lib.aod_conv2d_tile_order(256, 1, 2, ptrs, None, one) == -1
