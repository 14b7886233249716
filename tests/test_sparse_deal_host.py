"""CPU (no GPU): the block -> (tile, member) deal of the grouped conv launches, read through aod_conv2d_grouped_deal (the kernel and the entry
call the same __host__ __device__ function, conv_grouped_deal of csrc/conv.hip).

A launch without a row-activity map keeps the member-major order over xcd_swizzle (every XCD -- blockIdx % 8 -- a contiguous range of
tiles).  A launch that carries a map (sparse forward, sparse backward) deals each member's consecutive tiles over the eight classes, because
its live tiles cluster on the coarse pyramid levels -- the tail of the tile range -- and a contiguous range per XCD hands them all to two XCDs.

"No class holds tiles of a single member only" is checked for every class that receives at least two blocks: with 3 tiles x 2 members the
launch has six blocks, one per class, and no deal can give a class two members."""
import ctypes as C

import numpy as np
import pytest

NGROUPS = (2, 3)
TILES = (3, 8, 35, 168, 341)


@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd import _C
    return _C.lib


def _deal(lib, nwg, ng, mapped):
    n = nwg * ng
    tile, group = (C.c_int32 * n)(), (C.c_int32 * n)()
    assert lib.aod_conv2d_grouped_deal(nwg, ng, mapped, tile, group) == 0
    return np.array(tile[:], np.int64), np.array(group[:], np.int64)


def _xcd_swizzle(bid, nwg):
    """csrc/conv.hip xcd_swizzle as it stood before the deal existed"""
    q, r, xcd, j = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + j


@pytest.mark.parametrize('ng', NGROUPS)
@pytest.mark.parametrize('nwg', TILES)
def test_mapped_deal_is_a_bijection_that_spreads_every_member(lib, nwg, ng):
    tile, group = _deal(lib, nwg, ng, 1)
    n = nwg * ng
    assert ((0 <= tile) & (tile < nwg) & (0 <= group) & (group < ng)).all()
    assert len(set(zip(tile.tolist(), group.tolist()))) == n                      # a bijection of [0, nwg * ngroups)
    cls_of = np.full((ng, nwg), -1, np.int64)
    cls_of[group, tile] = np.arange(n) % 8
    assert (cls_of >= 0).all()
    # any 64 consecutive tiles of one member: 7 .. 9 on each class
    for g in range(ng):
        for s in range(0, nwg - 63):
            c = np.bincount(cls_of[g, s:s + 64], minlength=8)
            assert c.min() >= 7 and c.max() <= 9, (g, s, c)
    # every class that holds two blocks or more holds two members or more
    for c in range(8):
        members = group[np.arange(n) % 8 == c]
        assert len(members) < 2 or len(set(members.tolist())) >= 2, (c, members)
    # each member's tiles over the classes as a whole: level to within one
    if nwg >= 8:
        for g in range(ng):
            c = np.bincount(cls_of[g], minlength=8)
            assert c.max() - c.min() <= 1, (g, c)


@pytest.mark.parametrize('ng', NGROUPS + (1, 4))
@pytest.mark.parametrize('nwg', TILES)
def test_unmapped_launch_keeps_the_xcd_swizzle(lib, nwg, ng):
    tile, group = _deal(lib, nwg, ng, 0)
    wg = np.array([_xcd_swizzle(b, nwg * ng) for b in range(nwg * ng)], np.int64)
    assert sorted(wg.tolist()) == list(range(nwg * ng))
    assert np.array_equal(tile, wg % nwg) and np.array_equal(group, wg // nwg)


def test_bench_forward_live_tiles_land_on_all_eight_classes(lib):
    """The bench shape: 341 tiles, 3 members, the mapped members live on the last 85 tiles only (P4 - P7).  Old order (member-major over
    xcd_swizzle): those tiles sit on two classes.  New deal: 10 or 11 on each."""
    nwg, ng = 341, 3
    live = lambda t, g: g == 0 or t >= nwg - 85
    for mapped in (1, 0):
        tile, group = _deal(lib, nwg, ng, mapped)
        per = np.zeros(8, np.int64)
        for b in range(nwg * ng):
            per[b % 8] += live(tile[b], group[b])
        assert per.sum() == 341 + 2 * 85
        if mapped:
            assert per.min() >= 63 and per.max() <= 65, per                       # 511 live tiles / 8 = 63.9
        else:
            assert per.max() >= 120 and per.min() <= 45, per                      # whole XCDs of the dense member beside nearly idle ones


def test_entry_refuses_bad_arguments(lib):
    one = (C.c_int32 * 8)()
    assert lib.aod_conv2d_grouped_deal(0, 2, 1, one, one) == -1
    assert lib.aod_conv2d_grouped_deal(2, 5, 1, one, one) == -1
    assert lib.aod_conv2d_grouped_deal(2, 2, 1, None, one) == -1
