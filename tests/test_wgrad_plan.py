"""Which kernel a weight gradient runs on and how its pixel axis is split (csrc/conv_wgrad.hip wgrad_make_plan, reported by
aod_conv2d_wgrad_plan_ex): the full plan for a table of shapes, at least one case on each side of every rule.  Host logic: no device is needed.

form / splits / rows_per_split of every case were recorded from the three plan functions (aod_conv2d_wgrad_splits, _group_plan, _plan) of the
library built from commit 11f5e1a, the parent of the change that made the plan data; they are literals here.  The atomic case, which that
library could not report, and one member through the group planner, of which it reported the splits only, are derived by hand (see the cases).
instance / threads / lds_bytes / grid are derived by hand from the rule table of DESIGN.md 3.2:
    grid = sum over the members of ceil(N / T) * ceil(K / T) * splits, T = 128 * tile physical columns,
    lds_bytes = 2 stages * 2 * tile sub-images * (64 pixel rows, the wide forms 32) * 256 B + 4096 (+ 8192 when sparse).

Shapes are given in LOGICAL channels; in the reference-precision mode (x3) an operand has 2 * ceil32(c) physical columns.
The AOD_WGRAD_* switches are read once per process, so every table -- the default one and the cases under AOD_WGRAD_X3_WIDE=0 and under
AOD_WGRAD_W8=0 -- runs the same table function in a fresh child process of its own, whose environment the test sets."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOMIC, GROUPED = 1, 2
HAS_MAP = lambda g: 16 << g

# the ten tile instances (wide, waves, tile, x3, sparse): conv_wgrad_kernel<waves, tile, tile, x3, sparse> / conv_wgrad_x3w_kernel<waves, tile, sparse>
W4, W8, W8B = (0, 4, 1, 0, 0), (0, 8, 1, 0, 0), (0, 8, 2, 0, 0)
X4, X4S, X8B = (0, 4, 1, 1, 0), (0, 4, 1, 1, 1), (0, 8, 2, 1, 0)
XW4, XW4S, XW8, XW8S = (1, 4, 2, 1, 0), (1, 4, 2, 1, 1), (1, 8, 4, 1, 0), (1, 8, 4, 1, 1)
LDS_64K, LDS_128K, SLIST = 65536 + 4096, 131072 + 4096, 8192


def wdesc(cin, cout, k, segs, *, x3=True, gap=0):
    """forward descriptor of the conv cin -> cout (stride 1, pad k // 2) over the maps `segs` [(B, H, W), ...], as the weight gradient takes
    it: C / N = physical columns of x / dZ.  gap > 0: the dZ segments do not follow each other densely (a row-activity map then does not apply)"""
    from aod_meh_hua_amd._C import ConvDesc, ConvSeg
    phys = lambda c: 2 * ((c + 31) // 32 * 32) if x3 else (c + 7) // 8 * 8
    d = ConvDesc()
    d.R = d.S = k
    d.stride, d.pad, d.dil, d.nseg, d.x3 = 1, k // 2, 1, len(segs), int(x3)
    d.C, d.N = phys(cin), phys(cout)
    r = 0
    for i, (B, H, W) in enumerate(segs):
        d.seg[i] = ConvSeg(B, H, W, H, W, r, r + i * gap)
        r += B * H * W
    return d


ROWS = lambda m: [(1, 1, m)]                   # m pixel rows as one 1 x m map
B16 = lambda h: [(16, h, h)]
PYR = [(2, 32, 32), (2, 16, 16), (2, 8, 8), (2, 4, 4), (2, 2, 2)]      # a small pyramid: 2 728 rows
PYR_172 = [(2, 64, 64), (2, 32, 32), (2, 16, 16), (2, 8, 8), (2, 6, 6)]     # 10 952 rows = 172 steps of 64
T256 = (256, 256, 1, [(12, 64, 64)])           # 49 152 rows: the single launch's threshold of the big forms
G256 = (256, 256, 1, [(4, 64, 64)])            # 16 384 rows: a group member's
# name, members (cin, cout, k, segs[, descriptor options]), x3, options (atomic, grouped, maps = members that carry a map)
INPUTS = {
    'default': [
        # ---- bf16: 256 x 256 tile from 49 152 rows on alone, from 16 384 in a group, N and K multiples of 256
        ('b_big', [T256], False, {}),
        ('b_below', [(256, 256, 1, ROWS(49151))], False, {}),
        ('b_n128', [(256, 128, 1, [(12, 64, 64)])], False, {}),
        ('b_3x3', [(64, 64, 3, B16(56))], False, {}),
        ('b_map_ignored', [T256], False, dict(maps=(0,))),
        ('b_atomic', [(256, 256, 1, B16(32))], False, dict(atomic=True)),
        ('b_slabs', [(256, 256, 1, B16(32))], False, {}),
        ('b_group_big', [G256, G256], False, {}),
        ('b_group_below', [(256, 256, 1, ROWS(16383))] * 2, False, {}),
        ('b_group_block', [(64, 64, 1, B16(56)), (64, 64, 3, B16(56)), (64, 256, 1, B16(56))], False, {}),
        ('b_group_mixed_forms', [G256, (128, 128, 1, [(4, 64, 64)])], False, {}),
        ('b_group_of_one', [(64, 64, 3, B16(56))], False, dict(grouped=True)),
        ('mixed_precisions', [G256, G256 + (dict(x3=True),)], False, {}),
        # ---- x3: physical N = K = 512 here
        ('x_wide8', [T256], True, {}),
        ('x_wide8_map', [T256], True, dict(maps=(0,))),
        ('x_wide8_below', [(256, 256, 1, ROWS(49151))], True, {}),
        ('x_wide8_group', [G256, G256], True, {}),
        ('x_wide8_group_one_map', [G256, G256], True, dict(maps=(1,))),
        ('x_wide4_group_below', [(256, 256, 1, ROWS(16383))] * 2, True, dict(maps=(0, 1))),
        ('x_wide4', [(128, 128, 1, ROWS(4096 + 30))], True, {}),
        ('x_wide4_map', [(128, 128, 1, ROWS(4096 + 30))], True, dict(maps=(0,))),
        ('x_wide4_map_not_dense', [(128, 128, 1, [(1, 1, 2048), (1, 1, 2078)], dict(gap=64))], True, dict(maps=(0,))),
        # narrow dZ: 128 physical columns take the wide 4-wave form with a ragged tile from 16 384 rows on, 64 columns never
        ('x_ragged', [(128, 64, 1, ROWS(16384 + 30))], True, dict(maps=(0,))),
        ('x_ragged_below', [(128, 64, 1, ROWS(16383))], True, dict(maps=(0,))),
        ('x_ragged_384', [(128, 180, 1, ROWS(16384))], True, {}),
        ('x_n64', [(128, 32, 1, ROWS(16384 + 30))], True, {}),
        ('x_n64_map', [(128, 32, 1, ROWS(16384 + 30))], True, dict(maps=(0,))),
        ('x_n64_group_maps', [(128, 32, 1, ROWS(4096 + 30))] * 3, True, dict(maps=(0, 2))),
        ('x_group_mixed_forms', [G256, (128, 32, 1, [(4, 64, 64)])], True, {}),
        # four tower filters at a small pyramid, 4 x 36 tiles of 256 x 256 on 512 slots: three splits each, 58 steps per workgroup, against 13
        # steps each alone -- the cost rule prefers four launches (580 x 10 > 4 x 13 x 11); two of them, or four at the tiny pyramid, do group
        ('x_towers_alone', [(256, 256, 3, PYR_172)] * 4, True, dict(maps=(0, 1, 2, 3))),
        ('x_towers_pair', [(256, 256, 3, PYR_172)] * 2, True, {}),
        ('x_towers_tiny_group', [(256, 256, 3, PYR)] * 4, True, {}),
        ('x_tower', [(256, 256, 3, PYR)], True, dict(maps=(0,))),
        ('x_group_of_one', [(256, 256, 3, PYR)], True, dict(grouped=True)),
    ],
    # AOD_WGRAD_X3_WIDE=0: x3 on the tiles of the bf16 mode; its 256 x 256 form has no sparse instance and ignores a map
    'AOD_WGRAD_X3_WIDE': [
        ('x_big', [T256], True, dict(maps=(0,))),
        ('x_big_group', [G256, G256], True, dict(maps=(0, 1))),
        ('x_small_map', [(256, 256, 1, ROWS(49151))], True, dict(maps=(0,))),
    ],
    # AOD_WGRAD_W8=0: the 4-wave bf16 instance, which only the single launch has
    'AOD_WGRAD_W8': [
        ('b_w4', [(256, 256, 1, B16(32))], False, {}),
        ('b_w4_atomic', [(256, 256, 1, B16(32))], False, dict(atomic=True)),
        ('b_big_stays', [T256], False, {}),
        ('b_group_stays_w8', [(256, 256, 1, ROWS(16383))] * 2, False, {}),
    ],
}

# name -> None (return value 1: the members do not share a grid) or (form, instance, threads, lds_bytes, grid, splits, rows_per_split)
EXPECT = {
    'default': {
        'b_big': (1, W8B, 512, LDS_128K, 128, [128], [384]),
        'b_below': (0, W8, 512, LDS_64K, 256, [64], [768]),
        'b_n128': (0, W8, 512, LDS_64K, 256, [128], [384]),
        'b_3x3': (0, W8, 512, LDS_64K, 490, [98], [512]),
        'b_map_ignored': (1, W8B, 512, LDS_128K, 128, [128], [384]),
        # by hand: 4 tiles, cost(sp) = steps * (1.45, or 1.7 over 256 workgroups) + workgroups * 0.05 -- 7 steps x 37 splits 17.55, 6 x 43 17.3,
        # 5 x 52 17.65: 43 splits of 384 rows.  The slab form pays 0.012 + 0.105 per split instead (next case): 6 x 43 15.28, 5 x 52 15.21, 4 x 64 15.59
        'b_atomic': (0, W8, 512, LDS_64K, 172, [43], [384]),
        'b_slabs': (0, W8, 512, LDS_64K, 208, [52], [320]),
        'b_group_big': (1, W8B, 512, LDS_128K, 256, [128, 128], [128, 128]),
        'b_group_below': (0, W8, 512, LDS_64K, 512, [64, 64], [256, 256]),
        'b_group_block': (0, W8, 512, LDS_64K, 488, [61, 61, 61], [832, 832, 832]),
        'b_group_mixed_forms': None,
        # (the recorded splits; rows_per_split by hand: 5 tiles x ceil(784 steps / T) <= 512 slots first at T = 8 steps)
        'b_group_of_one': (0, W8, 512, LDS_64K, 490, [98], [512]),
        'mixed_precisions': None,
        'x_wide8': (2, XW8, 512, LDS_128K, 154, [154], [320]),
        'x_wide8_map': (2, XW8S, 512, LDS_128K + SLIST, 154, [154], [320]),
        'x_wide8_below': (3, XW4, 256, LDS_64K, 256, [64], [768]),
        'x_wide8_group': (2, XW8, 512, LDS_128K, 256, [128, 128], [128, 128]),
        'x_wide8_group_one_map': (2, XW8S, 512, LDS_128K + SLIST, 256, [128, 128], [128, 128]),
        'x_wide4_group_below': (3, XW4S, 256, LDS_64K + SLIST, 512, [64, 64], [256, 256]),
        'x_wide4': (3, XW4, 256, LDS_64K, 33, [33], [128]),
        'x_wide4_map': (3, XW4S, 256, LDS_64K + SLIST, 33, [33], [128]),
        'x_wide4_map_not_dense': (3, XW4, 256, LDS_64K, 33, [33], [128]),
        'x_ragged': (3, XW4S, 256, LDS_64K + SLIST, 86, [86], [192]),
        'x_ragged_below': (0, X4S, 256, LDS_64K + SLIST, 172, [86], [192]),
        'x_ragged_384': (3, XW4, 256, LDS_64K, 128, [64], [256]),
        'x_n64': (0, X4, 256, LDS_64K, 172, [86], [192]),
        'x_n64_map': (0, X4S, 256, LDS_64K + SLIST, 172, [86], [192]),
        'x_n64_group_maps': (0, X4S, 256, LDS_64K + SLIST, 390, [65, 65, 65], [64, 64, 64]),
        'x_group_mixed_forms': None,
        'x_towers_alone': None,
        'x_towers_pair': (3, XW4, 256, LDS_64K, 504, [7, 7], [1600, 1600]),
        'x_towers_tiny_group': (3, XW4, 256, LDS_64K, 432, [3, 3, 3, 3], [960, 960, 960, 960]),
        'x_tower': (3, XW4S, 256, LDS_64K + SLIST, 180, [5], [576]),
        # (the recorded splits; rows_per_split by hand: 36 tiles x ceil(43 steps / T) <= 512 slots first at T = 4 steps)
        'x_group_of_one': (3, XW4, 256, LDS_64K, 396, [11], [256]),
    },
    'AOD_WGRAD_X3_WIDE': {
        'x_big': (1, X8B, 512, LDS_128K, 256, [64], [768]),
        'x_big_group': (1, X8B, 512, LDS_128K, 256, [32, 32], [512, 512]),
        'x_small_map': (0, X4S, 256, LDS_64K + SLIST, 512, [32], [1536]),
    },
    'AOD_WGRAD_W8': {
        'b_w4': (0, W4, 256, LDS_64K, 208, [52], [320]),
        'b_w4_atomic': (0, W4, 256, LDS_64K, 172, [43], [384]),
        'b_big_stays': (1, W8B, 512, LDS_128K, 128, [128], [384]),
        'b_group_stays_w8': (0, W8, 512, LDS_64K, 512, [64, 64], [256, 256]),
    },
}


def plan(lib, members, x3, opts):
    from aod_meh_hua_amd._C import WgradPlan
    descs = []
    for m in members:
        kw = dict(x3=x3)
        kw.update(m[4] if len(m) > 4 else {})
        descs.append(wdesc(*m[:4], **kw))
    n = len(descs)
    flags = (ATOMIC if opts.get('atomic') else 0) | (GROUPED if opts.get('grouped') else 0)
    for g in opts.get('maps', ()):
        flags |= HAS_MAP(g)
    p = WgradPlan()
    rc = lib.aod_conv2d_wgrad_plan_ex((ctypes.c_void_p * n)(*[ctypes.addressof(d) for d in descs]), n, flags, ctypes.byref(p))
    assert rc in (0, 1), lib.aod_last_error()
    if rc:
        return None
    assert p.grouped == int(n > 1 or bool(opts.get('grouped')))
    assert p.grid == sum(p.tiles_n[g] * p.tiles_k[g] * p.splits[g] for g in range(n))
    return (p.form, (p.wide, p.waves, p.tile, p.x3, p.sparse), p.threads, p.lds_bytes, p.grid, list(p.splits[:n]), list(p.rows_per_split[:n]))


def check_table(which):
    """every case of INPUTS[which] against EXPECT; returns the number of cases (child processes print it)"""
    from aod_meh_hua_amd.build import build
    build(verbose=False)
    from aod_meh_hua_amd._C import lib
    for name, members, x3, opts in INPUTS[which]:
        got = plan(lib, members, x3, opts)
        assert got == EXPECT[which][name], (which, name, got, EXPECT[which][name])
    return len(INPUTS[which])


def test_table_covers_every_instance_and_both_outcomes():
    rows = [e for t in EXPECT.values() for e in t.values()]
    assert sum(len(t) for t in INPUTS.values()) == len(rows) >= 30
    assert {e[1] for e in rows if e} == {W4, W8, W8B, X4, X4S, X8B, XW4, XW4S, XW8, XW8S}
    assert {e[0] for e in rows if e} == {0, 1, 2, 3} and sum(e is None for e in rows) >= 4


def test_map_is_dropped_with_sparse_backward_off(monkeypatch):
    """AOD_SPARSE_BWD is a per-call switch: 0 -- no launch follows a map"""
    from aod_meh_hua_amd.build import build
    build(verbose=False)
    from aod_meh_hua_amd._C import lib
    rows = {r[0]: r for r in INPUTS['default']}
    for name in ('x_wide8_map', 'x_wide4_map', 'x_n64_map'):
        on = plan(lib, *rows[name][1:])
        assert on == EXPECT['default'][name] and on[1][4] == 1
        monkeypatch.setenv('AOD_SPARSE_BWD', '0')
        off = plan(lib, *rows[name][1:])
        monkeypatch.delenv('AOD_SPARSE_BWD')
        assert off == (on[0], on[1][:4] + (0,), on[2], on[3] - SLIST) + on[4:]


@pytest.mark.parametrize('var', ['default', 'AOD_WGRAD_X3_WIDE', 'AOD_WGRAD_W8'])
def test_plan_table_in_a_fresh_process(var):
    """every table in a child process whose environment holds no AOD_WGRAD_* variable but the table's own switch (`default`: none)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith('AOD_WGRAD_') and k != 'AOD_SPARSE_BWD'}
    if var != 'default':
        env[var] = '0'
    code = f'import tests.test_wgrad_plan as t; print("cases", t.check_table({var!r}))'
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f'cases {len(INPUTS[var])}' in r.stdout, r.stdout + r.stderr
