"""Which kernel a forward / dgrad convolution runs on (csrc/conv.hip conv_plan, reported by aod_conv2d_plan): the full plan for a table of
shapes, at least one case on each side of every rule.  Host logic: no device is needed, the CU count then counts as 256 (the MI355X's, so the
expectations hold on the GPU box as well).  The expectations are derived by hand from the rules (DESIGN.md "How a conv picks its kernel"); the
per-call switches are set with monkeypatch, the once-per-process ones are exercised in their default state only.

Shapes are given in LOGICAL channels; in the reference-precision mode (x3) the source of a launch has 2 * ceil32(c) physical columns, so a
K-step of 64 columns is 32 channels of one tap."""
import ctypes

import pytest

PW, SPLIT_K, X3P, IGEMM = 1, 2, 3, 4
PRE_SCALE, PRE_SHIFT, RES, RES_IS_DST, MASK, POST_SCALE, ZRAW, COLSUM, WORKSPACE = (1 << i for i in range(9))


@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd.build import build
    build(verbose=False)
    from aod_meh_hua_amd._C import lib
    return lib


def desc(cin, cout, k, segs, *, stride=1, dgrad=False, out_f32=False, x3=True):
    """forward: cin -> cout over source maps `segs` [(B, H, W), ...]; dgrad: the descriptor of that conv's input gradient (source = dZ)"""
    from aod_meh_hua_amd._C import ConvDesc, ConvSeg
    pad = k // 2
    phys = lambda c: 2 * ((c + 31) // 32 * 32) if x3 else c
    d = ConvDesc()
    d.R = d.S = k
    d.stride, d.pad, d.dil, d.transposed, d.out_f32, d.nseg, d.x3 = stride, pad, 1, int(dgrad), int(out_f32), len(segs), int(x3)
    d.C, d.N = (phys(cout), cin) if dgrad else (phys(cin), cout)
    r_in = r_out = 0
    for i, (B, H, W) in enumerate(segs):
        oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        d.seg[i] = ConvSeg(B, oh, ow, H, W, r_out, r_in) if dgrad else ConvSeg(B, H, W, oh, ow, r_in, r_out)
        r_in, r_out = r_in + B * H * W, r_out + B * oh * ow
    return d


def plan(lib, d, flags=0, ngroups=0):
    from aod_meh_hua_amd._C import ConvPlan
    p = ConvPlan()
    rc = lib.aod_conv2d_plan(ctypes.byref(d), ngroups, flags, ctypes.byref(p))
    assert rc == 0, lib.aod_last_error()
    if p.kind == X3P:
        return ('X3P', p.taps, p.wide, p.pre, p.lat, p.grid)
    if p.kind in (IGEMM, SPLIT_K):
        t = ('IGEMM', p.bm, p.bn, p.nt, p.ops, p.stages, p.x3, p.grouped)
        return t if p.kind == IGEMM else ('SPLIT_K', p.ksplit) + t[1:]
    return ({PW: 'PW_STREAM', 0: 'EMPTY'}[p.kind],)


def igemm(bm, bn, nt=256, ops=2, stages=2, x3=1, grouped=0):
    return ('IGEMM', bm, bn, nt, ops, stages, x3, grouped)


def x3p(taps, wide=0, pre=0, lat=0, grid=256):
    return ('X3P', taps, wide, pre, lat, grid)


B16 = lambda h: [(16, h, h)]
# (name, descriptor arguments, operand flags, environment, expected plan)            -- M = rows of the destination
X3_CASES = [
    # the 256 x 256 tile: N % 256 == 0, K >= 2048, no residual, 256 tiles = one full round
    ('t256', dict(cin=256, cout=256, k=3, segs=B16(64)), 0, {}, igemm(256, 256, 512, 0)),
    ('t256_mask', dict(cin=256, cout=256, k=3, segs=B16(64)), MASK, {}, igemm(256, 256, 512, 1)),
    ('t256_res', dict(cin=256, cout=256, k=3, segs=B16(64)), RES, {}, x3p(9, wide=1)),                    # residual: no big tile -> persistent kernel
    ('t256_over', dict(cin=256, cout=256, k=3, segs=B16(64)), 0, {'AOD_X3P_OVER_256': '1'}, x3p(9, wide=1)),
    # 64 big tiles fill a quarter of a round -> the persistent kernel: 72 K-steps, 256 tiles of 128 columns; 128 wide tiles < 192 -> not wide
    ('x3p', dict(cin=256, cout=256, k=3, segs=B16(32)), 0, {}, x3p(9)),
    ('x3p_bn256', dict(cin=256, cout=256, k=3, segs=B16(32)), 0, {'AOD_X3P_BN': '256'}, x3p(9, wide=1, grid=128)),
    ('x3p_off', dict(cin=256, cout=256, k=3, segs=B16(32)), 0, {'AOD_X3P': '0'}, igemm(64, 128, stages=3)),      # 256 tiles of 128 x 128 < 512, 512 of 64 x 128
    ('x3p_wide', dict(cin=512, cout=256, k=1, segs=B16(64)), 0, {}, x3p(1, wide=1)),                       # 512 wide tiles >= 192; 16 steps x 2 >= 24
    # expand 1x1 with residual: 4 K-steps < 24
    ('expand', dict(cin=128, cout=512, k=1, segs=B16(64)), RES, {}, igemm(128, 128)),
    ('expand_pre', dict(cin=128, cout=512, k=1, segs=B16(64)), RES, {'AOD_X3P_PRE_MIN_STEPS': '1'}, x3p(1, pre=1)),
    ('expand_min', dict(cin=128, cout=512, k=1, segs=B16(64)), RES, {'AOD_X3P_MIN_STEPS': '1'}, x3p(1, pre=1)),
    ('expand_nopre', dict(cin=128, cout=512, k=1, segs=B16(64)), RES, {'AOD_X3P_PRE_MIN_STEPS': '1', 'AOD_X3P_PRE': '0'}, igemm(128, 128)),
    ('expand_nopre_min', dict(cin=128, cout=512, k=1, segs=B16(64)), RES, {'AOD_X3P_MIN_STEPS': '1', 'AOD_X3P_PRE': '0'}, x3p(1, wide=1)),
    ('mask_pre', dict(cin=512, cout=128, k=1, segs=B16(64), dgrad=True), MASK | COLSUM, {'AOD_X3P_PRE_MIN_STEPS': '1'}, x3p(1, pre=2)),
    ('res_deep', dict(cin=1024, cout=256, k=1, segs=B16(32)), RES, {}, x3p(1, pre=1)),                      # 32 K-steps >= 24 even with a residual
    # retina_cls: 180 columns, fp32 destination
    ('t192', dict(cin=256, cout=180, k=3, segs=B16(64), out_f32=True), 0, {}, igemm(192, 192, 512, 0)),
    ('t192_off', dict(cin=256, cout=180, k=3, segs=B16(64), out_f32=True), 0, {'AOD_X3_TILE_192': '0'}, igemm(128, 64)),      # ragged: 3 x 64 columns
    ('t192_small', dict(cin=256, cout=180, k=3, segs=B16(16), out_f32=True), 0, {}, igemm(64, 64, stages=3)),                # 22 tiles of 192 x 192 < 240
    # split-K: 144 K-steps, 16 x 16 outputs per image, 128 tiles -> 4 slices; only with a workspace
    ('splitk', dict(cin=512, cout=512, k=3, segs=B16(16)), WORKSPACE, {}, ('SPLIT_K', 4, 128, 128, 256, 2, 2, 1, 0)),
    ('splitk_nows', dict(cin=512, cout=512, k=3, segs=B16(16)), 0, {}, igemm(64, 64, stages=3)),            # 128 tiles < 192: not the persistent kernel either
    ('splitk_nows_x3p', dict(cin=512, cout=512, k=3, segs=B16(16)), 0, {'AOD_X3P_MIN_TILES': '1'}, x3p(9, grid=128)),
    ('splitk_narrow', dict(cin=512, cout=64, k=3, segs=B16(16)), WORKSPACE, {}, ('SPLIT_K', 16, 128, 64, 256, 2, 2, 1, 0)),
    # narrow outputs: 128 x 64
    ('n64', dict(cin=128, cout=64, k=1, segs=B16(64)), 0, {}, igemm(128, 64)),
    # dgrads: stride 1 like the forward; AOD_X3P_DGRAD=0 (set under an overlapped all-reduce) keeps them on the general kernel
    ('dgrad', dict(cin=256, cout=256, k=3, segs=B16(32), dgrad=True), MASK | COLSUM, {}, x3p(9)),
    ('dgrad_off', dict(cin=256, cout=256, k=3, segs=B16(32), dgrad=True), MASK | COLSUM, {'AOD_X3P_DGRAD': '0'}, igemm(64, 128, stages=3)),
    ('fwd_dgrad_off', dict(cin=256, cout=256, k=3, segs=B16(32)), 0, {'AOD_X3P_DGRAD': '0'}, x3p(9)),
    # class-major stride-2 3x3 dgrad (lat 1): four classes x 128 row tiles, 18 K-steps per average class >= 12
    ('lat1', dict(cin=128, cout=256, k=3, segs=B16(64), stride=2, dgrad=True), 0, {}, x3p(4, lat=1)),
    ('lat1_off', dict(cin=128, cout=256, k=3, segs=B16(64), stride=2, dgrad=True), 0, {'AOD_X3P_LATTICE': '0'}, igemm(128, 128)),
    ('lat1_t256', dict(cin=256, cout=256, k=3, segs=B16(64), stride=2, dgrad=True), 0, {}, igemm(256, 256, 512, 0)),
    ('lat1_wide', dict(cin=256, cout=256, k=3, segs=B16(64), stride=2, dgrad=True), 0, {'AOD_X3P_OVER_256': '1'}, x3p(4, wide=1, lat=1)),
    ('lat1_odd', dict(cin=128, cout=256, k=3, segs=[(16, 63, 63)], stride=2, dgrad=True), 0, {}, igemm(64, 128, stages=3)),
    # in-place 1x1 stride-2 dgrad (res == dst, lat 2): a GEMM over the 16 384 dZ pixels; with another residual buffer a general stride-2 dgrad
    ('lat2', dict(cin=512, cout=1024, k=1, segs=B16(64), stride=2, dgrad=True), RES | RES_IS_DST, {}, x3p(1, wide=1, lat=2)),
    ('lat2_off', dict(cin=512, cout=1024, k=1, segs=B16(64), stride=2, dgrad=True), RES | RES_IS_DST, {'AOD_X3P_LATTICE': '0'}, igemm(128, 128)),
    ('lat2_res', dict(cin=512, cout=1024, k=1, segs=B16(64), stride=2, dgrad=True), RES, {}, igemm(128, 128)),
    # pyramids: a tile must not straddle two segments (288 rows in the middle level)
    ('segs', dict(cin=256, cout=256, k=3, segs=[(2, 32, 32), (2, 16, 16), (2, 8, 8)]), 0, {'AOD_X3P_MIN_TILES': '1'}, x3p(9, grid=42)),
    ('segs_ragged', dict(cin=256, cout=256, k=3, segs=[(2, 32, 32), (2, 12, 12), (2, 8, 8)]), 0, {'AOD_X3P_MIN_TILES': '1'}, igemm(64, 64, stages=3)),
    ('segs_ragged_last', dict(cin=256, cout=256, k=3, segs=[(2, 32, 32), (2, 16, 16), (2, 5, 6)]), 0, {'AOD_X3P_MIN_TILES': '1'}, x3p(9, grid=42)),
]


@pytest.mark.parametrize('name,args,flags,env,expect', X3_CASES, ids=[c[0] for c in X3_CASES])
def test_plan_of_reference_precision_launches(lib, monkeypatch, name, args, flags, env, expect):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert plan(lib, desc(**args), flags) == expect


BF16_CASES = [
    ('t256', dict(cin=256, cout=256, k=3, segs=B16(64)), 0, igemm(256, 256, 512, 0, x3=0)),
    ('t256_mask', dict(cin=256, cout=256, k=3, segs=B16(64), dgrad=True), MASK | COLSUM, igemm(256, 256, 512, 1, x3=0)),
    ('t256_res', dict(cin=256, cout=256, k=3, segs=B16(64)), RES, igemm(128, 128, x3=0)),
    ('t256_partial', dict(cin=256, cout=256, k=3, segs=B16(32)), 0, igemm(64, 128, 256, 2, 3, x3=0)),      # 64 big tiles; 256 of 128 x 128 < 512
    ('w8', dict(cin=256, cout=128, k=3, segs=B16(64)), 0, igemm(128, 128, 512, 0, x3=0)),
    ('w8_mask', dict(cin=256, cout=128, k=3, segs=B16(64)), MASK, igemm(128, 128, 512, 1, x3=0)),
    ('w8_shallow', dict(cin=64, cout=128, k=3, segs=B16(64)), 0, igemm(128, 128, x3=0)),                    # K = 576 < 1024
    ('ring3', dict(cin=256, cout=256, k=3, segs=B16(32)), RES, igemm(64, 128, 256, 2, 3, x3=0)),
    ('ring2', dict(cin=128, cout=256, k=1, segs=B16(32)), RES, igemm(64, 128, 256, 2, 2, x3=0)),           # K = 128 < 256: two stages
    ('small', dict(cin=128, cout=256, k=1, segs=B16(8)), RES, igemm(64, 64, 256, 2, 2, x3=0)),
    ('ragged', dict(cin=256, cout=180, k=3, segs=B16(64), out_f32=True), RES, igemm(128, 64, x3=0)),               # 128 + 52 columns -> 3 x 64
    ('ragged_w8', dict(cin=256, cout=180, k=3, segs=B16(64), out_f32=True), 0, igemm(128, 128, 512, 0, x3=0)),      # (no residual: eight waves first)
    ('splitk', dict(cin=512, cout=512, k=3, segs=B16(16)), WORKSPACE, ('SPLIT_K', 4, 128, 128, 256, 2, 2, 0, 0)),
    ('splitk_nows', dict(cin=512, cout=512, k=3, segs=B16(16)), 0, igemm(64, 64, 256, 2, 3, x3=0)),
]


@pytest.mark.parametrize('name,args,flags,expect', BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_plan_of_plain_bf16_launches(lib, name, args, flags, expect):
    assert plan(lib, desc(x3=False, **args), flags) == expect


def test_plan_of_pointwise_launches_follows_the_pointwise_mode(lib):
    """plain-bf16 1x1 / stride-1 launches: the streaming kernel by its own heuristic (64 columns over >= 65 536 rows), always (mode 1, when
    the shape allows) or never (mode 0)"""
    narrow, wide = desc(256, 64, 1, B16(64), x3=False), desc(256, 128, 1, B16(64), x3=False)
    prev = lib.aod_set_pointwise_mode(-1)
    try:
        assert plan(lib, narrow) == ('PW_STREAM',) and plan(lib, wide) == igemm(128, 128, x3=0)
        assert plan(lib, desc(256, 64, 1, B16(32), x3=False)) == igemm(64, 64, 256, 2, 3, x3=0)            # 16 384 rows
        assert plan(lib, desc(256, 64, 1, B16(64), stride=2, x3=False)) == igemm(64, 64, 256, 2, 3, x3=0)   # not stride 1
        lib.aod_set_pointwise_mode(1)
        assert plan(lib, narrow) == ('PW_STREAM',) and plan(lib, wide) == ('PW_STREAM',)
        assert plan(lib, desc(256, 64, 1, B16(64))) == igemm(128, 64)                                      # never in the x3 mode
        lib.aod_set_pointwise_mode(0)
        assert plan(lib, narrow) == igemm(128, 64, x3=0) and plan(lib, wide) == igemm(128, 128, x3=0)
    finally:
        lib.aod_set_pointwise_mode(prev)


def test_plan_of_grouped_tower_launches(lib, monkeypatch):
    tower = dict(cin=256, cout=256, k=3)
    # x3: always the grouped 256 x 256 tile (own instance with a mask), the persistent kernel on request
    d = desc(segs=B16(64), **tower)
    assert plan(lib, d, 0, 3) == igemm(256, 256, 512, 0, grouped=1)
    assert plan(lib, desc(segs=B16(64), dgrad=True, **tower), MASK | COLSUM, 3) == igemm(256, 256, 512, 1, grouped=1)
    assert plan(lib, desc(segs=B16(8), **tower), 0, 3) == igemm(256, 256, 512, 0, grouped=1)
    monkeypatch.setenv('AOD_X3P_GROUPED', '1')
    assert plan(lib, d, 0, 3) == x3p(9, wide=1)
    assert plan(lib, d, 0, 1) == x3p(9, wide=1)
    monkeypatch.setenv('AOD_X3P', '0')
    assert plan(lib, d, 0, 3) == igemm(256, 256, 512, 0, grouped=1)
    # plain bf16: 3 x 256 big tiles fill three rounds exactly -> 256 x 256; 3 x 16 of them fill 19 % of a round, 192 tiles of 128 x 128 fill
    # 37.5 % of the 512 slots -> 128 x 128 on eight waves
    assert plan(lib, desc(segs=B16(64), x3=False, **tower), 0, 3) == igemm(256, 256, 512, 0, x3=0, grouped=1)
    assert plan(lib, desc(segs=B16(16), x3=False, **tower), MASK, 3) == igemm(128, 128, 512, 1, x3=0, grouped=1)
    assert plan(lib, desc(segs=B16(16), x3=False, **tower), 0, 3) == igemm(128, 128, 512, 0, x3=0, grouped=1)


def test_plan_rejects_what_the_launch_rejects(lib):
    from aod_meh_hua_amd._C import ConvPlan
    p = ConvPlan()
    assert lib.aod_conv2d_plan(None, 0, 0, ctypes.byref(p)) == -1
    d = desc(256, 256, 3, B16(16))
    assert lib.aod_conv2d_plan(ctypes.byref(d), 5, 0, ctypes.byref(p)) == -1
    assert lib.aod_conv2d_plan(ctypes.byref(d), 0, ZRAW, ctypes.byref(p)) == -1 and b'zraw' in lib.aod_last_error()      # x3: no zraw
    d = desc(256, 64, 3, B16(16), x3=False)
    assert lib.aod_conv2d_plan(ctypes.byref(d), 3, 0, ctypes.byref(p)) == -1 and b'N >= 128' in lib.aod_last_error()
    assert plan(lib, desc(256, 256, 3, [(0, 16, 16)])) == ('EMPTY',)


@pytest.mark.gpu
def test_deterministic_column_sums_never_plan_the_atomic_kernels(lib):
    """With aod_set_deterministic(1) a launch that carries a column sum stays on the general kernel (ordered partial sums): neither the
    persistent x3 kernel nor the streaming 1x1 kernel, both of which add their column sums with atomics.  (The mode needs a device for its
    scratch, hence a GPU test.)"""
    import torch
    torch.cuda.init()
    dg = desc(256, 256, 3, B16(32), dgrad=True)
    pw = desc(64, 256, 1, B16(64), dgrad=True, x3=False)
    prev_pw = lib.aod_set_pointwise_mode(-1)
    prev = lib.aod_set_deterministic(0)
    try:
        assert plan(lib, dg, COLSUM) == x3p(9) and plan(lib, pw, COLSUM) == ('PW_STREAM',)
        assert lib.aod_set_deterministic(1) == 0
        assert plan(lib, dg, COLSUM) == igemm(64, 128, stages=3) and plan(lib, pw, COLSUM) == igemm(128, 64, x3=0)
        assert plan(lib, dg, MASK) == x3p(9) and plan(lib, pw, MASK) == ('PW_STREAM',)                     # no column sum: unchanged
    finally:
        lib.aod_set_deterministic(prev)
        lib.aod_set_pointwise_mode(prev_pw)
