"""One launch per kernel instance of the forward / dgrad convolution -- csrc/conv.hip CONV_IGEMM_INSTANCES, csrc/conv_x3p.hip X3P_INSTANCES, the
split-K path and the streaming 1x1 kernel --, each reached through hipops by a DEFAULT plan: no AOD_* switch, the product's own thresholds
(>= 512 tiles for the four-wave ladder, >= 192 tiles and >= 24 K-steps for the persistent kernel, whole rounds of the 256 CUs for the big
tiles).  The cases of tests/test_conv_instances_host.py (the plan of every case, no device) and tests/test_gpu_conv_instances.py (the launch
against an fp64 reference).

Row counts sit just above each rule's threshold and are ragged in the last row tile.  Operands come from a CPU generator seeded by the case
name, at unit scale; in the bf16 mode they are bf16-representable values, in the reference-precision mode (x3) the values the kernel is given,
x3_merge(x3_split(t)).  The reference is the documented epilogue (include/aod_hip.h, aod_conv2d) in fp64 on the device:
    v = acc * pre_scale + pre_shift + res;  mask > 0 ? v : 0;  relu;  colsum += sum_m v
with acc a sum over the filter taps of torch.matmul on shifted slices of the zero-padded operand (forward: strided slices of the source;
dgrad: the transpose scatter into the padded destination) -- no convolution library on either side.

The trailing comment of a case is its error measured on an MI355X (`python -m tests.conv_instances_util record`): bf16 mode -- the largest
absolute error and, in brackets, the largest |got - ref| / (atol + rtol |ref|), i.e. the used fraction of the allclose bound; x3 -- the
largest error relative to max|ref|; `cs`: the same for the column sums, relative to their max."""
import ctypes as C
import os
import re
import sys
import zlib
from collections import namedtuple

import torch

from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PW, SPLIT_K, X3P, IGEMM = 1, 2, 3, 4                                       # aod_conv_plan_t.kind
SC, SH, RES, RES_IS_DST, MASK, POST_SCALE, ZRAW, COLSUM, WORKSPACE = (1 << i for i in range(9))      # AOD_CONV_HAS_*: pre_scale, pre_shift, ...
PLAN_FIELDS = ('kind', 'bm', 'bn', 'nt', 'ops', 'stages', 'x3', 'grouped', 'ksplit', 'taps', 'wide', 'pre', 'lat', 'grid')


def igemm(bm, bn, nt=256, ops=2, stages=2, x3=0, grouped=0):
    return (IGEMM, bm, bn, nt, ops, stages, x3, grouped, 0, 0, 0, 0, 0, 0)


def splitk(ksplit, bn, x3=0):
    return (SPLIT_K, 128, bn, 256, 2, 2, x3, 0, ksplit, 0, 0, 0, 0, 0)


def x3p(taps, wide=0, pre=0, lat=0, grid=256):
    return (X3P, 0, 0, 0, 0, 0, 1, 0, 0, taps, wide, pre, lat, grid)


PW_STREAM = (PW,) + (0,) * 13

Case = namedtuple('Case', 'mode cin cout k stride segs dgrad members ops relu out_f32 inplace pw_mode pw_tile plan')
CASES = {}


def _case(name, mode, cin, cout, k, segs, plan, ops=0, *, stride=1, dgrad=False, members=0, relu=False, out_f32=False, inplace=False,
          pw_mode=None, pw_tile=None):
    """forward conv cin -> cout, k x k, pad k // 2 over the source maps `segs` [(B, H, W), ...]; dgrad: the input gradient of that conv (the
    source of the launch is dZ, its destination the maps `segs`).  members: 0 a plain launch, else the members of a grouped one.
    inplace: res == dst.  pw_mode: the case runs under aod_set_pointwise_mode(pw_mode); pw_tile: the streaming kernel's tile form, INFERRED
    from the rule in aod_pw_gemm -- the plan reports only PW_STREAM, so nothing asserts it."""
    assert name not in CASES
    CASES[name] = Case(mode, cin, cout, k, stride, segs, dgrad, members, ops, relu, out_f32, inplace, pw_mode, pw_tile, plan)


B, X = 'bf16', 'bf16x3'
# ---- plain bf16.  IGEMM (bm, bn, nt, ops, stages)
_case('b256_0', B, 128, 512, 3, [(2, 95, 161)], igemm(256, 256, 512, 0))      # 1.6e-02 (0.31)
_case('b256_1', B, 512, 128, 3, [(2, 95, 161)], igemm(256, 256, 512, 1), MASK | COLSUM, dgrad=True)      # 7.8e-03 (0.26), cs 3.0e-07
_case('b128w8_0', B, 128, 384, 3, [(3, 58, 126)], igemm(128, 128, 512, 0))      # 1.6e-02 (0.31)
_case('b128w8_1', B, 384, 128, 3, [(3, 58, 126)], igemm(128, 128, 512, 1), MASK | COLSUM, dgrad=True)      # 7.8e-03 (0.26), cs 3.6e-07
_case('b128_res', B, 128, 512, 1, [(2, 65, 127)], igemm(128, 128), SC | SH | RES, relu=True)      # 2.5e-02 (0.31)
_case('b128x64_ragged_f32', B, 64, 180, 3, [(3, 58, 126)], igemm(128, 64), RES, out_f32=True)      # 1.7e-06 (0.01)
_case('b128x64_ragged_bf16', B, 64, 180, 3, [(3, 58, 126)], igemm(128, 64), RES)      # 1.6e-02 (0.31); N % 8 != 0: the epilogue without vector stores
_case('b128x64_narrow', B, 64, 40, 3, [(4, 129, 127)], igemm(128, 64), SC)      # 1.6e-02 (0.31); pre_scale also keeps it off aod_halo_conv3x3
_case('b64x128_st2', B, 128, 256, 1, [(4, 65, 63)], igemm(64, 128), RES)      # 1.6e-02 (0.31); K = 128 < 256: two stages
_case('b64x128_st3', B, 256, 256, 3, [(4, 65, 63)], igemm(64, 128, stages=3), RES)      # 1.6e-02 (0.31)
_case('b64x64_st2', B, 8, 64, 5, [(1, 40, 41)], igemm(64, 64), SH, stride=2)      # 7.8e-03 (0.26); K = 200: a K tail, two stages
_case('b64x64_st3', B, 8, 64, 7, [(1, 40, 41)], igemm(64, 64, stages=3), SH, stride=2)      # 9.8e-03 (0.26); K = 392
_case('bg256_0', B, 256, 256, 3, [(8, 64, 63)], igemm(256, 256, 512, 0, grouped=1), SH, members=2, relu=True)      # 1.6e-02 (0.31)
_case('bg256_1', B, 256, 256, 3, [(8, 64, 63)], igemm(256, 256, 512, 1, grouped=1), MASK | COLSUM, members=2, dgrad=True)      # 1.6e-02 (0.31), cs 5.8e-07
_case('bg128_0', B, 256, 256, 3, [(2, 21, 19)], igemm(128, 128, 512, 0, grouped=1), members=2)      # 1.5e-02 (0.30)
_case('bg128_1', B, 256, 256, 3, [(2, 21, 19)], igemm(128, 128, 512, 1, grouped=1), MASK, members=2, dgrad=True)      # 1.4e-02 (0.28)
# split-K (the workspace as hipops._splitk_ws hands it; C = 512 / 2048 > 256 keeps the 3x3 launches off aod_halo_conv3x3)
_case('bsplit128', B, 512, 512, 3, [(2, 16, 16)], splitk(4, 128), SH)      # 1.3e-02 (0.26)
_case('bsplit64', B, 512, 64, 3, [(2, 16, 16)], splitk(9, 64), SH)      # 7.8e-03 (0.26)
_case('bsplitP6', B, 2048, 256, 3, [(2, 15, 17)], splitk(28, 128), SH, stride=2)      # 1.2e-02 (0.26)
# ... with column sums (conv_splitk_finalize_kernel's): K = 4608, 78 rows = 9 blocks of 8 and one of 6, 320 columns = a second, partly filled panel
_case('bsplit_d', B, 320, 512, 3, [(2, 6, 5), (2, 3, 3)], splitk(9, 128), MASK | COLSUM, dgrad=True)      # 1.6e-02 (0.28), cs 1.4e-07
# the streaming 1x1 kernel by its own heuristic (64 columns over >= 65 536 rows).  Its tile form follows from aod_pw_gemm: at 66 049 rows the
# 517 tiles of 128 rows waste more of their last round than the 1 033 of 64 rows -> <64, 64>; at exactly 65 536 rows -> <128, 64>
_case('bpw', B, 256, 64, 1, [(1, 257, 257)], PW_STREAM, pw_tile=(64, 64))      # 1.6e-02 (0.31)
_case('bpw_d', B, 64, 256, 1, [(1, 257, 257)], PW_STREAM, MASK | COLSUM, dgrad=True, pw_tile=(64, 64))      # 3.0e-02 (0.33), cs 3.3e-07
_case('bpw_even', B, 256, 64, 1, [(1, 256, 256)], PW_STREAM, SC | SH | RES, relu=True, pw_tile=(128, 64))      # 1.8e-02 (0.31)
# ... and its other tile forms under aod_set_pointwise_mode(1), which no default plan reaches below 65 536 rows or beyond 64 columns
_case('pw_64x128', B, 128, 128, 1, [(4, 65, 63)], PW_STREAM, SC | SH | RES, relu=True, pw_mode=1, pw_tile=(64, 128))      # 1.6e-02 (0.31); 128 big tiles
_case('pw_128x128', B, 128, 128, 1, [(3, 100, 109)], PW_STREAM, MASK | COLSUM, dgrad=True, pw_mode=1, pw_tile=(128, 128))      # 1.6e-02 (0.30), cs 3.4e-07; 256 tiles
_case('pw_128x64', B, 128, 64, 1, [(3, 100, 109)], PW_STREAM, SH, pw_mode=1, pw_tile=(128, 64))      # 1.6e-02 (0.31)

# ---- reference precision (x3)
_case('x256_0', X, 1024, 512, 1, [(2, 95, 161)], igemm(256, 256, 512, 0, x3=1), SC | SH, relu=True)      # 6.2e-06
_case('x256_1', X, 512, 128, 3, [(2, 95, 161)], igemm(256, 256, 512, 1, x3=1), MASK | COLSUM, dgrad=True)      # 7.5e-06, cs 2.9e-06
_case('x192', X, 256, 180, 3, [(2, 121, 191)], igemm(192, 192, 512, 0, x3=1), SH, out_f32=True)      # 2.6e-06
_case('x128_res', X, 128, 512, 1, [(2, 65, 127)], igemm(128, 128, x3=1), SC | SH | RES, relu=True)      # 4.9e-06
_case('x128x64', X, 128, 64, 1, [(4, 129, 127)], igemm(128, 64, x3=1), SH)      # 7.1e-06
_case('x128x64_ragged', X, 64, 192, 1, [(3, 58, 126)], igemm(128, 64, x3=1), SH)      # 6.3e-06
_case('x64x128_a', X, 64, 192, 1, [(4, 65, 63)], igemm(64, 128, stages=3, x3=1))      # 6.4e-06
_case('x64x128_b', X, 128, 256, 1, [(4, 65, 63)], igemm(64, 128, stages=3, x3=1), RES)      # 5.3e-06
_case('x64x64', X, 64, 64, 3, [(2, 17, 19)], igemm(64, 64, stages=3, x3=1), SC | SH, relu=True)      # 5.8e-06
_case('xg256_0', X, 256, 256, 3, [(2, 21, 19)], igemm(256, 256, 512, 0, x3=1, grouped=1), SH, members=2, relu=True)      # 7.4e-06
_case('xg256_1', X, 256, 256, 3, [(2, 21, 19)], igemm(256, 256, 512, 1, x3=1, grouped=1), MASK | COLSUM, members=2, dgrad=True)      # 7.6e-06, cs 3.6e-06
_case('xsplit128', X, 512, 512, 3, [(2, 16, 16)], splitk(4, 128, x3=1), SH)      # 5.7e-06
_case('xsplit64', X, 512, 64, 3, [(2, 16, 16)], splitk(16, 64, x3=1), SH)      # 6.3e-06
_case('xsplit_d', X, 320, 512, 3, [(2, 6, 5), (2, 3, 3)], splitk(18, 128, x3=1), MASK | COLSUM, dgrad=True)      # 4.6e-06, cs 2.4e-06
# the persistent kernel: X3P (taps, wide, pre, lat, grid)
_case('p1400', X, 768, 384, 1, [(2, 64, 65)], x3p(1, grid=195), SC | SH)      # 5.8e-06
_case('p1401', X, 1024, 256, 1, [(4, 64, 63)], x3p(1, pre=1, grid=252), SC | SH | RES, relu=True)      # 5.4e-06
_case('p1402', X, 256, 768, 1, [(3, 64, 65)], x3p(1, pre=2, grid=196), MASK | COLSUM, dgrad=True)      # 6.9e-06, cs 2.8e-06
_case('p1800', X, 512, 256, 1, [(6, 64, 65)], x3p(1, wide=1, grid=195), SC | SH)      # 5.7e-06
_case('p9400', X, 128, 128, 3, [(6, 64, 65)], x3p(9, grid=195), SC | SH, relu=True)      # 4.8e-06
_case('p9400_s2', X, 256, 128, 3, [(6, 128, 130)], x3p(9, grid=195), SC | SH, stride=2, relu=True)      # 5.5e-06
_case('p9400_segs', X, 256, 256, 3, [(12, 32, 32), (12, 16, 16), (12, 7, 9)], x3p(9, grid=252), SH, relu=True)      # 6.6e-06
_case('p9800', X, 256, 256, 3, [(6, 64, 65)], x3p(9, wide=1, grid=195), RES)      # 5.2e-06
_case('p9800_d', X, 256, 256, 3, [(6, 64, 65)], x3p(9, wide=1, grid=195), MASK | COLSUM, dgrad=True)      # 7.2e-06, cs 3.9e-06
_case('p4410', X, 128, 256, 3, [(6, 62, 66)], x3p(4, lat=1, grid=192), stride=2, dgrad=True)      # 6.7e-06
_case('p4810', X, 256, 256, 3, [(6, 62, 66)], x3p(4, wide=1, lat=1, grid=192), stride=2, dgrad=True)      # 5.9e-06
_case('p1420', X, 384, 1024, 1, [(2, 128, 130)], x3p(1, lat=2, grid=195), RES, stride=2, dgrad=True, inplace=True)      # 6.3e-06
_case('p1820', X, 512, 1024, 1, [(3, 128, 130)], x3p(1, wide=1, lat=2, grid=196), RES, stride=2, dgrad=True, inplace=True)      # 6.3e-06


def dispatch_variables_set():
    """the AOD_* variables in the environment that a forward / dgrad launch or its hipops wrapper reads (the knob tables of csrc/conv_params.h
    without the weight gradient's, AOD_PW_STREAM, and the three switches of hipops)"""
    names = {'AOD_PW_STREAM', 'AOD_SPLITK', 'AOD_HALO_CONV', 'AOD_HALO_X3'}
    with open(os.path.join(ROOT, 'aod_meh_hua_amd', 'csrc', 'conv_params.h')) as f:
        names |= {n for n in re.findall(r'"(AOD_[A-Z0-9_]+)"', f.read()) if not n.startswith('AOD_WGRAD_')}
    assert len(names) > 20, 'the knob tables of csrc/conv_params.h were not found'
    return sorted(n for n in names if n in os.environ)


def instance_lists():
    """the two X-macro lists that are the launch switch, read from the sources: tuples of ints (true / false -> 1 / 0)"""
    out = []
    for path, macro in (('conv.hip', 'CONV_IGEMM_INSTANCES'), ('conv_x3p.hip', 'X3P_INSTANCES')):
        with open(os.path.join(ROOT, 'aod_meh_hua_amd', 'csrc', path)) as f:
            m = re.search(r'#define\s+' + macro + r'\(X\)((?:[^\n]*\\\n)*[^\n]*)\n', f.read())
        assert m, f'{macro} not found in csrc/{path}'
        word = {'true': 1, 'false': 0}
        tuples = [tuple(word[v] if v in word else int(v) for v in re.split(r'\s*,\s*', t.strip())) for t in re.findall(r'\bX\(([^()]*)\)', m.group(1))]
        assert tuples, f'{macro}: no X(...) tuple parsed'
        out.append(tuples)
    return out


def instance_of(plan):
    """the tuple of the X-macro list a plan names: IGEMM / SPLIT_K (BM, BN, NT, OPS, GROUPED, ST, X3), X3P (TAPS, NBW, LAT, PRE), else None"""
    p = dict(zip(PLAN_FIELDS, plan))
    if p['kind'] in (IGEMM, SPLIT_K):
        return ('igemm', (p['bm'], p['bn'], p['nt'], p['ops'], p['grouped'], p['stages'], p['x3']))
    if p['kind'] == X3P:
        return ('x3p', (p['taps'], 8 if p['wide'] else 4, p['lat'], p['pre']))
    return None


class _mode:
    """the case's precision mode (hipops.X3 through functional.set_precision) and pointwise mode, restored on exit"""

    def __init__(self, c):
        self.c = c

    def __enter__(self):
        from aod_meh_hua_amd import functional as AF
        from aod_meh_hua_amd._C import lib
        self.prec = AF.get_precision()
        AF.set_precision(self.c.mode)
        self.pw = lib.aod_set_pointwise_mode(self.c.pw_mode) if self.c.pw_mode is not None else None

    def __exit__(self, *exc):
        from aod_meh_hua_amd import functional as AF
        from aod_meh_hua_amd._C import lib
        if self.pw is not None:
            lib.aod_set_pointwise_mode(self.pw)
        AF.set_precision(self.prec)
        return False


def geometry(c):
    """-> (source Segs, destination Segs, filter geometry) of the LAUNCH, in hipops' terms"""
    from aod_meh_hua_amd import hipops as ho
    x_segs, r = [], 0
    for (b, h, w) in c.segs:
        x_segs.append(ho.Seg(b, h, w, r))
        r += b * h * w
    z_segs = ho.out_segs(x_segs, c.k, c.k, c.stride, c.k // 2, 1)
    return (z_segs, x_segs) if c.dgrad else (x_segs, z_segs)


def descriptor(c):
    """the descriptor as hipops.conv2d_rows / conv2d_dgrad_rows / their grouped forms build it (hipops.make_desc with the widths of
    hipops.width); the caller holds the case's mode"""
    from aod_meh_hua_amd import hipops as ho
    assert ho.X3 == (c.mode == X)
    src, dst = geometry(c)
    if c.dgrad:
        return ho.make_desc(ho.width(c.cout), c.cin, c.k, c.k, c.stride, c.k // 2, 1, src, dst, True, False, c.out_f32)
    return ho.make_desc(ho.width(c.cin), c.cout, c.k, c.k, c.stride, c.k // 2, 1, src, dst, False, c.relu, c.out_f32)


def general_path(c, d):
    """whether hipops hands this launch to aod_conv2d_ws / aod_conv2d_grouped: neither halo route takes it, and split-K workspaces are on"""
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd._C import lib
    if not ho.SPLITK or not ho.HALO_CONV or ho.HALO_ALL:
        return False
    if c.members or c.dgrad or c.k != 3:          # (default routing: the halo kernels take forward 3x3 launches only)
        return True
    if c.mode == X:
        return not (c.out_f32 and c.cout <= 48 and not c.ops & (SC | RES | MASK) and lib.aod_halo_conv3x3_x3_applies(C.byref(d)))
    return bool(c.ops & (SC | RES | MASK)) or c.cout > 64 or not lib.aod_halo_conv3x3_applies(C.byref(d))


def planned(name):
    """the full plan (PLAN_FIELDS) of the case's launch: its descriptor, the flags of its operands, AOD_CONV_HAS_WORKSPACE exactly when
    hipops would hand a workspace"""
    from aod_meh_hua_amd._C import ConvPlan, lib
    c = CASES[name]
    with _mode(c):
        d = descriptor(c)
        assert general_path(c, d), f'{name}: hipops routes this launch past aod_conv2d_ws'
        flags = c.ops | (RES_IS_DST if c.inplace else 0)
        if not c.members and lib.aod_conv2d_ws_bytes(C.byref(d)):
            flags |= WORKSPACE
        p = ConvPlan()
        rc = lib.aod_conv2d_plan(C.byref(d), c.members, flags, C.byref(p))
        assert rc == 0, (name, lib.aod_last_error())
    return tuple(getattr(p, f) for f in PLAN_FIELDS)


# ---------------------------------------------------------------------------------------------------------- operands, launch, reference
SENTINEL = 0x5a5a          # per 16-bit word of the destination: as bf16 / fp32 ~ 1.5e16, so an element the launch skipped fails the comparison too
GUARD = 64


def _rows(t, mode):
    """CPU fp32 [M, C] -> (the rows the kernel is given, their values in fp64), on the device"""
    from aod_meh_hua_amd import hipops as ho
    if mode == X:
        xr = ho.x3_split(t.cuda())
        return xr, ho.x3_merge(xr, t.shape[1]).double()
    b = t.bfloat16().cuda()
    return b, b.double()


def _filter(w, c):
    """CPU fp32 [O, I, k, k] -> (the packed filter of the launch, its values as [k, k, source channels, destination channels] fp64)"""
    from aod_meh_hua_amd import hipops as ho
    O, I, k = c.cout, c.cin, c.k
    lead = (1, 2, 3, 0) if c.dgrad else (0, 2, 3, 1)          # dgrad packing [I][R][S][O], forward [O][R][S][I]
    if c.mode == X:
        m = w.permute(*lead).reshape(-1, O if c.dgrad else I).contiguous()
        packed, vals = _rows(m, X)
        packed, vals = packed.view(m.shape[0] // (k * k), k, k, -1), vals.view(m.shape[0] // (k * k), k, k, -1)
    else:
        wq = w.bfloat16().float().cuda()
        packed = ho.pack_weight_dgrad(wq, O) if c.dgrad else ho.pack_weight_fwd(wq, I)
        vals = wq.permute(*lead).double()
    return packed, vals.permute(1, 2, 3, 0).contiguous()


def _acc(c, src, wt):
    """the raw sums in fp64: src [rows of the launch's source, its channels], wt [k, k, source channels, destination channels] -> [M, N]"""
    k, st, pad = c.k, c.stride, c.k // 2
    out, r0 = [], 0
    for (b, h, w) in c.segs:
        oh, ow = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
        span = lambda t, n: slice(t, t + (n - 1) * st + 1, st)
        if c.dgrad:
            dz = src[r0:r0 + b * oh * ow]
            r0 += b * oh * ow
            dxp = torch.zeros(b, h + 2 * pad, w + 2 * pad, wt.shape[3], dtype=torch.float64, device=src.device)
            for r in range(k):
                for s in range(k):
                    dxp[:, span(r, oh), span(s, ow)] += torch.matmul(dz, wt[r, s]).view(b, oh, ow, -1)
            out.append(dxp[:, pad:pad + h, pad:pad + w].reshape(b * h * w, -1))
        else:
            x = src[r0:r0 + b * h * w].view(b, h, w, -1)
            r0 += b * h * w
            xp = torch.zeros(b, h + 2 * pad, w + 2 * pad, x.shape[3], dtype=torch.float64, device=src.device)
            xp[:, pad:pad + h, pad:pad + w] = x
            acc = torch.zeros(b * oh * ow, wt.shape[3], dtype=torch.float64, device=src.device)
            for r in range(k):
                for s in range(k):
                    acc += torch.matmul(xp[:, span(r, oh), span(s, ow)].reshape(b * oh * ow, -1), wt[r, s])
            out.append(acc)
    return torch.cat(out)


Member = namedtuple('Member', 'got ref full before cs_got cs_ref')


def _dims(c):
    from aod_meh_hua_amd import hipops as ho
    src_segs, dst_segs = geometry(c)
    N = c.cin if c.dgrad else c.cout
    return src_segs, dst_segs, sum(s.rows for s in src_segs), sum(s.rows for s in dst_segs), N, (N if (c.out_f32 or c.mode == B) else ho.xw(N))


def operands(name):
    """the operands of the case, one dict per group member (a plain launch: one), with the fp64 reference of the destination rows (`ref`) and of
    the column sums (`cs_ref`, from their start `cs0`) -- built once; launch() can run them any number of times"""
    c = CASES[name]
    with _mode(c):
        src_segs, dst_segs, rows_src, M, N, wide = _dims(c)
        c_src = c.cout if c.dgrad else c.cin
        k = c.k
        ops = []
        for g in range(max(c.members, 1)):          # every member its own operands and filter
            gen = synth.gen(zlib.crc32(name.encode()) % 100000 + g)
            o = {}
            o['src'], src64 = _rows(torch.randn(rows_src, c_src, generator=gen), c.mode)
            o['w'], wt = _filter(torch.randn(c.cout, c.cin, k, k, generator=gen) / (c.cin * k * k) ** 0.5, c)
            o['sc'] = (torch.rand(N, generator=gen) + 0.5).cuda() if c.ops & SC else None
            o['sh'] = (0.1 * torch.randn(N, generator=gen)).cuda() if c.ops & SH else None
            o['res'], res64 = _rows(torch.randn(M, N, generator=gen), c.mode) if c.ops & RES else (None, None)
            o['mask'], mask64 = _rows(torch.randn(M, N, generator=gen), c.mode) if c.ops & MASK else (None, None)
            o['cs0'] = cs0 = torch.randn(N, generator=gen).cuda() if c.ops & COLSUM else None          # colsum is +=: it starts non-zero
            v = _acc(c, src64, wt)
            if o['sc'] is not None:
                v = v * o['sc'].double()
            if o['sh'] is not None:
                v = v + o['sh'].double()
            if res64 is not None:
                v = v + res64
            if mask64 is not None:
                v = torch.where(mask64 > 0, v, torch.zeros_like(v))
            if c.relu:
                v = v.clamp_min(0)
            o['ref'], o['cs_ref'] = v, (cs0.double() + v.sum(0) if cs0 is not None else None)
            ops.append(o)
        return ops


def launch(name, members):
    """launches the case through hipops in its mode on the operands() `members`, into a fresh destination and fresh column sums -> one Member
    each: got / ref fp64 [M, N], `full` the destination buffer with its guard rows, `before` what an in-place destination held, the column
    sums fp32 and their fp64 reference"""
    from aod_meh_hua_amd import hipops as ho
    c = CASES[name]
    with _mode(c):
        src_segs, dst_segs, rows_src, M, N, wide = _dims(c)
        f32 = c.out_f32
        ops = []
        for o in members:
            o = dict(o)
            o['cs'] = o['cs0'].clone() if o['cs0'] is not None else None
            o['full'] = torch.full((M + GUARD, wide * (2 if f32 else 1)), SENTINEL, dtype=torch.int16, device='cuda').view(
                torch.float32 if f32 else torch.bfloat16)
            o['out'] = o['full'][:M]
            if c.inplace:
                o['out'].copy_(o['res'])
                o['res'], o['before'] = o['out'], o['out'].clone()
            ops.append(o)
        col = lambda key: [o[key] for o in ops]
        geo = (c.k, c.k, c.stride, c.k // 2, 1)
        if c.members and c.dgrad:
            ho.conv2d_dgrad_rows_grouped(col('src'), src_segs, dst_segs, col('w'), N, *geo, masks=col('mask') if c.ops & MASK else None,
                                         colsums=col('cs') if c.ops & COLSUM else None, outs=col('out'))
        elif c.members:
            assert not c.ops & ~SH
            ho.conv2d_rows_grouped(col('src'), src_segs, col('w'), N, *geo, pre_shifts=col('sh') if c.ops & SH else None, relu=c.relu, outs=col('out'))
        elif c.dgrad:
            o = ops[0]
            assert not c.ops & (SC | SH) and not c.relu
            ho.conv2d_dgrad_rows(o['src'], src_segs, dst_segs, o['w'], N, *geo, res=o['res'], mask=o['mask'], out=o['out'], colsum=o['cs'], out_f32=f32)
        else:
            o = ops[0]
            assert not c.ops & COLSUM
            ho.conv2d_rows(o['src'], src_segs, o['w'], N, *geo, pre_scale=o['sc'], pre_shift=o['sh'], res=o['res'], mask=o['mask'], relu=c.relu,
                           out_f32=f32, out=o['out'])
        torch.cuda.synchronize()
        res = []
        for o in ops:
            got = ho.x3_merge(o['out'], N).double() if (c.mode == X and not f32) else o['out'].double()
            res.append(Member(got, o['ref'], o['full'], o.get('before'), o['cs'], o['cs_ref']))
        return res


def run(name):
    """operands() and one launch() of the case"""
    return launch(name, operands(name))


def bounds(c):
    """(rtol, atol) of the allclose of a bf16-mode case, None for an x3 case (1e-4 of max|ref|); the bound of the column sums relative to their max"""
    if c.mode == X:
        return None, 1e-4
    return ((1e-4, 1e-4) if c.out_f32 else (1e-2, 1e-2)), 5e-3


def errors(c, m):
    """-> (the figure the bound is on: x3 max|got - ref| / max|ref|, bf16 max |got - ref| / (atol + rtol |ref|) with 1 the bound; max abs error;
    flat index of the worst element; column-sum error relative to max|ref| or None)"""
    tol, _ = bounds(c)
    diff = (m.got - m.ref).abs()
    diff = torch.where(torch.isfinite(diff), diff, torch.full_like(diff, float('inf')))
    rel = diff / float(m.ref.abs().max()) if tol is None else diff / (tol[1] + tol[0] * m.ref.abs())
    worst = int(rel.argmax())
    cs = float((m.cs_got.double() - m.cs_ref).abs().max() / m.cs_ref.abs().max()) if m.cs_ref is not None else None
    return float(rel.reshape(-1)[worst]), float(diff.max()), worst, cs


def record(names):
    for name in names:
        c = CASES[name]
        es = [errors(c, m) for m in run(name)]
        fig, mabs, cs = max(e[0] for e in es), max(e[1] for e in es), [e[3] for e in es if e[3] is not None]
        txt = f'{fig:.1e}' if c.mode == X else f'{mabs:.1e} ({fig:.2f})'
        print(f'{name}: {txt}' + (f', cs {max(cs):.1e}' if cs else ''), flush=True)


if __name__ == '__main__':
    if sys.argv[1] == 'record':
        record(sys.argv[2:] or list(CASES))
