"""Shared parts of tests/test_gpu_det_colsum.py: the deterministic mode's ordered column sums (csrc/determinism.hip) against fp64.

The mode.  `deterministic()` enters functional.set_deterministic(True) and leaves it in a finally: the switch is process-wide.

The poison.  Every producer writes its partial rows to the FRONT of one per-device scratch that is never cleared, so a row a launch fails to
write is read back as what the previous launch left there.  `poison(sign)` makes that visible: one aod_l2norm_bwd launch (the bf16 kernel,
whatever the precision mode) of 8 192 rows x 1 024 channels with x = 1 and g = sign * 1e32 leaves 2 048 partial rows of 1 024 floats, each
4 * 1e32 / (32 + eps) = sign * 1.25e31, i.e. POISON_FLOATS = 2 Mi floats from the start of the scratch; the vector its finalize wrote is
read back and must be 2 048 such rows in every column.  (aod_act_bwd on a constant fp32 gradient reaches 2048 / panels * N <= 512 Ki floats
by the launcher's rule in csrc/elementwise.hip: less than the 1 055 * 1 024 of the widest L2Norm case and the 1 001 * 720 of the widest
pad-cast case below.)  The operands are allocated once per process.  Every case lists the scratch floats its launch uses, by the launcher's
own rule; the largest must lie below POISON_FLOATS -- a condition of the tests, asserted there.

The plans.  DET_PLANS[name] is the plan aod_conv2d_plan returns for a COLSUM case of tests/conv_instances_util.py with the mode on, recorded
on an MI355X (`python -m tests.det_colsum_util record`; aod_set_deterministic needs a device): the persistent kernel and the streaming 1x1
kernel decline launches with column sums, everything else keeps its plan."""
import contextlib
import sys

import torch

from tests import conv_instances_util as U
from tests.conv_instances_util import igemm, splitk

COLSUM_CASES = [n for n, c in U.CASES.items() if c.ops & U.COLSUM]

# (trailing comment: the column sums' error with the mode on, relative to their largest, measured on an MI355X by tests/test_gpu_det_colsum.py)
DET_PLANS = {
    'b256_1': igemm(256, 256, 512, 1),                    # cs 2.0e-07
    'b128w8_1': igemm(128, 128, 512, 1),                  # cs 2.7e-07
    'bg256_1': igemm(256, 256, 512, 1, grouped=1),        # cs 5.9e-07
    'bsplit_d': splitk(9, 128),                           # cs 1.3e-07
    'bpw_d': igemm(128, 64),                              # cs 1.9e-07; PW_STREAM by default
    'pw_128x128': igemm(64, 64),                          # cs 1.8e-07; PW_STREAM under aod_set_pointwise_mode(1)
    'x256_1': igemm(256, 256, 512, 1, x3=1),              # cs 2.8e-06
    'xg256_1': igemm(256, 256, 512, 1, x3=1, grouped=1),  # cs 3.6e-06
    'xsplit_d': splitk(18, 128, x3=1),                    # cs 2.4e-06
    'p1402': igemm(64, 64, stages=3, x3=1),               # cs 2.7e-06; X3P (1 tap, pre 2) by default
    'p9800_d': igemm(64, 128, stages=3, x3=1),            # cs 3.9e-06; X3P (9 taps, wide) by default
}


@contextlib.contextmanager
def deterministic():
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd._C import lib
    AF.set_deterministic(True)
    try:
        assert lib.aod_get_deterministic() == 1
        yield
    finally:
        AF.set_deterministic(False)
    assert lib.aod_get_deterministic() == 0


def planned_det(name):
    """U.planned(name) with the mode on"""
    with deterministic():
        return U.planned(name)


# ------------------------------------------------------------------------------------------------------------------------------ poison
POISON_ROWS, POISON_C, POISON_G = 8192, 1024, 1e32
POISON_FLOATS = (POISON_ROWS // 4) * POISON_C          # aod_l2norm_bwd: one partial row of C floats per block of 4 rows
_POISON = {}


def poison(sign):
    """leaves sign * 1.25e31 in the first POISON_FLOATS floats of the scratch (the mode must be on)"""
    from aod_meh_hua_amd._C import call, lib, ptr, stream
    assert sign in (1, -1) and lib.aod_get_deterministic() == 1
    if not _POISON:
        one = torch.ones(POISON_ROWS, POISON_C, dtype=torch.bfloat16, device='cuda')
        _POISON.update(x=one, w=torch.ones(POISON_C, device='cuda'), gx=torch.empty_like(one), gw=torch.empty(POISON_C, device='cuda'))
        _POISON[1] = one * POISON_G
        _POISON[-1] = one * -POISON_G
    p = _POISON
    p['gw'].zero_()
    call('aod_l2norm_bwd', ptr(p['x']), ptr(p['w']), ptr(p[sign]), ptr(p['gx']), ptr(p['gw']), POISON_ROWS, POISON_C, 1e-10, stream())
    got = p['gw'].double() * sign / (POISON_ROWS // 4)          # the mean partial row: every row is the same value
    assert float(got.min()) >= 1e30 and float(got.max()) < 2e31, (float(got.min()), float(got.max()))


# ------------------------------------------------------------------------------------- scratch floats of a launch, by the launchers' rules
def conv_floats(name):
    """launch_conv: members * tiles_m * N; the split-K finalize: ceil(M / 8) * N (csrc/conv.hip)"""
    c = U.CASES[name]
    p = dict(zip(U.PLAN_FIELDS, DET_PLANS[name]))
    M, N = sum(b * h * w for b, h, w in c.segs), c.cin          # (every COLSUM case is a dgrad: its destination is the maps `segs`)
    assert c.dgrad
    if p['kind'] == U.SPLIT_K:
        return (M + 7) // 8 * N
    assert p['kind'] == U.IGEMM
    return max(c.members, 1) * ((M + p['bm'] - 1) // p['bm']) * N


def strips(M, panels):
    """gy of aod_act_bwd / aod_x3_act_bwd: ~2048 / panels strips of at least 64 rows, a multiple of 8"""
    want = max(2048 // panels, 1)
    rpb = max((M + want - 1) // want, 64)
    rpb = (rpb + 7) // 8 * 8
    return (M + rpb - 1) // rpb


def x3_act_floats(M, C):
    """aod_x3_act_bwd over C logical channels: gy * Q * 8 (C % 32 == 0 here: Q * 8 = C)"""
    assert C % 32 == 0
    Q = C // 8
    return strips(M, (Q + 31) // 32) * Q * 8


def act_floats(M, N):
    """aod_act_bwd: two stacked images, 2 * gy * N"""
    return 2 * strips(M, (N + 255) // 256) * N


def _blocks(M, floor):
    rpb = max((M + 1023) // 1024, floor)
    return (M + rpb - 1) // rpb


def x3_pad_cast_form(N):
    Np = (N + 31) // 32 * 32
    return 'v8' if N % 4 == 0 and Np <= 256 else 'scalar'


def x3_pad_cast_floats(M, N):
    """aod_x3_pad_cast_colsum: nb * N, blocks of at least 64 (8-column form) / 16 (scalar form) rows"""
    return _blocks(M, 64 if x3_pad_cast_form(N) == 'v8' else 16) * N


def pad_cast_floats(M, N):
    """aod_pad_cast_colsum: nb * N, blocks of at least 16 rows"""
    return _blocks(M, 16) * N


def l2norm_floats(rows, C):
    """aod_l2norm_bwd / aod_x3_l2norm_bwd: one partial row per block of 4 rows"""
    return (rows + 3) // 4 * C


# ------------------------------------------------------------------------------------------------------------------- the row-kernel cases
ACT_SHAPES = [(1, 64), (63, 320), (4099, 2048), (70001, 64)]          # x3: (M, logical C)
ACT_BF16_SHAPES = [(1, 8), (63, 320), (4099, 2048), (70001, 64)]      # (M, N)
X3_PAD_CAST = [(70001, 9), (70001, 36), (70001, 180), (70001, 256), (70001, 260), (20011, 720)] + [(M, N) for N in (9, 180, 720) for M in (1, 63)]
X3_PAD_CAST_MAP = [(70001, 180), (70001, 9)]
PAD_CAST_N = [9, 36, 180, 720]
PAD_CAST_M = lambda N: (63, 1237) + ((70001,) if N <= 180 else ())
L2NORM = [(3, 38, 37, 512), (3, 38, 37, 1024)]                        # (B, H, W, C); 1024: the largest width on the ordered path


def all_floats():
    """{case: scratch floats} of every launch of the tests"""
    out = {f'conv {n}': conv_floats(n) for n in COLSUM_CASES}
    out.update({f'x3_act_bwd {s}': x3_act_floats(*s) for s in ACT_SHAPES})
    out.update({f'act_bwd {s}': act_floats(*s) for s in ACT_BF16_SHAPES})
    out.update({f'x3_pad_cast_colsum {s}': x3_pad_cast_floats(*s) for s in X3_PAD_CAST + X3_PAD_CAST_MAP})
    out.update({f'pad_cast_colsum {(M, N)}': pad_cast_floats(M, N) for N in PAD_CAST_N for M in PAD_CAST_M(N)})
    out.update({f'l2norm_bwd {s}': l2norm_floats(s[0] * s[1] * s[2], s[3]) for s in L2NORM})
    return out


if __name__ == '__main__':
    if sys.argv[1] == 'record':
        for n in COLSUM_CASES:
            print(f'{n!r}: {planned_det(n)},', flush=True)
    if sys.argv[1] == 'floats':
        for k, v in sorted(all_floats().items(), key=lambda kv: -kv[1])[:8]:
            print(k, v)
        print('poisoned', POISON_FLOATS)
