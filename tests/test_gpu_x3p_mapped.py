"""GPU: the mapped form of the persistent x3 kernel (include/aod_hip.h aod_conv2d_ws_map_order; csrc/conv_x3p.hip SPARSE instance on the
128-column tile, csrc/conv.hip x3p_mapped_launch).  A plain 3 x 3 / pad 1 dgrad, 256 -> 256 channels, with ReLU mask and column sums -- the
retina_reg / MEH tower dgrads of the step -- on the smallest pyramid the kernel accepts: 2 images at 32 x 32, 16 x 16 and 8 x 8, 2 048 + 512 +
128 = 2 688 rows = 21 row tiles of 128 (every segment a whole number of them), 42 items on a grid of 32 workgroups: ten workgroups own two
items, so live counts below, at and above the grid all occur.

The reference of every comparison is the SAME launch under AOD_X3P_MAPPED=0 -- the 256-column tiles under the static walk, the form the
bench step ran before (AOD_X3P_BN=256 and AOD_X3P_MIN_TILES=1 only lift the tile-count thresholds of the small pyramid).  Only where, when
and in how many pieces a row tile runs may change: every dX row keeps its bits, dead tiles are +0 (heads and tails, over a NaN prefill), the
list the device wrote is the exported host rule (aod_conv2d_x3p_item_order) on the map the launch wrote, and the launch log names the form.
Column sums are fp32 atomics, whose last bit no two runs share: they are held to the bound tests/test_gpu_tile_order.py applies to the same
quantity against an fp64 contraction -- the mapped form's largest error (relative to the largest entry) at most 1.5 x the reference launch's,
and that one inside (0, 1e-4)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, SIZES = 2, ((32, 32), (16, 16), (8, 8))
CH = 256
PATTERNS = ('zero', 'ones', 'last_segment', 'straddle', 'random')


@pytest.fixture(autouse=True)
def x3_mode(monkeypatch):
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    AF.set_precision('bf16x3')
    ho.set_deterministic(False)
    monkeypatch.setenv('AOD_SPARSE_BWD', '1')
    monkeypatch.setenv('AOD_X3P_MIN_TILES', '1')
    monkeypatch.setenv('AOD_X3P_BN', '256')
    for k in ('AOD_X3P_MAPPED', 'AOD_X3P', 'AOD_X3P_DGRAD', 'AOD_X3P_MIN_STEPS'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(ho, 'SPLITK', False)
    monkeypatch.setattr(ho, 'X3P_MAP_LOG', [])
    yield
    AF.set_precision(os.environ.get('AOD_CONV_PREC', 'bf16x3'))


def _segs():
    from aod_meh_hua_amd import hipops as ho
    out, r = [], 0
    for h, w in SIZES:
        out.append(ho.Seg(B, h, w, r))
        r += B * h * w
    return out, r


class _Ops:
    """operands of the launch, made once: proper X-layout rows and filter (head + tail of fp32 values)"""

    def __init__(self):
        from aod_meh_hua_amd import hipops as ho
        self.segs, self.M = _segs()
        assert self.M == 2688 and all(s.rows % 128 == 0 for s in self.segs)
        self.nblk, self.ntiles = (self.M + 63) // 64, self.M // 128
        gen = torch.Generator(device='cuda').manual_seed(29)
        rnd = lambda *sh: torch.randn(*sh, device='cuda', generator=gen)
        self.dz = ho.x3_split(rnd(self.M, CH))
        self.w_f32 = rnd(CH, 9, CH) / (9 * CH / 2) ** 0.5                      # [out][tap][in]: the packed layout
        self.w = ho.x3_split(self.w_f32.reshape(CH * 9, CH)).reshape(CH, 9 * ho.xw(CH))
        self.mask = ho.x3_split(rnd(self.M, CH))
        self._ref = {}

    def in_map(self, name):
        m = torch.zeros(self.nblk, dtype=torch.uint8)
        s1, s2 = self.segs[1].row0 // 64, self.segs[2].row0 // 64             # first block of the second and of the last segment
        if name == 'ones':
            m[:] = 1
        elif name == 'last_segment':
            m[s2 + 1] = 1                                                      # the very last block of the pyramid
        elif name == 'straddle':
            m[s1 - 1] = m[s1] = 1                                              # the last block of segment 0 and the first of segment 1
            m[s2 - 1] = m[s2] = 1
        elif name == 'random':
            g = torch.Generator().manual_seed(3)
            m[torch.randperm(self.nblk, generator=g)[:4]] = 1                    # 4 of 42 blocks, ~10 %
        return m.cuda()

    def dz_for(self, in_map):
        """dZ that is zero outside the blocks its map marks"""
        keep = in_map.bool().repeat_interleave(64)[:self.M]
        return self.dz * keep[:, None].to(torch.bfloat16)

    def run(self, in_map, order=None):
        from aod_meh_hua_amd import hipops as ho
        out = torch.full((self.M, ho.xw(CH)), float('nan'), device='cuda', dtype=torch.bfloat16)
        cs = torch.zeros(CH, device='cuda')
        dx, omap = ho.conv2d_dgrad_rows(self.dz_for(in_map), self.segs, self.segs, self.w, CH, 3, 3, 1, 1, 1, mask=self.mask, colsum=cs,
                                        out=out, in_map=in_map, order=order)
        return dx, omap, cs

    def colsum_fp64(self, name, in_map):
        """column sums of (mask > 0) * conv_T(dZ, W) in fp64 from the operands' head + tail values: dX[y, x] = sum_rs dZ[y + 1 - r, x + 1 - s] W[r, s]"""
        from aod_meh_hua_amd import hipops as ho
        if name in self._ref:
            return self._ref[name]
        dz = ho.x3_merge(self.dz_for(in_map)).double().cpu()
        w = ho.x3_merge(self.w.reshape(CH * 9, ho.xw(CH))).double().cpu().reshape(CH, 3, 3, CH)
        k = w.flip(1, 2).permute(0, 3, 1, 2).contiguous()                     # cross-correlation kernel [out][in][i][j] = W[out][2 - i][2 - j][in]
        m = (ho.x3_merge(self.mask) > 0).double().cpu()
        tot = torch.zeros(CH, dtype=torch.float64)
        for s in self.segs:
            v = dz[s.row0:s.row0 + s.rows].reshape(s.B, s.H, s.W, CH).permute(0, 3, 1, 2)
            dx = torch.nn.functional.conv2d(v, k, padding=1).permute(0, 2, 3, 1).reshape(s.rows, CH)
            tot += (dx * m[s.row0:s.row0 + s.rows]).sum(0)
        self._ref[name] = tot
        return tot


@pytest.fixture(scope='module')
def ops():
    from aod_meh_hua_amd import functional as AF
    AF.set_precision('bf16x3')
    return _Ops()


def _host_items(M, omap):
    from aod_meh_hua_amd import _C
    n = (M + 127) // 128 * (CH // 128)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = _C.lib.aod_conv2d_x3p_mapped_grid(M, CH // 128, cus)
    assert grid > 0 and grid % 16 == 0
    keep = omap.cpu().numpy().copy()
    item, block, rnd = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_int32 * n)()
    assert _C.lib.aod_conv2d_x3p_item_order(M, CH // 128, grid, keep.ctypes.data, item, block, rnd) == 0
    return np.array(item[:], np.int64)


def test_the_plan_of_the_reference_launch_is_the_bench_steps(ops):
    """without a map (and with the switch off) the launch is the 256-column 3 x 3 instance of the persistent kernel"""
    from aod_meh_hua_amd import _C
    from aod_meh_hua_amd import hipops as ho
    d = ho.make_desc(ho.xw(CH), CH, 3, 3, 1, 1, 1, ops.segs, ops.segs, True, False, False)
    plan = _C.ConvPlan()
    _C.call('aod_conv2d_plan', C.byref(d), 0, 16 | 128, C.byref(plan))
    assert (plan.kind, plan.taps, plan.wide, plan.lat, plan.pre, plan.grid) == (3, 9, 1, 0, 0, 21)


@pytest.mark.parametrize('pattern', PATTERNS)
def test_mapped_form_keeps_every_bit_and_follows_the_host_rule(ops, pattern, monkeypatch):
    from aod_meh_hua_amd import _C
    from aod_meh_hua_amd import hipops as ho
    in_map = ops.in_map(pattern)
    nitems = ops.ntiles * (CH // 128)
    assert ho.x3p_item_list(ops.M, CH, 'cuda').numel() == nitems
    monkeypatch.setenv('AOD_X3P_MAPPED', '0')
    untouched = torch.full((nitems,), -7, dtype=torch.int32, device='cuda')
    n0 = _C.lib.aod_conv_x3p_count()
    ref, ref_map, ref_cs = ops.run(in_map, untouched)
    assert _C.lib.aod_conv_x3p_count() - n0 == 1
    assert int((untouched != -7).sum()) == 0                                   # the switch: no list is built, the planned launch runs
    monkeypatch.delenv('AOD_X3P_MAPPED')
    order = torch.full((nitems,), -7, dtype=torch.int32, device='cuda')
    got, got_map, got_cs = ops.run(in_map, order)
    assert _C.lib.aod_conv_x3p_count() - n0 == 2
    torch.cuda.synchronize()
    # the launch log: the reference ran as planned, this one in the 128-column mapped form
    assert ho.X3P_MAP_LOG == [((ops.M, ho.xw(CH)), False), ((ops.M, ho.xw(CH)), True)]
    assert torch.equal(got_map, ref_map)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    om = got_map.cpu().numpy()
    assert (om >= in_map.cpu().numpy()).all()                                  # (a dilation)
    live = np.array([om[2 * t:2 * t + 2].any() for t in range(ops.ntiles)])
    assert live.sum() == {'zero': 0, 'ones': ops.ntiles}.get(pattern, live.sum()) and (pattern in ('zero', 'ones') or 0 < live.sum() < ops.ntiles)
    for t, lv in enumerate(live):
        rows = got[128 * t:128 * t + 128]
        if not lv:
            assert int(rows.view(torch.int16).count_nonzero()) == 0, t         # +0 heads and tails over the NaN prefill
        else:
            assert bool(torch.isfinite(rows.float()).all()), t
    assert np.array_equal(order.cpu().numpy().astype(np.int64), _host_items(ops.M, got_map))
    want = ops.colsum_fp64(pattern, in_map)
    if float(want.abs().max()) == 0.0:                                         # (the zero map: nothing was added)
        assert int(got_cs.count_nonzero()) == 0 and int(ref_cs.count_nonzero()) == 0
        return
    err = lambda cs: float((cs.double().cpu() - want).abs().max() / want.abs().max())
    e_list, e_ref = err(got_cs), err(ref_cs)
    print(f'column sums, {pattern}: max error against fp64, mapped form {e_list:.3e}, reference launch {e_ref:.3e}')
    assert 0 < e_ref < 1e-4 and e_list <= 1.5 * e_ref, (e_list, e_ref)


def test_deterministic_mode_keeps_the_planned_launch(ops):
    """ordered column sums expect a partial row from every tile: no map reaches the kernel, no list is built, the form is not taken"""
    from aod_meh_hua_amd import hipops as ho
    ho.set_deterministic(True)
    try:
        in_map = ops.in_map('straddle')
        order = torch.full((ops.ntiles * 2,), -7, dtype=torch.int32, device='cuda')
        got, got_map, _ = ops.run(in_map, order)
        torch.cuda.synchronize()
        assert int((order != -7).sum()) == 0 and ho.X3P_MAP_LOG[-1][1] is False
        assert bool(torch.isfinite(got.float()).all()) and int(got_map.sum()) > 0
    finally:
        ho.set_deterministic(False)
