"""GPU: the sparse backward of the box-regression and MEH towers (reference-precision mode).  Their head gradients -- sign(diff) * bbox_weights * g
(csrc/losses.hip edl_l1_bwd_kernel) and g * 2 w^2 (lam - loss) (meh_bwd_kernel, loss_single_L of Lambda_L2.py) -- are exactly zero at every
anchor that is not positive, so a ROW-ACTIVITY MAP (one byte per 64 gradient rows, include/aod_hip.h aod_conv2d_ws_map) travels down the tower
and the dgrad kernels skip the tiles that only zero rows can reach.  Checked here: the producer's map, and for each of the three dgrad paths of
the bench step -- the paired 256 x 256 launch (cls member dense, reg member mapped), conv_x3p_kernel<9, 8> and the 128 x 128 conv_igemm_kernel
of retina_L's dgrad -- that skipped tiles store zeros, that every other bit is the dense launch's, and that the outgoing map lies between the
exact one-pixel dilation and the linear-range rule; then one whole training iteration with the switch on and off, eagerly and as a graph.

"Equal" is torch.equal against the same call without a map on the same operands (-0 equals +0)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PYRAMID = (2, ((128, 128), (64, 64), (32, 32)))      # 43 008 rows = 168 tiles of 256: the smallest pyramid that still plans the bench's kernels
RAGGED = (2, ((32, 32), (9, 13)))                    # 2 282 rows = 35 blocks + 42 rows: a ragged last block inside a partial last tile
CIN = 256


@pytest.fixture(autouse=True)
def x3_mode(monkeypatch):
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    AF.set_precision('bf16x3')
    monkeypatch.setenv('AOD_SPARSE_BWD', '1')
    monkeypatch.setattr(ho, 'SPLITK', False)
    yield
    AF.set_precision(os.environ.get('AOD_CONV_PREC', 'bf16x3'))


def _segs(B, sizes):
    from aod_meh_hua_amd import hipops as ho
    out, r = [], 0
    for h, w in sizes:
        out.append(ho.Seg(B, h, w, r))
        r += B * h * w
    return out, r


# ------------------------------------------------------------------------------------------------ numpy models of the maps
def _block_map(active_rows, M):
    m = np.zeros((M + 63) // 64, np.uint8)
    m[np.asarray(sorted(active_rows), np.int64) // 64] = 1
    return m


def _exact_dilation(rows, B, sizes):
    """rows (GEMM row indices) -> the rows a 3x3 / pad-1 dgrad can write a non-zero into: the 8-neighbourhood inside the same image"""
    out = set()
    r0 = 0
    for h, w in sizes:
        n = B * h * w
        for r in rows:
            if r0 <= r < r0 + n:
                b, rem = divmod(r - r0, h * w)
                y, x = divmod(rem, w)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if 0 <= y + dy < h and 0 <= x + dx < w:
                            out.add(r0 + b * h * w + (y + dy) * w + x + dx)
        r0 += n
    return out


def _linear_rule(in_map, B, sizes):
    """the loosest map the launch may write: block b is active when an input block overlaps rows [first - W - 1, last + W + 1] of the same segment"""
    M = sum(B * h * w for h, w in sizes)
    out = np.zeros_like(in_map)
    for b in range(len(in_map)):
        lo, hi = 64 * b, min(64 * b + 63, M - 1)
        r0 = 0
        for h, w in sizes:
            n = B * h * w
            a, z = max(lo, r0), min(hi, r0 + n - 1)
            if a <= z:
                a, z = max(a - w - 1, r0), min(z + w + 1, r0 + n - 1)
                if in_map[a // 64:z // 64 + 1].any():
                    out[b] = 1
            r0 += n
    return out


# ------------------------------------------------------------------------------------------------ producer
@pytest.mark.parametrize('N,relu', [(36, False), (9, True)])          # retina_reg (16-B loads) and retina_L (scalar form, fused ReLU mask)
def test_producer_writes_the_map_and_leaves_dz_and_the_column_sums_alone(N, relu):
    from aod_meh_hua_amd import hipops as ho
    M = 64 * 37 + 21                                                   # ragged tail block
    g = torch.zeros(M, N, device='cuda')
    gen = torch.Generator(device='cuda').manual_seed(3)
    plant = {64 * 5: 0, 64 * 5 + 63: N - 1, 64 * 9 + 63: 1, 64 * 10: 2, 64 * 37 + 20: 3, 64 * 20 + 7: N // 2}     # first / last row of a block, tail
    for r, c in plant.items():
        g[r, c] = float(torch.randn((), device='cuda', generator=gen)) + 2.0
    g[64 * 30:64 * 31] = -0.0                                          # a block of negative zeros only: inactive
    g[64 * 33 + 11, N - 1] = float('nan')                             # a NaN is something
    ro = torch.ones(M, N, device='cuda') if relu else None
    if relu:
        ro[64 * 20 + 7] = 0.0                                          # retina_L's ReLU was off there: that gradient is masked away, the block stays inactive
    dz0, cs0 = ho.pad_cast_colsum(g, ho.xw(N), ro)
    cs0 = cs0.clone()
    dz1, cs1, rmap = ho.pad_cast_colsum(g, ho.xw(N), ro, want_map=True)
    torch.cuda.synchronize()
    vals = g.cpu().numpy().copy()
    if relu:
        vals[64 * 20 + 7] = 0.0
    want = np.zeros((M + 63) // 64, np.uint8)
    for b in range(len(want)):
        want[b] = 0 if (vals[64 * b:64 * b + 64] == 0).all() else 1
    assert want.sum() == (5 if relu else 6) and want[30] == 0 and want[33] == 1 and want[37] == 1 and want[20] == (0 if relu else 1)
    assert np.array_equal(rmap.cpu().numpy(), want)
    assert torch.equal(dz0.view(torch.int16), dz1.view(torch.int16))
    a, b_ = cs0.cpu().numpy()[:N], cs1.cpu().numpy()[:N]
    assert np.array_equal(a, b_, equal_nan=True)                       # (at most two addends per column here: the atomics' order cannot show)


# ------------------------------------------------------------------------------------------------ dgrad paths
class _Dgrad:
    """one of the three dgrad launches on a pyramid, with its operands; run(in_map) -> (dX of the mapped member, out map, column sums)"""

    def __init__(self, path, pyramid, monkeypatch):
        from aod_meh_hua_amd import _C
        from aod_meh_hua_amd import hipops as ho
        self.path, (self.B, self.sizes) = path, pyramid
        self.segs, self.M = _segs(self.B, self.sizes)
        self.npad = ho.xw(9) if path == 'igemm128' else ho.xw(256)          # physical width of dZ: retina_L's 9 channels, else a tower's 256
        gen = torch.Generator(device='cuda').manual_seed(17)
        self.gen = gen
        rnd = lambda *sh: torch.randn(*sh, device='cuda', generator=gen)
        self.w = [(rnd(CIN, 9 * self.npad) / (9 * self.npad / 2) ** 0.5).bfloat16() for _ in range(2)]
        self.mask = [rnd(self.M, ho.xw(CIN)).bfloat16() for _ in range(2)]
        self.dz_dense = rnd(self.M, self.npad).bfloat16()                    # the unmapped (cls) member's gradient
        if pyramid is RAGGED:                                                # (tile-count thresholds only: the kernel instance stays the bench's)
            monkeypatch.setenv('AOD_X3P_MIN_TILES', '1')
            monkeypatch.setenv('AOD_X3P_BN', '256')
        # the plan of this launch must name the kernel the bench step runs it on
        d = ho.make_desc(self.npad, CIN, 3, 3, 1, 1, 1, self.segs, self.segs, True, False, False)
        plan = _C.ConvPlan()
        _C.call('aod_conv2d_plan', C.byref(d), 2 if path == 'pair' else 0, 16 | 128, C.byref(plan))
        self.plan = (plan.kind, plan.bm, plan.bn, plan.nt, plan.taps, plan.wide, plan.lat, plan.pre, plan.grouped)
        want = {'pair': (4, 256, 256, 512, 0, 0, 0, 0, 1), 'x3p': (3, 0, 0, 0, 9, 1, 0, 0, 0), 'igemm128': (4, 128, 128, 256, 0, 0, 0, 0, 0)}[path]
        if pyramid is PYRAMID and self.plan != want:
            pytest.skip(f'{path}: planned {self.plan}, the bench step runs {want}')
        if pyramid is RAGGED:                                                # (the small pyramid may take a smaller tile of the same kernel template)
            assert self.plan[0] == want[0] and (path != 'x3p' or self.plan[4:8] == want[4:8]), self.plan

    def run(self, dz, in_map, cs_init=None):
        from aod_meh_hua_amd import hipops as ho
        nan = lambda: torch.full((self.M, ho.xw(CIN)), float('nan'), device='cuda', dtype=torch.bfloat16)
        cs = [(cs_init.clone() if cs_init is not None else torch.zeros(CIN, device='cuda')) for _ in range(2)]
        if self.path == 'pair':
            outs = [nan(), nan()]
            r = ho.conv2d_dgrad_rows_grouped([self.dz_dense, dz], self.segs, self.segs, self.w, CIN, 3, 3, 1, 1, 1, masks=self.mask, colsums=cs,
                                             in_maps=[None, in_map] if in_map is not None else None, outs=outs)
            omap = r[1][1] if in_map is not None else None
            return outs[1], omap, cs[1], outs[0], cs[0]
        out = nan()
        r = ho.conv2d_dgrad_rows(dz, self.segs, self.segs, self.w[1], CIN, 3, 3, 1, 1, 1, mask=self.mask[1], colsum=cs[1], out=out, in_map=in_map)
        return out, (r[1] if in_map is not None else None), cs[1], None, None


def _planted(dg):
    """dZ that is zero but for single pixels: an image corner, a segment's first and last row, both sides of a block boundary"""
    B, sizes, M = dg.B, dg.sizes, dg.M
    h0, w0 = sizes[0]
    n0 = B * h0 * w0
    rows = [0, h0 * w0 - 1, n0 - 1, n0, M - 1]                 # corners of images, last row of segment 0, first row of segment 1, last row of all
    mid = (n0 // 2 // 64) * 64 + 64 * 3                        # a block boundary in the middle of segment 0 (second image)
    rows += [mid - 1, mid]
    rows = sorted(set(rows))
    dz = torch.zeros(M, dg.npad, device='cuda', dtype=torch.bfloat16)
    dz[rows] = torch.randn(len(rows), dg.npad, device='cuda', generator=dg.gen).bfloat16()
    return dz, rows


def _close(a, b):
    return float((a.double() - b.double()).abs().max()) <= 2e-6 * float(b.double().abs().max()) + 1e-30


@pytest.mark.parametrize('pyramid', [PYRAMID, RAGGED], ids=['pyramid', 'ragged'])
@pytest.mark.parametrize('path', ['pair', 'x3p', 'igemm128'])
def test_dgrad_skips_dead_tiles_and_hands_the_map_on(path, pyramid, monkeypatch):
    dg = _Dgrad(path, pyramid, monkeypatch)
    M, nblk = dg.M, (dg.M + 63) // 64
    dev = 'cuda'
    # (a) an all-zero map over a gradient that is NOT zero: nothing is computed -- zero rows, zero map, untouched column sums
    cs_init = torch.arange(CIN, device=dev, dtype=torch.float32) + 0.5
    out, omap, cs, out_cls, cs_cls = dg.run(dg.dz_dense, torch.zeros(nblk, dtype=torch.uint8, device=dev), cs_init)
    assert int(out.view(torch.int16).count_nonzero()) == 0                  # (+0 heads and tails everywhere, over the NaN prefill)
    assert int(omap.count_nonzero()) == 0
    assert torch.equal(cs, cs_init)
    if path == 'pair':                                                      # the dense member beside it is the plain launch's
        ref = dg.run(dg.dz_dense, None, cs_init)
        assert torch.equal(out_cls, ref[3]) and _close(cs_cls, ref[4])
    # (b) single active pixels
    dz, rows = _planted(dg)
    in_map = torch.from_numpy(_block_map(rows, M)).to(dev)
    ref = dg.run(dz, None)
    got = dg.run(dz, in_map)
    assert bool(torch.isfinite(ref[0].float()).all())
    assert torch.equal(got[0], ref[0])
    assert _close(got[2], ref[2])
    om = got[1].cpu().numpy()
    lower = _block_map(_exact_dilation(rows, dg.B, dg.sizes), M)
    upper = _linear_rule(in_map.cpu().numpy(), dg.B, dg.sizes)
    assert set(np.unique(om)) <= {0, 1}
    assert (om >= lower).all(), np.nonzero(om < lower)
    assert (om <= upper).all(), np.nonzero(om > upper)
    assert om.mean() < 0.5 or pyramid is RAGGED                            # most of the pyramid is skipped
    if path == 'pair':
        assert torch.equal(got[3], ref[3])
    # (c) an all-ones map is the dense launch
    ones = torch.ones(nblk, dtype=torch.uint8, device=dev)
    refd = dg.run(dg.dz_dense, None)
    gotd = dg.run(dg.dz_dense, ones)
    assert torch.equal(gotd[0], refd[0]) and _close(gotd[2], refd[2])
    assert int(gotd[1].count_nonzero()) == nblk
    # (d) race screen (tests/test_gpu_x3p.py): 40 launches back to back, cold and warm operands, all the first one's bits
    if pyramid is PYRAMID:
        junk = torch.empty(64 << 20, device=dev, dtype=torch.uint8)
        for i in range(40):
            if i % 4 == 0:
                junk.random_(0, 255)
            o = dg.run(dz, in_map)
            assert torch.equal(o[0], got[0]) and torch.equal(o[1], got[1]), i


# ------------------------------------------------------------------------------------------------ whole step
def _model():
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    from aod_meh_hua_amd.optim import FusedSGD
    from oracle import model as omodel
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg.model.backbone.pop('init_cfg')
    model = build_detector(cfg.model)
    model.load_state_dict(omodel.seeded_state_dict(), strict=True)
    model = model.cuda().train()
    head = model.bbox_head
    meh = set(id(p) for n in ('retina_L', 'L_convs') for p in getattr(head, n).parameters())
    opt = FusedSGD([p for p in model.parameters() if p.requires_grad and id(p) not in meh], lr=2e-4, momentum=0.9, weight_decay=1e-4)
    opt_L = FusedSGD([p for p in model.parameters() if id(p) in meh], lr=2e-4, momentum=0.9, weight_decay=1e-4)
    return model, opt, opt_L


def _data():
    """2 x 128^2 with one large box per image: its positive anchors sit on P4 and above, so P3 -- 8 of the pyramid's 11 row blocks at this size --
    carries no box-regression gradient at all"""
    from tests import synth
    H = W = 128
    gtb = [torch.tensor([[14., 10., 114., 112.]]), torch.tensor([[8., 20., 108., 118.]])]
    gtl = [torch.tensor([3]), torch.tensor([11])]
    return dict(img=synth.images(2, H, W).cuda(), img_metas=synth.metas(2, H, W), gt_bboxes=[b.cuda() for b in gtb], gt_labels=[l.cuda() for l in gtl])


def _iteration(model, data, log=None):
    from aod_meh_hua_amd import functional as AF
    pd = dict(model.named_parameters())
    AF.MAP_LOG = log
    try:
        out, head_out, feat_out, prev = model.train_step(data, Labeled=True, Pseudo=False)
        model.zero_grad()
        out['loss'].backward()
        grads = {k: p.grad.detach().clone() for k, p in pd.items() if p.grad is not None}
        n_main = len(log) if log is not None else 0
        lossL = model.train_step_L(prev, head_out, feat_out)
        model.zero_grad()
        lossL['loss'].backward()
        grads.update({k + '@L': p.grad.detach().clone() for k, p in pd.items() if p.grad is not None})
        torch.cuda.synchronize()
    finally:
        AF.MAP_LOG = None
    losses = {k: float(v) for k, v in {**out['log_vars'], **lossL['log_vars']}.items()}
    return losses, grads, n_main


def _dealt(name):
    """The filters whose weight gradient is summed in another fp32 order when the maps are on: retina_reg, retina_L and the eight reg / MEH tower
    filters (a mapped wgrad launch deals its active pixel blocks to the splits cyclically), and retina_cls (its launch partner retina_reg now
    waits in the mapped queue, so it runs on its stand-alone split plan).  Same products, other slab boundaries: held to 2e-6 of the largest
    entry, the bound the suite holds its other order-dependent fp32 sums to (the atomic column sums, tests/test_gpu_x3p.py); the per-launch
    error against fp64 is bounded in test_wgrad_walks_only_active_steps_alone_and_in_a_group_of_four."""
    n = name.split('@')[0]
    return n.endswith('.weight') and any(t in n for t in ('.reg_convs.', '.L_convs.', '.retina_reg.', '.retina_L.', '.retina_cls.'))


def test_whole_step_equals_the_dense_step_and_skips(monkeypatch):
    """Losses and parameter gradients of one iteration with AOD_SPARSE_BWD 1 and 0.  Every filter gradient (the wgrad slabs are summed in a fixed
    order: two dense runs give the same bits) must be bit-equal, but for the eleven head filters named in _dealt.  The bias vectors are fp32-ATOMIC column sums: their last bit depends on the
    arrival order of the workgroups' partial sums, which no two runs share, dense or not (seen here: retina_L.bias repeated between two dense
    runs and differed in the last bit in the mapped run) -- they are held to the 2e-6 tests/test_gpu_x3p.py holds the same sums to; that the
    column sums themselves are untouched is checked where the order cannot show (the producer test, the all-zero map of the dgrad tests)."""
    model, _, _ = _model()
    data = _data()
    monkeypatch.setenv('AOD_SPARSE_BWD', '0')
    log0 = []
    l0, g0, _ = _iteration(model, data, log0)
    l0b, g0b, _ = _iteration(model, data)
    assert log0 == []                                                       # switched off: no map anywhere
    monkeypatch.setenv('AOD_SPARSE_BWD', '1')
    log1 = []
    l1, g1, n_main = _iteration(model, data, log1)
    assert l1 == l0 == l0b, (l1, l0)
    assert set(g1) == set(g0)
    dealt = 0
    for k in g0:
        if g0[k].dim() == 4:
            assert torch.equal(g0b[k], g0[k]), k                            # (the premise: a filter gradient repeats bit for bit)
            if _dealt(k):
                assert _close(g1[k], g0[k]), k
                dealt += 1
            else:
                assert torch.equal(g1[k], g0[k]), k
        else:
            assert g0[k].dim() == 1 and _close(g1[k], g0[k]), k             # bias vectors: fp32 atomics, arrival order
            assert _close(g0b[k], g0[k]), k                                 # ... which is all that two dense runs share, too
    assert dealt == 11
    # main pass: retina_reg's dZ, then the dX of retina_reg's dgrad and of the four paired tower dgrads; MEH pass: retina_L's dZ and three dgrads
    assert n_main == 6 and len(log1) == 6 + 5, (n_main, len(log1))
    first_layer_in = log1[4][1]                                             # what reg_convs[0] receives: the dX map of reg_convs[1]'s dgrad
    frac = float(first_layer_in.float().mean())
    assert 0 < frac < 0.5, frac
    assert 0 < float(log1[n_main + 3][1].float().mean()) < 0.5              # ... and L_convs[1]


def test_whole_step_replays_as_a_graph(monkeypatch):
    """The maps are device data at fixed addresses of the graph's pool, so a replayed iteration follows ITS batch's positives: capture on one
    batch, replay on another, and compare the gradients the replay left behind with an eager DENSE iteration on that second batch.  The
    learning rate is zero -- the parameters stay what they were, so the two sets of gradients belong to the same weights and every filter
    gradient must be bit-equal (bias vectors and the filters of _dealt: 2e-6 as above)."""
    from aod_meh_hua_amd.graphs import GraphedTrainStep
    from tests import synth
    d0 = _data()
    gtb, gtl = synth.random_gts(2, 128, 128, seed=24, gmin=1, gmax=3)
    d1 = dict(img=synth.images(2, 128, 128, seed=5).cuda(), img_metas=synth.metas(2, 128, 128), gt_bboxes=[b.cuda() for b in gtb],
              gt_labels=[l.cuda() for l in gtl])
    model, opt, opt_L = _model()
    for o in (opt, opt_L):
        o.param_groups[0]['lr'] = 0.0
    gs = GraphedTrainStep(model, opt, opt_L, warmup=1, Labeled=True, Pseudo=False)
    gs(d0)                                                                  # eager warm-up + capture
    out = gs(d1)                                                            # replay: other boxes, other positives
    torch.cuda.synchronize()
    got = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    losses = {k: float(v) for k, v in out['log_vars'].items()}
    monkeypatch.setenv('AOD_SPARSE_BWD', '0')
    ref_losses, ref, _ = _iteration(model, d1)
    assert all(losses[k] == ref_losses[k] for k in ref_losses), (losses, ref_losses)
    meh = {k for k in got if '.retina_L.' in k or '.L_convs.' in k}
    assert meh and len(got) > len(meh)
    for k, g in got.items():
        r = ref[k + '@L'] if k in meh else ref[k]
        if g.dim() == 4 and not _dealt(k):
            assert torch.equal(g, r), k
        else:
            assert _close(g, r), k


# ------------------------------------------------------------------------------------------------ wgrad
TAIL = ((3, 5),)     # a last level of 2 x 15 rows: M % 64 = 30, so the last block is a partial one of less than a 32-row step
WGRAD_FORMS = {
    # the tower filters' form, wgrad_tile_x3w<8, 4>: alone from 49 152 rows on, in a group from 16 384
    '8x4': dict(alone=(2, ((128, 128), (96, 96)) + TAIL), group=(2, PYRAMID[1] + TAIL), n_log=256, O=256, form=2),
    # retina_reg's form, wgrad_tile_x3w<4, 2> with a ragged column tile (128 physical dZ columns)
    '4x2': dict(alone=(2, PYRAMID[1] + TAIL), group=(2, PYRAMID[1] + TAIL), n_log=64, O=36, form=3),
    # retina_L's form, conv_wgrad_kernel<4, 1, 1, true> (64 physical dZ columns)
    '4x1x1': dict(alone=(2, PYRAMID[1] + TAIL), group=(2, PYRAMID[1] + TAIL), n_log=32, O=9, form=0),
}


def _wgrad_plan(descs):
    from aod_meh_hua_amd import _C
    n = len(descs)
    form, sp, rps = C.c_int32(), (C.c_int32 * n)(), (C.c_int32 * n)()
    rc = _C.lib.aod_conv2d_wgrad_plan((C.c_void_p * n)(*[C.addressof(d) for d in descs]), n, C.byref(form), sp, rps)
    return (None, None, None) if rc else (form.value, list(sp), list(rps))


def _sparse_dz(M, n_log, splits, rps, gen):
    """fp32 dZ with a few active 64-row blocks: contiguous split 0 has none, split 1 only its first block, split 2 only its last, the others two
    inner ones; and the ragged last block of the tensor.  -> (fp32 values, X-layout rows, map)"""
    from aod_meh_hua_amd import hipops as ho
    dz = torch.zeros(M, n_log, device='cuda')
    blocks = [(M - 1) // 64]
    for s_ in range(1, splits):
        b0, b1 = s_ * rps // 64, (min(M, (s_ + 1) * rps) + 63) // 64 - 1
        blocks += [b0] if s_ == 1 else ([b1] if s_ == 2 else [b0 + (b1 - b0) // 3, b0 + 2 * (b1 - b0) // 3])
    blocks = sorted(set(blocks))
    for b in blocks:
        r0, r1 = 64 * b, min(64 * b + 64, M)
        dz[r0:r1] = torch.randn(r1 - r0, n_log, device='cuda', generator=gen)
    zmap = torch.zeros((M + 63) // 64, dtype=torch.uint8, device='cuda')
    zmap[blocks] = 1
    return dz, ho.x3_split(dz), zmap


def _dw_fp64(x, dz, B, sizes):
    """sum_m dZ[m, n] * x[pixel(m) + (r - 1, s - 1), c] in fp64 -> [N, 3, 3, C] (rows with dZ = 0 left out: they add nothing)"""
    ref = torch.zeros(dz.shape[1], 3, 3, x.shape[1], dtype=torch.float64, device=x.device)
    r0 = 0
    for h, w in sizes:
        n = B * h * w
        z = dz[r0:r0 + n].double()
        keep = (z != 0).any(1).nonzero().squeeze(1)
        xp = torch.nn.functional.pad(x[r0:r0 + n].double().view(B, h, w, -1), (0, 0, 1, 1, 1, 1))
        for r in range(3):
            for q in range(3):
                ref[:, r, q] += z[keep].T @ xp[:, r:r + h, q:q + w].reshape(n, -1)[keep]
        r0 += n
    return ref


def _err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('form', sorted(WGRAD_FORMS))
def test_wgrad_walks_only_active_steps_alone_and_in_a_group_of_four(form):
    """A mapped launch deals the active blocks to its splits cyclically: the slabs hold other partial sums than the dense launch's, their total
    is the same filter gradient in another fp32 summation order.  Both launches against an fp64 contraction of the same operands: the mapped
    launch's largest error may be at most 1.5 x the dense launch's.  M % 64 = 30 with the last block active: the mapped walk issues a step
    that starts beyond the last row, which the dense walk never does."""
    from aod_meh_hua_amd import hipops as ho
    f = WGRAD_FORMS[form]
    gen = torch.Generator(device='cuda').manual_seed(29)
    n_phys = 2 * f['n_log']
    # ---- alone
    B, sizes = f['alone']
    segs, M = _segs(B, sizes)
    assert 1 <= M % 64 <= 32
    xf = torch.randn(M, CIN, device='cuda', generator=gen)
    x = ho.x3_split(xf)
    d = ho.make_desc(ho.xw(CIN), n_phys, 3, 3, 1, 1, 1, segs, segs, False, False, False)
    got_form, sp, rps = _wgrad_plan([d])
    if got_form != f['form'] or sp[0] < 3:
        pytest.skip(f'{form} alone: planned form {got_form} with {sp} splits, the test needs form {f["form"]} and three splits')
    dzf, dz, zmap = _sparse_dz(M, f['n_log'], sp[0], rps[0], gen)
    ref = _dw_fp64(xf, dzf, B, sizes)
    dense = ho.conv2d_wgrad_rows(x, segs, dz, segs, 3, 3, 1, 1, 1).clone()
    assert dense.shape[0] == sp[0] and bool(torch.isfinite(dense).all())
    assert int(dense[0].count_nonzero()) == 0 and int(dense[1].count_nonzero()) > 0 and int(dense[2].count_nonzero()) > 0
    e_dense = _err(dense.double().sum(0), ref)
    for name, m in (('mapped', zmap), ('all-ones map', torch.ones_like(zmap))):
        sparse = ho.conv2d_wgrad_rows(x, segs, dz, segs, 3, 3, 1, 1, 1, zmap=m).clone()
        e = _err(sparse.double().sum(0), ref)
        print(f'{form} alone, {name}: max error {e:.3e}, dense {e_dense:.3e}')
        assert 0 < e_dense < 1e-4 and e <= 1.5 * e_dense, (name, e, e_dense)
    # ---- a group of four: all mapped, and two mapped members beside two without a map
    B, sizes = f['group']
    segs, M = _segs(B, sizes)
    assert 1 <= M % 64 <= 32
    d = ho.make_desc(ho.xw(CIN), n_phys, 3, 3, 1, 1, 1, segs, segs, False, False, False)
    got_form, sp, rps = _wgrad_plan([d] * 4)
    if got_form is None:                                                    # (the plan prefers four launches: wgrad_unpack_group then runs them so)
        got_form, sp, rps = _wgrad_plan([d])
    if got_form != f['form'] or sp[0] < 3:
        pytest.skip(f'{form} group: planned form {got_form} with {sp} splits')
    xfs = [torch.randn(M, CIN, device='cuda', generator=gen) for _ in range(4)]
    xs = [ho.x3_split(t) for t in xfs]
    dzfs, dzs, maps = zip(*[_sparse_dz(M, f['n_log'], sp[0], rps[0], gen) for _ in range(4)])
    refs = [_dw_fp64(xfs[i], dzfs[i], B, sizes)[:f['O']].permute(0, 3, 1, 2) for i in range(4)]

    def run(use):
        gws = [torch.full((f['O'], CIN, 3, 3), float('nan'), device='cuda') for _ in range(4)]
        jobs = [ho.WgradJob(xs[i], segs, dzs[i], segs, 3, 3, 1, 1, 1, (CIN, f['O']), f['O'], CIN, gws[i], zmap=maps[i] if use[i] else None)
                for i in range(4)]
        ho.wgrad_unpack_group(jobs)
        torch.cuda.synchronize()
        return [_err(g, r) for g, r in zip(gws, refs)]
    e_dense = run([False] * 4)
    assert all(0 < e < 1e-4 for e in e_dense), e_dense
    for use in ([True] * 4, [True, False, True, False]):
        e = run(use)
        print(f'{form} group {use}: max errors {e}, dense {e_dense}')
        assert all(a <= 1.5 * b_ for a, b_ in zip(e, e_dense)), (use, e, e_dense)
