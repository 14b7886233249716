"""GPU: the plain RetinaNet baseline (FocalLoss / MyRetinaHead / MyRetinaNet).

Loss kernels (aod_sigmoid_focal_l1_* / aod_sigmoid_focal_elem) against the reference's golden (tests/golden/plain_retina.npz: its own
MyRetinaHead + FocalLoss on the CPU) and against the float64 evaluation of mmcv's formula, with the tolerances the project applies to the
EDL form (tests/test_gpu_kernels.py: loss_noR rows rtol 2e-5 / atol 1e-7, the three sums rtol 1e-5, logit gradients rtol 5e-4 / atol 2e-7);
their bit properties (level-fused == per-level, bf16 dZ == rounded fp32 dZ) and edges (label C, zero weights, C = 80, ragged blocks,
saturated logits).  Mode 3 of the pre-NMS kernels against float64 sigmoid (4 * 2^-23 relative) and a float64 top-k (int-exact: the golden
keys are separated by more than twice that bound), detections against the golden with the tolerances of tests/test_gpu_scoring.py.
The model: one training step against a float32 CPU composition of the oracle's pieces (tolerances of tests/test_gpu_model.py), graph
replay == eager and run == run in the deterministic mode, and the train-then-score pipeline."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import plain_retina_util as U
from tests import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_TOL = dict(rtol=2e-5, atol=1e-7)
SUM_RTOL = 1e-5
GRAD_TOL = dict(rtol=5e-4, atol=2e-7)


@pytest.fixture(scope='module')
def ho():
    from aod_meh_hua_amd import hipops
    return hipops


@pytest.fixture(scope='module')
def gold():
    g = U.load_golden()
    lv = U.golden_level_inputs(g)
    cat = {k: torch.cat([li[k] for li in lv]).cuda() for k in lv[0]}
    f64 = [U.focal64(li['cls'].numpy(), li['labels'].numpy()) for li in lv]
    return dict(g=g, lv=lv, cat=cat, f64=f64, n=int(g['num_total_samples']))


def _close(a, b, rtol, atol=0.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b)
    print(f'    max abs err {err.max():.3e}, max err / (atol + rtol |ref|) {(err / (atol + rtol * np.abs(b) + 1e-300)).max():.3f}')
    return bool((err <= atol + rtol * np.abs(b)).all())


# ------------------------------------------------------------------------------------------------ loss kernels
def test_rows_sums_and_gradients_match_the_golden_and_float64(ho, gold):
    g, n = gold['g'], gold['n']
    one = torch.full((1,), 1.0 / n, device='cuda')
    for l, li in enumerate(gold['lv']):
        d = {k: v.cuda() for k, v in li.items()}
        rows = d['cls'].shape[0]
        noR, sums = ho.edl_focal_l1_fwd(d['cls'], d['labels'], d['lw'], d['reg'], d['bt'], d['bw'], form='sigmoid')
        torch.cuda.synchronize()
        l64, gz64 = gold['f64'][l]
        print(f'level {l}: {rows} rows')
        assert _close(noR.cpu(), g[f'loss_noR{l}'], **ROW_TOL) and _close(noR.cpu(), l64.sum(-1), **ROW_TOL)
        s = sums.double().cpu().numpy()
        assert _close(s[0] / n, g['loss_cls'][l], SUM_RTOL) and _close(s[1] / n, g['loss_bbox'][l], SUM_RTOL)
        assert _close(s[2] / rows, g[f'loss_noR{l}'].astype(np.float64).mean(), SUM_RTOL)
        assert _close(s[0], (l64 * li['lw'].double().numpy()[:, None]).sum(), SUM_RTOL) and _close(s[2], l64.sum(), SUM_RTOL)
        # gradients of loss_cls + loss_bbox + mean(loss_noR): g_cls = g_box = 1 / n, g_noR = 1 / rows for every row
        gc, gb = ho.edl_focal_l1_bwd(d['cls'], d['labels'], d['lw'], d['reg'], d['bt'], d['bw'], one, one, None, 1.0 / rows, form='sigmoid')
        want = U.rows_of(g[f'grad_cls{l}'], U.C).numpy()
        coef = li['lw'].double().numpy()[:, None] / n + 1.0 / rows
        assert _close(gc.cpu(), want, **GRAD_TOL) and _close(gc.cpu(), coef * gz64, **GRAD_TOL)
        assert np.array_equal(gb.cpu().numpy(), U.rows_of(g[f'grad_reg{l}'], 4).numpy())


def _per_level(ho, gold, bf16=False):
    outs = []
    one = torch.full((1,), 0.03125, device='cuda')
    for li in gold['lv']:
        d = {k: v.cuda() for k, v in li.items()}
        noR, sums = ho.edl_focal_l1_fwd(d['cls'], d['labels'], d['lw'], d['reg'], d['bt'], d['bw'], form='sigmoid')
        gc, gb = ho.edl_focal_l1_bwd(d['cls'], d['labels'], d['lw'], d['reg'], d['bt'], d['bw'], one, one * 2, None, 0.0, g_noR_is_scalar=False,
                                     out_bf16=bf16, A=U.A, form='sigmoid')
        outs.append((noR, sums, gc, gb))
    return outs


def test_level_fused_launch_is_bit_identical_to_per_level_launches(ho, gold):
    c = gold['cat']
    rows = list(U.LEVEL_ROWS)
    noR, sums = ho.edl_focal_l1_levels_fwd(c['cls'], c['labels'], c['lw'], c['reg'], c['bt'], c['bw'], rows, form='sigmoid')
    per = _per_level(ho, gold)
    assert torch.equal(noR, torch.cat([p[0] for p in per]))
    assert torch.equal(sums, torch.stack([p[1] for p in per], 1))
    L = len(rows)
    g_sums = torch.tensor([[0.03125] * L, [0.0625] * L, [0.0] * L], device='cuda')
    gc = torch.empty(sum(rows) // U.A, U.A * U.C, device='cuda')
    gb = torch.empty(sum(rows) // U.A, U.A * 4, device='cuda')
    ho.edl_focal_l1_levels_bwd(c['cls'], c['labels'], c['lw'], c['reg'], c['bt'], c['bw'], rows, g_sums, None, gc, gb, U.A, form='sigmoid')
    assert torch.equal(gc, torch.cat([p[2] for p in per])) and torch.equal(gb, torch.cat([p[3] for p in per]))
    assert float(gc.abs().max()) > 0
    # num_pos: the divided sums and the divisors, as the head uses them; the backward divides its upstream gradients itself
    num_pos = torch.tensor([20, 12], dtype=torch.int32, device='cuda')
    noR2, q, div, nt = ho.edl_focal_l1_levels_fwd(c['cls'], c['labels'], c['lw'], c['reg'], c['bt'], c['bw'], rows, num_pos=num_pos, form='sigmoid')
    assert torch.equal(noR2, noR) and float(nt) == 32.0
    want_div = torch.tensor([[32.0] * L, [32.0] * L, [float(r) for r in rows]], device='cuda')
    assert torch.equal(div, want_div) and torch.equal(q, sums / want_div)
    gc2, gb2 = torch.empty_like(gc), torch.empty_like(gb)
    ho.edl_focal_l1_levels_bwd(c['cls'], c['labels'], c['lw'], c['reg'], c['bt'], c['bw'], rows, g_sums * want_div, None, gc2, gb2, U.A,
                               divisors=div, form='sigmoid')
    assert torch.equal(gc2, gc) and torch.equal(gb2, gb)              # (g * d) / d == g for these power-of-two gradients
    # a gradient per loss_noR row replaces row 2
    g_rows = torch.rand(sum(rows), generator=torch.Generator().manual_seed(3)).cuda()
    gc3 = torch.empty_like(gc)
    ho.edl_focal_l1_levels_bwd(c['cls'], c['labels'], c['lw'], c['reg'], c['bt'], c['bw'], rows, g_sums * 0, g_rows, gc3, torch.empty_like(gb), U.A,
                               form='sigmoid')
    gz = np.concatenate([f[1] for f in gold['f64']])
    assert _close(gc3.view(-1, U.C).cpu(), g_rows.double().cpu().numpy()[:, None] * gz, **GRAD_TOL)


def test_bf16_dz_layout_is_the_rounded_fp32_one(ho, gold):
    """the (A, pitch) layout of the prediction conv's dZ buffer: pitch 184 >= 9 * 20 (rounded up to 8), box pitch 40; bf16 == fp32 rounded"""
    li = gold['lv'][0]
    d = {k: v.cuda() for k, v in li.items()}
    one = torch.full((1,), 1.0 / gold['n'], device='cuda')
    args = (d['cls'], d['labels'], d['lw'], d['reg'], d['bt'], d['bw'], one, one, None, 1.0 / 1152)
    g32, b32 = ho.edl_focal_l1_bwd(*args, A=U.A, pitch_cls=184, pitch_box=40, form='sigmoid')
    g16, b16 = ho.edl_focal_l1_bwd(*args, out_bf16=True, A=U.A, pitch_cls=184, pitch_box=40, form='sigmoid')
    flat, _ = ho.edl_focal_l1_bwd(*args, form='sigmoid')
    assert g32.shape == (128, 184) and g16.dtype == torch.bfloat16
    assert torch.equal(g32[:, :180].reshape(-1, U.C), flat) and (g32[:, 180:] == 0).all() and (g16[:, 180:] == 0).all()
    assert torch.equal(g16, g32.bfloat16()) and torch.equal(b16, b32.bfloat16()) and (b32[:, 36:] == 0).all()


@pytest.mark.parametrize('rows,C', [(330, 80), (1, 20), (257, 21), (64 * 3 + 5, 25), (700, 96)])
def test_wide_rows_ragged_blocks_label_C_and_zero_weights(ho, rows, C):
    """C = 80 / 96 / 25: four lanes per row, 64 rows per block (rows not a multiple of 64); C = 20 / 21: one lane per row, 256 per block.
    Every fifth row is background (label C: every column negative), every third has weight zero."""
    g = torch.Generator().manual_seed(rows * 131 + C)
    x = torch.rand(rows, C, generator=g) * 10 - 5
    lab = torch.randint(0, C, (rows,), generator=g)
    lab[::5] = C
    lw = torch.ones(rows)
    lw[::3] = 0
    bp, bt = torch.randn(rows, 4, generator=g), torch.randn(rows, 4, generator=g)
    bw = (lab < C).float()[:, None].expand(rows, 4).contiguous()
    l64, gz64 = U.focal64(x.numpy(), lab.numpy())
    dev = [t.cuda() for t in (x, lab, lw, bp, bt, bw)]
    noR, sums = ho.edl_focal_l1_fwd(*dev, form='sigmoid')
    assert _close(noR.cpu(), l64.sum(-1), **ROW_TOL)
    s = sums.double().cpu().numpy()
    assert _close(s[0], (l64.sum(-1) * lw.double().numpy()).sum(), SUM_RTOL) and _close(s[2], l64.sum(), SUM_RTOL)
    assert _close(s[1], ((bp - bt).abs() * bw).double().sum(), SUM_RTOL)
    # label C rows are what an all-negative row costs: -(1 - alpha) q^2 log(1 - q) summed over the columns
    q = U.sigmoid64(x.numpy()[::5])
    assert _close(noR.cpu()[::5], (-0.75 * q ** 2 * np.log(1 - q)).sum(-1), **ROW_TOL)
    g_rows = torch.rand(rows, generator=g)
    one = torch.ones(1, device='cuda')
    gc, gb = ho.edl_focal_l1_bwd(*dev, one * 0.5, one, g_rows.cuda(), 0.0, form='sigmoid')
    coef = 0.5 * lw.double().numpy() + g_rows.double().numpy()
    assert _close(gc.cpu(), coef[:, None] * gz64, **GRAD_TOL)
    # a zero-weight row without a row gradient gets an exactly zero gradient; its loss_noR row is unweighted
    gc0, _ = ho.edl_focal_l1_bwd(*dev, one, one, None, 0.0, form='sigmoid')
    assert (gc0[::3] == 0).all() and (rows == 1 or float(gc0.abs().max()) > 0) and float(noR[::3].min()) > 0
    assert torch.equal(gb.cpu(), torch.sign(bp - bt) * bw)
    # the elementwise entry: its class sum is the row kernel's row, its gradient the per-class derivative
    from aod_meh_hua_amd.models import build_loss
    mod = build_loss(dict(type='FocalLoss', last_activation='sigmoid'))
    xe = dev[0].clone().requires_grad_(True)
    el = mod(xe, dev[1], reduction_override='none')
    assert el.shape == (rows, C) and _close(el.sum(-1).detach().cpu(), noR.cpu(), **ROW_TOL)
    # (no element may be off by more than its row's tolerance: short of a cancellation the row check above would miss it)
    assert (np.abs(el.detach().double().cpu().numpy() - l64) <= 1e-7 + 2e-5 * np.abs(l64.sum(-1))[:, None]).all()
    w_e = torch.rand(rows, C, generator=g)
    (el * w_e.cuda()).sum().backward()
    assert _close(xe.grad.cpu(), w_e.double().numpy() * gz64, **GRAD_TOL)
    # reduction rules of the module: per-row weights + avg_factor go through the fused row kernel
    a = mod(dev[0], dev[1], dev[2], avg_factor=7.0)
    assert _close(float(a), (l64.sum(-1) * lw.double().numpy()).sum() / 7.0, SUM_RTOL)
    assert _close(float(mod(dev[0], dev[1])), l64.mean(), SUM_RTOL)
    assert _close(float(mod(dev[0], dev[1], w_e.cuda(), reduction_override='sum')), (l64 * w_e.double().numpy()).sum(), SUM_RTOL)


def test_saturated_logits_give_finite_losses_and_gradients(ho):
    """x in {+-30, +-100}: q rounds to 0 / 1 and the clamp bounds the term at -log(FLT_MIN), as in the reference (no softplus form)"""
    vals = torch.tensor([30.0, -30.0, 100.0, -100.0])
    x = vals.repeat(5)[None].repeat(8, 1).contiguous()            # [8, 20]
    lab = torch.tensor([0, 1, 2, 3, 20, 20, 7, 18])
    dev = (x.cuda(), lab.cuda(), torch.ones(8, device='cuda'))
    noR, sums = ho.edl_focal_l1_fwd(*dev, form='sigmoid')
    one = torch.ones(1, device='cuda')
    gc, _ = ho.edl_focal_l1_bwd(*dev, None, None, None, one, one, None, 1.0, form='sigmoid')
    assert torch.isfinite(noR).all() and torch.isfinite(sums).all() and torch.isfinite(gc).all()
    assert float(noR.min()) >= 0 and float(noR.max()) <= 20 * 87.4
    from aod_meh_hua_amd.models import build_loss
    el = build_loss(dict(type='FocalLoss'))(dev[0].clone().requires_grad_(True), dev[1], reduction_override='none')
    el.sum().backward()
    assert torch.isfinite(el).all()
    e, s = ho.edl_focal_l1_fwd(torch.zeros(0, 20, device='cuda'), torch.zeros(0, dtype=torch.long, device='cuda'), torch.zeros(0, device='cuda'),
                               form='sigmoid')
    assert e.numel() == 0 and float(s.sum()) == 0


# ------------------------------------------------------------------------------------------------ scoring
class Cfg(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope='module')
def scored(gold):
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd.core.anchor import AnchorGenerator
    from aod_meh_hua_amd.core.bbox import DeltaXYWHBBoxCoder

    class Head:
        last_activation, cls_out_channels, num_anchors = 'sigmoid', U.C, U.A
        bbox_coder = DeltaXYWHBBoxCoder()
    g = gold['g']
    cls = [torch.from_numpy(g[f'cls{l}']).cuda() for l in range(5)]
    reg = [torch.from_numpy(g[f'reg{l}']).cuda() for l in range(5)]
    mt = synth.metas(U.B, U.H, U.W, scale=1.25)
    ag = AnchorGenerator(octave_base_scale=4, scales_per_octave=3, ratios=[0.5, 1.0, 2.0], strides=[8, 16, 32, 64, 128])
    anchors = ag.grid_anchors([tuple(c.shape[-2:]) for c in cls], 'cuda')
    cfg = Cfg(nms_pre=U.NMS_PRE, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
    shapes, factors = [m['img_shape'] for m in mt], [m['scale_factor'] for m in mt]
    lam = [torch.zeros(U.B, U.A, *c.shape[-2:], device='cuda') for c in cls]
    out = {}
    for merged in ('1', '0'):            # the merged two-launch form and the per-level entry points
        os.environ['AOD_PRE_NMS_MERGED'] = merged
        try:
            out[merged] = scoring.pre_nms(cls, reg, lam, anchors, shapes, factors, U.NMS_PRE, U.C, (0., 0., 0., 0.), (1., 1., 1., 1.), rescale=True,
                                          activation='sigmoid')
        finally:
            os.environ.pop('AOD_PRE_NMS_MERGED', None)
    args = (Head(), cls, reg, anchors, shapes, factors, cfg)
    dets = scoring.score_batch(*args, rescale=True, with_nms=True, isEval=True, isUnc=False)
    padded = scoring.score_batch(*args, rescale=True, with_nms=True, isEval=True, isUnc=False, _padded=True)
    no_nms = scoring.score_batch(*args, rescale=True, with_nms=False, isEval=False, isUnc=False)
    torch.cuda.synchronize()
    return dict(cand=out['1'], cand_levels=out['0'], dets=dets, padded=padded, no_nms=no_nms, args=args, scoring=scoring)


def test_mode3_scores_and_selection_against_float64(gold, scored):
    g, cand = gold['g'], scored['cand']
    assert cand.level_start == [0] + list(np.cumsum(U.CAND_PER_LEVEL))
    for k in ('boxes', 'scores', 'cand_anchor'):
        assert torch.equal(getattr(cand, k), getattr(scored['cand_levels'], k)), k
    scores = cand.scores.double().cpu().numpy()
    anchor0 = 0
    for l, (h, w) in enumerate(U.LEVELS):
        keys = U.level_keys64(g[f'cls{l}'])                                    # [B, h*w*A]
        assert U.keys_separated(keys)                                          # the case is what it claims: fp32 cannot reorder these keys
        n, k = keys.shape[1], U.CAND_PER_LEVEL[l]
        rm = cand.rowmax[l].double().cpu().numpy()
        assert (np.abs(rm - keys) <= U.SCORE_RTOL * keys).all()
        order = np.argsort(-keys, axis=1, kind='stable')[:, :k] if k < n else np.tile(np.arange(n), (U.B, 1))
        if k < n:
            assert np.array_equal(cand.topk_idx[l].cpu().numpy(), order)       # int-exact against the float64 top-k, order included
        else:
            assert cand.topk_idx[l] is None
        s0 = cand.level_start[l]
        assert np.array_equal(cand.cand_anchor[:, s0:s0 + k].cpu().numpy(), order + anchor0)
        x = np.asarray(g[f'cls{l}'], np.float64).transpose(0, 2, 3, 1).reshape(U.B, n, U.C)
        want = U.sigmoid64(np.take_along_axis(x, order[:, :, None], 1))
        got = scores[:, s0:s0 + k]
        assert got.shape[-1] == U.C + 1 and (got[..., U.C] == 0).all()         # the zero background column of anchor_head.py:592-596
        rel = np.abs(got[..., :U.C] - want) / want
        print(f'level {l}: max rel score err {rel.max():.3e} (bound {U.SCORE_RTOL:.3e})')
        assert (rel <= U.SCORE_RTOL).all()
        anchor0 += n
    # the reference's own candidates (what it handed to multiclass_nms)
    assert np.allclose(cand.boxes.cpu().numpy(), g['cand_boxes'], rtol=1e-5, atol=1e-4)
    assert np.allclose(cand.scores.cpu().numpy(), g['cand_scores'], rtol=1e-5, atol=1e-8)


def test_detections_match_the_golden(gold, scored):
    g = gold['g']
    dets_p, labels_p, num_p = scored['padded']
    for b in range(U.B):
        d, lab = scored['dets'][b]
        gd = g[f'det{b}']
        assert d.shape[0] == gd.shape[0] > 0 and int(num_p[b]) == gd.shape[0]
        assert np.array_equal(lab.cpu().numpy(), gd[:, 5].astype(np.int64))
        assert np.allclose(d.cpu().numpy(), gd[:, :5], rtol=1e-5, atol=1e-4)
        assert torch.equal(dets_p[b, :d.shape[0]], d) and torch.equal(labels_p[b, :d.shape[0]], lab)
        boxes, sc = scored['no_nms'][b]
        assert torch.equal(boxes, scored['cand'].boxes[b]) and torch.equal(sc, scored['cand'].scores[b])
    with pytest.raises(ValueError, match='has no lambda'):
        scored['scoring'].score_batch(*scored['args'], rescale=True, with_nms=True, isEval=False, isUnc='Epistemic', uPool='Entropy_NMS',
                                      uPool2='objectSum_scaleMax_classSum')


def test_mode3_wide_rows(scored):
    """C = 80: the MAXC instantiation of the three kernels (no sum occurs in the sigmoid mode: nothing to split into partial sums)"""
    scoring = scored['scoring']
    C, A, B, h = 80, 3, 2, 5
    g = torch.Generator().manual_seed(81)
    cls = [(torch.rand(B, A * C, h, h, generator=g) * 10 - 5).cuda()]
    reg = [(0.1 * torch.randn(B, A * 4, h, h, generator=g)).cuda()]
    anchors = [(torch.rand(h * h * A, 2, generator=g) * 20).repeat(1, 2).add(torch.tensor([0., 0., 9., 9.])).cuda()]
    lam = [torch.zeros(B, A, h, h, device='cuda')]
    cand = scoring.pre_nms(cls, reg, lam, anchors, [(64, 64, 3)] * B, None, 40, C, (0., 0., 0., 0.), (1., 1., 1., 1.), rescale=False,
                           activation='sigmoid')
    x = cls[0].double().cpu().numpy().transpose(0, 2, 3, 1).reshape(B, h * h * A, C)
    keys = U.sigmoid64(x).max(-1)
    rm = cand.rowmax[0].double().cpu().numpy()
    assert (np.abs(rm - keys) <= U.SCORE_RTOL * keys).all()
    idx = cand.topk_idx[0].cpu().numpy()
    want = U.sigmoid64(np.take_along_axis(x, idx[:, :, None].astype(np.int64), 1))
    got = cand.scores.double().cpu().numpy()
    assert got.shape == (B, 40, C + 1) and (np.abs(got[..., :C] - want) <= U.SCORE_RTOL * want).all() and (got[..., C] == 0).all()
    # the selected keys are the 40 largest (ties aside: within the score bound of the float64 40th key)
    kth = np.sort(keys, axis=1)[:, -40]
    assert (np.take_along_axis(keys, idx.astype(np.int64), 1) >= kth[:, None] * (1 - 2 * U.SCORE_RTOL)).all()


# ------------------------------------------------------------------------------------------------ model
@pytest.fixture(params=['bf16x3', 'bf16'])
def precision(request):
    from aod_meh_hua_amd import functional as AF
    AF.set_precision(request.param)
    yield request.param
    AF.set_deterministic(False)
    AF.set_precision(os.environ.get('AOD_CONV_PREC', 'bf16x3'))


@pytest.fixture(scope='module')
def cpu_step():
    """the float32 CPU composition, computed once: loss terms and parameter gradients of one step at 2 x 64 x 64"""
    sd = {k: v.clone() for k, v in U.plain_state_dict().items()}
    for k, v in sd.items():
        if v.is_floating_point() and not any(s in k for s in ('running', 'backbone.conv1.', 'backbone.bn1.', 'layer1.')):
            v.requires_grad_(True)
    img = synth.images(U.B, U.H, U.W)
    gtb, gtl = synth.random_gts(U.B, U.H, U.W, seed=24, gmin=1, gmax=3)
    torch.set_num_threads(8)
    o = U.cpu_train_step(sd, img, gtb, gtl)
    o['loss'].backward()
    return dict(o=o, sd=sd, img=img, gtb=gtb, gtl=gtl)


def test_train_step_against_the_cpu_composition(cpu_step, precision):
    o, sd = cpu_step['o'], cpu_step['sd']
    model, _ = U.build_plain(ROOT, U.plain_state_dict(), 'cuda')
    model.train()
    data = dict(img=cpu_step['img'].cuda(), img_metas=synth.metas(U.B, U.H, U.W), gt_bboxes=[b.cuda() for b in cpu_step['gtb']],
                gt_labels=[l.cuda() for l in cpu_step['gtl']])
    out, head_out, feat_out, prev = model.train_step(data, Labeled=True, Pseudo=False)
    torch.cuda.synchronize()
    assert int(head_out[8]) == o['targets']['num_total_pos']                    # integer-exact assignment
    want = [float(sum(o['loss_cls']).detach()), float(sum(o['loss_bbox']).detach()), float(sum(t.mean() for t in o['loss_noR']).detach())]
    got = [float(out['log_vars'][k]) for k in ('loss_cls', 'loss_bbox', 'loss_noR')]
    print(precision, 'losses', got, 'cpu', want, 'total', float(out['loss']), float(o['loss']))
    assert list(out['log_vars'].keys()) == ['loss_cls', 'loss_bbox', 'loss_noR']
    assert np.allclose(got, want, rtol=2e-2) and np.allclose(float(out['loss']), float(o['loss']), rtol=2e-2)
    assert len(prev) == 5 and [int(p.numel()) for p in prev] == list(U.LEVEL_ROWS) and not any(p.requires_grad for p in prev)
    rel = lambda a, b: float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))
    assert rel(prev[0].cpu().numpy(), o['loss_noR'][0].detach().numpy()) < 3e-2
    model.zero_grad()
    out['loss'].backward()
    torch.cuda.synchronize()
    pd = dict(model.named_parameters())
    assert pd['backbone.conv1.weight'].grad is None
    for k in ['backbone.layer2.0.conv1.weight', 'backbone.layer2.0.bn1.weight', 'backbone.layer3.5.conv2.weight', 'backbone.layer4.2.bn3.weight',
              'neck.lateral_convs.1.conv.weight', 'neck.fpn_convs.0.conv.bias', 'bbox_head.cls_convs.2.conv.weight',
              'bbox_head.reg_convs.0.conv.bias', 'bbox_head.retina_cls.weight', 'bbox_head.retina_cls.bias', 'bbox_head.retina_reg.weight']:
        a, b = pd[k].grad.float().cpu().flatten(), sd[k].grad.flatten()
        cos = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))
        print(f'    {k}: cos {cos:.5f}, norm ratio {float(a.norm() / b.norm()):.4f}')
        assert cos > 0.995, (k, cos)
        assert abs(float(a.norm() / b.norm()) - 1) < 5e-2, (k, float(a.norm()), float(b.norm()))
    with pytest.raises(ValueError, match='no lambda'):
        model.train_step_L(prev, head_out, feat_out)


def _batch(seed):
    gtb, gtl = synth.random_gts(U.B, U.H, U.W, seed=seed, gmin=1, gmax=3)
    return dict(img=synth.images(U.B, U.H, U.W, seed=seed).cuda(), img_metas=synth.metas(U.B, U.H, U.W), gt_bboxes=gtb, gt_labels=gtl)


def _three_iterations(graphed):
    from aod_meh_hua_amd.apis.train_Lambda import build_optimizers
    model, cfg = U.build_plain(ROOT, U.plain_state_dict(cls_bias=-2.0), 'cuda')
    model.train()
    cfg.optimizer.lr = 2e-4
    opt, opt_L = build_optimizers(model, cfg)
    assert opt_L is None
    losses = []
    if graphed:
        from aod_meh_hua_amd.graphs import GraphedTrainStep
        gs = GraphedTrainStep(model, opt, None, warmup=2, Labeled=True, Pseudo=False)
    for seed in (31, 32, 33):
        d = _batch(seed)
        if graphed:
            o = gs(d)
            assert list(o['log_vars'].keys()) == ['loss_cls', 'loss_bbox', 'loss_noR']
            losses.append(float(o['loss']))
        else:
            out, *_ = model.train_step(d, Labeled=True, Pseudo=False)
            opt.zero_grad()
            out['loss'].backward()
            opt.step()
            losses.append(float(out['loss'].detach()))
    torch.cuda.synchronize()
    if graphed:
        assert len(gs.cache) == 1 and len(next(iter(gs.cache.values()))['graphs']) == 1
    return losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def test_three_iterations_graph_replay_equals_eager_bit_for_bit(precision):
    """deterministic mode (ordered column sums): the one-optimizer iteration replayed from its captured graph (segments a and c) ends in
    the parameter bits of the eager iteration, and two eager runs agree bit for bit"""
    from aod_meh_hua_amd import functional as AF
    AF.set_deterministic(True)
    l0, sd0 = _three_iterations(False)
    l1, sd1 = _three_iterations(False)
    l2, sd2 = _three_iterations(True)
    print(precision, 'losses eager', l0, 'replayed', l2)
    assert l0 == l1 and l0 == l2 and all(np.isfinite(l0))
    init = U.plain_state_dict(cls_bias=-2.0)
    assert float((sd0['bbox_head.retina_cls.weight'] - init['bbox_head.retina_cls.weight']).abs().max()) > 0
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), ('run vs run', k)
        assert torch.equal(sd0[k], sd2[k]), ('replay vs eager', k)


def test_runner_iteration_has_one_optimizer_and_skips_the_meh_half(monkeypatch):
    """MyEpochBasedRunnerLambda.run_iter on the plain detector: eager and replayed iterations, no loss_L / grad_norm_L in the log"""
    from aod_meh_hua_amd.apis.train_Lambda import build_optimizers
    from aod_meh_hua_amd.mmcv_lite import MMDataParallel, build_runner
    from aod_meh_hua_amd.utils import get_root_logger
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    model, cfg = U.build_plain(ROOT, U.plain_state_dict(cls_bias=-2.0), 'cuda')
    cfg.optimizer_config = dict(grad_clip=dict(max_norm=35, norm_type=2))
    model = MMDataParallel(model, device_ids=[0])
    opt, opt_L = build_optimizers(model, cfg)
    runner = build_runner(cfg.runner, default_args=dict(model=model, optimizer=opt, work_dir=None, logger=get_root_logger(log_level='ERROR'), meta=None))
    runner.optimizer_L = opt_L
    model.train()
    w0 = model.module.bbox_head.retina_cls.weight.detach().clone()
    seen = []
    for i, seed in enumerate((41, 42, 43, 44)):           # eager, capture + replay, replay, replay
        runner.run_iter(_batch(seed), train_mode=True, Labeled=True, Pseudo=False)
        lv = runner.outputs['log_vars']
        assert set(lv) == {'loss_cls', 'loss_bbox', 'loss_noR', 'grad_norm'}, set(lv)
        assert np.isfinite(float(runner.outputs['loss'])) and float(lv['grad_norm']) > 0
        seen.append(getattr(runner, '_graph_step', None) is not None and len(runner._graph_step[1].cache))
    assert seen[0] in (False, 0) and seen[-1] == 1
    assert float((model.module.bbox_head.retina_cls.weight.detach() - w0).abs().max()) > 0


# ------------------------------------------------------------------------------------------------ train, then score
def test_al_driver_two_cycles_on_the_plain_config():
    """tools/train_RetinaNet.py --config Config_RetinaNet_plain.py --uncertainty-pool Coreset on 16 synthetic 64 x 64 images, 2 cycles"""
    wd = f'pytest_plain_retina_{os.getpid()}'
    out = os.path.join(ROOT, 'work_dirs', wd)
    cmd = [sys.executable, os.path.join(ROOT, 'tools/train_RetinaNet.py'), '--config', os.path.join(ROOT, 'configs/_base_/Config_RetinaNet_plain.py'),
           '--uncertainty-pool', 'Coreset', '--synthetic', '16', '--cycles', '2', '--synthetic-size', '64', '--log-interval', '1', '--work-dir', wd]
    try:
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
        text = p.stdout + p.stderr
        for root, _, files in os.walk(out):
            text += ''.join(open(os.path.join(root, f), errors='ignore').read() for f in files if f.endswith('.log'))
        vals = [float(v) for v in re.findall(r'loss_cls: ([-+0-9.eE]+|nan|inf)', text)]
        assert vals and np.isfinite(vals).all(), (vals, text[-2000:])
        assert 'loss_L' not in text and 'mAP' in text
        xl0, xl1 = np.load(os.path.join(out, 'X_L_0.npy')), np.load(os.path.join(out, 'X_L_1.npy'))
        unc = np.load(os.path.join(out, 'Unc_1.npy'))
        assert len(xl1) == len(xl0) + 1 and set(xl0) <= set(xl1) and unc.shape == (16,)
        assert sorted(unc[unc > 0].tolist()) == [1.0] and set(np.nonzero(unc)[0]) == set(xl1) - set(xl0)          # the pick is the selection
    finally:
        shutil.rmtree(out, ignore_errors=True)


def _member_state(sd, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: (v + v.std() * 0.5 * torch.randn(v.shape, generator=g) if (k.startswith('bbox_head.') and v.dim() == 4 and 'cls' in k) else v.clone())
            for k, v in sd.items()}


def test_pool_passes_on_plain_members(monkeypatch):
    """Ensemble_uncertainty on two plain members against tests/ensemble_mi_util's float64 value within that file's bound; MCDropout_uncertainty,
    Coreset / CDAL run; single_gpu_map == eval_map(single_gpu_test(...)) bit for bit"""
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis.test import _unwrap, single_gpu_map, single_gpu_test
    from aod_meh_hua_amd.core.evaluation import eval_map
    from aod_meh_hua_amd.datasets import build_dataloader, build_dataset
    from aod_meh_hua_amd.mmcv_lite import MMDataParallel
    from tests.ensemble_mi_util import bound, mi_float64, mi_fp32_torch
    from tests.eval_device_util import assert_same_eval
    sd = U.plain_state_dict(cls_bias=1.0)
    models, cfg = [], None
    for s in range(2):
        m, cfg = U.build_plain(ROOT, _member_state(sd, 300 + s), 'cuda')
        models.append(MMDataParallel(m).eval())
    ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=5, size=(U.H, U.W)), dict(test_mode=True))
    dl = build_dataloader(ds, samples_per_gpu=2, workers_per_gpu=0, dist=False, shuffle=False)
    scores, e_ref, totals = [], 0.0, []
    with torch.no_grad():
        for data in dl:
            data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
            outs = [m(return_loss=False, rescale=True, isEval=True, justOut=True, **data) for m in models]
            assert all(isinstance(o, list) and len(o) == 5 and all(t.dtype == torch.float32 and t.shape[1] == U.A * U.C for t in o) for o in outs)
            members = [[t.float().cpu().contiguous().numpy() for t in o] for o in outs]
            want, tm = mi_float64(members, U.C)
            fp32 = mi_fp32_torch([[torch.from_numpy(t) for t in m] for m in members], U.C).double().numpy()
            e_ref = max(e_ref, float(np.abs(fp32 - want).max()))
            scores.append(want), totals.append(tm)
    want, tol = np.concatenate(scores), bound(e_ref, float(np.mean(totals)))
    assert want.shape == (5,) and want.min() > 1e-5                  # the members do disagree
    got = apis.Ensemble_uncertainty(cfg, *models, dl)
    err = np.abs(got.double().numpy() - want).max()
    print(f'ensemble of two plain members: max |pass - float64| = {err:.3e}, bound {tol:.3e}')
    assert got.shape == (5,) and np.isfinite(got.numpy()).all() and err <= tol
    model = models[0]
    mcd = apis.MCDropout_uncertainty(cfg, model, dl, n=3, rate=0.1, seed=5)
    assert mcd.shape == (5,) and torch.isfinite(mcd).all() and float(mcd.min()) > 0
    assert torch.equal(mcd, apis.MCDropout_uncertainty(cfg, model, dl, n=3, rate=0.1, seed=5))
    for fn in (apis.Coreset_uncertainty, apis.CDAL_uncertainty):
        picks = fn(cfg, model, dl, X_L=np.array([0]), budget=2)
        assert picks.shape == (5,) and sorted(picks[picks > 0].tolist()) == [1.0, 2.0] and float(picks[0]) == 0
    res = single_gpu_test(model, dl, isUnc=False)
    anns = [ds.get_ann_info(i) for i in range(len(ds))]
    assert sum(a.shape[0] for img in res for a in img) > 0
    host = eval_map(res, anns, iou_thr=0.5, dataset='voc07', logger='silent')
    for graph in ('1', '0'):
        monkeypatch.setenv('AOD_HIP_GRAPH', graph)
        assert_same_eval(single_gpu_map(model, dl, iou_thr=0.5, dataset='voc07', isUnc=False), host)
