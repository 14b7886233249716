"""GPU tests of the MEH ablation heads (Lambda_L1Net / Lambda_MSLENet / Lambda_L2Net_ablation / Lambda_L2Net_NoL) against what the REFERENCE
recorded for them (tests/golden/meh_variants.npz) and the restatements of tests/meh_variants_util.py: the L1 / MSLE loss forms (value,
gradient, exact zeros, determinism), the threshold kwargs and the lambda-free alpha of HUA (integer-exact pair lists, per-pair values,
statistics), the Entropy_Avg pool, graph capture with every new head, and two small end-to-end driver runs.

Every figure a bound is set on is printed before it is asserted (run with -s); DESIGN 3g holds the bounds' sources."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import hua as ohua
from oracle import model as omodel
from tests import synth
from tests.meh_variants_util import FORMS, LOSS_A, LOSS_B, LOSS_LEVELS, SCORING_CASES, avg_unc_philox, meh_loss_float64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
HEAD_OF_FORM = {'l2': 'Lambda_L2Net', 'l1': 'Lambda_L1Net', 'msle': 'Lambda_MSLENet'}
LVL_START = [0, 1000, 1576, 1720, 1756, 1765]          # candidates of the planted 128 x 128 batch (nms_pre = 1000)
UPOOL2 = 'objectSum_scaleMax_classSum'


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'meh_variants.npz'))


def _head(name):
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_head
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    hc = dict(cfg.model.bbox_head)
    hc['type'] = name
    return build_head(dict(hc, train_cfg=cfg.model.train_cfg, test_cfg=cfg.model.test_cfg)).cuda()


# ------------------------------------------------------------------------------------------------ loss forms
def _loss_inputs(gold):
    """The loss fixture as the training step lays it out: every operand of all levels in ONE buffer, the levels adjacent row ranges of it
    (L_score views are channels_last [B, A, h, w], as the level-batched prediction conv writes them)."""
    pix = [LOSS_B * h * w for h, w in LOSS_LEVELS]
    lam_buf = torch.cat([torch.from_numpy(np.ascontiguousarray(np.transpose(gold[f'loss_lam{l}'], (0, 2, 3, 1)))).reshape(-1, LOSS_A)
                         for l in range(len(pix))]).cuda().requires_grad_(True)
    prev_buf = torch.cat([torch.from_numpy(gold[f'loss_prev{l}']) for l in range(len(pix))]).cuda()
    w_all = torch.cat([torch.from_numpy(gold[f'loss_w{l}'].astype(np.float32)) for l in range(len(pix))]).cuda()
    bw_buf = w_all[:, None].expand(-1, 4).contiguous()
    L_scores, prevs, bws, lws, r = [], [], [], [], 0
    for (h, w), p in zip(LOSS_LEVELS, pix):
        L_scores.append(lam_buf[r:r + p].view(LOSS_B, h, w, LOSS_A).permute(0, 3, 1, 2))
        prevs.append(prev_buf[r * LOSS_A:(r + p) * LOSS_A])
        bws.append(bw_buf[r * LOSS_A:(r + p) * LOSS_A].view(LOSS_B, -1, 4))
        lws.append(w_all[r * LOSS_A:(r + p) * LOSS_A].view(LOSS_B, -1))
        r += p
    return lam_buf, L_scores, prevs, bws, lws


def _grad_levels(lam_buf):
    g, out, r = lam_buf.grad.detach().cpu().numpy().astype(np.float64), [], 0
    for h, w in LOSS_LEVELS:
        p = LOSS_B * h * w
        out.append(np.transpose(g[r:r + p].reshape(LOSS_B, h, w, LOSS_A), (0, 3, 1, 2)))
        r += p
    return out


def test_form_0_entry_points_are_bit_equal_to_the_old_ones(gold):
    from aod_meh_hua_amd import _C
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd._C import call, ptr, stream
    lam_buf, _, _, _, _ = _loss_inputs(gold)
    lam = lam_buf.detach().reshape(-1).contiguous()
    prev = torch.cat([torch.from_numpy(gold[f'loss_prev{l}']) for l in range(3)]).cuda()
    bw = torch.cat([torch.from_numpy(gold[f'loss_w{l}'].astype(np.float32)) for l in range(3)]).cuda()[:, None].expand(-1, 4).contiguous()
    rows = [LOSS_B * LOSS_A * h * w for h, w in LOSS_LEVELS]
    lr = ho._level_rows(rows)
    old = ho.meh_loss_levels_fwd(lam, prev, bw, rows)
    new = torch.empty_like(old)
    part = torch.empty(max(int(_C.lib.aod_loss_levels_partials_len(3, lr)), 1), device='cuda')
    call('aod_meh_loss_levels_fwd_ex', ptr(lam), ptr(prev), ptr(bw), 3, lr, 0, ptr(new), ptr(part), stream())
    assert torch.equal(old, new)
    gm = torch.tensor([0.7, 1.3, 0.9], device='cuda')
    for bf16 in (0, 1):
        dt = torch.bfloat16 if bf16 else torch.float32
        a, b = torch.zeros(lam.numel() // LOSS_A, LOSS_A, dtype=dt, device='cuda'), torch.zeros(lam.numel() // LOSS_A, LOSS_A, dtype=dt, device='cuda')
        call('aod_meh_loss_levels_bwd', ptr(lam), ptr(prev), ptr(bw), 3, lr, ptr(gm), ptr(a), bf16, LOSS_A, LOSS_A, stream())
        call('aod_meh_loss_levels_bwd_ex', ptr(lam), ptr(prev), ptr(bw), 3, lr, 0, ptr(gm), ptr(b), bf16, LOSS_A, LOSS_A, stream())
        assert torch.equal(a, b) and float(a.float().abs().sum()) > 0, bf16
    # the single-level pair
    n = rows[0]
    o1, o2 = ho.meh_loss_fwd(lam[:n], prev[:n], bw[:n]), torch.zeros(1, device='cuda')
    part1 = torch.empty(max(int(_C.lib.aod_loss_partials_len(n)), 1), device='cuda')
    call('aod_meh_loss_fwd_ex', ptr(lam), ptr(prev), ptr(bw), n, 0, ptr(o2), ptr(part1), stream())
    assert torch.equal(o1, o2)
    for bf16 in (False, True):
        g1 = ho.meh_loss_bwd(lam[:n], prev[:n], bw[:n], gm[:1].contiguous(), out_bf16=bf16, A=LOSS_A)
        g2 = torch.empty_like(g1)
        call('aod_meh_loss_bwd_ex', ptr(lam), ptr(prev), ptr(bw), n, 0, ptr(gm), ptr(g2), int(bf16), LOSS_A, LOSS_A, stream())
        assert torch.equal(g1, g2)


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('form', FORMS)
def test_loss_forms_value_gradient_zeros_and_determinism(gold, monkeypatch, form, fused):
    """loss_L (all levels in one launch per pass) and loss_single_L (per level) of the new heads against float64: at most 4 x the fixture's
    e_ref (the reference's own float32 error; the margin covers the device's different summation order)."""
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    head = _head(HEAD_OF_FORM[form])
    monkeypatch.setattr(AF, 'LOSS_LEVELS', fused)
    calls = []
    orig = ho.call
    monkeypatch.setattr(ho, 'call', lambda name, *a: (calls.append(name), orig(name, *a))[1])
    e_val, e_grad = float(gold[f'{form}_e_val']), float(gold[f'{form}_e_grad'])
    runs = []
    ho.set_deterministic(True)
    try:
        for _ in range(2):
            lam_buf, L_scores, prevs, bws, lws = _loss_inputs(gold)
            head_out = [None] * 5 + [lws, None, bws]
            out = head.loss_L(L_scores, head_out, prevs)['loss_L']
            vals = torch.stack([v.reshape(()) for v in out])
            vals.sum().backward()
            runs.append((vals.detach().cpu().numpy().astype(np.float64), _grad_levels(lam_buf)))
    finally:
        ho.set_deterministic(False)
    suffix = '' if form == 'l2' else '_ex'
    want = ['aod_meh_loss_levels_fwd' + suffix, 'aod_meh_loss_levels_bwd' + suffix] if fused else ['aod_meh_loss_fwd' + suffix, 'aod_meh_loss_bwd' + suffix]
    assert set(c for c in calls if c.startswith('aod_meh_loss')) == set(want), calls
    vals, grads = runs[0]
    assert np.array_equal(vals, runs[1][0]) and all(np.array_equal(a, b) for a, b in zip(grads, runs[1][1]))     # deterministic mode: same bits
    dv = np.abs(vals - gold[f'{form}_val64']).max()
    dg = max(np.abs(g - gold[f'{form}_grad64_{l}']).max() for l, g in enumerate(grads))
    print(f'MEH {form} fused={fused}: max |value - f64| {dv:.3e} (e_ref {e_val:.3e}), max |grad - f64| {dg:.3e} (e_ref {e_grad:.3e})')
    assert dv <= 4 * e_val, (dv, e_val)
    assert dg <= 4 * e_grad, (dg, e_grad)
    for l, g in enumerate(grads):
        gf = np.transpose(g, (0, 2, 3, 1)).reshape(-1)
        assert (gf[gold[f'loss_w{l}'] == 0] == 0).all()                       # w = 0: exactly 0 for every form
        if form == 'l1':
            tie = gold[f'loss_tie{l}']
            assert tie.any() and (gf[tie] == 0).all()                          # lambda + 1e-9 == loss: abs' = 0
            assert (gf[(gold[f'loss_w{l}'] == 1) & ~tie] != 0).all()


# ------------------------------------------------------------------------------------------------ scoring on the planted batch
@pytest.fixture(scope='module')
def planted():
    cls_p, reg_p, L_p = synth.planted_heads(2, 128, 128)
    mt = synth.metas(2, 128, 128, scale=1.25)
    return dict(cls=[c.cuda() for c in cls_p], reg=[r.cuda() for r in reg_p], L=[l.cuda() for l in L_p], mt=mt, cls_cpu=cls_p)


def _score(head, planted, pool='Entropy_NMS', **kw):
    from aod_meh_hua_amd.mmcv_lite import ConfigDict
    cfg = ConfigDict(nms_pre=1000, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
    with torch.no_grad():
        return head.get_bboxes(planted['cls'], planted['reg'], planted['mt'], cfg=cfg, rescale=True, with_nms=pool == 'Entropy_NMS',
                               L_scores=planted['L'], isUnc='Epistemic', uPool=pool, uPool2=UPOOL2, isEval=False, batchIdx=0,
                               _return_internals=True, **kw)


def _pairs(sc, it, **kw):
    ids = torch.arange(2, device='cuda', dtype=torch.int64)
    unc, pc, pout = sc.hua_score(it['cand'], it['dets'], it['num'], ids, 100, want_pairs=True, seed=20, **kw)
    return unc, pc.cpu().tolist(), pout.cpu().numpy()


@pytest.fixture(scope='module')
def heads():
    return {n: _head(n) for n in ('Lambda_L2Net', 'Lambda_L2Net_NoL', 'Lambda_L2Net_ablation')}


def test_scaled_lam_mode_is_bit_equal_to_the_call_without_it(heads, planted):
    from aod_meh_hua_amd import scoring as sc
    _, unc, it = _score(heads['Lambda_L2Net'], planted)
    ids = torch.arange(2, device='cuda', dtype=torch.int64)
    for est in ('mc', 'closed'):
        a = sc.hua_score(it['cand'], it['dets'], it['num'], ids, 100, seed=20, estimator=est)
        b = sc.hua_score(it['cand'], it['dets'], it['num'], ids, 100, seed=20, estimator=est, lam_mode='scaled')
        assert torch.equal(a, b) and float(a.min()) > 0, est
        if est == 'mc':
            assert torch.equal(a, unc)
    # the default head ignores the threshold kwargs (its reference does): same pairs, same bits
    _, unc2, it2 = _score(heads['Lambda_L2Net'], planted, score_thr=0.5, iou_thr=0.9)
    assert torch.equal(unc, unc2) and torch.equal(it['cand'].any_fg, it2['cand'].any_fg)


@pytest.mark.parametrize('case', [c for c in SCORING_CASES if c[4] == 'Entropy_NMS'], ids=lambda c: c[0])
def test_threshold_kwargs_and_pair_lists_are_integer_exact(gold, heads, planted, case):
    from aod_meh_hua_amd import scoring as sc
    name, head_name, sthr, ithr, _ = case
    head = heads[head_name]
    _, unc, it = _score(head, planted, score_thr=sthr, iou_thr=ithr)
    assert it['cand'].level_start == LVL_START
    kw = dict(obj_score_thr=sthr, obj_iou_thr=ithr, fg_thr=sthr, lam_mode=head._hua_lam)
    unc_d, pc, pout = _pairs(sc, it, **kw)
    assert torch.equal(unc, unc_d)                                             # score_batch hands exactly these to the kernel
    for b in range(2):
        exp = gold[f'{name}_pairs{b}']
        got = pout[b, :pc[b]]
        assert pc[b] == len(exp) > 0, (b, pc[b], len(exp))
        assert np.array_equal(got[:, 0].astype(np.int64), exp[:, 1] + np.asarray(LVL_START)[exp[:, 0]]), b      # nonzero() order
        assert np.array_equal(got[:, 1].astype(np.int64), exp[:, 2]), b
    # image scores against the reference's 20 reseeded runs: 4 sigma + 2 %
    mu, sd = gold[f'{name}_unc_runs'].mean(0), gold[f'{name}_unc_runs'].std(0)
    ids = torch.arange(2, device='cuda', dtype=torch.int64)
    vals = []
    for seed in (1, 2, 3, 20):
        u = sc.hua_score(it['cand'], it['dets'], it['num'], ids, 100, seed=seed, **kw).cpu().numpy().astype(np.float64)
        print(name, 'seed', seed, 'unc', u, 'reference mean', mu, 'std', sd)
        assert (np.abs(u - mu) <= 4 * sd + 0.02 * mu).all(), (seed, u, mu, sd)
        vals.append(u)
    assert np.std(np.stack(vals), 0).max() > 0


def test_lambda_free_pair_values_vs_philox_and_closed_form(heads, planted):
    """Lambda_L2Net_NoL at (0.3, 0.9): per pair alpha = the candidate's scores as they are."""
    from aod_meh_hua_amd import scoring as sc
    _, unc, it = _score(heads['Lambda_L2Net_NoL'], planted, score_thr=0.3, iou_thr=0.9)
    kw = dict(obj_score_thr=0.3, obj_iou_thr=0.9, fg_thr=0.3, lam_mode='none')
    _, pc, pout = _pairs(sc, it, **kw)
    _, cpc, cpout = _pairs(sc, it, estimator='closed', **kw)
    _, spc, spout = _pairs(sc, it, obj_score_thr=0.3, obj_iou_thr=0.9, fg_thr=0.3)            # lambda-scaled: same pairs, other values
    scores = it['cand'].scores.cpu().numpy()
    anchor = it['cand'].cand_anchor.cpu().numpy()
    for b in range(2):
        got = pout[b, :pc[b]]
        c, o = got[:, 0].astype(np.int64), got[:, 1].astype(np.int64)
        alpha = scores[b, c, :20]
        ale, epi = ohua.philox_dirichlet_stats(alpha, b, anchor[b, c], o, 20, 500)
        err_e, err_a = np.abs(got[:, 3] - epi), np.abs(got[:, 2] - ale)
        print('NoL pair epi err: median', np.median(err_e), 'max', err_e.max(), '| ale err max', err_a.max())
        assert np.median(err_e) < 2e-5 and (err_e < 5e-3).all(), (np.median(err_e), err_e.max())
        assert np.median(err_a) < 2e-5 and (err_a < 5e-3).all(), (np.median(err_a), err_a.max())
        # closed form in float64 (alpha > 0 everywhere: softmax)
        a64 = alpha.astype(np.float64)
        S = a64.sum(-1, keepdims=True)
        from scipy.special import digamma
        ale64 = digamma(S[:, 0] + 1) - ((a64 / S) * digamma(a64 + 1)).sum(-1)
        epi64 = -((a64 / S) * np.log(a64 / S)).sum(-1) - ale64
        cg = cpout[b, :cpc[b]]
        assert cpc[b] == pc[b] and np.array_equal(cg[:, :2], got[:, :2])
        assert (np.abs(cg[:, 3] - epi64) <= 1e-5 + 1e-5 * np.abs(epi64)).all(), np.abs(cg[:, 3] - epi64).max()
        assert (np.abs(cg[:, 2] - ale64) <= 1e-5 + 1e-5 * np.abs(ale64)).all(), np.abs(cg[:, 2] - ale64).max()
        sg = spout[b, :spc[b]]
        assert spc[b] == pc[b] and np.array_equal(sg[:, :2], got[:, :2]) and not np.allclose(sg[:, 3], got[:, 3])


# ------------------------------------------------------------------------------------------------ Entropy_Avg
def _avg_inputs(planted):
    """the planted batch + a third image whose logits sit at the prior (no row above 0.3)"""
    cls3 = [torch.cat([c, torch.zeros_like(c[:1])]) for c in planted['cls']]
    reg3 = [torch.cat([r, torch.zeros_like(r[:1])]) for r in planted['reg']]
    L3 = [torch.cat([l, torch.full_like(l[:1], 0.1)]) for l in planted['L']]
    return cls3, reg3, L3, synth.metas(3, 128, 128, scale=1.25)


def _avg(head, cls, reg, L, mt, ids, **kw):
    from aod_meh_hua_amd.mmcv_lite import ConfigDict
    cfg = ConfigDict(nms_pre=1000, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
    with torch.no_grad():
        return head.get_bboxes(cls, reg, mt, cfg=cfg, rescale=True, with_nms=False, L_scores=L, isUnc='Epistemic', uPool='Entropy_Avg',
                               uPool2=UPOOL2, isEval=False, image_ids=ids, _return_internals=True, **kw)


def test_entropy_avg_counts_values_statistics_and_partition_invariance(gold, heads, planted):
    from aod_meh_hua_amd import scoring as sc
    head = heads['Lambda_L2Net_NoL']
    cls3, reg3, L3, mt3 = _avg_inputs(planted)
    ids = torch.arange(3, device='cuda', dtype=torch.int64)
    _, unc, it = _avg(head, cls3, reg3, L3, mt3, ids, score_thr=0.3, iou_thr=0.9)
    cand = it['cand']
    u = unc.cpu().numpy().astype(np.float64)
    # foreground rows per (image, level): the pairs the kernel formed
    _, pc, pout = sc.hua_score(cand, None, None, ids, 1, (0, 0, 0), False, num_samples=50, seed=20, scale_mode='avg', lam_mode='none', want_pairs=True)
    pc, pout = pc.cpu().tolist(), pout.cpu().numpy()
    ls = np.asarray(cand.level_start)
    counts = np.array([[int(((pout[b, :pc[b], 0] >= ls[l]) & (pout[b, :pc[b], 0] < ls[l + 1])).sum()) for l in range(5)] for b in range(3)])
    assert np.array_equal(counts[:2], gold['nol_avg_fg_counts']) and (counts[2] == 0).all()
    assert u[2] == 0.0                                                          # nothing above 0.3: exactly 0 (the reference: NaN)
    # values against the Philox restatement (50 samples, alpha = softmax row, pseudo object 0)
    exp, ecounts, _ = avg_unc_philox([c.cpu().numpy() for c in cls3], 20, seed=20, image_ids=[0, 1, 2])
    assert np.array_equal(ecounts, counts)
    print('Entropy_Avg', u, 'philox restatement', exp, 'reference mean', gold['nol_avg_unc_runs'].mean(0), 'std', gold['nol_avg_unc_runs'].std(0))
    assert (np.abs(u - exp) <= 5e-3).all(), (u, exp)
    scores, anchor = cand.scores.cpu().numpy(), cand.cand_anchor.cpu().numpy()
    for b in range(2):                                                          # and pair by pair, at the tolerance of the scaled mode's test
        c = pout[b, :pc[b], 0].astype(np.int64)
        assert (pout[b, :pc[b], 1] == 0).all()
        _, epi = ohua.philox_dirichlet_stats(scores[b, c, :20], b, anchor[b, c], np.zeros(len(c), np.int64), 20, 50)
        err = np.abs(pout[b, :pc[b], 3] - epi)
        print('Entropy_Avg pair epi err: median', np.median(err), 'max', err.max())
        assert np.median(err) < 2e-5 and (err < 5e-3).all(), (np.median(err), err.max())
    # statistics against the reference's 20 runs of 50 samples: 4 sigma + 2 %, sigma from the fixture
    mu, sd = gold['nol_avg_unc_runs'].mean(0), gold['nol_avg_unc_runs'].std(0)
    for seed in (1, 2, 3, 20):
        _, us, _ = _avg(head, cls3, reg3, L3, mt3, ids, hua_seed=seed)
        us = us.cpu().numpy().astype(np.float64)
        assert (np.abs(us[:2] - mu) <= 4 * sd + 0.02 * mu).all(), (seed, us, mu, sd)
    # one by one (as another rank would), under other batch positions: the same bits
    for b in range(3):
        _, u1, _ = _avg(head, [c[b:b + 1].contiguous() for c in cls3], [r[b:b + 1].contiguous() for r in reg3],
                        [l[b:b + 1].contiguous() for l in L3], mt3[b:b + 1], ids[b:b + 1].contiguous())
        assert float(u1[0]) == float(unc[b]), (b, float(u1[0]), float(unc[b]))
    # the closed form is offered too: the n -> infinity limit, not the 50-sample value (H(mean of n samples) is biased at finite n)
    _, uc, _ = _avg(head, cls3, reg3, L3, mt3, ids, hua_estimator='closed')
    uc = uc.cpu().numpy()
    print('Entropy_Avg closed', uc)
    assert uc[2] == 0 and (uc[:2] > 0).all() and not np.allclose(uc[:2], u[:2], rtol=1e-3), (uc, u)


def test_entropy_avg_is_refused_by_heads_without_it(heads, planted):
    with pytest.raises(NotImplementedError, match='Lambda_L2Net_ablation'):
        _score(heads['Lambda_L2Net_ablation'], planted, pool='Entropy_Avg')
    with pytest.raises(NotImplementedError, match='Lambda_L2Net'):
        _score(heads['Lambda_L2Net'], planted, pool='Entropy_Avg')


# ------------------------------------------------------------------------------------------------ graphs
def _build(head_type, pool=None):
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    from aod_meh_hua_amd.optim import FusedSGD
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg.model.backbone.pop('init_cfg')
    cfg.model.bbox_head.type = head_type
    if pool:
        cfg.model.test_cfg.uncertainty_pool = pool
    model = build_detector(cfg.model)
    model.load_state_dict(omodel.seeded_state_dict(cls_bias=-2.0), strict=True)
    model = model.cuda().train()
    head = model.bbox_head
    meh = set(id(p) for n in ('retina_L', 'L_convs') for p in getattr(head, n).parameters())
    opt = FusedSGD([p for p in model.parameters() if p.requires_grad and id(p) not in meh], lr=2e-4, momentum=0.9, weight_decay=1e-4)
    opt_L = FusedSGD([p for p in model.parameters() if id(p) in meh], lr=2e-4, momentum=0.9, weight_decay=1e-4)
    return model, opt, opt_L


def _batch(seed, B=2, H=128):
    gtb, gtl = synth.random_gts(B, H, H, seed=seed, gmin=1, gmax=3)
    return dict(img=synth.images(B, H, H, seed=seed).cuda(), img_metas=synth.metas(B, H, H), gt_bboxes=gtb, gt_labels=gtl)


@pytest.mark.parametrize('head_type', ['Lambda_L1Net', 'Lambda_MSLENet', 'Lambda_L2Net_NoL', 'Lambda_L2Net_ablation'])
def test_graphed_train_step_captures_and_replays_with_each_head(head_type):
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd.graphs import GraphedTrainStep
    AF.set_deterministic(True)
    try:
        batches = [_batch(31), _batch(32), _batch(33)]
        model, opt, opt_L = _build(head_type)
        ref = []
        for d in batches:
            out, head_out, feat_out, prev = model.train_step(d, Labeled=True, Pseudo=False)
            rode = model.bbox_head._L_pre is not None
            opt.zero_grad()
            out['loss'].backward()
            opt.step()
            lossL = model.train_step_L(prev, head_out, feat_out)
            opt_L.zero_grad()
            lossL['loss'].backward()
            opt_L.step()
            ref.append((float(out['loss'].detach()), float(lossL['loss'].detach())))
        # the MEH rider is a forward matter: it engages exactly where it does for the default head
        base, _, _ = _build('Lambda_L2Net')
        base.train_step(batches[0], Labeled=True, Pseudo=False)
        assert rode == (base.bbox_head._L_pre is not None)
        model2, opt2, opt_L2 = _build(head_type)
        gs = GraphedTrainStep(model2, opt2, opt_L2, warmup=1, Labeled=True, Pseudo=False)
        got = []
        for d in batches:
            o = gs(d)
            got.append((float(o['loss']), float(o['log_vars']['loss_L'])))
        torch.cuda.synchronize()
        assert np.isfinite(np.array(got)).all() and np.allclose(np.array(got), np.array(ref), rtol=2e-3), (got, ref)
    finally:
        AF.set_deterministic(False)


@pytest.mark.parametrize('head_type,pool', [('Lambda_L2Net_NoL', 'Entropy_Avg'), ('Lambda_L2Net_NoL', 'Entropy_NMS'), ('Lambda_L2Net_ablation', 'Entropy_NMS')])
def test_graphed_score_equals_eager_with_the_new_heads_and_pool(head_type, pool):
    from aod_meh_hua_amd.graphs import GraphedScore
    model, _, _ = _build(head_type, pool)
    model.eval()
    kw = dict(rescale=True, isEval=False, isUnc='Epistemic', uPool=pool, uPool2=UPOOL2, scaleUnc=False, showNMS=False, saveUnc=False,
              saveMaxConf=False, clsW=False, batchIdx=0, score_thr=0.3, iou_thr=0.9)
    gsc = GraphedScore(model, **kw)
    assert gsc.pipe == (os.environ.get('AOD_SCORE_PIPELINE', '1') != '0')        # the two-graph pipeline serves the new pool too
    metas = synth.metas(2, 128, 128)
    for seed in (41, 42, 43):
        img = synth.images(2, 128, 128, seed=seed).cuda()
        ids = torch.tensor([seed * 2, seed * 2 + 1], device='cuda')
        with torch.no_grad():
            _, unc_e = model(img=[img], img_metas=[metas], return_loss=False, image_ids=ids, **kw)
        _, unc_g = gsc(img, metas, ids)
        ue, ug = torch.as_tensor(unc_e).float().cpu(), unc_g.float().cpu()
        print(head_type, pool, 'seed', seed, 'eager', ue.tolist(), 'replay', ug.tolist())
        assert torch.isfinite(ue).all() and torch.equal(ue, ug), (seed, ue, ug)


# ------------------------------------------------------------------------------------------------ end to end
def test_al_driver_two_cycles_with_the_ablation_heads():
    """tools/train_RetinaNet.py on a 16-image synthetic pool, 2 cycles: Lambda_MSLENet, then Lambda_L2Net_NoL with the Entropy_Avg pool (the
    second child starts only after the first passed; each under its own time limit)."""
    for extra in (['--bbox-head', 'Lambda_MSLENet'], ['--bbox-head', 'Lambda_L2Net_NoL', '--uncertainty-pool', 'Entropy_Avg']):
        wd = f'pytest_meh_variants_{extra[1]}_{os.getpid()}'
        out = os.path.join(ROOT, 'work_dirs', wd)
        cmd = [sys.executable, os.path.join(ROOT, 'tools/train_RetinaNet.py'), '--synthetic', '16', '--cycles', '2', '--synthetic-size', '128',
               '--log-interval', '1', '--work-dir', wd] + extra
        try:
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, (extra, p.stdout[-1500:], p.stderr[-3000:])
            text = p.stdout + p.stderr
            for root, _, files in os.walk(out):
                text += ''.join(open(os.path.join(root, f), errors='ignore').read() for f in files if f.endswith('.log'))
            vals = [float(v) for v in re.findall(r'loss_L: ([-+0-9.eE]+|nan|inf)', text)]
            assert vals and np.isfinite(vals).all(), (extra, vals, text[-2000:])
            xl0, xl1 = np.load(os.path.join(out, 'X_L_0.npy')), np.load(os.path.join(out, 'X_L_1.npy'))
            unc = np.load(os.path.join(out, 'Unc_1.npy'))
            assert len(xl1) > len(xl0) and set(xl0) <= set(xl1) and unc.shape == (16,) and np.isfinite(unc).all(), (extra, unc)
        finally:
            shutil.rmtree(out, ignore_errors=True)
