"""Golden for the MEH ablation heads: run the REFERENCE's Lambda_L1Net / Lambda_MSLENet / Lambda_L2Net (loss_single_L) and
Lambda_L2Net_NoL / Lambda_L2Net_ablation (get_bboxes: Entropy_NMS at several (score_thr, iou_thr), Entropy_Avg) on seeded inputs and record
inputs + outputs in tests/golden/meh_variants.npz.

    python tools/golden/make_golden_meh_variants.py

Loss cases (B = 2, A = 9, levels 8x8, 2x3, 1x2; inputs are multiples of 2^-10): lambda = relu(N(0, 1)) (about half exact zeros), loss >= 0,
w in {0, 1}; per level some rows with lambda + 1e-9 == loss in float32 (the L1 tie: gradient 0) and some with lambda = loss = 0.
  loss_lam{l} [B, A, h, w], loss_prev{l} [rows], loss_w{l} [rows] uint8, loss_tie{l} [rows] bool
  {form}_val [3] / {form}_grad{l}: the reference's loss_single_L value per level and its autograd gradient w.r.t. L_score (float32)
  {form}_val64 [3] / {form}_grad64_{l}: tests.meh_variants_util.meh_loss_float64;  {form}_e_val / {form}_e_grad: max |reference - float64|
Scoring cases (the inputs of tests/golden/scoring.npz: synth.planted_heads(2, 128, 128), metas scale 1.25), 20 reseeded runs each:
  {case}_unc_runs [20, B]; {case}_pairs{b} [n, 3] int64 = (level, candidate within the level, object) of ComputeObjUnc in nonzero() order;
  nol_avg_fg_counts [B, L]: foreground rows per (image, level) of ComputeAvgUnc."""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')
import mmcv_shim  # noqa: E402

mmcv_shim.install()
try:
    import cv2  # noqa: F401
except Exception:      # noqa: BLE001
    sys.modules['cv2'] = types.ModuleType('cv2')
from mmdet.models import build_head  # noqa: E402

from tests import synth  # noqa: E402
from tests.meh_variants_util import FORMS, LOSS_A, LOSS_B, LOSS_LEVELS, SCORING_CASES, meh_loss_float64  # noqa: E402

torch.set_num_threads(8)
cfg, ns = mmcv_shim.load_reference_model_cfg('/root/reference/configs/_base_/Config_RetinaNet.py')


def head_of(name):
    hc = cfg.bbox_head.copy()
    hc['type'] = name
    hc['train_cfg'], hc['test_cfg'] = cfg.train_cfg, cfg.test_cfg
    return build_head(hc)


out = {}
# ---------------------------------------------------------------- loss forms
g = torch.Generator().manual_seed(5201)
q = lambda t: torch.round(t * 1024) / 1024
inputs = []
for l, (h, w) in enumerate(LOSS_LEVELS):
    rows = LOSS_B * LOSS_A * h * w
    lam = q(torch.relu(torch.randn(LOSS_B, LOSS_A, h, w, generator=g)))
    prev = q(torch.randn(rows, generator=g).abs() * 0.7)
    wt = (torch.rand(rows, generator=g) > 0.4).float()
    flat = lam.permute(0, 2, 3, 1).reshape(-1)                          # (a copy: the head's row order)
    pos = (flat >= 0.03125).nonzero()[:, 0]
    zer = (flat == 0).nonzero()[:, 0]
    nt = 12 if l == 0 else 4
    tie_rows, zero_rows = pos[:nt], zer[:nt]
    prev[tie_rows] = flat[tie_rows]                                      # lambda + 1e-9 == loss in float32 (1e-9 < ulp / 2)
    prev[zero_rows] = 0.
    wt[tie_rows[: nt // 2]] = 1.
    wt[zero_rows[: nt // 2]] = 1.
    tie = (flat + 1e-9) == prev
    assert int(tie.sum()) >= nt and int(((flat == 0) & (prev == 0)).sum()) >= nt and 0 < wt.sum() < rows
    assert bool((wt[tie] == 1).any()) and bool((prev >= 0).all())
    inputs.append((lam, prev, wt))
    out[f'loss_lam{l}'], out[f'loss_prev{l}'] = lam.numpy(), prev.numpy()
    out[f'loss_w{l}'], out[f'loss_tie{l}'] = wt.numpy().astype(np.uint8), tie.numpy()
assert sum(int(out[f'loss_tie{l}'].sum()) for l in range(3)) >= 8
for form, name in zip(FORMS, ('Lambda_L2Net', 'Lambda_L1Net', 'Lambda_MSLENet')):
    head = head_of(name)
    vals, vals64, e_val, e_grad = [], [], 0.0, 0.0
    for l, (lam, prev, wt) in enumerate(inputs):
        x = lam.clone().requires_grad_(True)
        bw = wt.view(LOSS_B, -1, 1).expand(LOSS_B, wt.numel() // LOSS_B, 4).contiguous()
        loss_L, _ = head.loss_single_L(x, prev, wt.view(LOSS_B, -1), bw)
        loss_L.backward()
        v64, g64 = meh_loss_float64(form, lam.numpy(), prev.numpy(), wt.numpy())
        vals.append(float(loss_L)), vals64.append(v64)
        out[f'{form}_grad{l}'], out[f'{form}_grad64_{l}'] = x.grad.numpy(), g64
        e_val = max(e_val, abs(float(loss_L) - v64))
        e_grad = max(e_grad, float(np.abs(x.grad.numpy().astype(np.float64) - g64).max()))
        if form == 'l1':
            gt = x.grad.permute(0, 2, 3, 1).reshape(-1)
            assert bool((gt[torch.from_numpy(out[f'loss_tie{l}'])] == 0).all())
    out[f'{form}_val'], out[f'{form}_val64'] = np.array(vals, np.float32), np.array(vals64, np.float64)
    out[f'{form}_e_val'], out[f'{form}_e_grad'] = np.float64(e_val), np.float64(e_grad)
    print(form, 'val', vals, 'e_val', e_val, 'e_grad', e_grad)

# ---------------------------------------------------------------- scoring
B, H, W = 2, 128, 128
cls_p, reg_p, L_p = synth.planted_heads(B, H, W)
mt = synth.metas(B, H, W, scale=1.25)
pair_lists = {}
for case, name, sthr, ithr, pool in SCORING_CASES:
    head = head_of(name).eval()
    cap = {}
    if pool == 'Entropy_NMS':
        orig = head.ComputeObjUnc

        def spy(mlvl_cls_scores, pos_bboxes, mlvl_scores, mlvl_Ls, mlvl_idces, _orig=orig, _cap=cap, **kw):
            # the integer facts: (level, candidate, object) of FG_pos_bbox.nonzero() per image, restated from the call's own arguments
            thr = kw.get('score_thr') or 0.3
            pairs = [[] for _ in range(len(pos_bboxes))]
            start = 0
            for s, (raw, sc) in enumerate(zip(mlvl_cls_scores, mlvl_scores)):
                n = sc.shape[1]
                for b in range(len(pos_bboxes)):
                    conf = raw[b].permute(1, 2, 0).reshape(-1, sc.shape[2]).softmax(dim=1).max(dim=1)[0]
                    pb = pos_bboxes[b][start:start + n]
                    if not bool((conf > thr).any()) or len(pb.nonzero()) == 0:
                        continue
                    fg = pb & (sc[b].max(dim=1)[0] > thr)[:, None].expand_as(pb)
                    for c, o in fg.nonzero().tolist():
                        pairs[b].append((s, c, o))
                start += n
            _cap['pairs'] = pairs
            return _orig(mlvl_cls_scores, pos_bboxes, mlvl_scores, mlvl_Ls, mlvl_idces, **kw)
        head.ComputeObjUnc = spy
    else:
        orig = head.ComputeAvgUnc

        def spy_avg(mlvl_cls_scores, L_scores, _orig=orig, _cap=cap):
            _cap['counts'] = [[int((c[b].permute(1, 2, 0).reshape(-1, 20).softmax(dim=1).max(dim=1)[0] > 0.3).sum()) for c in mlvl_cls_scores]
                              for b in range(mlvl_cls_scores[0].shape[0])]
            o = _orig(mlvl_cls_scores, L_scores)
            _cap['levels'] = o
            return o
        head.ComputeAvgUnc = spy_avg
    kw = dict(rescale=True, with_nms=pool == 'Entropy_NMS', isEval=False, isUnc='Epistemic', uPool=pool, uPool2='objectSum_scaleMax_classSum',
              scaleUnc=False, showNMS=False, saveUnc=False, saveMaxConf=False, clsW=False, batchIdx=0, score_thr=sthr, iou_thr=ithr)
    runs = []
    with torch.no_grad():
        for seed in range(20):
            torch.manual_seed(seed)
            _, unc = head.get_bboxes(cls_p, reg_p, mt, L_scores=L_p, **kw)
            runs.append([float(u) for u in unc])
    runs = np.array(runs, np.float64)
    assert np.isfinite(runs).all() and (runs.mean(0) > 0).all(), (case, runs.mean(0))
    out[f'{case}_unc_runs'] = runs
    if pool == 'Entropy_NMS':
        for b in range(B):
            out[f'{case}_pairs{b}'] = np.array(cap['pairs'][b], np.int64).reshape(-1, 3)
        pair_lists[case] = cap['pairs']
        print(case, 'mean', runs.mean(0), 'std', runs.std(0), 'pairs', [len(p) for p in cap['pairs']])
    else:
        counts = np.array(cap['counts'], np.int64)
        # a level counts iff it has a foreground row: check that the reference's `if sUncs:` dropped no level for another reason here
        assert all(bool(cap['levels'][b][l]) == bool(counts[b, l]) for b in range(B) for l in range(counts.shape[1]))
        assert (counts == 0).any(1).any() and (counts > 0).any(1).all(), counts          # a level without rows, and levels with some
        out[f'{case}_fg_counts'] = counts
        print(case, 'mean', runs.mean(0), 'std', runs.std(0), 'fg counts', counts.tolist())
assert pair_lists['nol_030_050'] != pair_lists['nol_030_090'], 'iou_thr does not change the pair lists: the threshold plumbing is not tested'
assert pair_lists['abl_030_090'] != pair_lists['abl_050_050']
assert pair_lists['abl_030_090'] == pair_lists['nol_030_090']
path = os.path.join(ROOT, 'tests', 'golden', 'meh_variants.npz')
np.savez_compressed(path, **out)
size = os.path.getsize(path)
print('meh_variants golden:', size, 'bytes')
assert size <= 150 * 1024, size
