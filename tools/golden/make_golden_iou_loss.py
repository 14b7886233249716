"""Golden for the IoU / GIoU box losses on decoded boxes: run the REFERENCE's own MyRetinaHead (CPU) with reg_decoded_bbox=True and
GIoULoss(loss_weight=1.0), IoULoss() and IoULoss(linear=True) on the seeded inputs of tests/plain_retina_util.py (the inputs of
tests/golden/plain_retina.npz) and record the numbers in tests/golden/iou_box_loss.npz.

    python tools/golden/make_golden_iou_loss.py

C = 20, 2 images of 64 x 64: levels 8^2, 4^2, 2^2, 1^2, 1^2 with 9 anchors (1 152 / 288 / 72 / 18 / 18 rows).
  reg{l} [B, A*4, h, w]: the box maps (tests.plain_retina_util.make_maps; the cls maps are those of plain_retina.npz)
  gt_boxes{b}, gt_labels{b}: synth.random_gts(2, 64, 64, seed=24, gmin=1, gmax=3)
  anchors{l} [A_l, 4], bt{l} [B, A_l, 4] (with reg_decoded_bbox the targets are the ground-truth BOXES, anchor_head.py:220-224), bw{l},
  labels{l}, num_total_samples: what head.loss() computed (head_out)
  per form f in giou | iou | iou_linear: loss_bbox_{f} [5] (loss()'s per-level terms), grad_reg{l}_{f} = d sum(loss_bbox) / d reg{l}
Data only: no program text of the reference is stored."""
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

from tests import iou_loss_util as IU  # noqa: E402
from tests import plain_retina_util as U  # noqa: E402
from tests import synth  # noqa: E402

torch.set_num_threads(8)
cfg, ns = mmcv_shim.load_reference_model_cfg('/root/reference/configs/_base_/Config_RetinaNet.py')
npy = lambda t: t.detach().cpu().numpy()
out = {}
cls, reg = U.make_maps()
gtb, gtl = synth.random_gts(U.B, U.H, U.W, seed=24, gmin=1, gmax=3)
metas = synth.metas(U.B, U.H, U.W)
for b in range(U.B):
    out[f'gt_boxes{b}'], out[f'gt_labels{b}'] = npy(gtb[b]), npy(gtl[b])
LOSSES = dict(giou=dict(type='GIoULoss', loss_weight=1.0), iou=dict(type='IoULoss'), iou_linear=dict(type='IoULoss', linear=True))
for form in IU.FORMS:
    hc = dict(cfg.bbox_head)
    hc.update(type='MyRetinaHead', reg_decoded_bbox=True, loss_bbox=LOSSES[form],
              loss_cls=dict(type='FocalLoss', last_activation='sigmoid', gamma=2.0, alpha=0.25, loss_weight=1.0),
              train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    head = build_head(hc)
    assert type(head).__name__ == 'MyRetinaHead' and head.reg_decoded_bbox and type(head.loss_bbox).__name__ == LOSSES[form]['type']
    rs = [r.clone().requires_grad_(True) for r in reg]
    losses, head_out = head.loss([c.clone() for c in cls], rs, gtb, gtl, metas, Labeled=True, Pseudo=False)
    sum(losses['loss_bbox']).backward()
    out[f'loss_bbox_{form}'] = np.array([float(t) for t in losses['loss_bbox']], np.float32)
    for l in range(len(U.LEVELS)):
        out[f'grad_reg{l}_{form}'] = npy(rs[l].grad)
    if form == IU.FORMS[0]:
        out['num_total_samples'] = np.int64(head_out[8])
        for l in range(len(U.LEVELS)):
            out[f'reg{l}'] = npy(reg[l])
            out[f'anchors{l}'] = npy(head_out[3][l][0])
            out[f'labels{l}'] = npy(head_out[4][l])
            out[f'bt{l}'], out[f'bw{l}'] = npy(head_out[6][l]), npy(head_out[7][l])
    print(form, 'loss_bbox', out[f'loss_bbox_{form}'])
# keep away from where the pixel and the anchor frame differ: no degenerate ground truth, no clamped size, IoU well above eps
npos = 0
for l in range(len(U.LEVELS)):
    bt, bw = out[f'bt{l}'].reshape(-1, 4), out[f'bw{l}'].reshape(-1, 4)
    pos = bw[:, 0] > 0
    npos += int(pos.sum())
    if pos.any():
        assert (bt[pos, 2] - bt[pos, 0]).min() > 1 and (bt[pos, 3] - bt[pos, 1]).min() > 1
    assert np.abs(out[f'reg{l}']).max() < 1.0
assert npos > 0 and int(out['num_total_samples']) >= npos
print('positives', npos, 'num_total_samples', int(out['num_total_samples']))
np.savez_compressed(IU.GOLDEN, **out)
size = os.path.getsize(IU.GOLDEN)
print('iou_box_loss golden:', size, 'bytes')
assert size <= 600 * 1024, size
