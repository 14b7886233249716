"""Golden for the plain RetinaNet baseline: run the REFERENCE's own MyRetinaHead + FocalLoss (CPU) on the seeded inputs of
tests/plain_retina_util.py and record inputs + outputs in tests/golden/plain_retina.npz.

    python tools/golden/make_golden_plain_retina.py

C = 20, 2 images of 64 x 64: levels 8^2, 4^2, 2^2, 1^2, 1^2 with 9 anchors (1 152 / 288 / 72 / 18 / 18 rows).
  cls{l} [B, A*C, h, w], reg{l} [B, A*4, h, w]: the inputs (logits in [-5, 5], tests.plain_retina_util.make_maps);
  gt_boxes{b}, gt_labels{b}: synth.random_gts(2, 64, 64, seed=24, gmin=1, gmax=3) (the generator make_golden.py uses)
  labels{l}, lw{l}, bt{l}, bw{l}, num_total_samples: the targets head.loss() computed (head_out)
  loss_cls [5], loss_bbox [5], loss_noR{l} [rows]: loss()'s per-level terms and loss_noR rows
  grad_cls{l}, grad_reg{l}: autograd gradients of the _parse_losses total (sum loss_cls + sum loss_bbox + sum_l mean(loss_noR_l)), total
  det{b} [n, 6] (x1, y1, x2, y2, score, label), cand_boxes [B, n, 4], cand_scores [B, n, 21], keep{b}: get_bboxes with nms_pre = 100
    (rescale, scale factor 1.25) and what it handed to multiclass_nms
  state_keys / state_shapes: state_dict of the reference's MyRetinaNet (Config_RetinaNet.py with the three types swapped)."""
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
from mmdet.models import build_detector, build_head  # noqa: E402

from tests import plain_retina_util as U  # noqa: E402
from tests import synth  # noqa: E402

torch.set_num_threads(8)
cfg, ns = mmcv_shim.load_reference_model_cfg('/root/reference/configs/_base_/Config_RetinaNet.py')
cfg.type = 'MyRetinaNet'
cfg.bbox_head['type'] = 'MyRetinaHead'
cfg.bbox_head['loss_cls'] = dict(type='FocalLoss', last_activation='sigmoid', gamma=2.0, alpha=0.25, loss_weight=1.0)
cfg.test_cfg['nms_pre'] = U.NMS_PRE
cfg.test_cfg['uncertainty_pool'] = 'Random'
npy = lambda t: t.detach().cpu().numpy()
out = {}

model = build_detector(cfg)
sd = model.state_dict()
out['state_keys'] = np.array(list(sd.keys()))
out['state_shapes'] = np.array([str(tuple(v.shape)) for v in sd.values()])
head = model.bbox_head
assert type(head).__name__ == 'MyRetinaHead' and type(head.loss_cls).__name__ == 'FocalLoss' and head.cls_out_channels == U.C

# ---------------------------------------------------------------- loss()
cls, reg = U.make_maps()
gtb, gtl = synth.random_gts(U.B, U.H, U.W, seed=24, gmin=1, gmax=3)
metas = synth.metas(U.B, U.H, U.W)
xs = [c.clone().requires_grad_(True) for c in cls]
rs = [r.clone().requires_grad_(True) for r in reg]
losses, head_out = head.loss(xs, rs, gtb, gtl, metas, Labeled=True, Pseudo=False)
total = sum(losses['loss_cls']) + sum(losses['loss_bbox']) + sum(t.mean() for t in losses['loss_noR'])
total.backward()
for b in range(U.B):
    out[f'gt_boxes{b}'], out[f'gt_labels{b}'] = npy(gtb[b]), npy(gtl[b])
out['loss_cls'] = np.array([float(t) for t in losses['loss_cls']], np.float32)
out['loss_bbox'] = np.array([float(t) for t in losses['loss_bbox']], np.float32)
out['total'] = np.float32(float(total))
out['num_total_samples'] = np.int64(head_out[8])
for l in range(len(U.LEVELS)):
    out[f'cls{l}'], out[f'reg{l}'] = npy(cls[l]), npy(reg[l])
    out[f'labels{l}'], out[f'lw{l}'] = npy(head_out[4][l]), npy(head_out[5][l])
    out[f'bt{l}'], out[f'bw{l}'] = npy(head_out[6][l]), npy(head_out[7][l])
    out[f'loss_noR{l}'] = npy(losses['loss_noR'][l])
    out[f'grad_cls{l}'], out[f'grad_reg{l}'] = npy(xs[l].grad), npy(rs[l].grad)
    assert out[f'loss_noR{l}'].shape == (U.LEVEL_ROWS[l],)
npos = sum(int((out[f'labels{l}'] < U.C).sum()) for l in range(len(U.LEVELS)))
assert npos > 0 and int(out['num_total_samples']) >= npos
# the reference's CPU path (py_sigmoid_focal_loss) against the float64 evaluation of mmcv's formula: the error the tolerances budget for
e_row = e_grad = 0.0
for l, li in enumerate(U.golden_level_inputs(out)):
    l64, g64 = U.focal64(li['cls'].numpy(), li['labels'].numpy())
    e_row = max(e_row, float(np.abs(out[f'loss_noR{l}'] - l64.sum(-1)).max()))
print('reference rows vs float64: max abs err', e_row, ' positives', npos, ' num_total_samples', int(out['num_total_samples']))

# ---------------------------------------------------------------- get_bboxes()
import mmdet.models.dense_heads.anchor_head as AHmod  # noqa: E402

cap = {}
orig_nms = AHmod.multiclass_nms


def spy_nms(*a, **k):
    r = orig_nms(*a, **k)
    cap.setdefault('keep', []).append(r[2].clone())
    cap.setdefault('nms_in', []).append((a[0].clone(), a[1].clone()))
    return r


AHmod.multiclass_nms = spy_nms
head.eval()
mt = synth.metas(U.B, U.H, U.W, scale=1.25)
with torch.no_grad():
    dets = head.get_bboxes(cls, reg, mt, rescale=True, with_nms=True, isEval=True, isUnc=False)
AHmod.multiclass_nms = orig_nms
for b, (d, lab) in enumerate(dets):
    out[f'det{b}'] = npy(torch.cat([d, lab[:, None].float()], 1))
    out[f'keep{b}'] = npy(cap['keep'][b])
    assert d.shape[0] > 0, 'no detections: the case tests nothing'
out['cand_boxes'] = npy(torch.stack([x[0] for x in cap['nms_in']]))
out['cand_scores'] = npy(torch.stack([x[1] for x in cap['nms_in']]))
assert out['cand_scores'].shape == (U.B, sum(U.CAND_PER_LEVEL), U.C + 1)
for l in range(len(U.LEVELS)):
    assert U.keys_separated(U.level_keys64(out[f'cls{l}']))
print('detections per image:', [len(out[f'det{b}']) for b in range(U.B)])

path = U.GOLDEN
np.savez_compressed(path, **out)
size = os.path.getsize(path)
print('plain_retina golden:', size, 'bytes')
assert size <= 600 * 1024, size
