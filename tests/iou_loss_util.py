"""Shared by tests/test_iou_loss_host.py and tests/test_gpu_iou_loss.py: a torch restatement of delta2bbox (delta_xywh_bbox_coder.py:205-246,
no max_shape) + bbox_overlaps(is_aligned=True) (iou2d_calculator.py:212-260) + the IoU / linear IoU / GIoU row losses (iou_loss.py:14-36,
87-102), float64 by default, with the gradients autograd takes -- torch.max(a, b) / torch.min(a, b) / clamp are the very calls of the
reference, so their subgradients (a tie gets half, clamp passes at equality) are the definition the kernels follow.

Two frames: `pixel` decodes both delta rows from real anchors, `anchor` from the unit anchor (-.5, -.5, .5, .5) -- what the kernels do.
tests/test_iou_loss_host.py shows they give the same numbers to 1e-12."""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'iou_box_loss.npz')
FORMS = ('giou', 'iou', 'iou_linear')          # the golden's three cases; (box_form, linear) = ('giou', False), ('iou', False), ('iou', True)
UNIT_ANCHOR = (-0.5, -0.5, 0.5, 0.5)


def split_form(form):
    """'giou' | 'iou' | 'iou_linear' -> (box_form, linear)"""
    return ('iou', True) if form == 'iou_linear' else (form, False)


def max_ratio_f32(wh_ratio_clip):
    """|ln(wh_ratio_clip)| as the library forms it: the clip as fp32, the logarithm in double, rounded to fp32 once"""
    return float(np.float32(abs(math.log(float(np.float32(wh_ratio_clip))))))


def decode(anchors, deltas, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), max_ratio=abs(math.log(16 / 1000))):
    """delta2bbox without max_shape: anchors [n, 4] (x1, y1, x2, y2), deltas [n, 4] -> boxes [n, 4], in deltas' dtype"""
    means, stds = deltas.new_tensor(means), deltas.new_tensor(stds)
    d = deltas * stds + means
    px, py = (anchors[:, 0] + anchors[:, 2]) * 0.5, (anchors[:, 1] + anchors[:, 3]) * 0.5
    pw, ph = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    dw, dh = d[:, 2].clamp(min=-max_ratio, max=max_ratio), d[:, 3].clamp(min=-max_ratio, max=max_ratio)
    gw, gh = pw * dw.exp(), ph * dh.exp()
    gx, gy = px + pw * d[:, 0], py + ph * d[:, 1]
    return torch.stack([gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5], -1)


def overlaps(b1, b2, mode='iou', eps=1e-6):
    """bbox_overlaps(b1, b2, mode, is_aligned=True, eps), mode 'iou' | 'giou'"""
    area1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    area2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    lt, rb = torch.max(b1[:, :2], b2[:, :2]), torch.min(b1[:, 2:], b2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    union = area1 + area2 - overlap
    e = union.new_tensor([eps])
    union = torch.max(union, e)
    ious = overlap / union
    if mode == 'iou':
        return ious
    elt, erb = torch.min(b1[:, :2], b2[:, :2]), torch.max(b1[:, 2:], b2[:, 2:])
    ewh = (erb - elt).clamp(min=0)
    earea = torch.max(ewh[:, 0] * ewh[:, 1], e)
    return ious - (earea - union) / earea


def box_loss(b1, b2, box_form, eps=1e-6, linear=False):
    """the unweighted row loss [n]: iou_loss / giou_loss of iou_loss.py"""
    if box_form == 'giou':
        return 1 - overlaps(b1, b2, 'giou', eps)
    ious = overlaps(b1, b2, 'iou').clamp(min=eps)
    return 1 - ious if linear else -ious.log()


def rows(pred, tgt, box_form, eps=1e-6, linear=False, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), max_ratio=abs(math.log(16 / 1000)),
         anchors=None, dtype=torch.float64):
    """pred / tgt [n, 4] deltas (any float dtype, taken as they are) -> (row loss [n], d sum(loss) / d pred [n, 4], IoU [n]) evaluated in
    `dtype`.  anchors None: the anchor-normalised frame; [n, 4]: the pixel frame."""
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    t = tgt.detach().to(dtype)
    a = torch.tensor([UNIT_ANCHOR], dtype=dtype).expand(p.shape[0], 4) if anchors is None else anchors.detach().to(dtype)
    b1, b2 = decode(a, p, means, stds, max_ratio), decode(a, t, means, stds, max_ratio)
    loss = box_loss(b1, b2, box_form, eps, linear)
    g, = torch.autograd.grad(loss.sum(), p)
    return loss.detach(), g, overlaps(b1, b2, 'iou').detach()


def make_anchors(n, seed=0, dtype=torch.float64):
    """n anchors of aspect 0.5 / 1 / 2 at strides 8 .. 128 (octave scale 4, three scales per octave), centres on a 1 024-pixel image"""
    g = torch.Generator().manual_seed(seed)
    stride = torch.tensor([8., 16., 32., 64., 128.], dtype=dtype)[torch.randint(0, 5, (n,), generator=g)]
    ratio = torch.tensor([0.5, 1.0, 2.0], dtype=dtype)[torch.randint(0, 3, (n,), generator=g)]
    scale = 4.0 * 2.0 ** (torch.randint(0, 3, (n,), generator=g).to(dtype) / 3)
    w, h = stride * scale / ratio.sqrt(), stride * scale * ratio.sqrt()
    cx, cy = torch.rand(n, generator=g, dtype=dtype) * 1024, torch.rand(n, generator=g, dtype=dtype) * 1024
    return torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1)
