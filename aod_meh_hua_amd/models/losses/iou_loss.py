"""IoULoss / GIoULoss plugins (mmdet/models/losses/iou_loss.py:14-36, 87-102, 220-366; losses/utils.py:28-100) on decoded
(x1, y1, x2, y2) boxes, with the reference's constructor and call signature.  `forward` is plain torch and runs wherever its tensors live:
it is the public API for stand-alone callers.  On the RetinaNet hot path (reg_decoded_bbox=True on Lambda_L2Net / MyRetinaHead) the same
row terms are a box form of the fused focal + box kernels (functional.RetinaLossFn, hipops.BOX_FORMS), which decode the two
delta rows themselves.  DIoU / CIoU / bounded IoU are not built: they are not invariant under the anisotropic scaling the kernels rest on."""
import torch
import torch.nn as nn

from ..builder import LOSSES
from .smooth_l1_loss import weight_reduce_loss


def aligned_overlaps(b1, b2, mode='iou', eps=1e-6):
    """bbox_overlaps(b1, b2, mode, is_aligned=True, eps) of iou2d_calculator.py:212-260 for [n, 4] boxes: IoU or GIoU per row"""
    area1 = (b1[..., 2] - b1[..., 0]) * (b1[..., 3] - b1[..., 1])
    area2 = (b2[..., 2] - b2[..., 0]) * (b2[..., 3] - b2[..., 1])
    lt, rb = torch.max(b1[..., :2], b2[..., :2]), torch.min(b1[..., 2:], b2[..., 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = area1 + area2 - overlap
    e = union.new_tensor([eps])
    union = torch.max(union, e)
    ious = overlap / union
    if mode == 'iou':
        return ious
    if mode != 'giou':
        raise ValueError(f"aligned_overlaps: mode must be 'iou' or 'giou', got {mode!r}")
    elt, erb = torch.min(b1[..., :2], b2[..., :2]), torch.max(b1[..., 2:], b2[..., 2:])
    ewh = (erb - elt).clamp(min=0)
    earea = torch.max(ewh[..., 0] * ewh[..., 1], e)
    return ious - (earea - union) / earea


def iou_loss(pred, target, linear=False, eps=1e-6):
    ious = aligned_overlaps(pred, target, 'iou').clamp(min=eps)
    return 1 - ious if linear else -ious.log()


def giou_loss(pred, target, eps=1e-7):
    return 1 - aligned_overlaps(pred, target, 'giou', eps)


def _weighted(loss_fn, self, pred, target, weight, avg_factor, reduction_override, **kwargs):
    if reduction_override not in (None, 'none', 'mean', 'sum'):
        raise ValueError(f'reduction_override must be None, "none", "mean" or "sum", got {reduction_override!r}')
    reduction = reduction_override if reduction_override else self.reduction
    if weight is not None and weight.dim() > 1:
        # (n, 4) box weights -> (n,): the row loss has one value per box (iou_loss.py:275-280)
        assert weight.shape == pred.shape
        weight = weight.mean(-1)
    return self.loss_weight * weight_reduce_loss(loss_fn(pred, target, **kwargs), weight, reduction, avg_factor)


def _no_positive(pred, weight):
    if pred.dim() == weight.dim() + 1:
        weight = weight.unsqueeze(1)
    return (pred * weight).sum()      # 0, attached to pred's graph


@LOSSES.register_module()
class IoULoss(nn.Module):
    def __init__(self, linear=False, eps=1e-6, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.linear, self.eps, self.reduction, self.loss_weight = linear, eps, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        reduction = reduction_override if reduction_override else self.reduction
        if weight is not None and not torch.any(weight > 0) and reduction != 'none':
            return _no_positive(pred, weight)
        return _weighted(iou_loss, self, pred, target, weight, avg_factor, reduction_override, linear=self.linear, eps=self.eps, **kwargs)


@LOSSES.register_module()
class GIoULoss(nn.Module):
    def __init__(self, eps=1e-6, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.eps, self.reduction, self.loss_weight = eps, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        if weight is not None and not torch.any(weight > 0):
            return _no_positive(pred, weight)
        return _weighted(giou_loss, self, pred, target, weight, avg_factor, reduction_override, eps=self.eps, **kwargs)
