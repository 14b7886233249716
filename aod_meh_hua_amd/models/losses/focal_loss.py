"""FocalLoss plugin (mmdet/models/losses/focal_loss.py:105-181): the sigmoid focal loss of the plain RetinaNet baseline
(MyRetinaHead) -- mmcv.ops.sigmoid_focal_loss on the raw logits, no softmax in front of it.  The module keeps the fork's
constructor (`last_activation` instead of `use_sigmoid`) and call signature; the arithmetic is the fused HIP kernels
aod_sigmoid_focal_l1_{fwd,bwd} / aod_sigmoid_focal_elem, the 'sigmoid' form of the kernels EDL_Softmax_FocalLoss runs on.
Inside MyRetinaHead.loss_single the classification and L1 box losses share ONE launch (functional.RetinaLossFn)."""
import torch.nn as nn

from ..builder import LOSSES
from .edl_softmax_focal_loss import focal_forward


@LOSSES.register_module()
class FocalLoss(nn.Module):
    def __init__(self, last_activation='sigmoid', gamma=2.0, alpha=0.25, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.use_sigmoid = last_activation == 'sigmoid'
        assert self.use_sigmoid is True, 'Only sigmoid focal loss supported now.'      # focal_loss.py:129-130
        self.last_activation = last_activation
        self.gamma, self.alpha, self.reduction, self.loss_weight = gamma, alpha, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        """focal_loss.py:136-181 -> sigmoid_focal_loss (:59-102) + weight_reduce_loss: the reduction rules of EDL_Softmax_FocalLoss here
        (per-row or no weight: the fused row kernel; 'none' or per-element weights: the elementwise kernel)."""
        return focal_forward(self, 'sigmoid', pred, target, weight, avg_factor, reduction_override)
