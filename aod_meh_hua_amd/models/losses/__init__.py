from .edl_softmax_focal_loss import EDL_Softmax_FocalLoss
from .focal_loss import FocalLoss
from .iou_loss import GIoULoss, IoULoss
from .smooth_l1_loss import L1Loss, SmoothL1Loss

__all__ = ['EDL_Softmax_FocalLoss', 'FocalLoss', 'L1Loss', 'SmoothL1Loss', 'IoULoss', 'GIoULoss']
