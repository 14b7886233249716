"""The RetinaNet ablation heads of the reference (mmdet/models/dense_heads/__init__.py:38-51): how the Model Evidence Head is trained, and
whether its lambda enters HUA at all.  Each is Lambda_L2Net with class attributes set and nothing else: the same _init_layers, so the same
state_dict keys -- a checkpoint of one loads into another.

    Lambda_L1Net           Lambda_L1.py:236-241            loss_L = ||lambda + 1e-9 - loss| * w|.mean() * 5
    Lambda_MSLENet         Lambda_MSLE.py:236-242          loss_L = (|log(lambda + 1e-9 + 1) - log(loss + 1)| * w).pow(2).mean() * 5
    Lambda_L2Net_ablation  Lambda_L2_ablation.py:261-265,355,496-518
                           the score_thr / iou_thr kwargs replace the 0.3 / 0.5 of GetObjectIdx, of the FGIdx level gate and of the
                           candidate filter of ComputeObjUnc (a falsy or missing value falls back to 0.3 / 0.5); lambda still scales alpha
    Lambda_L2Net_NoL       Lambda_L2_noL.py:261-265,355,367-369,499-572,631-640
                           the same thresholds; lambda does NOT scale alpha (ComputeObjUnc :530-531, ComputeScaleUnc :589-590: Dirichlet of the
                           scores as they are); adds uncertainty_pool = 'Entropy_Avg' (ComputeAvgUnc + AggregateAvgUnc, see scoring.score_batch)

Not built: Lambda_L2Net_ReLU (differs in more than the above), Lambda_L2Net_reverse (in no __all__), the pseudo-label branch and every
visualisation / JSON side effect of those files."""
from ..builder import HEADS
from .Lambda_L2 import Lambda_L2Net


@HEADS.register_module()
class Lambda_L1Net(Lambda_L2Net):
    _meh_form = 'l1'


@HEADS.register_module()
class Lambda_MSLENet(Lambda_L2Net):
    _meh_form = 'msle'


@HEADS.register_module()
class Lambda_L2Net_ablation(Lambda_L2Net):
    _hua_thr_kwargs = True


@HEADS.register_module()
class Lambda_L2Net_NoL(Lambda_L2Net):
    _hua_lam = 'none'
    _hua_thr_kwargs = True
    _hua_entropy_avg = True
