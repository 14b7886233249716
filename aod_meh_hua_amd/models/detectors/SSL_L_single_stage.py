"""SSL_L_SingleStageDetector / SSL_L_RetinaNet / SSD_L_SingleStageDetector plugins
(mmdet/models/detectors/SSL_L_single_stage.py:10-98, SSL_L_retinanet.py, SSD_L_single_stage.py) and the plain baseline detectors
MyRetinaSingleStageDetector / MyRetinaNet (MyRetinaSingleStage.py:10-75, MyRetinanet.py)."""
import warnings

from ...core.bbox import bbox2result, unc2result
from ..builder import DETECTORS, build_backbone, build_head, build_neck
from .SSL_Lambda import SSLBase_L_Detector


@DETECTORS.register_module()
class SSL_L_SingleStageDetector(SSLBase_L_Detector):
    def __init__(self, backbone, neck=None, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None, init_cfg=None):
        super().__init__(init_cfg)
        if pretrained:
            warnings.warn('DeprecationWarning: pretrained is deprecated, please use "init_cfg" instead')
            backbone.pretrained = pretrained
        self.backbone = build_backbone(backbone)
        if neck is not None:
            self.neck = build_neck(neck)
        bbox_head.update(train_cfg=train_cfg)
        bbox_head.update(test_cfg=test_cfg)
        self.bbox_head = build_head(bbox_head)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    def extract_feat(self, img):
        from ... import hipops as ho
        with ho.scope('backbone'):
            x = self.backbone(img)
        if self.with_neck:
            with ho.scope('neck'):
                x = self.neck(x)
        return x

    def forward_train(self, img, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None, **kwargs):
        """SSL_L_single_stage.py:51-62 -> (losses, head_out, feat_out)."""
        super().forward_train(img, img_metas)
        x = self.extract_feat(img)
        losses, head_out = self.bbox_head.forward_train(x, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore, **kwargs)
        feat_out = [i.detach() for i in x]
        return losses, head_out, feat_out

    def forward_train_L(self, loss, head_out, feat_out, **kwargs):
        return self.bbox_head.forward_train_L(loss, head_out, feat_out, **kwargs)

    def simple_test(self, img, img_metas, rescale=False, **kwargs):
        """SSL_L_single_stage.py:68-98."""
        mcd = kwargs.get('mc_dropout')
        if mcd is not None:
            # one stochastic forward of the MC-dropout baseline (apis/test.py single_gpu_mcdropout; CalMCDropoutUnc.py:137-163): mcd = a
            # functional.MCDropoutState (factor table, sites); the classification maps of a forward with a Dropout2d behind every ReLU that feeds them
            from ... import functional as AF
            assert kwargs['isEval'] and kwargs.get('justOut'), 'MC-dropout forwards return classification maps only (isEval=True, justOut=True)'
            with AF.mc_dropout(mcd.table, mcd.sites):
                return list(self.bbox_head.forward_cls_dropout(self.extract_feat(img)))
        if kwargs['isEval'] and kwargs.get('justFeat'):
            # Core-set descriptors (apis/test.py single_gpu_descriptors): the neck outputs as they lie in the pyramid buffer; no head is launched
            return self._just_feat(img)
        if kwargs.get('objUnc') and not kwargs.get('objDesc'):
            raise ValueError('objUnc is offered together with objDesc only: it appends the per-object measure in the descriptors\' slots')
        if kwargs.get('objPost') and not kwargs.get('objDesc'):
            raise ValueError('objPost is offered together with objDesc only: it appends the posterior rows in the descriptors\' slots')
        if kwargs['isEval'] and kwargs.get('objDesc'):
            # CCMS object descriptors (apis/test.py single_gpu_object_descriptors): the static (dets, labels, num, unc, feat, cls, w, cnt,
            # missing) of the padded evaluation form, max_obj = objDesc; objUnc=True (ENMS / DivProto, single_gpu_enms) appends h,
            # objPost=True (BADGE, single_gpu_badge_embeddings) post
            if not kwargs.get('_padded'):
                raise ValueError('objDesc is offered with the padded evaluation outputs only (isEval=True, _padded=True)')
            self._check_obj_desc()
        feat = self.extract_feat(img)
        if kwargs['isEval'] and kwargs.get('justOut'):
            # MyRetinaSingleStage.py:46-49 (honoured with isEval only): the per-level classification maps [B, A*C, h, w] fp32 of an ensemble
            # member (apis/test.py single_gpu_ensemble) -- no decode, no NMS, no HUA
            head = self.bbox_head
            return list(head.test_heads(feat)[0][0] if hasattr(head, 'test_heads') else head.forward(feat)[0])
        if kwargs['isEval']:
            _results_list = self.bbox_head.simple_test(feat, img_metas, rescale=rescale, **kwargs)
            if kwargs.get('_padded'):     # device metric: (dets [B,max,5], labels [B,max], num [B]) stay on the device, no bbox2result
                return _results_list
            if kwargs.get('detUnc'):      # (bbox_results, unc_results): unc_results[i][c] is (k, 2) (aleatoric, epistemic), row-aligned with bbox_results[i][c]
                nc = self.bbox_head.num_classes
                return ([bbox2result(d, l, nc) for d, l, _ in _results_list], [unc2result(u, l, nc) for _, l, u in _results_list])
            results_list = _results_list[0] if kwargs.get('isUnc') else _results_list
            return [bbox2result(det_bboxes, det_labels, self.bbox_head.num_classes) for det_bboxes, det_labels in results_list]
        results_list, *uncertainties = self.bbox_head.simple_test(feat, img_metas, rescale=rescale, **kwargs)
        if self.test_cfg.uncertainty_pool in ('Entropy_NoNMS', 'Entropy_ALL', 'Entropy_NMS', 'Entropy_Avg'):
            return (results_list, *uncertainties)
        from ...scoring import POSTERIOR_POOLS
        if kwargs.get('isUnc') and kwargs.get('uPool') in POSTERIOR_POOLS:      # the posterior pools: (results_list, unc) as above
            return (results_list, *uncertainties)
        bbox_results = [bbox2result(det_bboxes, det_labels, self.bbox_head.num_classes) for det_bboxes, det_labels in results_list]
        return bbox_results, uncertainties

    def _just_feat(self, img):
        return tuple(self.extract_feat(img))

    def _check_obj_desc(self):
        pass

    def aug_test(self, imgs, img_metas, rescale=False):
        raise NotImplementedError('test-time augmentation is not on the MEH/HUA path')


@DETECTORS.register_module()
class SSL_L_RetinaNet(SSL_L_SingleStageDetector):
    """mmdet/models/detectors/SSL_L_retinanet.py:1-18."""

    def __init__(self, backbone, neck, bbox_head, train_cfg=None, test_cfg=None, pretrained=None, init_cfg=None):
        super().__init__(backbone, neck, bbox_head, train_cfg, test_cfg, pretrained, init_cfg)


@DETECTORS.register_module()
class SSD_L_SingleStageDetector(SSL_L_SingleStageDetector):
    """mmdet/models/detectors/SSD_L_single_stage.py:10-134 (same control flow as SSL_L_SingleStageDetector)."""

    def _just_feat(self, img):
        raise NotImplementedError('justFeat / Core-set descriptors are built for the FPN pyramid of the RetinaNet detectors, not for SSD '
                                  '(its six source maps have different channel counts and do not lie in one row buffer)')

    def _check_obj_desc(self):
        raise NotImplementedError('objDesc / CCMS object descriptors are built for the FPN pyramid of the RetinaNet detectors, not for SSD '
                                  '(its six source maps have different channel counts: the objects of an image would not share a feature space)')


@DETECTORS.register_module()
class MyRetinaSingleStageDetector(SSL_L_SingleStageDetector):
    """mmdet/models/detectors/MyRetinaSingleStage.py:10-75: the plain single-stage detector of the baselines (MyRetinaHead: no Model
    Evidence Head).  On SSLBase_L_Detector -- MyRetinaBase._parse_losses (MyRetinaBase.py:128-156) is the base's, `loss_noR` in the total
    included, and train_step returns the same 4-tuple -- with the control flow of SSL_L_SingleStageDetector: justOut (the classification
    maps of an ensemble member), justFeat, _padded, isUnc=False and mc_dropout are honoured there.  What it does not have is lambda: the
    HUA pools and detUnc raise before anything is launched, and there is no MEH step (train_step_L)."""

    def simple_test(self, img, img_metas, rescale=False, **kwargs):
        from ...scoring import refuse_hua
        refuse_hua(self.bbox_head, **kwargs)
        return super().simple_test(img, img_metas, rescale=rescale, **kwargs)

    def forward_train_L(self, loss, head_out, feat_out, **kwargs):
        raise ValueError(f'{type(self.bbox_head).__name__} has no lambda (no Model Evidence Head): there is no MEH step to train')


@DETECTORS.register_module()
class MyRetinaNet(MyRetinaSingleStageDetector):
    """mmdet/models/detectors/MyRetinanet.py."""

    def __init__(self, backbone, neck, bbox_head, train_cfg=None, test_cfg=None, pretrained=None, init_cfg=None):
        super().__init__(backbone, neck, bbox_head, train_cfg, test_cfg, pretrained, init_cfg)
