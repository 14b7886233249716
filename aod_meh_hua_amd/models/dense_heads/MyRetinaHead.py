"""MyRetinaHead: the plain RetinaNet head of the reference's baseline detector (mmdet/models/dense_heads/MyRetinaHead.py:13-160) --
cls / reg towers + retina_cls / retina_reg, sigmoid FocalLoss + L1, NO Model Evidence Head: no lambda tower, no `L_names`, no HUA.
It is what the Ensemble / MC-dropout / Random / Core-set / CDAL baselines of the paper are trained on (CalEnsembleUnc.py:164-180 takes
the sigmoid of ITS classification maps).

Same MI355X design as Lambda_L2Net, whose methods it borrows where the code is the same:
  * the two towers run LEVEL-BATCHED and advance together (functional.conv_pair_act: one grouped launch per depth), without the MEH rider;
  * loss_single (:91-109) is one fused launch per level, loss_all_levels one per pass for all levels -- the 'sigmoid' form of the fused
    focal + L1 kernels (aod_sigmoid_focal_l1_*): (loss_cls, loss_bbox, loss_noR) with the PackedLosses / deferred-average handling of
    L_AnchorHead.loss;
  * scoring (anchor_head.py:535-596) = mode 3 of the pre-NMS kernels (per-class sigmoid, row key = max over the C columns), then the
    stable top-k, class-aware NMS and max_per_img stages every head shares (scoring.score_batch)."""
import torch
import torch.nn as nn

from ... import functional as AF
from ...mmcv_lite import Conv2d, ConvModule
from ..builder import HEADS
from .L_anchor_head import L_AnchorHead
from .Lambda_L2 import Lambda_L2Net


@HEADS.register_module()
class MyRetinaHead(L_AnchorHead):
    def __init__(self, num_classes, in_channels, stacked_convs=4, conv_cfg=None, norm_cfg=None,
                 anchor_generator=dict(type='AnchorGenerator', octave_base_scale=4, scales_per_octave=3, ratios=[0.5, 1.0, 2.0],
                                       strides=[8, 16, 32, 64, 128]),
                 init_cfg=dict(type='Normal', layer='Conv2d', std=0.01,
                               override=dict(type='Normal', name='retina_cls', std=0.01, bias_prob=0.01)), **kwargs):
        self.stacked_convs, self.conv_cfg, self.norm_cfg = stacked_convs, conv_cfg, norm_cfg
        super().__init__(num_classes, in_channels, anchor_generator=anchor_generator, init_cfg=init_cfg, **kwargs)
        if (self.last_activation != 'sigmoid' or type(self.loss_cls).__name__ != 'FocalLoss'
                or type(self.loss_bbox).__name__ not in ('L1Loss', 'IoULoss', 'GIoULoss')):
            raise ValueError("MyRetinaHead is built for loss_cls=FocalLoss(last_activation='sigmoid') + loss_bbox=L1Loss, or IoULoss / GIoULoss "
                             f'with reg_decoded_bbox=True (got {type(self.loss_cls).__name__}/{self.last_activation} + '
                             f'{type(self.loss_bbox).__name__})')

    def _init_layers(self):
        """MyRetinaHead.py:47-78 (same attribute names -> same state_dict keys)."""
        self.relu = nn.ReLU(inplace=True)
        self.cls_convs, self.reg_convs = nn.ModuleList(), nn.ModuleList()
        for i in range(self.stacked_convs):
            chn = self.in_channels if i == 0 else self.feat_channels
            for tower in (self.cls_convs, self.reg_convs):
                tower.append(ConvModule(chn, self.feat_channels, 3, stride=1, padding=1, conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg))
        self.retina_cls = Conv2d(self.feat_channels, self.num_anchors * self.cls_out_channels, 3, padding=1)
        self.retina_reg = Conv2d(self.feat_channels, self.num_anchors * 4, 3, padding=1)

    # ------------------------------------------------------------------ forward
    forward_train = Lambda_L2Net.forward_train            # forward -> loss(cls_scores, bbox_preds, None, gt_bboxes, gt_labels, img_metas)

    def forward_train_L(self, *args, **kwargs):
        raise ValueError('MyRetinaHead has no lambda (no Model Evidence Head): there is no MEH step to train')

    def forward(self, feats, **kwargs):
        """MyRetinaHead.py:80-89, all levels per launch.  Returns (cls_scores[L], bbox_preds[L]) fp32 [B, A*C, h, w]."""
        feats = list(feats)
        cls_feat, reg_feat = (list(t) for t in zip(*[AF.fork(f, 2) for f in feats]))      # (every level feeds both towers)
        if all(m.with_activation for m in list(self.cls_convs) + list(self.reg_convs)):
            for i, (cc, rc) in enumerate(zip(self.cls_convs, self.reg_convs)):          # the two towers advance together
                cls_feat, reg_feat = AF.conv_pair_act(cls_feat, reg_feat, cc.conv, rc.conv, sole_consumer=i > 0)
        else:
            for i, conv in enumerate(self.cls_convs):
                cls_feat = conv(cls_feat, sole_consumer=i > 0)
            for i, conv in enumerate(self.reg_convs):
                reg_feat = conv(reg_feat, sole_consumer=i > 0)
        return (self.retina_cls(cls_feat, out_f32=True, sole_consumer=len(self.cls_convs) > 0),
                self.retina_reg(reg_feat, out_f32=True, sole_consumer=len(self.reg_convs) > 0, sparse_grad=True))

    forward_single = Lambda_L2Net.forward_single

    def forward_cls_dropout(self, feats):
        """The classification maps of one MC-dropout forward (functional.mc_dropout active, no autograd): the cls tower alone, one Dropout2d
        per (conv, level) behind its ReLU, then retina_cls (CalMCDropoutUnc.py:137-163 on this head's maps)."""
        assert AF.mc_dropout_active() and not torch.is_grad_enabled()
        cls_feat = list(feats)
        for i, conv in enumerate(self.cls_convs):
            cls_feat = conv(cls_feat)
            if conv.with_activation:
                AF.dropout_apply(cls_feat, [f'.cls_convs.{i}@{l}' for l in range(len(cls_feat))], self)
        return self.retina_cls(cls_feat, out_f32=True)

    # ------------------------------------------------------------------ losses (the fused launches of Lambda_L2Net in their 'sigmoid' form)
    _can_defer_avg = True
    _focal_form = 'sigmoid'
    _loss_cls_type = 'FocalLoss'
    loss_single = Lambda_L2Net.loss_single
    loss_all_levels = Lambda_L2Net.loss_all_levels

    def loss_L(self, *args, **kwargs):
        raise ValueError('MyRetinaHead has no lambda (no Model Evidence Head): there is no MEH loss')

    # ------------------------------------------------------------------ scoring
    def test_heads(self, feats):
        """the conv half of simple_test: ((cls_scores, bbox_preds), None) -- there is no lambda map.  Without autograd the two towers of one
        depth are ONE grouped launch (functional.conv_towers_nograd), as in Lambda_L2Net.forward_all_towers."""
        import os
        x3_ok = AF.get_precision() == 'bf16' or all(m.conv.weight.shape[0] % 256 == 0 and m.conv.weight.shape[1] % 32 == 0 for m in self.cls_convs)
        if (not torch.is_grad_enabled() and x3_ok and os.environ.get('AOD_GROUP_TOWERS', '1') != '0'
                and len(self.cls_convs) == len(self.reg_convs) > 0 and all(m.with_activation for m in list(self.cls_convs) + list(self.reg_convs))):
            c = r = list(feats)
            for cc, rc in zip(self.cls_convs, self.reg_convs):
                c, r = AF.conv_towers_nograd([c, r], [cc.conv, rc.conv], relu=True)
            return (self.retina_cls(c, out_f32=True), self.retina_reg(r, out_f32=True)), None
        return self.forward(feats), None

    def simple_test(self, feats, img_metas, rescale=False, _preds=None, **kwargs):
        """anchor_head.py simple_test -> get_bboxes: detections only.  isEval (with or without _padded) and the with_nms=False candidates
        of uPool='Entropy_NoNMS'; the HUA pools and detUnc need lambda and raise.  The posterior pools (uPool in scoring.POSTERIOR_POOLS)
        read the sigmoid scores alone: (det_results, unc) like the evidence heads' Entropy_NMS."""
        from ...scoring import refuse_hua
        refuse_hua(self, **kwargs)
        outs, _ = _preds if _preds is not None else self.test_heads(feats)
        with_nms = not (not kwargs['isEval'] and kwargs.get('uPool') == 'Entropy_NoNMS')
        if kwargs['isEval'] and kwargs.get('objDesc'):      # CCMS object descriptors: score_batch reads the neck outputs
            kwargs = dict(kwargs, _feats=list(feats))
        results_list = self.get_bboxes(*outs, img_metas, rescale=rescale, with_nms=with_nms, **kwargs)
        if not kwargs['isEval']:
            from ...scoring import POSTERIOR_POOLS
            if kwargs.get('isUnc') and kwargs.get('uPool') in POSTERIOR_POOLS:      # (det_results, unc): DESIGN 3l, no lambda needed
                return (results_list[0], *results_list[1:])
            return (results_list,)
        return results_list

    _get_bboxes = Lambda_L2Net._get_bboxes
