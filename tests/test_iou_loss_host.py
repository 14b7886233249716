"""IoU / GIoU box losses on decoded boxes, the parts that need no GPU: the registry and the torch modules against the float64
oracle of tests/iou_loss_util.py and against the reference's own numbers (tests/golden/iou_box_loss.npz, written by
tools/golden/make_golden_iou_loss.py), the frame invariance the kernels rest on, the head / driver / C-ABI plumbing."""
import copy
import importlib.util
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import iou_loss_util as IU
from tests import plain_retina_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('aod_focal_box_fwd_ex', 'aod_focal_box_bwd_ex', 'aod_focal_box_levels_fwd_ex', 'aod_focal_box_levels_bwd_ex')


def _module(form, **kw):
    from aod_meh_hua_amd.models import build_loss
    box, linear = IU.split_form(form)
    cfg = dict(type='GIoULoss', **kw) if box == 'giou' else dict(type='IoULoss', linear=linear, **kw)
    return build_loss(cfg)


def test_registry_builds_both_types_with_mmdet_arguments():
    from aod_meh_hua_amd import models
    from aod_meh_hua_amd.models import LOSSES, build_loss
    a = build_loss(dict(type='IoULoss', linear=True, eps=1e-5, reduction='sum', loss_weight=3.0))
    b = build_loss(dict(type='GIoULoss', eps=1e-7, reduction='mean', loss_weight=2.0))
    assert type(a) is models.IoULoss and type(b) is models.GIoULoss
    assert (a.linear, a.eps, a.reduction, a.loss_weight) == (True, 1e-5, 'sum', 3.0)
    assert (b.eps, b.reduction, b.loss_weight) == (1e-7, 'mean', 2.0)
    d = build_loss(dict(type='IoULoss'))
    assert (d.linear, d.eps, d.reduction, d.loss_weight) == (False, 1e-6, 'mean', 1.0)
    assert build_loss(dict(type='GIoULoss')).eps == 1e-6
    assert 'IoULoss' in models.__all__ and 'GIoULoss' in models.__all__
    assert LOSSES.get('IoULoss') is models.IoULoss and LOSSES.get('GIoULoss') is models.GIoULoss


def _random_boxes(n, seed):
    g = torch.Generator().manual_seed(seed)
    a = IU.make_anchors(n, seed)
    p = torch.randn(n, 4, generator=g, dtype=torch.float64) * 0.4
    t = torch.randn(n, 4, generator=g, dtype=torch.float64) * 0.3
    return IU.decode(a, p), IU.decode(a, t)


@pytest.mark.parametrize('form', IU.FORMS)
def test_module_forward_against_float64_oracle(form):
    box, linear = IU.split_form(form)
    b1, b2 = _random_boxes(257, 3)
    ref = IU.box_loss(b1, b2, box, 1e-6, linear)
    w = (torch.rand(257, generator=torch.Generator().manual_seed(4)) > 0.3).double()
    m = _module(form, loss_weight=1.5)
    # float64 in, float64 arithmetic: the same formulas
    assert torch.allclose(m(b1, b2, reduction_override='none'), 1.5 * ref, rtol=1e-12, atol=0)
    assert torch.allclose(m(b1, b2, w, avg_factor=7.0), 1.5 * (ref * w).sum() / 7.0, rtol=1e-12, atol=0)
    assert torch.allclose(m(b1, b2, w[:, None].expand(-1, 4).contiguous()), 1.5 * (ref * w).mean(), rtol=1e-12, atol=0)      # weight.mean(-1)
    assert torch.allclose(m(b1, b2, reduction_override='sum'), 1.5 * ref.sum(), rtol=1e-12, atol=0)
    # float32 in: rows agree with float64 to a few ulps of their size (IoU in (0, 1], the loss O(1))
    got = m(b1.float(), b2.float(), reduction_override='none').double()
    ref32 = 1.5 * IU.box_loss(b1.float().double(), b2.float().double(), box, 1e-6, linear)
    assert float((got - ref32).abs().max()) <= 1e-5 * float(ref32.abs().max())
    with pytest.raises(ValueError):
        m(b1, b2, reduction_override='average')


def _golden_levels(g):
    """per level: decoded prediction boxes (fp32, this project's delta2bbox), target boxes, weights [rows, 4] in the head's row order"""
    from aod_meh_hua_amd.core.bbox import delta2bbox
    out = []
    for l in range(len(PU.LEVELS)):
        reg = PU.rows_of(g[f'reg{l}'], 4)
        anc = torch.from_numpy(g[f'anchors{l}'])[None].expand(PU.B, -1, 4).reshape(-1, 4)
        out.append((delta2bbox(anc, reg, max_shape=None), torch.from_numpy(g[f'bt{l}']).reshape(-1, 4), torch.from_numpy(g[f'bw{l}']).reshape(-1, 4)))
    return out


@pytest.mark.parametrize('form', IU.FORMS)
def test_module_forward_against_reference_numbers(form):
    g = np.load(IU.GOLDEN)
    m = _module(form)
    n = float(g['num_total_samples'])
    got = [float(m(p, t, w, avg_factor=n)) for p, t, w in _golden_levels(g)]
    want = g[f'loss_bbox_{form}']
    assert want[0] > 0.1 and not want[1:].any()          # level 0 holds the positives; the others take the early return
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)


@pytest.mark.parametrize('form', IU.FORMS)
def test_no_positive_weight_returns_zero_attached_to_pred(form):
    m = _module(form)
    b1, b2 = (b.float() for b in _random_boxes(9, 5))
    b1.requires_grad_(True)
    for w in (torch.zeros(9, 4), torch.zeros(9)):
        out = m(b1, b2, w, avg_factor=3.0)
        assert out.shape == () and float(out.detach()) == 0.0 and out.requires_grad
        gr, = torch.autograd.grad(out, b1)
        assert not gr.any()
    rows = m(b1, b2, torch.zeros(9), reduction_override='none')
    if form == 'giou':                  # GIoULoss returns early whatever the reduction (iou_loss.py:345-348); IoULoss keeps the rows
        assert rows.shape == ()
    else:
        assert rows.shape == (9,) and not rows.any()


def _frame_case(n=600, seed=11):
    """anchors of aspect 0.5 / 1 / 2 at strides 8..128; deltas that put sizes in [1/8, 8] anchor units; disjoint, nested, equal and clamped rows"""
    g = torch.Generator().manual_seed(seed)
    a = IU.make_anchors(n, seed)
    lim = math.log(8.0)
    def draw():
        return torch.cat([(torch.rand(n, 2, generator=g, dtype=torch.float64) - 0.5) * 2.0,
                          (torch.rand(n, 2, generator=g, dtype=torch.float64) * 2 - 1) * lim], 1)
    p, t = draw(), draw()
    p[0:40, :2] = t[0:40, :2] + 20.0                      # disjoint: centres twenty anchor sizes apart
    p[40:80, :2] = t[40:80, :2]                           # nested: same centre, prediction smaller on both axes ...
    p[40:80, 2:] = t[40:80, 2:] - 0.7
    p[80:120, :2] = t[80:120, :2]                         # ... and larger
    p[80:120, 2:] = t[80:120, 2:] + 0.7
    p[120:160] = t[120:160]                               # equal
    p[160:200, 2] = 9.0                                   # beyond the clamp (a wh_ratio_clip of 1 / 64 below: |ln| = 4.16), both signs
    p[200:240, 3] = -9.0
    return a, p, t


@pytest.mark.parametrize('form', IU.FORMS)
def test_pixel_and_anchor_frames_agree(form):
    """the invariance the kernels rest on: decoded from real anchors or from the unit anchor, loss and delta gradients are the same numbers"""
    box, linear = IU.split_form(form)
    a, p, t = _frame_case()
    kw = dict(means=(0.02, -0.01, 0.05, -0.03), stds=(0.1, 0.1, 0.2, 0.2), max_ratio=abs(math.log(1 / 64)))
    p, t = p / torch.tensor(kw['stds'], dtype=torch.float64), t / torch.tensor(kw['stds'], dtype=torch.float64)
    lp, gp, ip = IU.rows(p, t, box, 1e-6, linear, anchors=a, **kw)
    la, ga, ia = IU.rows(p, t, box, 1e-6, linear, anchors=None, **kw)
    assert float(ip[:40].max()) == 0.0 and float(ip[120:160].min()) > 1 - 1e-9 and 0 < float(ip[40:120].min())      # the rows are what they claim
    assert not ga[160:200, 2].any() and not ga[200:240, 3].any()                                                     # clamped sizes: no gradient
    if not (box == 'iou' and not linear):
        assert float((lp - la).abs().max()) <= 1e-12 * float(la.abs().max())
        assert float((gp - ga).abs().max()) <= 1e-12 * float(ga.abs().max())
    else:
        # -log(max(IoU, eps)): the disjoint rows sit on the eps clamp (loss -ln eps, gradient 0) in both frames; elsewhere relative per row
        assert torch.equal(lp[:40], la[:40]) and not gp[:40].any() and not ga[:40].any()
        assert float(((lp - la).abs() / la.abs().clamp(min=1.0)).max()) <= 1e-12
        scale = ga.abs().amax(1, keepdim=True).clamp(min=1.0)
        assert float(((gp - ga).abs() / scale).max()) <= 1e-12


def _head_cfg(head_type, loss_bbox, decoded):
    from aod_meh_hua_amd.mmcv_lite import Config
    name = 'Config_RetinaNet_plain.py' if head_type == 'MyRetinaHead' else 'Config_RetinaNet.py'
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_', name))
    hc = copy.deepcopy(dict(cfg.model.bbox_head))
    hc.update(loss_bbox=loss_bbox, reg_decoded_bbox=decoded, train_cfg=cfg.model.train_cfg, test_cfg=cfg.model.test_cfg)
    return hc


@pytest.mark.parametrize('head_type', ['Lambda_L2Net', 'MyRetinaHead'])
def test_reg_decoded_bbox_goes_with_the_loss_type(head_type):
    from aod_meh_hua_amd.models import build_head
    for loss_bbox, decoded in ((dict(type='L1Loss', loss_weight=1.0), False), (dict(type='GIoULoss', loss_weight=2.0), True),
                               (dict(type='IoULoss', linear=True), True)):
        head = build_head(_head_cfg(head_type, loss_bbox, decoded))
        assert head.reg_decoded_bbox is decoded and type(head.loss_bbox).__name__ == loss_bbox['type']
        form = head._box_loss_form()
        if not decoded:
            assert form is None
        else:
            assert form['box_form'] == ('giou' if loss_bbox['type'] == 'GIoULoss' else 'iou') and form['box_eps'] == 1e-6
            assert form['box_linear'] is bool(loss_bbox.get('linear', False))
            assert form['coder'] == ((0., 0., 0., 0.), (1., 1., 1., 1.), 16 / 1000)
    for loss_bbox, decoded in ((dict(type='L1Loss', loss_weight=1.0), True), (dict(type='GIoULoss'), False), (dict(type='IoULoss'), False)):
        with pytest.raises(ValueError) as e:
            build_head(_head_cfg(head_type, loss_bbox, decoded))
        assert f'reg_decoded_bbox={decoded}' in str(e.value) and f"loss_bbox={loss_bbox['type']}" in str(e.value)


def test_heads_refuse_other_box_losses_by_name():
    from aod_meh_hua_amd.models import build_head
    with pytest.raises(ValueError, match='SmoothL1Loss'):
        build_head(_head_cfg('MyRetinaHead', dict(type='SmoothL1Loss'), False))
    head = build_head(_head_cfg('Lambda_L2Net', dict(type='SmoothL1Loss'), False))
    with pytest.raises(ValueError, match='L1Loss, IoULoss or GIoULoss'):
        head._box_loss_form()


def test_giou_config_builds_the_plain_baseline_with_giou():
    from aod_meh_hua_amd.mmcv_lite import Config
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet_plain_giou.py'))
    base = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet_plain.py'))
    h = cfg.model.bbox_head
    assert h.reg_decoded_bbox is True and h.loss_bbox.type == 'GIoULoss' and h.loss_bbox.loss_weight == 2.0
    assert h.type == 'MyRetinaHead' and dict(h.loss_cls) == dict(base.model.bbox_head.loss_cls)
    assert dict(cfg.optimizer) == dict(base.optimizer) and cfg.cycles == base.cycles


def test_driver_parser_accepts_loss_bbox(monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location('train_RetinaNet_for_iou_loss', os.path.join(ROOT, 'tools', 'train_RetinaNet.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from aod_meh_hua_amd.mmcv_lite import Config
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--loss-bbox', 'GIoU', '--loss-bbox-weight', '2.0', '--synthetic', '8'])
    args = mod.parse_args()
    assert args.loss_bbox == 'GIoU' and args.loss_bbox_weight == 2.0
    cfg = mod.set_loss_bbox(Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py')), args.loss_bbox, args.loss_bbox_weight)
    assert cfg.model.bbox_head.reg_decoded_bbox is True and dict(cfg.model.bbox_head.loss_bbox) == dict(type='GIoULoss', loss_weight=2.0)
    cfg = mod.set_loss_bbox(cfg, 'L1', None)
    assert cfg.model.bbox_head.reg_decoded_bbox is False and dict(cfg.model.bbox_head.loss_bbox) == dict(type='L1Loss', loss_weight=1.0)
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py'])
    assert mod.parse_args().loss_bbox is None
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--loss-bbox', 'DIoU'])
    with pytest.raises(SystemExit):
        mod.parse_args()
    assert 'GIoU' in capsys.readouterr().err


def test_new_entries_are_exported_and_declared():
    from aod_meh_hua_amd import _C
    header = open(os.path.join(ROOT, 'include', 'aod_hip.h')).read()
    for name in ENTRIES:
        assert getattr(_C.lib, name) is not None
        assert re.search(r'\bint\s+' + name + r'\s*\(int focal_form, int box_form, float box_eps, int box_linear, const float\* means4, '
                         r'const float\* stds4,\s*float wh_ratio_clip,', header), name


def test_entries_refuse_bad_box_arguments_by_name():
    """the checks in front of every launch (they read no device memory): each message names its entry"""
    import ctypes as ct
    from aod_meh_hua_amd import _C
    F4 = ct.c_float * 4
    ok_m, ok_s = F4(0, 0, 0, 0), F4(1, 1, 1, 1)
    one = ct.c_void_p(16)                      # a non-NULL bbox_pred: the refusals below come before anything is dereferenced
    tails = {'aod_focal_box_fwd_ex': (0, 20, 2.0, 0.25, None, None, None, None),
             'aod_focal_box_bwd_ex': (0, 20, 2.0, 0.25, None, None, None, 0.0, 0, None, None, 0, 1, 20, 4, None),
             'aod_focal_box_levels_fwd_ex': (1, None, 20, 2.0, 0.25, None, None, None, None, 0, None, None, None),
             'aod_focal_box_levels_bwd_ex': (1, None, 20, 2.0, 0.25, None, None, None, None, None, 0, 1, 20, 4, None)}
    nan, inf = float('nan'), float('inf')
    for name in ENTRIES:
        short = name[len('aod_'):]

        def refused(focal, box, eps, means, stds, clip, bp=one, name=name):
            rc = getattr(_C.lib, name)(focal, box, eps, 0, means, stds, clip, None, None, None, bp, None, None, *tails[name])
            msg = _C.lib.aod_last_error().decode()
            assert rc != 0 and msg.startswith(short + ':'), (name, rc, msg)
            return msg
        assert 'box form' in refused(0, 3, 1e-6, ok_m, ok_s, 0.016) and 'box form' in refused(1, -1, 1e-6, ok_m, ok_s, 0.016)
        assert 'focal form' in refused(2, 1, 1e-6, ok_m, ok_s, 0.016)
        assert 'needs bbox_pred' in refused(0, 2, 1e-6, ok_m, ok_s, 0.016, bp=None)
        assert 'means and stds' in refused(0, 1, 1e-6, None, ok_s, 0.016)
        assert 'eps' in refused(0, 1, nan, ok_m, ok_s, 0.016) and 'eps' in refused(0, 2, inf, ok_m, ok_s, 0.016)
        assert 'finite' in refused(0, 2, 1e-6, F4(0, nan, 0, 0), ok_s, 0.016) and 'finite' in refused(0, 2, 1e-6, ok_m, F4(1, 1, inf, 1), 0.016)
        assert 'stds must be > 0' in refused(0, 1, 1e-6, ok_m, F4(1, 0, 1, 1), 0.016) and 'stds must be > 0' in refused(0, 1, 1e-6, ok_m, F4(1, 1, 1, -1), 0.016)
        for clip in (0.0, -1.0, nan, inf):
            assert 'wh_ratio_clip' in refused(0, 2, 1e-6, ok_m, ok_s, clip)


def test_cpu_tensor_is_refused():
    from aod_meh_hua_amd import _C
    from aod_meh_hua_amd import hipops as ho
    cls, lab, lw = torch.zeros(4, 20), torch.full((4,), 20, dtype=torch.int64), torch.ones(4)
    bp, bt, bw = torch.zeros(4, 4), torch.zeros(4, 4), torch.ones(4, 4)
    for box_form in ('iou', 'giou'):
        with pytest.raises(_C.AodHipError, match='no CPU fallback'):
            ho.edl_focal_l1_fwd(cls, lab, lw, bp, bt, bw, form='sigmoid', box_form=box_form)
    with pytest.raises(ValueError, match='unknown box form'):
        ho._box_entry('edl', 'diou', 1e-6, False, None, 'fwd', ())
