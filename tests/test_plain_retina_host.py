"""Host tests (no GPU) of the plain RetinaNet baseline -- FocalLoss / MyRetinaHead / MyRetinaNet, the one-optimizer training iteration, the
sigmoid-focal C entries and the driver's config: registries, state_dict keys against the reference's recorded list, optimizers, the HUA
refusal, argument validation before any launch."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import plain_retina_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ('aod_sigmoid_focal_l1_fwd', 'aod_sigmoid_focal_l1_bwd', 'aod_sigmoid_focal_l1_levels_fwd', 'aod_sigmoid_focal_l1_levels_bwd',
               'aod_sigmoid_focal_elem')


@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.aod_last_error.restype = ctypes.c_char_p
    return lib


@pytest.fixture(scope='module')
def plain():
    return U.build_plain(ROOT)


def test_registries_resolve_the_plain_types():
    from aod_meh_hua_amd.models import DETECTORS, HEADS, LOSSES, build_loss
    assert LOSSES.get('FocalLoss') is not None and HEADS.get('MyRetinaHead') is not None
    assert DETECTORS.get('MyRetinaNet') is not None and DETECTORS.get('MyRetinaSingleStageDetector') is not None
    loss = build_loss(dict(type='FocalLoss', last_activation='sigmoid', gamma=2.0, alpha=0.25, loss_weight=1.0))
    assert (loss.use_sigmoid, loss.gamma, loss.alpha, loss.reduction, loss.loss_weight) == (True, 2.0, 0.25, 'mean', 1.0)
    with pytest.raises(AssertionError, match='Only sigmoid focal loss'):       # focal_loss.py:129-130
        build_loss(dict(type='FocalLoss', last_activation='softmax'))


def test_config_builds_and_state_dict_keys_are_the_references(plain):
    model, cfg = plain
    assert type(model).__name__ == 'MyRetinaNet' and type(model.bbox_head).__name__ == 'MyRetinaHead'
    assert type(model.bbox_head.loss_cls).__name__ == 'FocalLoss' and cfg.uncertainty_pool == 'Random'
    assert cfg.model.test_cfg.uncertainty_pool == 'Random' and model.bbox_head.last_activation == 'sigmoid'
    g = U.load_golden()
    sd = model.state_dict()
    assert list(sd.keys()) == list(g['state_keys'])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(g['state_shapes'])
    head = model.bbox_head
    assert not hasattr(head, 'L_names') and not hasattr(head, 'L_convs') and not hasattr(head, 'retina_L')
    assert head.cls_out_channels == 20 and head.num_anchors == 9 and not head.sampling
    assert hasattr(head, 'forward_cls_dropout')
    # the bias == 'uniform' branch of the driver keys on retina_cls; init_cfg: Normal(0.01) + retina_cls bias_prob = 0.01
    model.init_weights()
    assert abs(float(head.retina_cls.bias[0].detach()) + np.log(99)) < 1e-5 and float(head.retina_reg.bias.detach().abs().max()) == 0
    with pytest.raises(ValueError, match='FocalLoss'):
        from aod_meh_hua_amd.models import build_head
        build_head(dict(cfg.model.bbox_head, loss_cls=dict(type='EDL_Softmax_FocalLoss', last_activation='relu', num_classes=20, annealing_step=10),
                        train_cfg=cfg.model.train_cfg, test_cfg=cfg.model.test_cfg))


def test_lambda_checkpoint_loads_with_only_lambda_keys_unexpected(plain):
    from oracle import model as omodel
    model, _ = plain
    res = model.load_state_dict(omodel.seeded_state_dict(), strict=False)
    assert list(res.missing_keys) == []
    assert res.unexpected_keys and all('L_convs' in k or 'retina_L' in k for k in res.unexpected_keys)
    assert len(res.unexpected_keys) == 10
    assert list(U.plain_state_dict().keys()) == list(model.state_dict().keys())


def test_build_optimizers_one_for_the_plain_head_two_for_lambda(plain):
    from aod_meh_hua_amd.apis.train_Lambda import build_optimizers
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    model, cfg = plain
    opt, opt_L = build_optimizers(model, cfg)
    assert opt_L is None
    ids = {id(p) for g in opt.param_groups for p in g['params']}
    assert ids == {id(p) for p in model.parameters() if p.requires_grad} and len(ids) > 100
    cfg2 = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg2.model.backbone.pop('init_cfg')
    m2 = build_detector(cfg2.model)
    o2, o2L = build_optimizers(m2, cfg2)
    meh = {id(p) for n, p in m2.named_parameters() if 'retina_L' in n or 'L_convs' in n}
    main = {id(p) for g in o2.param_groups for p in g['params']}
    assert o2L is not None and {id(p) for g in o2L.param_groups for p in g['params']} == meh and len(meh) == 10
    assert main == {id(p) for p in m2.parameters() if p.requires_grad} - meh and not (main & meh)


@pytest.mark.parametrize('kw', [dict(isEval=False, uPool='Entropy_NMS'), dict(isEval=False, uPool='Entropy_ALL'),
                                dict(isEval=False, uPool='Entropy_Avg'), dict(isEval=True, detUnc=True)])
def test_hua_pools_raise_on_the_plain_head(plain, kw):
    model, _ = plain
    with pytest.raises(ValueError, match=r'MyRetinaHead has no lambda'):
        model.simple_test(None, None, **kw)
    with pytest.raises(ValueError, match=r'MyRetinaHead has no lambda'):
        model.bbox_head.simple_test(None, None, **kw)
    with pytest.raises(ValueError, match=r'no lambda'):
        model.forward_train_L(None, None, None)


def test_new_entries_are_exported_declared_and_listed(lib):
    from aod_meh_hua_amd import _C
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'aod_hip.h')).read(), flags=re.S)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for n in NEW_ENTRIES:
        assert hasattr(lib, n), n
        assert re.search(r'\b%s\s*\(' % n, hdr), n
        assert n in _C._SIGS and n in doc, n
        assert _C._SIGS[n] == _C._SIGS[n.replace('aod_sigmoid_focal', 'aod_edl_focal')], n         # exactly the counterpart's argument list
    assert 'focal_loss.py:85' in open(os.path.join(ROOT, 'include', 'aod_hip.h')).read()


def test_new_entries_validate_before_any_launch(lib):
    """null pointers, C outside 1..96, a bad level count and negative row counts: -1 + a message, nothing is launched (no GPU here)"""
    one, f = ctypes.c_void_p(16), ctypes.c_float
    i64 = ctypes.c_int64
    rows = (ctypes.c_int64 * 3)(1000, 10, 0)
    neg = (ctypes.c_int64 * 3)(1000, -1, 0)
    err = lambda: lib.aod_last_error()

    def fwd(cls=one, n=100, C=20):
        return lib.aod_sigmoid_focal_l1_fwd(cls, one, one, None, None, None, i64(n), C, f(2.0), f(0.25), one, one, one, None)

    def bwd(cls=one, n=100, C=20, A=1, pitch=20):
        return lib.aod_sigmoid_focal_l1_bwd(cls, one, one, None, None, None, i64(n), C, f(2.0), f(0.25), one, None, None, f(0.0), 0, one, None, 0, A, pitch,
                                            4, None)

    def lfwd(cls=one, nlev=3, lr=rows, C=20, num_pos=None, nimg=0, div=None):
        return lib.aod_sigmoid_focal_l1_levels_fwd(cls, one, one, None, None, None, nlev, lr, C, f(2.0), f(0.25), one, one, one, num_pos, nimg, div,
                                                   None, None)

    def lbwd(cls=one, nlev=3, lr=rows, C=20, A=9, pitch=180):
        return lib.aod_sigmoid_focal_l1_levels_bwd(cls, one, one, None, None, None, nlev, lr, C, f(2.0), f(0.25), one, None, None, one, None, 0, A, pitch,
                                                   36, None)

    def elem(cls=one, n=100, C=20):
        return lib.aod_sigmoid_focal_elem(cls, one, i64(n), C, f(2.0), f(0.25), None, one, None)
    for call in (fwd, bwd, lfwd, lbwd, elem):
        assert call(cls=None) == -1 and b'null pointer' in err(), call.__name__
        for C in (0, 97):
            assert call(C=C) == -1 and (b'out of range' in err() or b'bad C' in err()), (call.__name__, C)
    for call in (fwd, bwd, elem):
        assert call(n=-5) == -1 and b'negative row count' in err(), call.__name__
        assert call(cls=None, n=0) == 0                                     # an empty call is a no-op, as for the EDL entries
    for call in (lfwd, lbwd):
        for nlev in (0, 9):
            assert call(nlev=nlev) == -1 and b'1..8 levels' in err(), call.__name__
        assert call(lr=neg) == -1 and b'negative row count' in err(), call.__name__
    assert lfwd(num_pos=one, nimg=16) == -1 and b'divisor' in err()
    assert bwd(A=4, pitch=79) == -1 and b'pitch' in err()
    # the sigmoid mode of the pre-NMS entries: mode 3 has no background column, unknown modes are refused
    assert lib.aod_softmax_rowmax(one, 2, i64(10), 20, f(0.3), one, one, 3, None) == -1 and b'has_bg' in err()
    assert lib.aod_gather_decode(one, one, one, one, None, 2, i64(10), 10, 20, i64(10), one, None, None, None, f(0.016), one, one, one, one,
                                 i64(10), i64(0), i64(0), 4, None) == -1 and b'normalize' in err()


def test_driver_parser_accepts_the_plain_config(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import train_RetinaNet as drv
    finally:
        sys.path.pop(0)
    cfg_path = os.path.join(ROOT, 'configs/_base_/Config_RetinaNet_plain.py')
    for pool in (None, 'Random', 'Coreset', 'CDAL'):
        argv = ['train_RetinaNet.py', '--config', cfg_path, '--synthetic', '64', '--cycles', '2', '--synthetic-size', '256']
        monkeypatch.setattr(sys, 'argv', argv + (['--uncertainty-pool', pool] if pool else []))
        args = drv.parse_args()
        assert args.config == cfg_path and args.uncertainty_pool == pool and args.synthetic == 64 and args.cycles == 2
    from aod_meh_hua_amd.apis.test import Uncertainty_fns
    from aod_meh_hua_amd.mmcv_lite import Config
    cfg = Config.fromfile(cfg_path)
    assert hasattr(Uncertainty_fns, cfg.uncertainty_pool)
    assert cfg.model.type == 'MyRetinaNet' and cfg.model.bbox_head.type == 'MyRetinaHead'
    assert dict(cfg.model.bbox_head.loss_cls) == dict(type='FocalLoss', last_activation='sigmoid', gamma=2.0, alpha=0.25, loss_weight=1.0)
    # everything else is Config_RetinaNet.py's
    base = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    for k in ('optimizer', 'lr_config', 'runner', 'data', 'evaluation', 'X_S_size', 'X_L_0_size', 'cycles', 'epoch_ratio', 'outer_epoch'):
        assert cfg[k] == base[k], k
    assert cfg.model.backbone == base.model.backbone and cfg.model.neck == base.model.neck and cfg.model.train_cfg == base.model.train_cfg


def test_float64_formula_against_the_golden_rows():
    """the util's float64 evaluation is the formula the reference ran: its rows equal the recorded loss_noR within the float32 rounding of
    the reference's CPU path (2.1e-7 relative on rows of magnitude <= 20, measured when the golden was made: 4.2e-6 absolute)"""
    g = U.load_golden()
    for l, li in enumerate(U.golden_level_inputs(g)):
        l64, _ = U.focal64(li['cls'].numpy(), li['labels'].numpy())
        assert np.allclose(g[f'loss_noR{l}'], l64.sum(-1), rtol=2e-6, atol=1e-7)
        assert float(li['cls'].abs().max()) <= 5.0
        assert U.keys_separated(U.level_keys64(g[f'cls{l}']))
    assert [int(U.golden_level_inputs(g)[l]['cls'].shape[0]) for l in range(5)] == list(U.LEVEL_ROWS)
