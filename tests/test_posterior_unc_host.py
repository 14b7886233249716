"""CPU tests (no GPU) of the posterior uncertainty pools: the float64 restatement of tests/posterior_unc_util.py on
hand-worked rows, the argument checks of scoring.det_uncertainty and apis.Posterior_uncertainty, the C entry's declaration and validation,
the pool names in Uncertainty_fns / apis.__all__ / the driver's parser, and refuse_hua letting a plain head through."""
import ctypes
import importlib.util
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import posterior_unc_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = float(np.log(2.0))


# ---------------------------------------------------------------------------------------------------------------- the reference by hand
def test_measures_on_hand_computed_rows():
    for K in (2, 5, 20, 21):
        uni = np.full(K, 1.0 / K)
        assert np.isclose(U.measure64(uni, 'cat', 'entropy'), np.log(K), rtol=1e-14)
        assert np.isclose(U.measure64(uni, 'cat_bg', 'entropy'), np.log(K), rtol=1e-14)
        assert np.isclose(U.measure64(uni, 'cat', 'margin'), 1.0, rtol=1e-15)              # equal top two: margin 1
        assert np.isclose(U.measure64(uni, 'cat', 'leastconf'), 1.0 - 1.0 / K, rtol=1e-15)
        hot = np.eye(K)[K // 2]
        assert U.measure64(hot, 'cat', 'entropy') == 0 and U.measure64(hot, 'sigmoid', 'entropy') == 0      # 0 ln 0 = 0 on both sides
        assert U.measure64(hot, 'cat', 'margin') == 0 and U.measure64(hot, 'cat', 'leastconf') == 0
    for C in (1, 3, 20):
        assert np.isclose(U.measure64(np.full(C, 0.5), 'sigmoid', 'entropy'), C * LN2, rtol=1e-14)
    p = np.array([0.6, 0.3, 0.1])
    assert np.isclose(U.measure64(p, 'cat', 'entropy'), -(0.6 * np.log(0.6) + 0.3 * np.log(0.3) + 0.1 * np.log(0.1)), rtol=1e-14)
    assert np.isclose(U.measure64(p, 'cat', 'margin'), 0.7, rtol=1e-14) and np.isclose(U.measure64(p, 'cat', 'leastconf'), 0.4, rtol=1e-14)
    h = lambda q: -(q * np.log(q) + (1 - q) * np.log(1 - q))
    assert np.isclose(U.measure64(p, 'sigmoid', 'entropy'), h(0.6) + h(0.3) + h(0.1), rtol=1e-14)
    assert np.isclose(U.measure64([0.2, 0.9, 0.9], 'sigmoid', 'margin'), 1.0, rtol=1e-15)
    with pytest.raises(ValueError, match='two used columns'):
        U.measure64([0.4], 'sigmoid', 'margin')
    assert U.used_columns(21, 'cat') == 20 and U.used_columns(21, 'cat_bg') == 21 and U.used_columns(21, 'sigmoid') == 20


def _hand_case():
    """two images, n = 4 candidates, W = 4 (three used columns + the pad), max_num = 3"""
    boxes = np.arange(2 * 4 * 4, dtype=np.float32).reshape(2, 4, 4)
    boxes[0, 3] = boxes[0, 1]                                         # a second candidate with row 1's box: another score, no match
    scores = np.array([[[.6, .3, .1, 0], [.2, .5, .3, 0], [.05, .9, .05, 0], [.2, .4, .4, 0]],
                       [[.1, .1, .8, 0], [.3, .3, .4, 0], [.25, .5, .25, 0], [1., 0., 0., 0]]], np.float32)
    dets = np.zeros((2, 3, 5), np.float32)
    labels = np.full((2, 3), -1, np.int64)
    for b, picks in enumerate((((2, 1), (0, 0), (1, 1)), ((3, 0), (0, 2)))):
        for j, (k, c) in enumerate(picks):
            dets[b, j, :4], dets[b, j, 4], labels[b, j] = boxes[b, k], scores[b, k, c], c
    return boxes, scores, dets, labels, np.array([3, 2], np.int32)


def test_lookup_gate_and_aggregates_on_a_hand_case():
    boxes, scores, dets, labels, num = _hand_case()
    r = U.reference(boxes, scores, dets, labels, num, 'cat', 'leastconf', 'max', thr=0.3)
    assert r['rows'].tolist() == [[2, 0, 1], [3, 0, -1]] and r['missing'].tolist() == [0, 0] and r['count'].tolist() == [3, 2]
    assert np.allclose(r['obj'][0], 1 - np.array([.9, .6, .5], np.float32).astype(np.float64), rtol=1e-15) and np.isnan(r['obj'][1, 2])
    assert np.isclose(r['unc'][0], 1 - np.float64(np.float32(.5))) and r['unc'][1] == 1 - np.float64(np.float32(.8))
    s = U.reference(boxes, scores, dets, labels, num, 'cat', 'leastconf', 'sum', thr=0.3)['unc']
    m = U.reference(boxes, scores, dets, labels, num, 'cat', 'leastconf', 'mean', thr=0.3)['unc']
    assert np.allclose(s, [np.nansum(r['obj'][0]), np.nansum(r['obj'][1])], rtol=1e-15) and np.allclose(m, s / [3, 2], rtol=1e-15)
    # the gate is strict: a threshold equal to a detection's score drops it; rows >= num are never read
    thr = float(dets[0, 2, 4])
    g = U.reference(boxes, scores, dets, labels, num, 'cat', 'entropy', 'max', thr=thr)
    assert g['rows'][0].tolist() == [2, 0, -1] and g['count'].tolist() == [2, 2]
    poisoned, plab = dets.copy(), labels.copy()
    poisoned[1, 2], plab[1, 2] = np.nan, 10 ** 12
    assert np.array_equal(U.lookup(boxes, scores, poisoned, plab, num, 0.3), r['rows'])
    # nothing above the threshold (image 0; image 1 keeps its one-hot row: entropy 0) / num = 0: the image scores 0
    assert U.reference(boxes, scores, dets, labels, num, 'cat', 'entropy', 'sum', thr=0.95)['count'].tolist() == [0, 1]
    assert U.reference(boxes, scores, dets, labels, num, 'cat', 'entropy', 'sum', thr=0.95)['unc'].tolist() == [0, 0]
    assert U.reference(boxes, scores, dets, labels, np.zeros(2, np.int32), 'cat', 'entropy', 'sum')['unc'].tolist() == [0, 0]
    # a detection that matches no candidate is counted and skipped; a one-hot row has zero entropy
    lost = dets.copy()
    lost[0, 1, 0] += 1
    q = U.reference(boxes, scores, lost, labels, num, 'cat', 'entropy', 'max')
    assert q['rows'][0].tolist() == [2, -2, 1] and q['missing'].tolist() == [1, 0] and np.isnan(q['obj'][0, 1]) and q['obj'][1, 0] == 0
    # the same rows read as SSD rows use the fourth column too; as sigmoid rows they are Bernoulli posteriors
    assert np.isclose(U.reference(boxes, scores, dets, labels, num, 'cat_bg', 'entropy')['obj'][0, 1], r2 := U.measure64(scores[0, 0], 'cat_bg', 'entropy'))
    assert np.isclose(r2, U.measure64(scores[0, 0, :3], 'cat', 'entropy'))          # (the pad column is 0: 0 ln 0 = 0)
    assert U.reference(boxes, scores, dets, labels, num, 'sigmoid', 'entropy')['obj'][0, 1] > r2
    (ro, ao), (ru, au) = U.tolerances('margin', 'max')
    assert (ro, ao, ru, au) == (0.0, 4 * 2.0 ** -24, 0.0, 4 * 2.0 ** -24) and U.tolerances('margin', 'sum')[1] == (2e-5, 1e-7)
    assert U.tolerances('entropy', 'max') == ((2e-5, 1e-7), (2e-5, 1e-7))


def test_the_input_maker_is_seeded_and_keeps_its_range():
    a, b = U.make_maps(3, 20, 11), U.make_maps(3, 20, 11)
    assert all(torch.equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
    assert [tuple(t.shape) for t in a[0]] == [(3, U.A * 20, h, w) for h, w in U.LEVELS] and a[1][0].shape == (3, U.A * 4, 8, 8)
    assert all(float(t.abs().max()) <= 5 for t in a[0]) and float(a[0][0][2].abs().max()) <= 0.5        # the last image is quiet
    s = U.make_maps(2, 20, 11, sigmoid=True)[0][0]
    assert -3 <= float(s[1].min()) and float(s[1].max()) <= -1.5
    rows = a[0][0].permute(0, 2, 3, 1).reshape(3, -1, 20)
    assert float(rows[0, 5].max()) > 4.4 and float(rows[0, 5].sort().values[-3]) <= -2      # a pushed row: one class high, a runner-up, the rest low


# ---------------------------------------------------------------------------------------------------------------- argument checks
def _args(B=2, n=5, W=21, max_num=7):
    cand = SimpleNamespace(boxes=torch.zeros(B, n, 4), scores=torch.zeros(B, n, W))
    return cand, torch.zeros(B, max_num, 5), torch.zeros(B, max_num, dtype=torch.int64), torch.zeros(B, dtype=torch.int32)


def test_det_uncertainty_refuses_what_it_cannot_score():
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd._C import AodHipError
    assert scoring.POSTERIOR_POOLS == ('Entropy', 'Margin', 'LeastConf')
    assert scoring.UNC_LAYOUTS == {'cat': 0, 'cat_bg': 1, 'sigmoid': 2} and scoring.UNC_MEASURES == {'entropy': 0, 'margin': 1, 'leastconf': 2}
    assert scoring.UNC_AGGREGATES == {'max': 0, 'mean': 1, 'sum': 2}
    cand, dets, labels, num = _args()
    du = scoring.det_uncertainty
    for bad in ('softmax', 0, None):
        with pytest.raises(ValueError, match='unknown layout'):
            du(cand, dets, labels, num, bad)
    with pytest.raises(ValueError, match='unknown measure'):
        du(cand, dets, labels, num, 'cat', measure='Entropy')
    with pytest.raises(ValueError, match='unknown aggregate'):
        du(cand, dets, labels, num, 'cat', aggregate='avg')
    with pytest.raises(ValueError, match='score_thr is NaN'):
        du(cand, dets, labels, num, 'cat', score_thr=float('nan'))
    with pytest.raises(ValueError, match=r'cand\.scores is not a 3-D float32'):
        du(SimpleNamespace(boxes=cand.boxes, scores=cand.scores.double()), dets, labels, num, 'cat')
    with pytest.raises(ValueError, match=r'cand\.boxes is not a 3-D float32'):
        du(SimpleNamespace(boxes=cand.boxes[0], scores=cand.scores), dets, labels, num, 'cat')
    with pytest.raises(ValueError, match='labels is not a 2-D int64'):
        du(cand, dets, labels.int(), num, 'cat')
    with pytest.raises(ValueError, match='num is not a 1-D int32'):
        du(cand, dets, labels, num.long(), 'cat')
    with pytest.raises(ValueError, match='dets is not contiguous'):
        du(cand, torch.zeros(2, 7, 10)[:, :, ::2], labels, num, 'cat')
    with pytest.raises(ValueError, match=r'cand\.boxes has shape'):
        du(SimpleNamespace(boxes=torch.zeros(2, 4, 4), scores=cand.scores), dets, labels, num, 'cat')
    with pytest.raises(ValueError, match='dets has shape'):
        du(cand, torch.zeros(2, 7, 6), labels, num, 'cat')
    with pytest.raises(ValueError, match='1 <= max_num <= 1024'):
        du(cand, torch.zeros(2, 1025, 5), torch.zeros(2, 1025, dtype=torch.int64), num, 'cat')
    with pytest.raises(ValueError, match='labels has shape'):
        du(cand, dets, labels[:, :6].contiguous(), num, 'cat')
    with pytest.raises(ValueError, match='num has shape'):
        du(cand, dets, labels, torch.zeros(3, dtype=torch.int32), 'cat')
    with pytest.raises(ValueError, match='at least 2 columns'):
        du(SimpleNamespace(boxes=cand.boxes, scores=torch.zeros(2, 5, 1)), dets, labels, num, 'cat_bg')
    two = SimpleNamespace(boxes=cand.boxes, scores=torch.zeros(2, 5, 2))
    for layout in ('cat', 'sigmoid'):
        with pytest.raises(ValueError, match="'margin' needs two used columns"):
            du(two, dets, labels, num, layout, measure='margin')
    # what passes every check still needs the GPU: there is no CPU fallback
    for c, layout, measure in ((cand, 'cat', 'entropy'), (two, 'cat_bg', 'margin'), (two, 'sigmoid', 'leastconf')):
        with pytest.raises(AodHipError, match='CPU tensor'):
            du(c, dets, labels, num, layout, measure=measure, want_objects=True)


def _detector(config):
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, config))
    cfg.model.backbone.pop('init_cfg', None)
    return cfg, build_detector(cfg.model)


def test_pool_names_are_offered_and_a_plain_head_passes_refuse_hua():
    from aod_meh_hua_amd import apis, scoring
    from aod_meh_hua_amd.apis.test import Uncertainty_fns
    assert 'Posterior_uncertainty' in apis.__all__ and callable(apis.Posterior_uncertainty)
    for name in scoring.POSTERIOR_POOLS:
        assert callable(getattr(Uncertainty_fns, name)) and name not in scoring.HUA_POOLS
    assert scoring.ACTIVATION_LAYOUT == {'relu': 'cat', 'softmax': 'cat_bg', 'sigmoid': 'sigmoid'}
    cfg, model = _detector('configs/_base_/Config_RetinaNet_plain.py')
    head = model.bbox_head
    assert head.last_activation == 'sigmoid'
    for name in scoring.POSTERIOR_POOLS:
        scoring.refuse_hua(head, isEval=False, isUnc='Epistemic', uPool=name)              # no lambda is needed: not refused
    with pytest.raises(ValueError, match='has no lambda'):
        scoring.refuse_hua(head, isEval=False, isUnc='Epistemic', uPool='Entropy_NMS')     # (the HUA pools still are)
    with pytest.raises(ValueError, match='unknown measure'):
        apis.Posterior_uncertainty(cfg, model, None, measure='Entropy')
    with pytest.raises(ValueError, match='unknown aggregate'):
        apis.Posterior_uncertainty(cfg, model, None, aggregate='avg')
    with pytest.raises(ValueError, match='NaN'):
        apis.Posterior_uncertainty(cfg, model, None, score_thr=float('nan'))
    assert _detector('configs/_base_/Config_SSD.py')[1].bbox_head.last_activation == 'softmax'
    assert _detector('configs/_base_/Config_RetinaNet.py')[1].bbox_head.last_activation == 'relu'


def test_the_driver_parser_names_the_pools_and_the_aggregate(monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location('train_RetinaNet_for_posterior', os.path.join(ROOT, 'tools', 'train_RetinaNet.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--uncertainty-pool', 'Entropy', '--synthetic', '8'])
    args = drv.parse_args()
    assert args.uncertainty_pool == 'Entropy' and args.unc_aggregate == 'max' and args.hua_score_thr == 0.3
    for agg in ('max', 'mean', 'sum'):
        monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--uncertainty-pool', 'Margin', '--unc-aggregate', agg])
        assert drv.parse_args().unc_aggregate == agg
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--unc-aggregate', 'avg'])
    with pytest.raises(SystemExit):
        drv.parse_args()
    capsys.readouterr()
    monkeypatch.setattr(sys, 'argv', ['train_RetinaNet.py', '--help'])
    with pytest.raises(SystemExit):
        drv.parse_args()
    out = capsys.readouterr().out
    assert all(w in out for w in ('Entropy', 'Margin', 'LeastConf', '--unc-aggregate'))
    assert 'from train_RetinaNet import main' in open(os.path.join(ROOT, 'tools', 'train_SSD.py')).read()      # SSD gets both through the shared main


# ---------------------------------------------------------------------------------------------------------------- the C entry
@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.aod_last_error.restype = ctypes.c_char_p
    P, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    lib.aod_det_uncertainty.restype = ctypes.c_int
    lib.aod_det_uncertainty.argtypes = [P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, F32, P, P, P, P]
    return lib


def test_the_entry_is_declared_exported_and_documented(lib):
    hdr = open(os.path.join(ROOT, 'include', 'aod_hip.h')).read()
    assert 'DESIGN 3l' in hdr and 'Brust' in hdr and 'Roy' in hdr
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+aod_det_uncertainty\s*\(', hdr) and hasattr(lib, 'aod_det_uncertainty')
    from aod_meh_hua_amd import _C
    assert len(_C._SIGS['aod_det_uncertainty'][1]) == 17
    assert 'aod_det_uncertainty' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '3l' in design and 'aod_det_uncertainty' in design
    assert 'Posterior_uncertainty' in open(os.path.join(ROOT, 'README.md')).read()


def _call(lib, boxes=16, scores=16, dets=16, labels=16, num=16, B=2, n=300, W=21, max_num=100, layout=0, measure=0, aggregate=0, thr=0.3,
          unc=16, obj=16, missing=16):
    return lib.aod_det_uncertainty(boxes, scores, dets, labels, num, B, n, W, max_num, layout, measure, aggregate, thr, unc, obj, missing, None)


@pytest.mark.parametrize('kw, msg', [
    (dict(layout=3), b'layout 3'), (dict(layout=-1), b'layout -1'), (dict(measure=3), b'measure 3'), (dict(measure=-1), b'measure -1'),
    (dict(aggregate=3), b'aggregate 3'), (dict(aggregate=-2), b'aggregate -2'), (dict(W=1), b'at least 2 columns'), (dict(W=0), b'at least 2 columns'),
    (dict(W=2, measure=1), b'margin needs two used columns'), (dict(W=2, measure=1, layout=2), b'margin needs two used columns'),
    (dict(boxes=None), b'null pointer'), (dict(scores=None), b'null pointer'), (dict(dets=None), b'null pointer'), (dict(labels=None), b'null pointer'),
    (dict(num=None), b'null pointer'), (dict(unc=None), b'null pointer'), (dict(thr=float('nan')), b'score_thr is NaN'),
    (dict(max_num=0), b'max_num must be in 1..1024'), (dict(max_num=1025), b'max_num must be in 1..1024'), (dict(n=0), b'candidate row'),
    (dict(B=0), b'batch'), (dict(dets=18), b'aligned'), (dict(labels=20), b'aligned'),
])
def test_bad_arguments_are_rejected_without_a_gpu(lib, kw, msg):
    """validation precedes the launch: this machine has no GPU, a launch attempt would fail differently (-3) or crash"""
    assert _call(lib, **kw) == -1
    assert msg in lib.aod_last_error()
