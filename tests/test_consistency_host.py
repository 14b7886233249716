"""CPU tests (no GPU) of the consistency pool: the float64 restatement of tests/consistency_util.py on hand cases, the argument
checks of hipops.flip_images, scoring.det_posterior, scoring.det_consistency, apis.single_gpu_consistency and of the four C entries (all
before any launch), the pool name in Uncertainty_fns / apis.__all__, and the drivers' parser."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import consistency_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---------------------------------------------------------------------------------------------------------------- the restatement by hand
def _slots(V, B=1, max_num=3, W=4):
    dets = np.zeros((V + 1, B, max_num, 5), F)
    labels = np.zeros((V + 1, B, max_num), np.int64)
    num = np.zeros((V + 1, B), np.int32)
    post = np.zeros((V + 1, B, max_num, W), F)
    return dets, labels, num, post


def _mirror(box, code, ew, eh):
    x1, y1, x2, y2 = box
    if code & 1:
        x1, x2 = ew - x2, ew - x1
    if code & 2:
        y1, y2 = eh - y2, eh - y1
    return [x1, y1, x2, y2]


def test_exact_mirror_slots_with_equal_posteriors_score_exactly_zero():
    views = ('hflip', 'vflip', 'hvflip')
    dets, labels, num, post = _slots(3)
    ext = np.array([[64, 48]], F)
    clean = [[2, 3, 30, 40, .9], [5, 5, 9, 25, .5], [0, 0, 4, 4, .2]]
    rows = np.array([[.7, .2, .1, 0], [.25, .25, .5, 0], [.1, .1, .8, 0]], F)
    dets[0, 0], post[0, 0], num[0, 0] = clean, rows, 3
    for v, name in enumerate(views):
        dets[v + 1, 0] = [_mirror(r[:4], U.VIEWS[name], 64, 48) + [r[4]] for r in clean]
        post[v + 1, 0], num[v + 1, 0] = rows, 3
    for layout in U.LAYOUTS:
        for mode in U.MODES:
            for aggregate in U.AGGREGATES:
                r = U.reference(dets, labels, num, post, views, ext, layout, mode, aggregate)
                assert r['unc'].tolist() == [0.0] and r['count'].tolist() == [2]
                assert r['obj'][0, :2].tolist() == [0.0, 0.0] and np.isnan(r['obj'][0, 2])
                assert (r['iou'][:, 0, :2] == 1.0).all() and (r['js'][:, 0, :2] == 0.0).all() and np.isnan(r['iou'][:, 0, 2]).all()
                assert (r['match'][:, 0, :2] == [0, 1]).all() and (r['match'][:, 0, 2] == -1).all()


def test_empty_view_the_strict_gate_and_rows_behind_num():
    dets, labels, num, post = _slots(1, B=2)
    ext = np.array([[32, 32], [32, 32]], F)
    dets[0, 0, 0] = [0, 0, 10, 10, .8]
    dets[0, 1, 0] = [0, 0, 10, 10, F(.3)]                             # exactly the threshold: no object
    post[0, :, 0] = [.5, .5, 0, 0]
    num[0] = [1, 1]
    for mode in ('box', 'cls', 'both'):
        r = U.reference(dets, labels, num, post, ('hflip',), ext, 'cat', mode)
        assert r['unc'].tolist() == [1.0, 0.0] and r['count'].tolist() == [1, 0]
        assert r['match'][0, 0, 0] == -1 and r['iou'][0, 0, 0] == 0.0 and r['js'][0, 0, 0] == 1.0 and np.isnan(r['obj'][1]).all()
    below = float(np.nextafter(F(.3), F(0)))
    assert U.reference(dets, labels, num, post, ('hflip',), ext, 'cat', score_thr=below)['count'].tolist() == [1, 1]
    # rows >= num are never read: NaN there changes nothing
    want = U.reference(dets, labels, num, post, ('hflip',), ext, 'cat')
    dets[1:], post[1:], dets[0, :, 1:], post[0, :, 1:] = np.nan, np.nan, np.nan, np.nan
    labels[1:], labels[0, :, 1:] = 10 ** 12, -7
    got = U.reference(dets, labels, num, post, ('hflip',), ext, 'cat')
    for k in ('unc', 'obj', 'iou', 'js', 'match', 'count'):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    # a box that touches nothing: a best IoU of 0 is no match
    dets[1, 0, 0], num[1, 0] = [0, 0, 5, 5, .9], 1                     # un-flipped: x in 27..32
    post[1, 0, 0] = [.5, .5, 0, 0]
    r = U.reference(dets, labels, num, post, ('hflip',), ext, 'cat', 'cls')
    assert r['match'][0, 0, 0] == -1 and r['unc'][0] == 1.0
    num[0] = [0, 0]
    assert U.reference(dets, labels, num, post, ('hflip',), ext, 'cat')['unc'].tolist() == [0.0, 0.0]


def test_same_class_hides_a_better_box_and_the_lowest_index_wins_a_tie():
    dets, labels, num, post = _slots(1, max_num=4)
    ext = np.array([[40, 40]], F)
    dets[0, 0, 0], labels[0, 0, 0], num[0, 0] = [10, 10, 20, 20, .9], 1, 1
    post[0, 0, 0] = [.5, .25, .25, 0]
    # the view, already in un-flipped terms: row 0 shifted by 5 (IoU 50 / 150) with label 1, row 1 the box itself with label 2, rows 2
    # and 3 equal copies shifted by 2 in y (IoU 80 / 120) with label 1
    back = [[15, 10, 25, 20], [10, 10, 20, 20], [10, 12, 20, 22], [10, 12, 20, 22]]
    dets[1, 0, :, :4] = [_mirror(b, 1, 40, 40) for b in back]
    dets[1, 0, :, 4], labels[1, 0], num[1, 0] = .5, [1, 2, 1, 1], 4
    post[1, 0] = [[.5, .25, .25, 0], [.25, .5, .25, 0], [.5, .25, .25, 0], [0, 0, 1, 0]]
    off = U.reference(dets, labels, num, post, ('hflip',), ext, 'cat', 'box')
    on = U.reference(dets, labels, num, post, ('hflip',), ext, 'cat', 'box', same_class=True)
    assert off['match'][0, 0, 0] == 1 and off['iou'][0, 0, 0] == 1.0 and off['unc'][0] == 0.0
    assert on['match'][0, 0, 0] == 2 and np.isclose(on['iou'][0, 0, 0], float(F(80) / F(120)), rtol=0, atol=0)      # rows 2, 3 tie: the lower
    assert np.isclose(on['unc'][0], 1 - float(F(80) / F(120)), rtol=1e-15)
    # the class term follows the match: row 1 has other posteriors, row 2 the same
    assert U.reference(dets, labels, num, post, ('hflip',), ext, 'cat', 'cls', same_class=True)['unc'][0] == 0.0
    p, q = np.array([.5, .25, .25]), np.array([.25, .5, .25])
    m = (p + q) / 2
    js = 0.5 * float(np.sum(p * np.log(p / m) + q * np.log(q / m))) / np.log(2)
    r = U.reference(dets, labels, num, post, ('hflip',), ext, 'cat', 'cls')
    assert np.isclose(r['js'][0, 0, 0], js, rtol=1e-13) and np.isclose(r['unc'][0], js, rtol=1e-13)
    both = U.reference(dets, labels, num, post, ('hflip',), ext, 'cat', 'both')
    assert np.isclose(both['unc'][0], 0.5 * ((1 - 1.0) + js), rtol=1e-13)


def test_layouts_known_values_views_in_order_and_aggregates():
    # disjoint one-hot rows are one bit apart; cat drops the last column, cat_bg reads it
    assert U.js64(np.array([1, 0, 0, 0], F), np.array([0, 1, 0, 0], F), 'cat') == 1.0
    assert U.js64(np.array([0, 0, 0, 1], F), np.array([0, 0, 1, 0], F), 'cat_bg') == 1.0
    assert np.isclose(U.js64(np.array([0, 0, 0, 1], F), np.array([0, 0, 1, 0], F), 'cat'), 0.5, rtol=1e-15)      # (sub-distributions: t >= 0 still)
    # sigmoid: the mean over the used columns of the Bernoulli divergence; Bernoulli(1) against Bernoulli(0) is one bit, equal ones 0
    assert U.js64(np.array([1, .5, 9], F), np.array([0, .5, 7], F), 'sigmoid') == 0.5
    a, b = 0.75, 0.25
    m = 0.5
    bern = (0.5 * (a * np.log(a / m) + b * np.log(b / m)) + 0.5 * ((1 - a) * np.log((1 - a) / m) + (1 - b) * np.log((1 - b) / m))) / np.log(2)
    assert np.isclose(U.js64(np.array([.75, 0], F), np.array([.25, 0], F), 'sigmoid'), bern, rtol=1e-14)
    assert np.isclose(bern, 1 - (-(.75 * np.log2(.75) + .25 * np.log2(.25))), rtol=1e-14)          # H(1/2) - H(3/4) in bits
    assert (U.term64(np.array([.3, 0, 1e-30]), np.array([.3, 0, 1e-30])) == 0).all() and (U.term64(np.random.default_rng(0).random(99), .5) >= 0).all()
    # two objects, two views: u_j is the mean over the views, then max / mean / sum
    dets, labels, num, post = _slots(2, max_num=2, W=3)
    ext = np.array([[50, 60]], F)
    dets[0, 0], num[0, 0] = [[0, 0, 10, 10, .9], [20, 20, 30, 40, .5]], 2
    dets[1, 0, :, :4] = [_mirror(b, 1, 50, 60) for b in ([5, 0, 15, 10], [20, 20, 30, 40])]             # hflip: IoU 50 / 150 and 1
    dets[2, 0, :1, :4] = [_mirror([0, 0, 10, 5], 2, 50, 60)]                                             # vflip: IoU 1 / 2, object 1 unmatched
    num[1:, 0] = [2, 1]
    post[:] = [.5, .5, 0]
    pt = U.parts(dets, labels, num, post, ('hflip', 'vflip'), ext, 'cat')
    assert pt['match'][:, 0].tolist() == [[0, 1], [0, -1]]
    u0, u1 = ((1 - 1 / 3) + .5) / 2, (0 + 1) / 2
    for aggregate, want in (('max', max(u0, u1)), ('mean', (u0 + u1) / 2), ('sum', u0 + u1)):
        r = U.combine(pt, 'box', aggregate)
        assert np.isclose(r['unc'][0], want, rtol=1e-7) and np.allclose(r['obj'][0], [u0, u1], rtol=1e-7)
    assert U.bound_obj(21, 'cat', 1) == (80 + 4 + 32) * 2.0 ** -24 and U.bound_obj(21, 'cat_bg', 3) == (84 + 12 + 32) * 2.0 ** -24
    assert U.bound_obj(21, 'sigmoid', 1) == (160 + 4 + 32) * 2.0 ** -24
    assert U.bound_unc(3, 'cat', 1, 'sum', [0, 2]).tolist() == [0.0, 2 * (8 + 4 + 32 + 16) * 2.0 ** -24]
    assert U.fraction_of_bound([0.0, 1e-9], [0.0, 0.0], 1.0) == np.inf and U.fraction_of_bound([0.0, np.nan], [0.0, np.nan], 1.0) == 0.0


# ---------------------------------------------------------------------------------------------------------------- wrappers
def _stack(V=1, B=2, max_num=4, W=5):
    return (torch.zeros(V + 1, B, max_num, 5), torch.zeros(V + 1, B, max_num, dtype=torch.int64), torch.zeros(V + 1, B, dtype=torch.int32),
            torch.zeros(V + 1, B, max_num, W))


def test_det_consistency_wrapper_refuses_before_any_launch():
    from aod_meh_hua_amd import _C, scoring
    d, l, n, p = _stack()
    ext = torch.ones(2, 2)
    with pytest.raises(ValueError, match='unknown view'):
        scoring.det_consistency(d, l, n, p, ('flip',), ext, 'cat')
    with pytest.raises(ValueError, match='sequence of view names'):
        scoring.det_consistency(d, l, n, p, 'hflip', ext, 'cat')
    with pytest.raises(ValueError, match='distinct'):
        scoring.det_consistency(*_stack(V=2), ('hflip', 'hflip'), ext, 'cat')
    for views in ((), ('hflip', 'vflip', 'hvflip', 'hflip')):
        with pytest.raises(ValueError, match='1..3 views'):
            scoring.det_consistency(d, l, n, p, views, ext, 'cat')
    with pytest.raises(ValueError, match='slots'):
        scoring.det_consistency(d, l, n, p, ('hflip', 'vflip'), ext, 'cat')
    with pytest.raises(ValueError, match='unknown layout'):
        scoring.det_consistency(d, l, n, p, ('hflip',), ext, 'softmax')
    with pytest.raises(ValueError, match='unknown mode'):
        scoring.det_consistency(d, l, n, p, ('hflip',), ext, 'cat', mode='iou')
    with pytest.raises(ValueError, match='unknown aggregate'):
        scoring.det_consistency(d, l, n, p, ('hflip',), ext, 'cat', aggregate='min')
    with pytest.raises(ValueError, match='score_thr is NaN'):
        scoring.det_consistency(d, l, n, p, ('hflip',), ext, 'cat', score_thr=float('nan'))
    for max_num in (0, 1025):
        with pytest.raises(ValueError, match='max_num'):
            scoring.det_consistency(*_stack(max_num=max_num), ('hflip',), ext, 'cat')
    with pytest.raises(ValueError, match='labels has shape'):
        scoring.det_consistency(d, l[:, :, :3].contiguous(), n, p, ('hflip',), ext, 'cat')
    with pytest.raises(ValueError, match='num has shape'):
        scoring.det_consistency(d, l, n[:, :1].contiguous(), p, ('hflip',), ext, 'cat')
    with pytest.raises(ValueError, match='post has shape'):
        scoring.det_consistency(d, l, n, p[..., :1].contiguous(), ('hflip',), ext, 'cat')
    with pytest.raises(ValueError, match='post has shape'):
        scoring.det_consistency(d, l, n, p[:, :, :3].contiguous(), ('hflip',), ext, 'cat')
    with pytest.raises(ValueError, match='ext has shape'):
        scoring.det_consistency(d, l, n, p, ('hflip',), torch.ones(3, 2), 'cat')
    with pytest.raises(ValueError, match='4-D float32'):
        scoring.det_consistency(d.double(), l, n, p, ('hflip',), ext, 'cat')
    with pytest.raises(ValueError, match='2-D float32'):
        scoring.det_consistency(d, l, n, p, ('hflip',), ext.double(), 'cat')
    with pytest.raises(ValueError, match='not contiguous'):
        scoring.det_consistency(d, l, n, p.transpose(1, 2).contiguous().transpose(1, 2), ('hflip',), ext, 'cat')
    with pytest.raises(_C.AodHipError, match='no CPU fallback'):
        scoring.det_consistency(d, l, n, p, ('hflip',), ext, 'cat')
    assert scoring.CONSISTENCY_VIEWS == {'hflip': 1, 'vflip': 2, 'hvflip': 3} and scoring.CONSISTENCY_MODES == {'box': 0, 'cls': 1, 'both': 2}
    assert scoring.CONSISTENCY_MAX_VIEWS == 3


def test_det_posterior_wrapper_refuses_before_any_launch():
    from aod_meh_hua_amd import _C, scoring
    cand = scoring.Candidates(torch.zeros(2, 7, 4), torch.zeros(2, 7, 5), None, None, None, None, None)
    d, l, n = torch.zeros(2, 4, 5), torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match='labels has shape'):
        scoring.det_posterior(cand, d, l[:, :3].contiguous(), n)
    with pytest.raises(ValueError, match='num has shape'):
        scoring.det_posterior(cand, d, l, n[:1].contiguous())
    with pytest.raises(ValueError, match='dets has shape'):
        scoring.det_posterior(cand, torch.zeros(2, 1025, 5), l, n)
    with pytest.raises(ValueError, match='cand.boxes'):
        scoring.det_posterior(object(), d, l, n)
    with pytest.raises(ValueError, match='3-D float32'):
        scoring.det_posterior(cand, d.double(), l, n)
    with pytest.raises(_C.AodHipError, match='no CPU fallback'):
        scoring.det_posterior(cand, d, l, n)


def test_flip_images_wrapper_refuses_before_any_launch():
    from aod_meh_hua_amd import _C
    from aod_meh_hua_amd import hipops as ho
    src, dst = torch.zeros(2, 3, 8, 15), torch.zeros(2, 3, 8, 15)
    hw = torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match='out of place'):
        ho.flip_images(src, src, hw, 'hflip')
    with pytest.raises(ValueError, match='out of place'):
        buf = torch.zeros(3, 3, 8, 15)
        ho.flip_images(buf[:2], buf[1:], hw, 'hflip')
    for view in ('flip', 0, 4, None, True, 1.0):
        with pytest.raises(ValueError, match='unknown view'):
            ho.flip_images(src, dst, hw, view)
    with pytest.raises(ValueError, match='dst has shape'):
        ho.flip_images(src, torch.zeros(2, 3, 8, 16), hw, 'hflip')
    with pytest.raises(ValueError, match='contiguous fp32'):
        ho.flip_images(src.double(), dst, hw, 'hflip')
    with pytest.raises(ValueError, match='contiguous fp32'):
        ho.flip_images(src, torch.zeros(2, 3, 15, 8).transpose(2, 3), hw, 'hflip')
    with pytest.raises(ValueError, match='contiguous fp32'):
        ho.flip_images(src[0], dst[0], hw, 'hflip')
    with pytest.raises(ValueError, match='hw must be'):
        ho.flip_images(src, dst, hw.float(), 'vflip')
    with pytest.raises(ValueError, match='hw must be'):
        ho.flip_images(src, dst, hw[:1], 'vflip')
    for view in ('hflip', 'vflip', 'hvflip', 1, 2, 3):
        with pytest.raises(_C.AodHipError, match='no CPU fallback'):
            ho.flip_images(src, dst, hw, view)
    assert ho.FLIP_VIEWS == {'hflip': 1, 'vflip': 2, 'hvflip': 3}


def test_pool_pass_refuses_bad_options_and_computes_the_frame_extent():
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis import test as T
    for views in ((), ('hflip', 'vflip', 'hvflip', 'hflip'), 'hflip', 3):
        with pytest.raises(ValueError, match='views'):
            apis.single_gpu_consistency(None, None, views=views)
    with pytest.raises(ValueError, match='unknown view'):
        apis.single_gpu_consistency(None, None, views=('hflip', 'rot90'))
    with pytest.raises(ValueError, match='distinct'):
        apis.single_gpu_consistency(None, None, views=['vflip', 'vflip'])
    with pytest.raises(ValueError, match='unknown mode'):
        apis.single_gpu_consistency(None, None, mode='js')
    with pytest.raises(ValueError, match='unknown aggregate'):
        apis.single_gpu_consistency(None, None, aggregate='median')
    with pytest.raises(ValueError, match='score_thr is NaN'):
        apis.single_gpu_consistency(None, None, score_thr=float('nan'))
    metas = [dict(img_shape=(300, 400, 3), scale_factor=np.array([0.8, 0.75, 0.8, 0.75], np.float32)), dict(img_shape=(128, 96, 3)),
             dict(img_shape=(10, 20, 3), scale_factor=2.0)]
    assert T._frame_extent(metas) == ((400.0 / float(F(0.8)), 300.0 / 0.75), (96.0, 128.0), (10.0, 5.0))
    with pytest.raises(ValueError, match='finite positive'):
        T._frame_extent([dict(img_shape=(10, 20, 3), scale_factor=[1.0, 0.0, 1.0, 0.0])])


def test_pool_name_exists_and_ignores_the_hua_kwargs(monkeypatch):
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis import test as T
    assert 'Consistency_uncertainty' in apis.__all__ and 'single_gpu_consistency' in apis.__all__
    assert callable(apis.Consistency_uncertainty) and callable(apis.single_gpu_consistency)
    seen = []
    monkeypatch.setattr(T, 'Consistency_uncertainty', lambda cfg, model, loader, **kw: seen.append(kw) or torch.zeros(3))
    cfg = type('Cfg', (), {})()
    cfg.uncertainty_pool = 'Consistency'
    hua = dict(return_box=False, showNMS=False, saveUnc=False, saveMaxConf=False, clsW=False, scaleUnc=False, score_thr=0.25, iou_thr=0.9)
    out = apis.calculate_uncertainty(cfg, 'model', 'loader', views=('hflip', 'vflip'), mode='cls', unc_aggregate='mean', **hua)
    assert torch.equal(out, torch.zeros(3))
    assert seen[-1] == dict(score_thr=0.25, views=('hflip', 'vflip'), mode='cls', aggregate='mean')
    apis.calculate_uncertainty(cfg, 'model', 'loader', **dict(hua, score_thr=None), same_class=True)
    assert seen[-1] == dict(score_thr=0.3, same_class=True)


def test_both_drivers_parse_the_new_flags(monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location('train_RetinaNet_for_consistency', os.path.join(ROOT, 'tools', 'train_RetinaNet.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    monkeypatch.setenv('LOCAL_RANK', '0')
    for config, size in (('configs/_base_/Config_RetinaNet.py', 512), ('configs/_base_/Config_SSD.py', 300)):      # train_SSD.py: main(config, 300)
        monkeypatch.setattr(sys, 'argv', ['drv.py', '--uncertainty-pool', 'Consistency'])
        args = drv.parse_args(config, size)
        assert args.uncertainty_pool == 'Consistency' and args.consistency_view_names == ('hflip',) and args.consistency_mode == 'both'
        assert args.unc_aggregate == 'max'
        monkeypatch.setattr(sys, 'argv', ['drv.py', '--uncertainty-pool', 'Consistency', '--consistency-views', 'hflip,vflip, hvflip',
                                          '--consistency-mode', 'box', '--unc-aggregate', 'mean'])
        args = drv.parse_args(config, size)
        assert args.consistency_view_names == ('hflip', 'vflip', 'hvflip') and args.consistency_mode == 'box' and args.unc_aggregate == 'mean'
    for flag, bad in (('--consistency-views', 'hflip,rot90'), ('--consistency-views', ''), ('--consistency-views', 'hflip,hflip'),
                      ('--consistency-views', 'hflip,vflip,hvflip,hflip'), ('--consistency-mode', 'iou'), ('--consistency-mode', '')):
        monkeypatch.setattr(sys, 'argv', ['drv.py', flag, bad])                                    # refused at start-up
        with pytest.raises(SystemExit):
            drv.parse_args()
    capsys.readouterr()
    monkeypatch.setattr(sys, 'argv', ['drv.py', '--help'])
    with pytest.raises(SystemExit):
        drv.parse_args()
    out = capsys.readouterr().out
    assert all(w in out for w in ('Consistency', '--consistency-views', '--consistency-mode', 'Elezi', 'CALD'))
    assert 'from train_RetinaNet import main' in open(os.path.join(ROOT, 'tools', 'train_SSD.py')).read()          # SSD shares the parser and the loop


# ---------------------------------------------------------------------------------------------------------------- the C entries
@pytest.fixture(scope='module')
def lib():
    from aod_meh_hua_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.aod_last_error.restype = ctypes.c_char_p
    P, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    lib.aod_flip_images.restype = lib.aod_det_posterior.restype = lib.aod_det_consistency.restype = ctypes.c_int
    lib.aod_flip_images.argtypes = [P, P, I32, I32, I32, I32, P, I32, P]
    lib.aod_det_posterior.argtypes = [P, P, P, I32, I32, I32, I32, P, P, P]
    lib.aod_det_consistency.argtypes = [P, P, P, P, I32, P, P, I32, I32, I32, I32, I32, I32, F32, I32, P, P, P, P, P, P]
    return lib


def test_the_entries_are_declared_exported_and_documented(lib):
    hdr = open(os.path.join(ROOT, 'include', 'aod_hip.h')).read()
    assert 'DESIGN 3q' in hdr and 'Elezi' in hdr and 'CALD' in hdr
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    from aod_meh_hua_amd import _C
    for name, n in (('aod_flip_images', 9), ('aod_det_posterior', 10), ('aod_det_consistency', 21), ('aod_consistency_max_views', 0)):
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr) and hasattr(lib, name) and len(_C._SIGS[name][1]) == n
        assert name in open(os.path.join(ROOT, 'DESIGN.md')).read()
    for name in ('aod_flip_images', 'aod_det_posterior', 'aod_det_consistency'):
        assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert '3q' in open(os.path.join(ROOT, 'DESIGN.md')).read()
    from aod_meh_hua_amd import scoring
    assert lib.aod_consistency_max_views() == scoring.CONSISTENCY_MAX_VIEWS == 3          # written once, in the C source
    assert 'Consistency' in open(os.path.join(ROOT, 'README.md')).read()


def _flip(lib, src=4096, dst=1 << 20, B=2, C=3, Hp=8, Wp=15, hw=16, flip=1):
    return lib.aod_flip_images(src, dst, B, C, Hp, Wp, hw, flip, None)


@pytest.mark.parametrize('kw, msg', [
    (dict(flip=0), b'flip 0'), (dict(flip=4), b'flip 4'), (dict(flip=-1), b'flip -1'), (dict(Wp=0), b'padded width'), (dict(Wp=262145), b'padded width'),
    (dict(Hp=0), b'padded height'), (dict(Hp=65537), b'padded height'), (dict(C=0), b'channels'), (dict(B=0), b'batch'), (dict(B=65536), b'batch'),
    (dict(dst=4096), b'dst == src'), (dict(dst=4096 + 64), b'overlaps'), (dict(src=(1 << 20) + 64), b'overlaps'), (dict(src=None), b'null pointer'),
    (dict(dst=None), b'null pointer'), (dict(hw=None), b'null pointer'), (dict(src=4098), b'aligned'), (dict(dst=(1 << 20) + 1), b'aligned'),
    (dict(hw=18), b'aligned'),
])
def test_flip_images_entry_rejects_bad_arguments_without_a_gpu(lib, kw, msg):
    """validation precedes the launch: this machine has no GPU, a launch attempt would fail differently (-3) or crash"""
    assert _flip(lib, **kw) == -1
    assert msg in lib.aod_last_error()


def _post(lib, scores=16, cand=32, num=48, B=2, n=100, W=21, max_num=100, post=1 << 20, missing=64):
    return lib.aod_det_posterior(scores, cand, num, B, n, W, max_num, post, missing, None)


@pytest.mark.parametrize('kw, msg', [
    (dict(B=0), b'batch'), (dict(n=0), b'candidate rows'), (dict(W=1), b'columns'), (dict(max_num=0), b'max_num must be in 1..1024'),
    (dict(max_num=1025), b'max_num must be in 1..1024'), (dict(scores=None), b'null pointer'), (dict(cand=None), b'null pointer'),
    (dict(num=None), b'null pointer'), (dict(post=None), b'null pointer'), (dict(scores=18), b'aligned'), (dict(cand=33), b'aligned'),
    (dict(num=50), b'aligned'), (dict(post=(1 << 20) + 2), b'aligned'), (dict(missing=66), b'aligned'),
])
def test_det_posterior_entry_rejects_bad_arguments_without_a_gpu(lib, kw, msg):
    assert _post(lib, **kw) == -1
    assert msg in lib.aod_last_error()


def _cons(lib, dets=16, labels=32, num=48, post=64, V=2, flips=(1, 2, 0), ext=80, B=2, max_num=100, W=21, layout=0, mode=2, aggregate=0, thr=0.3,
          same_class=0, unc=96, obj=112, iou=128, js=144, match=160):
    fl = (ctypes.c_int32 * 3)(*flips) if flips is not None else None
    return lib.aod_det_consistency(dets, labels, num, post, V, fl, ext, B, max_num, W, layout, mode, aggregate, thr, same_class, unc, obj, iou, js,
                                   match, None)


@pytest.mark.parametrize('kw, msg', [
    (dict(V=0), b'V must be in 1..3'), (dict(V=4), b'V must be in 1..3'), (dict(B=0), b'batch'), (dict(max_num=0), b'max_num must be in 1..1024'),
    (dict(max_num=1025), b'max_num must be in 1..1024'), (dict(W=1), b'columns'), (dict(layout=3), b'layout 3'), (dict(layout=-1), b'layout -1'),
    (dict(mode=3), b'mode 3'), (dict(mode=-1), b'mode -1'), (dict(aggregate=3), b'aggregate 3'), (dict(aggregate=-1), b'aggregate -1'),
    (dict(same_class=2), b'same_class'), (dict(thr=float('nan')), b'score_thr is NaN'), (dict(flips=(1, 0, 0)), b'flips[1] = 0'),
    (dict(flips=(4, 1, 0)), b'flips[0] = 4'), (dict(V=3), b'flips[2] = 0'), (dict(dets=None), b'null pointer'), (dict(labels=None), b'null pointer'),
    (dict(num=None), b'null pointer'), (dict(post=None), b'null pointer'), (dict(flips=None), b'null pointer'), (dict(ext=None), b'null pointer'),
    (dict(unc=None), b'null pointer'), (dict(dets=18), b'aligned'), (dict(labels=36), b'aligned'), (dict(num=49), b'aligned'),
    (dict(post=66), b'aligned'), (dict(ext=82), b'aligned'), (dict(unc=97), b'aligned'), (dict(obj=114), b'aligned'), (dict(iou=130), b'aligned'),
    (dict(js=146), b'aligned'), (dict(match=161), b'aligned'),
])
def test_det_consistency_entry_rejects_bad_arguments_without_a_gpu(lib, kw, msg):
    assert _cons(lib, **kw) == -1
    assert msg in lib.aod_last_error()
