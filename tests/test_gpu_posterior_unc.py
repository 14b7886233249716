"""GPU: the posterior uncertainty pools -- aod_det_uncertainty (scoring.det_uncertainty) behind the real pre_nms +
multiclass_nms_batch outputs of small maps against the float64 restatement of tests/posterior_unc_util.py, its edges and bit properties,
and the pool pass apis.Posterior_uncertainty on the three detector families (eager, replayed, batch sizes), and the driver.

Tolerances (posterior_unc_util, derived in the issue): entropy values and every sum / mean aggregate rtol 2e-5, atol 1e-7; margin / least
confidence per object and their max atol 4 * 2^-24."""
import functools
import itertools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import posterior_unc_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(layout, C, B=3, max_num=100, thr=0.3):
    """the device path's own tensors for seeded maps: pre_nms (nms_pre = 100 on levels of 576 / 144 / 36 / 9 / 9 anchors per image) and
    multiclass_nms_batch (score_thr 0.05, IoU 0.5); checked on the host by posterior_unc_util.check_case"""
    from aod_meh_hua_amd import scoring
    from aod_meh_hua_amd.core.anchor import AnchorGenerator
    has_bg, sigmoid = layout == 'cat_bg', layout == 'sigmoid'
    C_ = C + 1 if has_bg else C
    cls, reg = U.make_maps(B, C_, 1000 + 7 * C + len(layout), quiet_scale=0.02 if C == 2 else 0.1, sigmoid=sigmoid, has_bg=has_bg)
    cls, reg = [c.cuda() for c in cls], [r.cuda() for r in reg]
    ag = AnchorGenerator(octave_base_scale=4, scales_per_octave=3, ratios=[0.5, 1.0, 2.0], strides=[8, 16, 32, 64, 128])
    anchors = ag.grid_anchors([tuple(c.shape[-2:]) for c in cls], 'cuda')
    lam = [torch.zeros(B, U.A, *c.shape[-2:], device='cuda') for c in cls]
    cand = scoring.pre_nms(cls, reg, lam, anchors, [(64, 64, 3)] * B, None, U.NMS_PRE, C_, (0., 0., 0., 0.), (1., 1., 1., 1.), rescale=False,
                           has_bg=has_bg, activation='sigmoid' if sigmoid else None)
    dets, labels, keep, num = scoring.multiclass_nms_batch(cand.boxes, cand.scores, 0.05, 0.5, max_num)
    torch.cuda.synchronize()
    host = tuple(_np(t) for t in (cand.boxes, cand.scores, dets, labels, num))
    assert cand.scores.shape == (B, 254, C_ if has_bg else C + 1)
    n_obj = U.check_case(*host, thr)
    print(f'case {layout} C={C} B={B} max_num={max_num} thr={thr}: num {host[4].tolist()}, objects {n_obj.tolist()}')
    return SimpleNamespace(cand=cand, dets=dets, labels=labels, num=num, host=host, n_obj=n_obj, thr=thr, layout=layout)


def _compare(c, measure, aggregate, what, thr=None):
    from aod_meh_hua_amd import scoring
    thr = c.thr if thr is None else thr
    unc, obj, missing = scoring.det_uncertainty(c.cand, c.dets, c.labels, c.num, c.layout, measure, aggregate, thr, want_objects=True)
    alone = scoring.det_uncertainty(c.cand, c.dets, c.labels, c.num, c.layout, measure, aggregate, thr)
    want = U.reference(*c.host, c.layout, measure, aggregate, thr)
    tol_obj, tol_unc = U.tolerances(measure, aggregate)
    eo = np.nanmax(np.abs(_np(obj).astype(np.float64) - want['obj'])) if np.isfinite(want['obj']).any() else 0.0
    eu = np.abs(_np(unc).astype(np.float64) - want['unc']).max()
    print(f'{what} {measure}/{aggregate}: unc {_np(unc).tolist()}, max obj err {eo:.3e} (rtol {tol_obj[0]:g} atol {tol_obj[1]:.3g}), '
          f'max unc err {eu:.3e} (rtol {tol_unc[0]:g} atol {tol_unc[1]:.3g})')
    assert unc.dtype == torch.float32 and unc.shape == (c.dets.shape[0],) and obj.shape == tuple(c.dets.shape[:2]) and missing.dtype == torch.int32
    assert _np(missing).tolist() == [0] * c.dets.shape[0] and want['missing'].sum() == 0
    assert np.array_equal(np.isnan(_np(obj)), want['rows'] < 0)              # NaN exactly on the rows that are no object
    assert U.close(_np(obj), want['obj'], tol_obj), what
    assert U.close(_np(unc), want['unc'], tol_unc), what
    assert torch.equal(_bits(alone), _bits(unc))                            # the nullable outputs change nothing
    assert (_np(unc) >= 0).all() and _np(unc)[-1] == 0 and (_np(unc)[:-1] > 0).all()
    return unc, obj, want


# ---------------------------------------------------------------------------------------------------------------- kernel against the util
@pytest.mark.parametrize('layout, measure, aggregate', list(itertools.product(U.LAYOUTS, U.MEASURES, U.AGGREGATES)))
def test_kernel_matches_float64(layout, measure, aggregate):
    _compare(_case(layout, 20), measure, aggregate, f'{layout} C=20')


@pytest.mark.parametrize('layout, C, B, max_num, thr', [('cat', 20, 3, 7, 0.3), ('cat_bg', 20, 2, 7, 0.3), ('sigmoid', 20, 3, 7, 0.3),
                                                        ('sigmoid', 80, 2, 100, 0.3), ('cat', 80, 2, 100, 0.3), ('cat', 2, 3, 100, 0.6),
                                                        ('sigmoid', 2, 2, 100, 0.3)])
def test_kernel_matches_float64_at_other_widths_and_detection_counts(layout, C, B, max_num, thr):
    c = _case(layout, C, B, max_num, thr)
    if max_num == 7:
        assert int(c.num.max()) == max_num                               # num = max_num: the last row is an object candidate too
    for measure, aggregate in itertools.product(U.MEASURES, U.AGGREGATES):
        _compare(c, measure, aggregate, f'{layout} C={C} max_num={max_num}')


# ---------------------------------------------------------------------------------------------------------------- edges
def test_no_detection_scores_zero_and_the_tail_is_never_read():
    from aod_meh_hua_amd import scoring
    c = _case('cat', 20)
    zero = torch.zeros_like(c.num)
    for measure, aggregate in itertools.product(U.MEASURES, U.AGGREGATES):
        unc, obj, missing = scoring.det_uncertainty(c.cand, c.dets, c.labels, zero, 'cat', measure, aggregate, want_objects=True)
        assert _np(unc).tolist() == [0.0] * 3 and bool(torch.isnan(obj).all()) and _np(missing).tolist() == [0] * 3
    # rows >= num filled with NaN and garbage labels: the same bits as the zero tail the NMS kernel leaves
    num = torch.minimum(c.num, torch.tensor([60, 100, 5], dtype=torch.int32, device='cuda'))          # (the case fills all 100 rows: cut two lists short)
    tail = torch.arange(c.dets.shape[1], device='cuda')[None, :] >= num[:, None]
    assert bool(tail[0].any()) and bool(tail[2].any()) and int(c.n_obj[0]) >= 2
    zd, zl, gd, gl = c.dets.clone(), c.labels.clone(), c.dets.clone(), c.labels.clone()
    zd[tail], zl[tail] = 0.0, -1
    gd[tail], gl[tail] = float('nan'), 10 ** 12
    gl[:, -1][tail[:, -1]] = -7
    for measure, aggregate in (('entropy', 'sum'), ('margin', 'mean'), ('leastconf', 'max')):
        ref = scoring.det_uncertainty(c.cand, zd, zl, num, 'cat', measure, aggregate, want_objects=True)
        got = scoring.det_uncertainty(c.cand, gd, gl, num, 'cat', measure, aggregate, want_objects=True)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ref, got))
        want = U.reference(*c.host[:2], _np(gd), _np(gl), _np(num), 'cat', measure, aggregate)
        assert U.close(_np(got[0]), want['unc'], U.tolerances(measure, aggregate)[1]) and np.array_equal(np.isnan(_np(got[1])), want['rows'] < 0)


def test_a_score_equal_to_the_threshold_is_no_object():
    from aod_meh_hua_amd import scoring
    c = _case('sigmoid', 20)
    rows = U.lookup(*c.host, 0.3)
    b = 0
    j = int(np.nonzero(rows[b] >= 0)[0][-1])                              # the weakest object of image 0
    v = float(c.host[2][b, j, 4])
    assert v > 0.3 and (rows[b, :j] >= 0).all()
    below = float(np.nextafter(np.float32(v), np.float32(0)))
    for thr, is_obj in ((v, False), (below, True)):
        unc, obj, _ = scoring.det_uncertainty(c.cand, c.dets, c.labels, c.num, 'sigmoid', 'entropy', 'sum', thr, want_objects=True)
        want = U.reference(*c.host, 'sigmoid', 'entropy', 'sum', thr)
        assert bool(torch.isnan(obj[b, j])) != is_obj and (want['rows'][b, j] >= 0) == is_obj
        assert np.array_equal(np.isnan(_np(obj)), want['rows'] < 0) and U.close(_np(unc), want['unc'], (U.RTOL, U.ATOL))


def test_one_candidate_and_one_image():
    from aod_meh_hua_amd import scoring
    # n = 1: one candidate per image, found (or not) by its one detection
    boxes = torch.tensor([[[1., 2., 30., 40.]], [[5., 6., 20., 9.]], [[0., 0., 8., 8.]]], device='cuda')
    scores = torch.tensor([[[.1, .7, .2, 0.]], [[.25, .25, .5, 0.]], [[.2, .1, .1, 0.]]], device='cuda')
    dets, labels, keep, num = scoring.multiclass_nms_batch(boxes, scores, 0.05, 0.5, 5)
    cand = SimpleNamespace(boxes=boxes, scores=scores)
    host = tuple(_np(t) for t in (boxes, scores, dets, labels, num))
    assert host[4].tolist() == [3, 3, 3]
    for layout, measure, aggregate in itertools.product(('cat', 'cat_bg', 'sigmoid'), U.MEASURES, U.AGGREGATES):
        unc, obj, missing = scoring.det_uncertainty(cand, dets, labels, num, layout, measure, aggregate, want_objects=True)
        want = U.reference(*host, layout, measure, aggregate)
        assert want['count'].tolist() == [1, 1, 0] and _np(missing).tolist() == [0, 0, 0]
        tol_obj, tol_unc = U.tolerances(measure, aggregate)
        assert U.close(_np(obj), want['obj'], tol_obj) and U.close(_np(unc), want['unc'], tol_unc), (layout, measure, aggregate)
    # B = 1, max_num = 1
    c = _case('cat_bg', 20)
    d1, l1, _, n1 = scoring.multiclass_nms_batch(c.cand.boxes[:1], c.cand.scores[:1], 0.05, 0.5, 1)
    one = SimpleNamespace(boxes=c.cand.boxes[:1], scores=c.cand.scores[:1])
    unc, obj, missing = scoring.det_uncertainty(one, d1, l1, n1, 'cat_bg', 'margin', 'mean', want_objects=True)
    want = U.reference(*(_np(t) for t in (one.boxes, one.scores, d1, l1, n1)), 'cat_bg', 'margin', 'mean')
    assert want['count'].tolist() == [1] and U.close(_np(unc), want['unc'], (U.RTOL, U.ATOL)) and _np(missing).tolist() == [0]
    assert torch.equal(_bits(unc), _bits(obj[:, 0]))                       # one object: its value is the mean


def test_wide_detection_lists_take_the_single_part_lookup():
    """max_num = 300 and 1024 (more than the NMS kernel hands out: synthetic detection lists copied from the candidates): more than two
    waves of detection rows, several rows per thread, a tree of 512 / 1024 leaves"""
    from aod_meh_hua_amd import scoring
    c = _case('sigmoid', 20)
    boxes, scores = c.host[0], c.host[1]
    B, n, W = scores.shape
    g = np.random.default_rng(3)
    for max_num in (300, 1024):
        dets, labels = np.zeros((B, max_num, 5), np.float32), np.full((B, max_num), -1, np.int64)
        num = np.array([max_num, max_num // 2 + 1, 0], np.int32)
        for b in range(B):
            above = np.argwhere(scores[b, :, :W - 1] > 0.3)               # (candidate, class) entries that pass the gate: two rows in three
            for j in range(num[b]):
                k, cl = above[g.integers(len(above))] if len(above) and g.random() < 0.67 else (int(g.integers(n)), int(g.integers(W - 1)))
                dets[b, j, :4], dets[b, j, 4], labels[b, j] = boxes[b, k], scores[b, k, cl], cl
        dev = [torch.from_numpy(x).cuda() for x in (dets, labels, num)]
        for measure, aggregate in (('entropy', 'sum'), ('entropy', 'mean'), ('margin', 'max'), ('leastconf', 'sum')):
            unc, obj, missing = scoring.det_uncertainty(c.cand, *dev, 'sigmoid', measure, aggregate, 0.3, want_objects=True)
            want = U.reference(boxes, scores, dets, labels, num, 'sigmoid', measure, aggregate, 0.3)
            assert want['count'][0] > 64 and want['count'][2] == 0 and _np(missing).tolist() == [0, 0, 0]
            tol_obj, tol_unc = U.tolerances(measure, aggregate)
            assert np.array_equal(np.isnan(_np(obj)), want['rows'] < 0)
            assert U.close(_np(obj), want['obj'], tol_obj) and U.close(_np(unc), want['unc'], tol_unc), (max_num, measure, aggregate)


def test_an_image_has_the_same_bits_alone_and_anywhere_in_a_batch():
    from aod_meh_hua_amd import scoring
    for layout in U.LAYOUTS:
        c = _case(layout, 20)
        for measure, aggregate in (('entropy', 'sum'), ('entropy', 'mean'), ('margin', 'max'), ('leastconf', 'mean')):
            ref_u, ref_o, _ = scoring.det_uncertainty(c.cand, c.dets, c.labels, c.num, layout, measure, aggregate, want_objects=True)
            for order, row, img in (([1], 0, 1), ([1, 0, 2], 0, 1), ([0, 1, 2], 1, 1), ([2, 0, 1], 2, 1), ([0], 0, 0), ([2, 0], 1, 0)):
                pick = lambda t: t[order].contiguous()
                cand = SimpleNamespace(boxes=pick(c.cand.boxes), scores=pick(c.cand.scores))
                u, o, _ = scoring.det_uncertainty(cand, pick(c.dets), pick(c.labels), pick(c.num), layout, measure, aggregate, want_objects=True)
                assert torch.equal(_bits(u[row]), _bits(ref_u[img])) and torch.equal(_bits(o[row]), _bits(ref_o[img])), (layout, measure, order)


# ---------------------------------------------------------------------------------------------------------------- the pool pass
def _loader(ds, bs):
    from aod_meh_hua_amd.datasets import build_dataloader
    return build_dataloader(ds, samples_per_gpu=bs, workers_per_gpu=0, dist=False, shuffle=False)


def _build(kind):
    from aod_meh_hua_amd.datasets import build_dataset
    from aod_meh_hua_amd.mmcv_lite import Config, MMDataParallel
    from aod_meh_hua_amd.models import build_detector
    from oracle import model as om
    from oracle import model_ssd as ossd
    from tests import plain_retina_util as PU
    config, sd, size = {'SSL_L_RetinaNet': ('configs/_base_/Config_RetinaNet.py', lambda: om.seeded_state_dict(cls_bias=-2.0), (64, 64)),
                        'MyRetinaNet': ('configs/_base_/Config_RetinaNet_plain.py', lambda: PU.plain_state_dict(cls_bias=-0.5), (64, 64)),
                        'SSD_L_SingleStageDetector': ('configs/_base_/Config_SSD.py', lambda: ossd.seeded_state_dict(), (300, 300))}[kind]
    cfg = Config.fromfile(os.path.join(ROOT, config))
    cfg.model.backbone.pop('init_cfg', None)
    model = build_detector(cfg.model)
    assert type(model).__name__ == kind
    model.load_state_dict(sd(), strict=True)
    ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=6, size=size), dict(test_mode=True))
    return cfg, MMDataParallel(model.cuda()).eval(), ds


def _internals(model, ds, pool, aggregate, thr):
    """the model's own eager scoring batches of 3 with _return_internals: the tensors score_batch handed to det_uncertainty, and its scores"""
    from aod_meh_hua_amd.apis.test import _unwrap
    out = []
    with torch.no_grad():
        for data in _loader(ds, 3):
            data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
            _, unc, it = model(return_loss=False, rescale=True, isEval=False, isUnc='Epistemic', uPool=pool, unc_aggregate=aggregate, score_thr=thr,
                               _return_internals=True, **data)
            out.append((unc, it))
    return out


@pytest.mark.parametrize('kind', ['SSL_L_RetinaNet', 'MyRetinaNet', 'SSD_L_SingleStageDetector'])
def test_pool_pass_eager_replayed_and_batch_sizes(kind, monkeypatch):
    from aod_meh_hua_amd import apis, scoring
    from aod_meh_hua_amd.apis import test as apis_test
    cfg, model, ds = _build(kind)
    head = model.module.bbox_head
    layout = scoring.ACTIVATION_LAYOUT[head.last_activation]
    assert layout == {'SSL_L_RetinaNet': 'cat', 'MyRetinaNet': 'sigmoid', 'SSD_L_SingleStageDetector': 'cat_bg'}[kind]
    # the object gate: the random heads' posteriors are nearly flat, so the gate sits just above the NMS kernel's own 0.05
    thr = 0.3 if kind == 'MyRetinaNet' else 0.06
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    eager = {}
    for measure, aggregate in (('entropy', 'mean'), ('margin', 'max'), ('leastconf', 'sum')):
        eager[measure] = apis.Posterior_uncertainty(cfg, model, _loader(ds, 3), measure=measure, aggregate=aggregate, score_thr=thr)
        e = eager[measure]
        assert e.shape == (6,) and e.dtype == torch.float32 and not e.is_cuda and bool(torch.isfinite(e).all()) and bool((e >= 0).all())
        assert torch.equal(apis.Posterior_uncertainty(cfg, model, _loader(ds, 1), measure=measure, aggregate=aggregate, score_thr=thr), e)
        # against the util on the tensors score_batch itself handed to the kernel
        pool = {'entropy': 'Entropy', 'margin': 'Margin', 'leastconf': 'LeastConf'}[measure]
        want, direct, counts = [], [], []
        for unc, it in _internals(model, ds, pool, aggregate, thr):
            host = tuple(_np(t) for t in (it['cand'].boxes, it['cand'].scores, it['dets'], it['labels'], it['num']))
            r = U.reference(*host, layout, measure, aggregate, thr)
            assert r['missing'].sum() == 0
            want.append(r['unc']), direct.append(unc.cpu()), counts.extend(r['count'].tolist())
        print(f'{kind} {measure}/{aggregate} thr {thr}: objects per image {counts}, unc {e.tolist()}')
        assert sum(1 for n in counts if n > 0) >= 2, counts                       # not vacuous: images with objects
        assert torch.equal(_bits(torch.cat(direct)), _bits(e))
        assert U.close(e.numpy(), np.concatenate(want), U.tolerances(measure, aggregate)[1])
    # replayed: one captured graph per batch shape contains the new launch; the same bits at batch sizes 3 and 1
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    for measure, aggregate in (('entropy', 'mean'), ('margin', 'max'), ('leastconf', 'sum')):
        for bs in (3, 1):
            got = apis.Posterior_uncertainty(cfg, model, _loader(ds, bs), measure=measure, aggregate=aggregate, score_thr=thr)
            assert torch.equal(_bits(got), _bits(eager[measure])), (measure, bs)
    gs = list(apis_test._GSCORE.get(model, {}).values())
    assert len(gs) == 3 and all(len(g.cache) == 2 and g.kw['uPool'] in scoring.POSTERIOR_POOLS for g in gs)      # three pools x two batch shapes, all replayed
    # calculate_uncertainty reaches the same pool by its name
    cfg.uncertainty_pool = 'Entropy'
    again = apis.calculate_uncertainty(cfg, model, _loader(ds, 3), unc_aggregate='mean', score_thr=thr)
    assert torch.equal(_bits(again), _bits(eager['entropy']))


# ---------------------------------------------------------------------------------------------------------------- the driver
def test_the_driver_runs_the_entropy_pool_on_the_plain_detector():
    wd = f'pytest_posterior_unc_{os.getpid()}'
    out = os.path.join(ROOT, 'work_dirs', wd)
    cmd = [sys.executable, os.path.join(ROOT, 'tools/train_RetinaNet.py'), '--config', os.path.join(ROOT, 'configs/_base_/Config_RetinaNet_plain.py'),
           '--synthetic', '64', '--cycles', '2', '--synthetic-size', '256', '--uncertainty-pool', 'Entropy', '--unc-aggregate', 'mean',
           '--work-dir', wd]
    try:
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
        xl0, xl1 = np.load(os.path.join(out, 'X_L_0.npy')), np.load(os.path.join(out, 'X_L_1.npy'))
        unc = np.load(os.path.join(out, 'Unc_1.npy'))
        x_s = 64 // 16                                                       # the driver's X_S_size of a synthetic pool
        assert len(xl1) == len(xl0) + x_s and set(xl0) <= set(xl1) and unc.shape == (64,) and np.isfinite(unc).all() and (unc >= 0).all()
    finally:
        import shutil
        shutil.rmtree(out, ignore_errors=True)
