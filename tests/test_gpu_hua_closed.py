"""GPU: the closed-form Dirichlet estimator (hua_closed_kernel, estimator='closed') and the per-object outputs of the reduce kernel
(want_objects / detUnc) against float64 evaluations, the CPU oracle's closed form, the reference's Monte-Carlo runs (golden/scoring.npz)
and against themselves (no randomness, fold invariants, graph replay).  The planted fixture is the one of tests/test_gpu_scoring.py."""
import os

import numpy as np
import pytest
import torch
from scipy.special import digamma

from oracle import hua as ohua
from oracle import model as omodel
from tests import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), 'golden')
MODES = ('objectAvg_scaleAvg_classAvg', 'objectMax_scaleSum_classMax', 'objectSum_scaleMax_classSum', 'objectSum_scaleAvg_classMax')
LVL_OFF = np.cumsum([0, 1000, 576, 144, 36, 9])


class Cfg(dict):
    __getattr__ = dict.__getitem__


class Head:
    last_activation, cls_out_channels, num_anchors = 'relu', 20, 9


def _planted():
    from aod_meh_hua_amd.core.anchor import AnchorGenerator
    from aod_meh_hua_amd.core.bbox import DeltaXYWHBBoxCoder
    Head.bbox_coder = DeltaXYWHBBoxCoder()
    cls_p, reg_p, L_p = synth.planted_heads(2, 128, 128)
    mt = synth.metas(2, 128, 128, scale=1.25)
    ag = AnchorGenerator(octave_base_scale=4, scales_per_octave=3, ratios=[0.5, 1.0, 2.0], strides=[8, 16, 32, 64, 128])
    anchors = ag.grid_anchors([tuple(c.shape[-2:]) for c in cls_p], 'cuda')
    cfg = Cfg(nms_pre=1000, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
    return cls_p, reg_p, L_p, mt, anchors, cfg


@pytest.fixture(scope='module')
def run():
    from aod_meh_hua_amd import scoring
    cls_p, reg_p, L_p, mt, anchors, cfg = _planted()
    det, unc, it = scoring.score_batch(Head(), [c.cuda() for c in cls_p], [r.cuda() for r in reg_p], anchors, [m['img_shape'] for m in mt],
                                       [m['scale_factor'] for m in mt], cfg, rescale=True, with_nms=True, isUnc='Epistemic', uPool='Entropy_NMS',
                                       uPool2='objectSum_scaleMax_classSum', isEval=False, L_scores=[l.cuda() for l in L_p],
                                       _return_internals=True, batchIdx=0, hua_estimator='closed')
    ids = torch.arange(2, device='cuda', dtype=torch.int64)
    args = (it['cand'], it['dets'], it['num'], ids, 100)
    cu, cpc, cpout = scoring.hua_score(*args, estimator='closed', want_pairs=True)
    mu, mpc, mpout = scoring.hua_score(*args, want_pairs=True, seed=20)
    torch.cuda.synchronize()
    o = omodel.score_images(None, torch.zeros(2, 3, 128, 128), [m['img_shape'] for m in mt], [m['scale_factor'] for m in mt],
                            sampler='closed', heads=(cls_p, reg_p, L_p))
    dets = it['dets'].cpu().numpy()
    num = it['num'].cpu().tolist()
    rows = [np.nonzero(dets[b, :num[b], 4] > 0.3)[0] for b in range(2)]          # detection row of each HUA object, in object order
    return dict(sc=scoring, it=it, args=args, unc=unc, cu=cu, pc=cpc.cpu().tolist(), pout=cpout.cpu().numpy(), mpc=mpc.cpu().tolist(),
                mpout=mpout.cpu().numpy(), munc=mu, o=o, rows=rows, num=num, dets=dets, gold=np.load(os.path.join(G, 'scoring.npz')))


def _oracle_pairs(o, b):
    exp = sorted([p for p in o['pairs'] if p['image'] == b], key=lambda p: p['level'])
    return (np.concatenate([p['cand'].numpy() + LVL_OFF[p['level']] for p in exp]), np.concatenate([p['obj'].numpy() for p in exp]),
            np.concatenate([p['alpha'].numpy() for p in exp]))


def _ale64(alpha):
    a = np.asarray(alpha, np.float64)
    S = a.sum(-1)
    return digamma(S + 1) - ((a / S[:, None]) * digamma(a + 1)).sum(-1)


def _epi64_zero_safe(alpha):
    """the closed form in float64 with 0 * log 0 = 0 (columns with alpha == 0 contribute nothing)"""
    a = np.asarray(alpha, np.float64)
    S = a.sum(-1, keepdims=True)
    m = a / S
    with np.errstate(divide='ignore', invalid='ignore'):
        total = -np.where(m > 0, m * np.log(m), 0.0).sum(-1)
    return total - _ale64(a), _ale64(a)


def _bins(cand, pc, pout, nobj, col):
    """(object, level, class) bins rebuilt on the host from the kernel's own per-pair values (column 2 aleatoric, 3 epistemic); the method of
    tests/test_gpu_scoring.py::_bins_from_kernel_pairs"""
    ls, sc, out = cand.level_start, cand.scores.cpu(), []
    for b in range(pout.shape[0]):
        img = [[{} for _ in range(len(ls) - 1)] for _ in range(nobj[b])]
        acc = {}
        for k in range(pc[b]):
            c, o, v = int(pout[b, k, 0]), int(pout[b, k, 1]), float(pout[b, k, col])
            lvl = max(l for l in range(len(ls) - 1) if c >= ls[l])
            acc.setdefault((o, lvl, int(sc[b, c, :-1].argmax())), []).append(v)
        for (o, lvl, cls), v in sorted(acc.items()):
            img[o][lvl][cls] = float(np.mean(np.asarray(v, np.float32), dtype=np.float32))
        out.append(img)
    return out


def _fold_object(obj_bins, mode):
    """class -> scale folds of one object's bins (None when it owns no bin) and the number of bins folded"""
    f = ohua.extract_agg_func(mode)
    scales = [f['class'](list(lvl.values())) for lvl in obj_bins if lvl]
    return (f['scale'](scales) if scales else None), sum(len(lvl) for lvl in obj_bins)


def _fold_rows_f32(vals, code):
    """the object fold of hua_reduce_kernel: sequential, float32, in row order"""
    acc = np.float32(0)
    for i, v in enumerate(vals):
        v = np.float32(v)
        acc = v if i == 0 else (np.maximum(acc, v) if code == 2 else np.float32(acc + v))
    if not len(vals):
        return np.float32(0)
    return np.float32(acc / np.float32(len(vals))) if code == 1 else acc


# ------------------------------------------------------------------------------------------------ 1. per-pair closed form
def test_per_pair_closed_form_vs_float64(run):
    worst_e = worst_a = 0.0
    total = 0
    for b in range(2):
        ec, eo, alpha = _oracle_pairs(run['o'], b)
        n = run['pc'][b]
        got, mc = run['pout'][b, :n], run['mpout'][b, :run['mpc'][b]]
        assert n == len(ec) == run['mpc'][b]
        assert np.array_equal(got[:, 0].astype(np.int64), ec) and np.array_equal(got[:, 1].astype(np.int64), eo)
        assert np.array_equal(got[:, :2], mc[:, :2])                                  # pair order equals the Monte-Carlo path's
        epi, ale = ohua.epistemic_closed_form(alpha), _ale64(alpha)
        ee, ea = np.abs(got[:, 3] - epi), np.abs(got[:, 2] - ale)
        worst_e, worst_a = max(worst_e, ee.max()), max(worst_a, ea.max())
        print(f'image {b}: {n} pairs, closed-form max |err| epistemic {ee.max():.3e} aleatoric {ea.max():.3e}; MC vs limit median rel '
              f'{np.median(np.abs(mc[:, 3] - epi) / np.abs(epi)):.3f}')
        assert (ee <= 1e-5 + 1e-5 * np.abs(epi)).all(), ee.max()
        assert (ea <= 1e-5 + 1e-5 * np.abs(ale)).all(), ea.max()
        total += n
    print('pairs', total, 'max abs err epi', worst_e, 'ale', worst_a)
    assert total == 993


# ------------------------------------------------------------------------------------------------ 2. image score
def test_image_score_vs_oracle_bins_and_reference_runs(run):
    sc, o, args = run['sc'], run['o'], run['args']
    cu = run['cu'].cpu().numpy()
    print('closed image scores', cu.tolist(), 'oracle', o['unc'])
    assert np.allclose(cu, np.array(o['unc']), rtol=5e-4), (cu, o['unc'])
    assert np.array_equal(cu, run['unc'].cpu().numpy())                               # score_batch(hua_estimator='closed') == hua_score
    nobj = [len(r) for r in run['rows']]
    assert nobj == [47, 48] or sorted(nobj) == [47, 48]
    bins = _bins(run['it']['cand'], run['pc'], run['pout'], nobj, 3)
    for mode in MODES:
        u = sc.hua_score(*args, agg=sc.extract_agg_codes(mode), estimator='closed').cpu().numpy()
        assert np.allclose(u, ohua.aggregate_obj_scale_unc(bins, mode), rtol=1e-5), mode
        assert np.allclose(u, ohua.aggregate_obj_scale_unc(o['bins'], mode), rtol=5e-4), mode
    u = sc.hua_score(*args, clsW=True, estimator='closed').cpu().numpy()
    assert np.allclose(u, ohua.aggregate_obj_scale_unc(bins, 'objectSum_scaleMax_classSum', clsW=True), rtol=1e-5)
    assert np.allclose(u, ohua.aggregate_obj_scale_unc(o['bins'], 'objectSum_scaleMax_classSum', clsW=True), rtol=5e-4)
    g = run['gold']['unc_runs']
    mu, sd = g.mean(0), g.std(0)
    assert (np.abs(cu - mu) <= 5 * sd + 0.04 * mu).all(), (cu, mu, sd)


# ------------------------------------------------------------------------------------------------ 3. no randomness
def test_closed_form_has_no_seed_no_sample_count_no_image_id(run):
    sc, it = run['sc'], run['it']
    cand, dets, num, ids, mx = run['args']
    base = run['cu']
    for kw in (dict(seed=1), dict(seed=20), dict(num_samples=50), dict(num_samples=500)):
        assert torch.equal(sc.hua_score(cand, dets, num, ids, mx, estimator='closed', **kw), base), kw
    for pair in ((0, 1), (7, 9)):
        assert torch.equal(sc.hua_score(cand, dets, num, torch.tensor(pair, device='cuda', dtype=torch.int64), mx, estimator='closed'), base)
    for b in range(2):
        sub = sc.Candidates(cand.boxes[b:b + 1].contiguous(), cand.scores[b:b + 1].contiguous(), cand.lam[b:b + 1].contiguous(),
                            cand.cand_anchor[b:b + 1].contiguous(), cand.level_start, cand.any_fg[:, b:b + 1].contiguous(), None)
        u1 = sc.hua_score(sub, dets[b:b + 1].contiguous(), num[b:b + 1].contiguous(), ids[b:b + 1].contiguous(), mx, estimator='closed')
        assert float(u1[0]) == float(base[b])


# ------------------------------------------------------------------------------------------------ 4. per-object outputs, self-consistent
@pytest.mark.parametrize('estimator', ['closed', 'mc'])
def test_per_object_outputs_are_self_consistent(run, estimator):
    sc, args = run['sc'], run['args']
    kw = dict(estimator=estimator, seed=20)
    pout, pc = (run['pout'], run['pc']) if estimator == 'closed' else (run['mpout'], run['mpc'])
    nobj = [len(r) for r in run['rows']]
    bins_a, bins_e = _bins(run['it']['cand'], pc, pout, nobj, 2), _bins(run['it']['cand'], pc, pout, nobj, 3)
    for mode in MODES:
        agg = sc.extract_agg_codes(mode)
        plain = sc.hua_score(*args, agg=agg, **kw)
        unc, obj_out, obj_pairs = sc.hua_score(*args, agg=agg, want_objects=True, **kw)
        assert torch.equal(unc, plain), mode                                          # the object instance folds to the same bits
        assert obj_out.shape == (2, 100, 2) and obj_pairs.shape == (2, 100) and obj_pairs.dtype == torch.int32
        oo, op, u = obj_out.cpu().numpy(), obj_pairs.cpu().numpy(), unc.cpu().numpy()
        for b in range(2):
            rows = run['rows'][b]
            not_obj = np.setdiff1d(np.arange(100), rows)
            assert (run['dets'][b, not_obj[not_obj < run['num'][b]], 4] <= 0.3).all()
            assert np.isnan(oo[b, not_obj]).all() and (op[b, not_obj] == 0).all()     # score <= 0.3 or row >= num_det
            cnt = np.bincount(pout[b, :pc[b], 1].astype(np.int64), minlength=nobj[b])
            assert np.array_equal(op[b, rows], cnt)
            valid = []
            for k, r in enumerate(rows):
                ea, nb_a = _fold_object(bins_a[b][k], mode)
                ee, nb_e = _fold_object(bins_e[b][k], mode)
                if ee is None:
                    assert cnt[k] == 0 and np.isnan(oo[b, r]).all()
                    continue
                valid.append(r)
                assert np.isclose(oo[b, r, 0], ea, rtol=1e-5, atol=0) and np.isclose(oo[b, r, 1], ee, rtol=1e-5, atol=0), (mode, b, r, oo[b, r], ea, ee)
                assert oo[b, r, 0] >= 0
            assert len(valid) > 10
            folded = _fold_rows_f32(oo[b, valid, 1], agg[2])
            assert folded == u[b], (mode, b, folded, u[b])                             # fold invariant, bit for bit


# ------------------------------------------------------------------------------------------------ 5. per-object outputs vs the oracle
def test_per_object_epistemic_vs_oracle_closed_bins(run):
    sc, args, o = run['sc'], run['args'], run['o']
    worst = 0.0
    for mode in MODES:
        _, obj_out, _ = sc.hua_score(*args, agg=sc.extract_agg_codes(mode), estimator='closed', want_objects=True)
        oo = obj_out.cpu().numpy()
        for b in range(2):
            assert len(o['bins'][b]) == len(run['rows'][b])
            for k, r in enumerate(run['rows'][b]):
                exp, nb = _fold_object(o['bins'][b][k], mode)
                if exp is None:
                    assert np.isnan(oo[b, r]).all()
                    continue
                err = abs(oo[b, r, 1] - exp)
                worst = max(worst, err)
                assert err <= 1e-5 * nb + 1e-5 * abs(exp), (mode, b, r, oo[b, r, 1], exp, nb)
    print('per-object epistemic vs oracle: max abs err', worst)


# ------------------------------------------------------------------------------------------------ 6. edge cases on hand-made candidates
def _handmade(C, zero_row=False, seed=5):
    """B = 2 images, n = 64 candidates on one level, 2 detections per image; every candidate sits on one of the two detections"""
    from aod_meh_hua_amd import scoring
    g = synth.gen(seed + C)
    B, n = 2, 64
    logits = torch.randn(B, n, C + 1, generator=g) * 3
    logits[:, 1::2].scatter_add_(2, torch.randint(0, C, (B, n // 2, 1), generator=g), torch.full((B, n // 2, 1), 10.0))   # confident rows
    scores = logits.softmax(-1)
    if zero_row:                         # logit gaps beyond fp32 softmax range: columns exactly 0
        logits[:, ::4, 3:] = -200.0
        scores = logits.softmax(-1)
        assert (scores[:, ::4, 3:] == 0).all()
    det_boxes = torch.tensor([[10., 10., 50., 60.], [70., 20., 120., 90.]])
    which = torch.randint(0, 2, (B, n), generator=g)
    boxes = det_boxes[which] + torch.rand(B, n, 4, generator=g) * 2 - 1
    boxes[:, -4:] = torch.tensor([200., 200., 210., 210.])            # a few candidates on no detection
    lam = torch.rand(B, n, generator=g) + 0.2
    dets = torch.zeros(B, 2, 5)
    dets[:, :, :4] = det_boxes
    dets[:, 0, 4], dets[:, 1, 4] = 0.9, 0.6
    cand = scoring.Candidates(boxes.cuda(), scores.cuda().contiguous(), lam.cuda(), torch.arange(B * n, dtype=torch.int32).reshape(B, n).cuda(),
                              [0, n], torch.ones(1, B, dtype=torch.int32).cuda(), None)
    return cand, dets.cuda(), torch.full((B,), 2, dtype=torch.int32).cuda(), scores.numpy(), lam.numpy()


def _check_pairs64(pout, pc, scores, lam, nd, scale_mode):
    n_pairs = 0
    for b in range(2):
        got = pout[b, :pc[b]]
        c = got[:, 0].astype(np.int64)
        lam64 = lam[b].astype(np.float64)
        mean = lam64.mean() if scale_mode else lam64[c].mean()
        alpha = scores[b, c, :nd].astype(np.float64) * (mean / (lam64[c] + 1e-7) * 25)[:, None]
        epi, ale = _epi64_zero_safe(alpha)
        assert np.isfinite(got).all()
        assert (np.abs(got[:, 3] - epi) <= 1e-5 + 1e-5 * np.abs(epi)).all(), np.abs(got[:, 3] - epi).max()
        assert (np.abs(got[:, 2] - ale) <= 1e-5 + 1e-5 * np.abs(ale)).all(), np.abs(got[:, 2] - ale).max()
        n_pairs += pc[b]
    return n_pairs


@pytest.mark.parametrize('C,cols,zero_row', [(20, 21, False), (80, 0, False), (80, 81, False), (20, 21, True), (80, 81, True)])
def test_edge_column_counts_and_exact_zero_columns_vs_float64(C, cols, zero_row):
    from aod_meh_hua_amd import scoring
    cand, dets, num, scores, lam = _handmade(C, zero_row)
    if not cols:
        cand.scores[..., -1] = 0             # evidence head: zero-padded background column
        scores = cand.scores.cpu().numpy()
    nd = cols or C
    ids = torch.arange(2, device='cuda', dtype=torch.int64)
    # object mode
    unc, pc, pout, obj_out, obj_pairs = scoring.hua_score(cand, dets, num, ids, 2, estimator='closed', want_pairs=True, want_objects=True,
                                                          dirichlet_cols=cols)
    pc, pout = pc.cpu().tolist(), pout.cpu().numpy()
    assert _check_pairs64(pout, pc, scores, lam, nd, False) > 20
    assert torch.isfinite(unc).all() and torch.isfinite(obj_out).all()
    assert np.array_equal(obj_pairs.cpu().numpy().sum(1), np.array(pc))
    for b in range(2):
        assert pc[b] == int(((scores[b].max(-1) > 0.3) & (np.arange(64) < 60)).sum())
    # scale mode: every foreground candidate is a pair of one pseudo object, lambda mean over the whole level
    unc_s, pc_s, pout_s = scoring.hua_score(cand, None, None, ids, 1, (1, 1, 0), estimator='closed', want_pairs=True, scale_mode=True,
                                            dirichlet_cols=cols)
    pc_s, pout_s = pc_s.cpu().tolist(), pout_s.cpu().numpy()
    assert _check_pairs64(pout_s, pc_s, scores, lam, nd, True) > 20
    assert pc_s == [int((scores[b].max(-1) > 0.3).sum()) for b in range(2)]
    assert torch.isfinite(unc_s).all() and (unc_s > 0).all()
    with pytest.raises(ValueError):
        scoring.hua_score(cand, None, None, ids, 1, estimator='closed', scale_mode=True, want_objects=True)
    # no detections: score 0, every row NaN
    z = torch.zeros_like(num)
    unc0, oo0, op0 = scoring.hua_score(cand, dets, z, ids, 2, estimator='closed', want_objects=True, dirichlet_cols=cols)
    assert (unc0 == 0).all() and torch.isnan(oo0).all() and (op0 == 0).all()


# ------------------------------------------------------------------------------------------------ 7. Entropy_ALL
def test_entropy_all_closed_vs_oracle():
    from aod_meh_hua_amd import scoring
    cls_p, reg_p, L_p, mt, anchors, cfg = _planted()
    alphas = [omodel.nhwc_flat(c, 20).softmax(dim=2) for c in cls_p]
    lam = [omodel.nhwc_flat(l, 1)[..., 0] for l in L_p]
    obins = ohua.compute_scale_unc(alphas, lam, sampler='closed')
    for mode in ('scaleAvg_classAvg', 'scaleSum_classSum'):
        det, unc = scoring.score_batch(Head(), [c.cuda() for c in cls_p], [r.cuda() for r in reg_p], anchors, [m['img_shape'] for m in mt],
                                       [m['scale_factor'] for m in mt], cfg, rescale=True, with_nms=False, isUnc='Epistemic',
                                       uPool='Entropy_ALL', uPool2=mode, isEval=False, L_scores=[l.cuda() for l in L_p], batchIdx=0,
                                       hua_estimator='closed')
        u = unc.cpu().numpy()
        print(mode, u, ohua.aggregate_scale_unc(obins, mode))
        assert np.allclose(u, ohua.aggregate_scale_unc(obins, mode), rtol=5e-4), (mode, u)


# ------------------------------------------------------------------------------------------------ 8. detection path
def _check_detunc(model, loader, num_classes, estimators=('mc', 'closed')):
    from aod_meh_hua_amd.apis.test import single_gpu_test
    plain = single_gpu_test(model, loader)
    assert isinstance(plain, list) and isinstance(plain[0], list)                     # without the flag: what it returns today
    seen_obj = 0
    for est in estimators:
        res, unc = single_gpu_test(model, loader, detUnc=True, hua_estimator=est)
        assert len(res) == len(unc) == len(plain)
        for i in range(len(plain)):
            assert len(res[i]) == len(unc[i]) == len(plain[i]) == num_classes
            for c in range(num_classes):
                assert np.array_equal(res[i][c], plain[i][c])
                k = plain[i][c].shape[0]
                assert unc[i][c].shape == (k, 2) and unc[i][c].dtype == np.float32
                s, u = plain[i][c][:, 4], unc[i][c]
                assert np.isnan(u[s <= 0.3]).all()
                obj = u[s > 0.3]
                own = obj[~np.isnan(obj[:, 0])]                                        # (an object without a pair stays NaN)
                assert np.isfinite(own).all() and (own[:, 0] >= 0).all()
                if est == 'closed':
                    assert (own[:, 1] >= -1e-5).all()
                seen_obj += len(own)
    print('detections with an uncertainty:', seen_obj)
    return seen_obj


def test_detection_path_retinanet_carries_per_box_uncertainty():
    from aod_meh_hua_amd.datasets import build_dataloader, build_dataset
    from aod_meh_hua_amd.mmcv_lite import Config, MMDataParallel
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg.model.backbone.pop('init_cfg')
    model = build_detector(cfg.model)
    model.load_state_dict(omodel.seeded_state_dict(cls_bias=1.0), strict=True)
    with torch.no_grad():
        model.bbox_head.retina_cls.weight.mul_(40.0)                                  # confident logits: detections above the 0.3 object threshold
    model = MMDataParallel(model.cuda())
    ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=2, size=(128, 128)), dict(test_mode=True))
    dl = build_dataloader(ds, samples_per_gpu=2, workers_per_gpu=0, dist=False, shuffle=False)
    assert _check_detunc(model, dl, 20) > 0


def test_detection_path_ssd300_carries_per_box_uncertainty():
    from aod_meh_hua_amd.datasets import build_dataloader, build_dataset
    from aod_meh_hua_amd.mmcv_lite import Config, MMDataParallel
    from aod_meh_hua_amd.models import build_detector
    from oracle import model_ssd as ossd
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_SSD.py'))
    cfg.model.backbone.pop('init_cfg')
    model = build_detector(cfg.model)
    model.load_state_dict(ossd.seeded_state_dict(), strict=True)
    with torch.no_grad():
        for conv in model.bbox_head.cls_convs:
            (conv[-1] if isinstance(conv, torch.nn.Sequential) else conv).weight.mul_(40.0)
    model = MMDataParallel(model.cuda())
    ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=1, size=(300, 300)), dict(test_mode=True))
    dl = build_dataloader(ds, samples_per_gpu=1, workers_per_gpu=0, dist=False, shuffle=False)
    _check_detunc(model, dl, 20)


# ------------------------------------------------------------------------------------------------ 9. graph replay
def test_closed_estimator_replays_under_the_scoring_graph(monkeypatch):
    import bench
    from aod_meh_hua_amd.apis import calculate_uncertainty
    from aod_meh_hua_amd.apis import test as apis_test
    from aod_meh_hua_amd.datasets import DevicePhiloxPool
    dev = torch.device('cuda', 0)
    model, _ = bench.build_model(dev, dict(bench.CONFIGS['voc512']))
    ds = DevicePhiloxPool(8, (128, 128), seed=21)
    bench.calibrate_head(model, ds.device_batch([0, 1, 2, 3], dev)['img'][0].clone(), target_frac=0.02)
    model.eval()

    class Loader:
        dataset, batch_size, collate_fn = ds, 4, None
    cfg = Cfg(uncertainty_type='Epistemic', uncertainty_pool='Entropy_NMS', uncertainty_pool2='objectSum_scaleMax_classSum')
    kw = dict(scaleUnc=False, showNMS=False, saveUnc=False, saveMaxConf=False, clsW=False)
    seen = []
    orig = apis_test.single_gpu_uncertainty
    monkeypatch.setattr(apis_test, 'single_gpu_uncertainty', lambda *a, **k: (seen.append(k.get('hua_estimator')), orig(*a, **k))[1])
    mc = calculate_uncertainty(cfg, model, Loader(), **kw).numpy()
    model.test_cfg.hua_estimator = 'mc'
    assert np.array_equal(calculate_uncertainty(cfg, model, Loader(), **kw).numpy(), mc)
    model.test_cfg.hua_estimator = 'closed'
    graphed = calculate_uncertainty(cfg, model, Loader(), **kw).numpy()
    assert seen == [None, None, 'closed']                      # forwarded only when set and not 'mc': default kwargs (graph-cache keys) unchanged
    gs = [g for key, g in apis_test._GSCORE[model].items() if ('hua_estimator', 'str', 'closed') in key]
    assert len(gs) == 1 and len(gs[0].cache) == 1              # the second batch was captured and replayed
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    eager = calculate_uncertainty(cfg, model, Loader(), **kw).numpy()
    print('closed pool scores', graphed.tolist(), 'mc', mc.tolist())
    assert graphed.shape == (8,) and np.isfinite(graphed).all()
    assert np.array_equal(graphed, eager)
    assert not np.array_equal(graphed, mc) or not graphed.any()
