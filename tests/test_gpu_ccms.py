"""GPU: the CCMS acquisition -- aod_object_descriptors (scoring.object_descriptors), aod_ccms_distance
(scoring.ccms_distance) and aod_kcenter_greedy_matrix (scoring.kcenter_greedy_matrix) against the float64 restatements of
tests/ccms_util.py, their bit properties, and the pool pass apis.single_gpu_object_descriptors / apis.CCMS_uncertainty (graph replay and
eager, evidence head and plain RetinaNet).

Bounds (derived, not measured):
  descriptor   |device - float64| <= 1e-5 per element: v is exact in fp32 (bf16, or head + tail), the fp32 sum of <= 256 squares has a
               relative error below 256 2^-24, its square root half of that, the division one rounding: ~8e-6 on a unit vector
  distance     |device - float64| <= 3e-5: every dot product of two unit vectors is off by at most 256 2^-24 ~ 1.5e-5 (sum |a_k b_k| <= 1),
               a weighted mean of such values by no more, and the two means, their half-sum and 1 - x add less than 1e-5 of rounding
  greedy       exact: the selection only compares and takes minima of the matrix entries"""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import ccms_util as U
from tests.coreset_util import pad_mask, x_layout_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- gather
HWS, NA, B_G, MAX_NUM, N_CAND, THR = [(4, 5), (2, 3)], 9, 3, 8, 12, 0.3


def _pyramid(values, C, x3):
    """values: per-level fp32 arrays [B, h, w, C] -> (per-level device maps [B, width, h, w] inside ONE buffer whose other rows -- before,
    between and behind the levels -- and X-layout pad columns are NaN; per-level float64 values [B, h * w, C] the rows represent)"""
    B = values[0].shape[0]
    parts, exact, spans = [], [], []
    width = 2 * ((C + 31) // 32 * 32) if x3 else C
    poison = lambda n: torch.full((n, width), float('nan'), dtype=torch.bfloat16)
    r0 = 0
    for v in values:
        flat = v.reshape(-1, C)
        if x3:
            r, e = x_layout_rows(flat)
            r[:, torch.from_numpy(pad_mask(C))] = float('nan')
        else:
            r = torch.from_numpy(flat).to(torch.bfloat16)
            e = r.double().numpy()
        parts += [poison(3), r]
        spans.append((r0 + 3, r.shape[0]))
        r0 += 3 + r.shape[0]
        exact.append(e.reshape(B, -1, C))
    buf = torch.cat(parts + [poison(5)]).cuda()
    maps = [buf[s:s + n].view(B, v.shape[1], v.shape[2], width).permute(0, 3, 1, 2) for (s, n), v in zip(spans, values)]
    return maps, exact


@pytest.fixture(scope='module', params=[(256, True), (256, False), (72, True), (72, False)], ids=['256-x_layout', '256-bf16', '72-x_layout', '72-bf16'])
def gather_case(request):
    """image 0: no object (scores at or below the threshold); image 1: six objects, one of them without a candidate row, one more row
    behind num; image 2: three objects, the first on an all-zero feature row"""
    C, x3 = request.param
    g = np.random.default_rng(C + int(x3))
    values = [g.standard_normal((B_G, h, w, C)).astype(np.float32) for h, w in HWS]
    values[0][2, 1, 2] = 0.0                                        # image 2, level 0, cell 1 * 5 + 2 = 7
    maps, exact = _pyramid(values, C, x3)
    A0 = HWS[0][0] * HWS[0][1] * NA
    total = A0 + HWS[1][0] * HWS[1][1] * NA
    cand_anchor = g.integers(0, total, (B_G, N_CAND)).astype(np.int32)
    cand_anchor[2, 4] = 7 * NA + 5                                  # the all-zero cell
    cand_anchor[1, 0], cand_anchor[1, 1] = A0 - 1, A0               # the last anchor of level 0, the first of level 1
    cand_anchor[1, 2] = total - 1
    dets = np.zeros((B_G, MAX_NUM, 5), np.float32)
    dets[..., :4] = g.uniform(0, 60, (B_G, MAX_NUM, 4))
    dets[0, :, 4] = [0.3, 0.29, 0.1, 0.9, 0.9, 0.9, 0.9, 0.9]       # 0.3 is no object (strict); rows >= num = 3 are never read
    dets[1, :, 4] = [0.95, 0.9, 0.2, 0.8, 0.7, 0.6, 0.5, 0.99]
    dets[2, :, 4] = [0.85, 0.31, 0.05, 0.6, 0.0, 0.0, 0.0, 0.0]
    num = np.array([3, 7, 4], np.int32)
    labels = g.integers(0, 20, (B_G, MAX_NUM)).astype(np.int64)
    obj_cand = g.integers(0, N_CAND, (B_G, MAX_NUM)).astype(np.int32)
    obj_cand[1, :3] = [0, 1, 2]
    obj_cand[1, 4] = -1                                             # an object without a candidate row
    obj_cand[2, 0] = 4
    obj_cand[2, 1], obj_cand[2, 3] = 5, 6                           # ... and the other two on cells that are not
    cand_anchor[2, 5], cand_anchor[2, 6] = 3, A0 + 10
    obj_cand[0, :] = -1
    return dict(C=C, x3=x3, maps=maps, exact=exact, cand_anchor=cand_anchor, dets=dets, labels=labels, num=num, obj_cand=obj_cand)


class _Cand:
    def __init__(self, anchor):
        self.cand_anchor = anchor


def _gather(case, max_obj, sl=slice(None)):
    from aod_meh_hua_amd import scoring
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[sl])).cuda()
    return scoring.object_descriptors([m[sl] for m in case['maps']], _Cand(dev(case['cand_anchor'])), dev(case['dets']), dev(case['labels']),
                                      dev(case['num']), dev(case['obj_cand']), NA, max_obj, THR, channels=case['C'], x3=case['x3'])


@pytest.mark.parametrize('max_obj', [2, 8])
def test_gather_matches_float64_and_is_batch_invariant(gather_case, max_obj):
    c = gather_case
    want = U.object_descriptors_float64(c['exact'], [NA, NA], c['cand_anchor'], c['dets'], c['labels'], c['num'], c['obj_cand'], max_obj, THR)
    w_feat, w_cls, w_w, w_cnt, w_miss = want
    assert w_cnt.tolist() == [0, min(5, max_obj), min(3, max_obj)] and w_miss.tolist() == [0, 1, 0]          # the case is what it claims
    assert not w_feat[2, 0].any() and w_feat[2, 1].any()                                                       # the all-zero row
    feat, cls, w, cnt, missing = _gather(c, max_obj)
    assert feat.shape == (B_G, max_obj, c['C']) and feat.dtype == torch.float32 and cls.dtype == torch.int32 and cnt.dtype == torch.int32
    assert _np(cnt).tolist() == w_cnt.tolist() and _np(missing).tolist() == w_miss.tolist()
    assert np.array_equal(_np(cls), w_cls) and np.array_equal(_np(w).astype(np.float64), w_w)
    assert bool(torch.isfinite(feat).all())                                                                    # no poisoned row or pad column was read
    err = np.abs(_np(feat).astype(np.float64) - w_feat).max()
    print(f"gather C={c['C']} x3={c['x3']} max_obj={max_obj}: max |device - float64| = {err:.3e} (bound 1e-5)")
    assert err <= 1e-5
    for b in range(B_G):
        alone = _gather(c, max_obj, slice(b, b + 1))
        for got, ref in zip(alone, (feat, cls, w, cnt, missing)):
            assert got.shape[0] == 1 and torch.equal(_bits(got[0]) if got.dtype == torch.float32 else got[0], _bits(ref[b]) if ref.dtype == torch.float32 else ref[b]), b


# ---------------------------------------------------------------------------------------------------------------- distance
def _unit(g, n, C):
    v = g.standard_normal((n, C)).astype(np.float32)
    return (v / np.sqrt((v.astype(np.float64) ** 2).sum(axis=1, keepdims=True))).astype(np.float32)


def _distance_case(max_obj, C):
    """7 images, 3 classes.  0: no object; 1: one object of class 0; 2: three objects (0, 1, 1); 3: max_obj objects; 4: a copy of 3;
    5: three objects of class 2 (no class shared with 1 and 6); 6: one object of class 0, the negated feature of image 1's.
    The pad rows hold NaN features, a valid-looking class and a weight: none of them may be read."""
    g = np.random.default_rng(100 * max_obj + C)
    M = 7
    feat = np.full((M, max_obj, C), np.nan, np.float32)
    cls = np.ones((M, max_obj), np.int32)
    w = np.full((M, max_obj), 5.0, np.float32)
    cnt = np.array([0, 1, 3, max_obj, max_obj, 3, 1], np.int32)
    for a, classes in ((1, [0]), (2, [0, 1, 1]), (3, g.integers(0, 3, max_obj)), (5, [2, 2, 2])):
        n = len(classes)
        feat[a, :n], cls[a, :n], w[a, :n] = _unit(g, n, C), classes, g.uniform(0.31, 1.0, n)
    # correlated features, so that the matched cosines are not all ~ 0: image 2 and 3 lean on image 1's object
    feat[2, :3] = _renorm(feat[2, :3] + 0.8 * feat[1, 0])
    feat[3, :max_obj] = _renorm(feat[3, :max_obj] + 0.5 * feat[1, 0])
    feat[4], cls[4], w[4] = feat[3], cls[3], w[3]
    feat[6, 0], cls[6, 0], w[6, 0] = -feat[1, 0], 0, 0.7
    return feat, cls, w, cnt


def _renorm(v):
    return (v / np.sqrt((v.astype(np.float64) ** 2).sum(axis=-1, keepdims=True))).astype(np.float32)


def _dist(feat, cls, w, cnt, idx=None):
    from aod_meh_hua_amd import scoring
    idx = slice(None) if idx is None else list(idx)
    return scoring.ccms_distance(*(torch.from_numpy(np.ascontiguousarray(a[idx])).cuda() for a in (feat, cls, w, cnt)))


@pytest.mark.parametrize('C', [256, 64])
@pytest.mark.parametrize('max_obj', [5, 32, 40])
def test_distance_matches_float64_is_symmetric_and_a_function_of_the_pair(max_obj, C):
    feat, cls, w, cnt = _distance_case(max_obj, C)
    want = U.distance_matrix(np.nan_to_num(feat).astype(np.float64), cls, w.astype(np.float64), cnt)
    assert want[1, 5] == 1.0 and want[1, 6] == 1.0 and want[0, 3] == 1.0 and want[3, 4] < 1e-6 and 0.05 < want[1, 2] < 0.95      # the case is what it claims
    d = _dist(feat, cls, w, cnt)
    assert d.shape == (7, 7) and d.dtype == torch.float32 and bool(torch.isfinite(d).all())
    got = _np(d).astype(np.float64)
    err = np.abs(got - want).max()
    print(f'distance max_obj={max_obj} C={C}: max |device - float64| = {err:.3e} (bound 3e-5); d[1] = {got[1].round(4).tolist()}')
    assert err <= 3e-5
    assert torch.equal(_bits(d), _bits(d.t())) and _np(d.diagonal()).tolist() == [0.0] * 7 and bool((d >= 0).all())
    assert got[1, 5] == 1.0 and got[1, 6] == 1.0                                                  # no shared class / a negative cosine: exactly 1
    g = np.random.default_rng(7)
    for combo in itertools.combinations(range(7), 4):
        idx = g.permutation(combo)
        sub = _dist(feat, cls, w, cnt, idx)
        assert torch.equal(_bits(sub), _bits(d[idx][:, idx])), idx


def test_distance_across_many_groups_and_chunks():
    """131 images of up to 8 objects: 33 resident a-groups, two b-chunks -- pairs written from either side of the diagonal"""
    g = np.random.default_rng(3)
    M, K, C = 131, 8, 64
    cnt = g.integers(0, K + 1, M).astype(np.int32)
    feat = _unit(g, M * K, C).reshape(M, K, C)
    feat = _renorm(feat + 0.7 * feat[:1, :1])
    cls = g.integers(0, 3, (M, K)).astype(np.int32)
    w = g.uniform(0.31, 1.0, (M, K)).astype(np.float32)
    want = U.distance_matrix(feat.astype(np.float64), cls, w.astype(np.float64), cnt)
    d = _dist(feat, cls, w, cnt)
    err = np.abs(_np(d).astype(np.float64) - want).max()
    print(f'distance 131 x 131: max |device - float64| = {err:.3e} (bound 3e-5), mean d {want.mean():.4f}')
    assert err <= 3e-5 and torch.equal(_bits(d), _bits(d.t())) and not bool(d.diagonal().any())
    idx = [130, 5, 64, 129, 0, 127, 128]
    assert torch.equal(_bits(_dist(feat, cls, w, cnt, idx)), _bits(d[idx][:, idx]))


# ---------------------------------------------------------------------------------------------------------------- k-center on a matrix
def _tied_matrix(N, seed):
    g = np.random.default_rng(seed)
    D = g.integers(1, 6, (N, N)).astype(np.float32) * 0.25           # few distinct values: ties at nearly every step
    D = np.maximum(D, D.T)
    np.fill_diagonal(D, 0.0)
    D[N // 2] = D[1]                                                 # a duplicated image: distance 0 to its twin
    D[:, N // 2] = D[:, 1]
    D[N // 2, 1] = D[1, N // 2] = D[N // 2, N // 2] = 0.0
    assert np.array_equal(D, D.T)
    return D


@pytest.mark.parametrize('N, labelled, budget', [(50, [], 50), (50, [], 7), (50, [3, 41, 17], 47), (50, [49], 12), (600, [5, 300], 40)])
def test_matrix_greedy_is_exact_ties_included(N, labelled, budget):
    from aod_meh_hua_amd import scoring
    D = _tied_matrix(N, N + len(labelled))
    picks, radius, ties = U.greedy_matrix(D, labelled, budget)
    assert ties >= min(budget, 5)
    dev = torch.from_numpy(D).cuda()
    got_p, got_r = scoring.kcenter_greedy_matrix(dev, labelled, budget)
    assert got_p.dtype == torch.int64 and got_r.dtype == torch.float32 and got_p.shape == (budget,) and got_r.shape == (budget,)
    assert _np(got_p).tolist() == picks.tolist() and np.array_equal(_np(got_r), radius)
    if not labelled:
        assert got_p[0].item() == 0 and np.isinf(got_r[0].item())
    if budget == N - len(labelled):
        assert sorted(_np(got_p).tolist() + list(labelled)) == list(range(N))
    if len(labelled) > 1:                                            # the order of the centers does not matter
        p2, r2 = scoring.kcenter_greedy_matrix(dev, torch.tensor(labelled[::-1]), budget)
        assert torch.equal(p2, got_p) and torch.equal(_bits(r2), _bits(got_r))
    p3, r3 = scoring.kcenter_greedy_matrix(dev, labelled, max(budget // 2, 1))      # a shorter budget is a prefix
    assert torch.equal(p3, got_p[:len(p3)]) and torch.equal(_bits(r3), _bits(got_r[:len(r3)]))


# ---------------------------------------------------------------------------------------------------------------- the whole pass
N_POOL = 14


def _loader(ds, bs):
    from aod_meh_hua_amd.datasets import build_dataloader
    return build_dataloader(ds, samples_per_gpu=bs, workers_per_gpu=0, dist=False, shuffle=False)


def _batches(ds, bs):
    from aod_meh_hua_amd.apis.test import _unwrap
    for data in _loader(ds, bs):
        data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
        yield data['img'][0].cuda(), data['img_metas'][0]


def _build(kind):
    """the small synthetic detectors of the CDAL / posterior / stability GPU tests, their classification heads calibrated so that
    detections pass a gate (bench.calibrate_head)"""
    from aod_meh_hua_amd.datasets import build_dataset
    from aod_meh_hua_amd.mmcv_lite import Config, MMDataParallel
    from aod_meh_hua_amd.models import build_detector
    from oracle import model as om
    from tests import plain_retina_util as PU
    config, sd = {'SSL_L_RetinaNet': ('configs/_base_/Config_RetinaNet.py', lambda: om.seeded_state_dict(cls_bias=-2.0)),
                  'MyRetinaNet': ('configs/_base_/Config_RetinaNet_plain.py', lambda: PU.plain_state_dict(cls_bias=-0.5))}[kind]
    cfg = Config.fromfile(os.path.join(ROOT, config))
    cfg.model.backbone.pop('init_cfg', None)
    model = build_detector(cfg.model)
    assert type(model).__name__ == kind
    model.load_state_dict(sd(), strict=True)
    model = model.cuda().eval()
    ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=N_POOL, size=(64, 64)), dict(test_mode=True))
    if kind == 'SSL_L_RetinaNet':
        import bench
        bench.calibrate_head(model, next(_batches(ds, 4))[0])
    return cfg, MMDataParallel(model).eval(), ds


def _detections(model, ds):
    """the padded detections of the whole pool, eagerly, in batches of 4 -> (dets [N, max, 5], labels, num) numpy"""
    out = []
    for img, metas in _batches(ds, 4):
        with torch.no_grad():
            o = model(return_loss=False, rescale=True, isEval=True, _padded=True, isUnc=False, img=[img], img_metas=[metas])
        out.append([_np(t) for t in o])
    return tuple(np.concatenate([o[i] for o in out]) for i in range(3))


def _fixture_threshold(dets, num):
    """the gate of this fixture: the smallest of the images' top scores -- that image has no object (the gate is strict), every image
    with two larger scores has at least two"""
    top = np.array([dets[b, :num[b], 4].max() if num[b] else 0.0 for b in range(len(num))], np.float32)
    return float(top.min())


@pytest.fixture(scope='module', params=['SSL_L_RetinaNet', 'MyRetinaNet'])
def pool(request):
    cfg, model, ds = _build(request.param)
    dets, labels, num = _detections(model, ds)
    return dict(kind=request.param, cfg=cfg, model=model, ds=ds, dets=dets, labels=labels, num=num, thr=_fixture_threshold(dets, num))


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k])
               for k in ('unc', 'feat', 'cls', 'w', 'cnt', 'missing'))


def test_pool_pass_precondition_posterior_bits_eager_replayed_and_batch_sizes(pool, monkeypatch):
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis import test as apis_test
    cfg, model, ds, thr, K = pool['cfg'], pool['model'], pool['ds'], pool['thr'], 8
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    ref = apis.single_gpu_object_descriptors(model, _loader(ds, 4), max_obj=K, score_thr=thr)
    cnt = _np(ref['cnt'])
    n_obj = np.array([int((pool['dets'][b, :pool['num'][b], 4] > np.float32(thr)).sum()) for b in range(N_POOL)])
    print(f"{pool['kind']}: score_thr {thr:.6f}, objects per image {n_obj.tolist()}, kept {cnt.tolist()}, unc {ref['unc'].tolist()}")
    # the precondition: the pass is not vacuous
    assert int((n_obj >= 2).sum()) >= N_POOL // 2 and int((n_obj == 0).sum()) >= 1
    assert _np(ref['missing']).tolist() == [0] * N_POOL
    assert ref['feat'].shape == (N_POOL, K, 256) and ref['feat'].is_cuda and cnt.tolist() == np.minimum(n_obj, K).tolist()
    # class, weight: the gated detections in row order; features: unit rows, zeros behind cnt
    for b in range(N_POOL):
        rows = [j for j in range(pool['num'][b]) if pool['dets'][b, j, 4] > np.float32(thr)][:K]
        assert _np(ref['cls'][b]).tolist() == pool['labels'][b, rows].tolist() + [-1] * (K - len(rows))
        assert np.array_equal(_np(ref['w'][b, :len(rows)]), pool['dets'][b, rows, 4]) and not bool(ref['w'][b, len(rows):].any())
        nrm = _np(ref['feat'][b]).astype(np.float64)
        assert np.abs(np.sqrt((nrm[:len(rows)] ** 2).sum(axis=1)) - 1.0).max(initial=0.0) <= 1e-5 and not nrm[len(rows):].any()
    # stage 1 is the posterior pool's score, bit for bit
    post = apis.Posterior_uncertainty(cfg, model, _loader(ds, 4), measure='entropy', aggregate='sum', score_thr=thr)
    assert torch.equal(_bits(ref['unc'].cpu()), _bits(post)) and bool((post[n_obj > 0] > 0).all()) and bool((post[n_obj == 0] == 0).all())
    assert _same(apis.single_gpu_object_descriptors(model, _loader(ds, 1), max_obj=K, score_thr=thr), ref)
    # replayed: one graph per batch shape; the ragged last batch of 2 is seen once and runs eagerly
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    for bs in (4, 1):
        assert _same(apis.single_gpu_object_descriptors(model, _loader(ds, bs), max_obj=K, score_thr=thr), ref), bs
    gs = [v for k, v in apis_test._GSCORE.get(model).items() if k[0] == 'obj_desc']
    assert len(gs) == 1 and len(gs[0].cache) == 2 and not gs[0].pipe


def test_descriptors_are_the_neck_rows_of_the_matched_anchors(pool):
    """one batch by hand: the conv half, the selection with its internals, the matched candidate rows (checked against the matching rule)
    and the float64 restatement on the neck outputs read back as fp32"""
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import scoring
    model, thr = pool['model'].module, pool['thr']
    head = model.bbox_head
    img, metas = next(_batches(pool['ds'], 4))
    with torch.no_grad():
        feats = model.extract_feat(img)
        outs = head.test_heads(feats, with_L=False)[0] if pool['kind'] == 'SSL_L_RetinaNet' else head.test_heads(feats)[0]
        _, unc, it = head.get_bboxes(*outs, metas, rescale=True, isEval=False, isUnc='Epistemic', uPool='Entropy', unc_aggregate='sum', score_thr=thr,
                                     _return_internals=True)
        cand, dets, labels, num = it['cand'], it['dets'], it['labels'], it['num']
        layout = scoring.ACTIVATION_LAYOUT[head.last_activation]
        unc2, obj_cand = scoring.det_uncertainty(cand, dets, labels, num, layout, 'entropy', 'sum', thr, want_cand=True)
        assert torch.equal(_bits(unc2), _bits(unc))                                                # the _ex entry: the same score bits
        got = scoring.object_descriptors(feats, cand, dets, labels, num, obj_cand, head.num_anchors, 8, thr, channels=256)
        vals = [AF.x3_to_f32(f, 256).double().permute(0, 2, 3, 1).reshape(f.shape[0], -1, 256).cpu().numpy() for f in feats]
    boxes, scores, oc, d, lb = _np(cand.boxes), _np(cand.scores), _np(obj_cand), _np(dets), _np(labels)
    seen = 0
    for b in range(d.shape[0]):
        for j in range(d.shape[1]):
            if j < int(num[b]) and d[b, j, 4] > np.float32(thr):
                hit = np.nonzero((boxes[b].view(np.int32) == d[b, j, :4].view(np.int32)).all(axis=1)
                                 & (scores[b, :, lb[b, j]].view(np.int32) == d[b, j, 4:5].view(np.int32)))[0]
                assert hit.size and oc[b, j] == hit[0], (b, j)                                     # the lowest matching candidate row
                seen += 1
            else:
                assert oc[b, j] == -1
    assert seen >= 2
    want = U.object_descriptors_float64(vals, [head.num_anchors] * len(vals), _np(cand.cand_anchor), d, lb, _np(num), oc, 8, thr)
    assert _np(got[3]).tolist() == want[3].tolist() and _np(got[4]).tolist() == [0] * d.shape[0] and np.array_equal(_np(got[1]), want[1])
    err = np.abs(_np(got[0]).astype(np.float64) - want[0]).max()
    print(f"{pool['kind']}: {seen} objects in the batch, max |device - float64| = {err:.3e} (bound 1e-5)")
    assert err <= 1e-5


def test_ccms_uncertainty_marks_the_picks_and_update_X_L_takes_them(pool, monkeypatch):
    from aod_meh_hua_amd import apis, scoring
    from aod_meh_hua_amd.utils.active_datasets import update_X_L
    cfg, model, ds, thr = pool['cfg'], pool['model'], pool['ds'], pool['thr']
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    X_L, budget, factor, K = np.array([0, 9]), 3, 2, 8
    unc = apis.CCMS_uncertainty(cfg, model, _loader(ds, 4), X_L=X_L, budget=budget, candidate_factor=factor, max_obj=K, score_thr=thr)
    assert unc.shape == (N_POOL,) and unc.dtype == torch.float32 and not unc.is_cuda
    assert sorted(unc.tolist()) == [0.0] * (N_POOL - budget) + [1.0, 2.0, 3.0] and unc[0] == 0 and unc[9] == 0
    # the same selection by hand: stage 1 on the host, the device's own matrix, the host greedy on it
    store = apis.single_gpu_object_descriptors(model, _loader(ds, 4), max_obj=K, score_thr=thr)
    cand = scoring.ccms_candidates(store['unc'], X_L, budget, factor)
    assert len(cand) == 6 and not set(cand.tolist()) & {0, 9}
    u = _np(store['unc'])
    assert u[cand[0]] == np.delete(u, X_L).max() and (np.diff(u[cand]) <= 0).all()
    ci = torch.from_numpy(cand).cuda()
    dist = scoring.ccms_distance(*(store[k][ci].contiguous() for k in ('feat', 'cls', 'w', 'cnt')))
    assert torch.equal(_bits(dist), _bits(dist.t())) and not bool(dist.diagonal().any())
    picks, radius, _ = U.greedy_matrix(_np(dist), [], budget)
    chosen = cand[picks]
    print(f"{pool['kind']}: candidates {cand.tolist()}, picks {chosen.tolist()}, radius {radius.tolist()}")
    assert [unc[i].item() for i in chosen] == [3.0, 2.0, 1.0] and chosen[0] == cand[0]             # the first pick: the most uncertain candidate
    assert set(chosen.tolist()) <= set(cand.tolist())
    keep, cfg.uncertainty_pool = cfg.uncertainty_pool, 'CCMS'
    try:
        again = apis.calculate_uncertainty(cfg, model, _loader(ds, 4), X_L=X_L, budget=budget, candidate_factor=factor, max_obj=K, score_thr=thr,
                                           clsW=False, iou_thr=0.5)
    finally:
        cfg.uncertainty_pool = keep
    assert torch.equal(again, unc)
    X_L_next, _ = update_X_L(unc, np.arange(N_POOL), X_L, budget, zeroRate=0)
    assert X_L_next.tolist() == sorted([0, 9] + chosen.tolist())


def test_ssd_detector_raises():
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_SSD.py'))
    cfg.model.backbone.pop('init_cfg', None)
    model = build_detector(cfg.model).cuda().eval()
    with pytest.raises(NotImplementedError, match='SSD'):
        model.simple_test(torch.zeros(1, 3, 300, 300, device='cuda'), [{}], isEval=True, _padded=True, objDesc=8)

    class _L:
        batch_size, dataset, collate_fn = 2, [0] * 4, None
    with pytest.raises(NotImplementedError, match='SSD'):
        apis.CCMS_uncertainty(cfg, model, _L(), X_L=[0], budget=1)
