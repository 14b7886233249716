"""GPU: the ENMS + DivProto acquisition -- aod_enms_prototypes (scoring.enms_prototypes) and aod_divproto_select
(scoring.divproto_select) against the float64 restatements of tests/divproto_util.py, their bit properties, and the pool pass
apis.single_gpu_enms / apis.ENMS_uncertainty / apis.DivProto_uncertainty (graph replay and eager, evidence head and plain RetinaNet).

The float64 side asserts ZERO ambiguous decisions for the seeds used here (no product within 1e-5 of its threshold, no two measures of an
image within 1e-6 relative unless bit-equal): the fp32 device path then has to take every decision as float64 does.

Bounds (derived, not measured):
  enms     |device - float64| <= kept * 2^-24 * E: a running fp32 sum of `kept` non-negative terms takes kept - 1 roundings
  pconf    bit-equal: a maximum rounds nothing
  proto    divproto_util.proto_bound per element: with u = 2^-24, n objects in the class and C channels, |dv| <= (n + 1) u sum_k |w_k f_k|
           (one rounding for the weight h + 2^-10, one for the product, n - 1 for the running sum), the norm inherits ||dv|| and adds
           (C / 2 + 3) u relative (C squares and additions under a square root, the root, the division); a factor 1.01 for second order
  kept, pcls, pcnt, the pick order, picks, stage: exact"""
import os

import numpy as np
import pytest
import torch

from tests import divproto_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------- kernel 1
GROUPS = {8: 4, 72: 6, 256: 6}


def _enms_case(K, C):
    """image 0: no object; 1: K planted objects; 2: one class, identical rows (kept 1, E = max h); 3: all classes distinct (kept = cnt,
    E = sum h); 4: planted, measures tied bit for bit in pairs; 5: planted, a random count"""
    seed = 1000 * K + C
    feat, cls, w, h, cnt = U.planted_images(seed, 6, K, C, GROUPS[C], 3, cnt=[0, K, K, K, K, max(K // 2, 1)])
    g = np.random.default_rng(seed + 1)
    feat[2, :K] = feat[2, 0]
    cls[2, :K] = 2
    cls[3, :K] = g.permutation(K) + 7
    for k in range(0, K - 1, 2):
        h[4, k + 1] = h[4, k]
    return feat, cls, w, h, cnt


@pytest.mark.parametrize('C', [8, 72, 256])
@pytest.mark.parametrize('K', [1, 5, 33, 64])
def test_enms_and_prototypes_match_float64_and_are_batch_and_replay_invariant(K, C):
    from aod_meh_hua_amd import scoring
    feat, cls, w, h, cnt = _enms_case(K, C)
    want = []
    for b in range(6):
        E, kept, picks, amb = U.enms_float64(np.nan_to_num(feat[b]), cls[b], h[b], cnt[b])
        assert amb == [], (b, amb)                                   # never skipped: an ambiguous seed is changed
        want.append((E, kept, picks) + U.prototypes_float64(np.nan_to_num(feat[b]), cls[b], w[b], h[b], cnt[b]))
    assert want[0][:2] == (0.0, 0) and want[2][1] == 1 and want[2][0] == float(h[2, :K].max()) and want[3][1] == K      # the case is what it claims
    if K >= 33:
        assert 1 < want[1][1] < K and want[1][6] == 3                # the planted image: some suppression, all three classes
    args = [_dev(a) for a in (feat, cls, w, h, cnt)]
    enms, kept, proto, pcls, pconf, pcnt, pick = scoring.enms_prototypes(*args, want_picks=True)
    assert proto.shape == (6, K, C) and proto.dtype == torch.float32 and pick.dtype == torch.int32 and bool(torch.isfinite(proto).all())
    worst = 0.0
    for b, (E, kp, picks, p64, c64, conf64, n64, bound) in enumerate(want):
        assert int(kept[b]) == kp and _np(pick[b]).tolist() == picks + [-1] * (K - kp), b
        assert int(pcnt[b]) == n64 and np.array_equal(_np(pcls[b]), c64), b
        assert np.array_equal(_np(pconf[b]).view(np.int32), conf64.view(np.int32)), b
        assert abs(float(enms[b]) - E) <= kp * 2.0 ** -24 * E, (b, float(enms[b]), E)
        err = np.abs(_np(proto[b]).astype(np.float64) - p64)
        assert (err <= bound).all(), (b, float((err - bound).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-30)).max()))
    print(f'enms K={K} C={C}: kept {_np(kept).tolist()}, pcnt {_np(pcnt).tolist()}, max |proto err| / bound = {worst:.3f}')
    assert float(enms[3]) > 0 and abs(float(enms[3]) - float(h[3, :K].astype(np.float64).sum())) <= K * 2.0 ** -24 * want[3][0]
    outs = (enms, kept, proto, pcls, pconf, pcnt, pick)
    for b in range(6):                                               # an image alone: the bits of its rows in the batch
        alone = scoring.enms_prototypes(*(a[b:b + 1] for a in args), want_picks=True)
        for got, ref in zip(alone, outs):
            assert torch.equal(_bits(got[0]), _bits(ref[b])), b
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed = scoring.enms_prototypes(*args, want_picks=True)
    for _ in range(2):
        for t in replayed:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip(replayed, outs):
            assert torch.equal(_bits(got), _bits(ref))


def test_enms_hand_case_and_the_threshold_of_one():
    from aod_meh_hua_amd import scoring
    c = U.hand_enms_case()
    args = [_dev(a[None]) for a in (c['feat'], c['cls'], c['w'], c['h'])] + [torch.tensor([4], dtype=torch.int32, device='cuda')]
    enms, kept, proto, pcls, pconf, pcnt, pick = scoring.enms_prototypes(*args, want_picks=True)
    assert _np(pick[0]).tolist() == [1, 2, 3, -1] and int(kept[0]) == 3 and abs(float(enms[0]) - c['E']) <= 3 * 2.0 ** -24 * c['E']
    assert _np(pcls[0]).tolist() == [0, 1, -1, -1] and int(pcnt[0]) == 2 and _np(pconf[0]).tolist() == [np.float32(0.9), np.float32(0.6), 0.0, 0.0]
    # t_enms = 1 suppresses nothing, identical rows included
    args[0] = args[0].clone()
    args[0][0, 1] = args[0][0, 0]
    enms, kept, *_, pick = scoring.enms_prototypes(*args, t_enms=1.0, want_picks=True)
    assert _np(pick[0]).tolist() == [1, 2, 0, 3] and int(kept[0]) == 4


# ---------------------------------------------------------------------------------------------------------------- selection
def _select(order, pool, n_cls, budget, **kw):
    from aod_meh_hua_amd import scoring
    picks, stage = scoring.divproto_select(np.asarray(order), *(_dev(a) for a in pool), n_cls, budget, **kw)
    assert picks.dtype == torch.int64 and stage.dtype == torch.int32 and picks.shape == stage.shape == (budget,)
    return _np(picks).tolist(), _np(stage).tolist()


@pytest.mark.parametrize('budget', [7, 4, 2])
def test_selection_on_the_hand_pool(budget):
    c = U.hand_pool()
    pool = (c['proto'], c['pcls'], c['pconf'], c['pcnt'])
    assert _select(range(7), pool, 3, budget) == c['answers'][budget]
    assert _select(range(7), pool, 3, budget, _chunk=1) == c['answers'][budget]
    if budget == 7:
        assert _select(range(7), pool, 3, 7, class_balance=False) == ([0, 2, 3, 4, 6, 1, 5], [1] * 5 + [3, 3])


N48 = 48


@pytest.fixture(scope='module')
def pool48():
    pool = U.planted_pool(48, N48, 4, 8, 4, 4, empty=(3, 17, 40))
    g = np.random.default_rng(49)
    enms = (g.integers(0, 6, N48) / 4).astype(np.float32)            # few distinct scores: ties in the sweep order
    return pool, enms


@pytest.mark.parametrize('beta', [0.75, 1.0])
@pytest.mark.parametrize('balance', [True, False])
@pytest.mark.parametrize('budget', [1, 7, 44])
def test_selection_on_the_planted_pool_is_exact(pool48, budget, balance, beta):
    from aod_meh_hua_amd import scoring
    pool, enms = pool48
    X_L = [0, 5, 11, 30]
    order = scoring.divproto_order(torch.from_numpy(enms), X_L)
    assert order.tolist() == U.sweep_order(enms, X_L).tolist() and len(order) == 44 and not set(order.tolist()) & set(X_L)
    picks, stage, amb = U.select_float64(order, *pool, 4, budget, beta=beta, class_balance=balance)
    assert amb == []
    got = _select(order, pool, 4, budget, beta=beta, class_balance=balance)
    print(f'select N=48 budget={budget} balance={balance} beta={beta}: stages {np.bincount(stage, minlength=4)[1:].tolist()}')
    assert got == (picks.tolist(), stage.tolist())
    assert not set(got[0]) & set(X_L) and len(set(got[0])) == budget
    if budget == 44:
        assert sorted(got[0]) == sorted(order.tolist()) and 3 in got[1]                  # the whole sweep: the fill runs
        if balance and beta == 0.75:
            assert set(got[1]) == {1, 2, 3}
    if balance and beta == 1.0:
        assert 2 not in got[1]                                                            # free = 0: no stage-2 accept
    # the order of X_L does not matter
    assert scoring.divproto_order(torch.from_numpy(enms), X_L[::-1]).tolist() == order.tolist()


def test_selection_across_launch_boundaries():
    """M = 2 * chunk + 3 candidates: three sweep launches; the same inputs through one oversized launch and through launches of 7"""
    from aod_meh_hua_amd import scoring
    M = 2 * scoring.divproto_chunk() + 3
    N = M + 5
    pool = U.planted_pool(7, N, 3, 8, 4, 4, empty=(2, 100))
    g = np.random.default_rng(8)
    order = g.permutation(N)[:M]
    for budget in (20, 100):
        picks, stage, amb = U.select_float64(order, *pool, 4, budget)
        assert amb == []
        ref = (picks.tolist(), stage.tolist())
        print(f'select M={M} budget={budget}: stages {np.bincount(stage, minlength=4)[1:].tolist()}')
        assert _select(order, pool, 4, budget) == ref
        assert _select(order, pool, 4, budget, _chunk=65536) == ref
        assert _select(order, pool, 4, budget, _chunk=7) == ref
    assert 3 in ref[1] and 1 in ref[1]                               # budget 100: the 16 (class, group) pairs run out, the fill takes over


def test_selection_with_64_slots_and_256_channels():
    """the widest candidate: 64 classes of 128, C = 256 -- every LDS row, every lane group"""
    g = np.random.default_rng(5)
    N, K, C, n_cls = 40, 64, 256, 128
    cen = U.centres(g, C, 6)
    proto = np.zeros((N, K, C), np.float32)
    pcls = np.full((N, K), -1, np.int32)
    pconf = np.zeros((N, K), np.float32)
    pcnt = g.integers(1, K + 1, N).astype(np.int32)
    pcnt[0] = K
    for i in range(N):
        n = int(pcnt[i])
        proto[i, :n] = U.planted_rows(g, cen, g.integers(0, 6, n))
        pcls[i, :n] = np.sort(g.choice(n_cls, n, replace=False))
        pconf[i, :n] = g.uniform(0.05, 1.0, n)
    pool = (proto, pcls, pconf, pcnt)
    picks, stage, amb = U.select_float64(range(N), *pool, n_cls, 25)
    assert amb == []
    assert _select(range(N), pool, n_cls, 25) == (picks.tolist(), stage.tolist())


# ---------------------------------------------------------------------------------------------------------------- the whole pass
N_POOL, SIZE, BS, BUDGET, K_E2E = 12, 128, 4, 4, 8


def _loader(ds, bs):
    from aod_meh_hua_amd.datasets import build_dataloader
    return build_dataloader(ds, samples_per_gpu=bs, workers_per_gpu=0, dist=False, shuffle=False)


def _batches(ds, bs):
    from aod_meh_hua_amd.apis.test import _unwrap
    for data in _loader(ds, bs):
        data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
        yield data['img'][0].cuda(), data['img_metas'][0]


def _build(kind):
    """the small synthetic detectors of tests/test_gpu_ccms.py, on a pool of 12 images of 128 x 128"""
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
    model.load_state_dict(sd(), strict=True)
    model = model.cuda().eval()
    ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=N_POOL, size=(SIZE, SIZE)), dict(test_mode=True))
    if kind == 'SSL_L_RetinaNet':
        import bench
        bench.calibrate_head(model, next(_batches(ds, BS))[0])
    return cfg, MMDataParallel(model).eval(), ds


def _objects(model, ds, kind, thr_of):
    """every batch of 4 by hand: the padded detections and det_uncertainty's per-object values -> (dets, num, obj_out, thr) numpy"""
    from aod_meh_hua_amd import scoring
    m = model.module
    head = m.bbox_head
    layout = scoring.ACTIVATION_LAYOUT[head.last_activation]
    keep = []
    with torch.no_grad():
        for img, metas in _batches(ds, BS):
            feats = m.extract_feat(img)
            outs = head.test_heads(feats, with_L=False)[0] if kind == 'SSL_L_RetinaNet' else head.test_heads(feats)[0]
            _, _, it = head.get_bboxes(*outs, metas, rescale=True, isEval=False, isUnc='Epistemic', uPool='Entropy', unc_aggregate='sum',
                                       score_thr=0.3, _return_internals=True)
            keep.append((it['cand'], it['dets'], it['labels'], it['num']))
        dets = np.concatenate([_np(k[1]) for k in keep])
        num = np.concatenate([_np(k[3]) for k in keep])
        thr = thr_of(dets, num)
        obj = [scoring.det_uncertainty(c, d, l, n, layout, 'entropy', 'sum', thr, want_objects=True)[1] for c, d, l, n in keep]
    return dets, np.concatenate([_np(k[2]) for k in keep]), num, np.concatenate([_np(o) for o in obj]), thr


def _gate(dets, num):
    """the gate of this fixture: the smallest of the images' top scores -- that image has no object (the gate is strict)"""
    top = np.array([dets[b, :num[b], 4].max() if num[b] else 0.0 for b in range(len(num))], np.float32)
    return float(top.min())


@pytest.fixture(scope='module', params=['SSL_L_RetinaNet', 'MyRetinaNet'])
def pool(request):
    cfg, model, ds = _build(request.param)
    dets, labels, num, obj_out, thr = _objects(model, ds, request.param, _gate)
    return dict(kind=request.param, cfg=cfg, model=model, ds=ds, dets=dets, labels=labels, num=num, obj_out=obj_out, thr=thr)


STORE = ('enms', 'kept', 'proto', 'pcls', 'pconf', 'pcnt', 'missing', 'h', 'w', 'cls', 'cnt')


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in STORE)


def test_pool_pass_objects_bits_eager_replayed_and_batch_sizes(pool, monkeypatch):
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis import test as apis_test
    cfg, model, ds, thr, K = pool['cfg'], pool['model'], pool['ds'], pool['thr'], K_E2E
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    ref = apis.single_gpu_enms(model, _loader(ds, BS), max_obj=K, score_thr=thr, keep_objects=True)
    assert set(ref) == set(STORE) and ref['proto'].shape == (N_POOL, K, 256) and _np(ref['missing']).tolist() == [0] * N_POOL
    n_obj = np.array([int((pool['dets'][b, :pool['num'][b], 4] > np.float32(thr)).sum()) for b in range(N_POOL)])
    print(f"{pool['kind']}: score_thr {thr:.6f}, objects per image {n_obj.tolist()}, kept {_np(ref['kept']).tolist()}, pcnt {_np(ref['pcnt']).tolist()}, "
          f"enms {[round(v, 4) for v in ref['enms'].tolist()]}")
    assert int((n_obj >= 2).sum()) >= N_POOL // 3 and int((n_obj == 0).sum()) >= 1          # the pass is not vacuous
    assert _np(ref['cnt']).tolist() == np.minimum(n_obj, K).tolist()
    # h and w: det_uncertainty's per-object values and the detections' scores at the gated rows, in row order
    for b in range(N_POOL):
        rows = [j for j in range(pool['num'][b]) if pool['dets'][b, j, 4] > np.float32(thr)][:K]
        n = len(rows)
        assert np.array_equal(_np(ref['h'][b, :n]).view(np.int32), pool['obj_out'][b, rows].view(np.int32)) and not bool(ref['h'][b, n:].any()), b
        assert np.array_equal(_np(ref['w'][b, :n]), pool['dets'][b, rows, 4]) and not bool(ref['w'][b, n:].any()), b
        assert _np(ref['cls'][b]).tolist() == pool['labels'][b, rows].tolist() + [-1] * (K - n)
        assert np.isfinite(pool['obj_out'][b, rows]).all()
    # ENMS and the prototypes of the store: the restatement on the CCMS pass's own features
    ccms = apis.single_gpu_object_descriptors(model, _loader(ds, BS), max_obj=K, score_thr=thr)
    assert torch.equal(ccms['cls'], ref['cls']) and torch.equal(_bits(ccms['w']), _bits(ref['w'])) and torch.equal(ccms['cnt'], ref['cnt'])
    feat, cls, w, h, cnt = (_np(t) for t in (ccms['feat'], ref['cls'], ref['w'], ref['h'], ref['cnt']))
    for b in range(N_POOL):
        E, kept, _, amb = U.enms_float64(feat[b], cls[b], h[b], cnt[b])
        p64, c64, conf64, n64, bound = U.prototypes_float64(feat[b], cls[b], w[b], h[b], cnt[b])
        assert amb == [], (b, amb)
        assert int(ref['kept'][b]) == kept and abs(float(ref['enms'][b]) - E) <= kept * 2.0 ** -24 * E
        assert int(ref['pcnt'][b]) == n64 and np.array_equal(_np(ref['pcls'][b]), c64) and np.array_equal(_np(ref['pconf'][b]), conf64)
        assert (np.abs(_np(ref['proto'][b]).astype(np.float64) - p64) <= bound).all(), b
    assert torch.equal(_bits(apis.ENMS_uncertainty(cfg, model, _loader(ds, BS), max_obj=K, score_thr=thr)), _bits(ref['enms'].cpu()))
    assert _same(apis.single_gpu_enms(model, _loader(ds, 1), max_obj=K, score_thr=thr, keep_objects=True), ref)
    # replayed: one graph per batch shape
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    for bs in (BS, 1):
        assert _same(apis.single_gpu_enms(model, _loader(ds, bs), max_obj=K, score_thr=thr, keep_objects=True), ref), bs
    gs = [v for k, v in apis_test._GSCORE.get(model).items() if k[0] == 'enms']
    assert len(gs) == 1 and len(gs[0].cache) == 2
    small = apis.single_gpu_enms(model, _loader(ds, BS), max_obj=K, score_thr=thr)
    assert set(small) == set(STORE[:7]) and torch.equal(_bits(small['proto']), _bits(ref['proto']))       # no larger than the CCMS store


def test_divproto_uncertainty_is_the_restatement_on_the_store_and_update_X_L_takes_it(pool, monkeypatch):
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.utils.active_datasets import update_X_L
    cfg, model, ds, thr, K = pool['cfg'], pool['model'], pool['ds'], pool['thr'], K_E2E
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    X_L = np.array([0, 9])
    n_cls = int(model.module.bbox_head.num_classes)
    store = apis.single_gpu_enms(model, _loader(ds, BS), max_obj=K, score_thr=thr)
    tensors = [_np(store[k]) for k in ('proto', 'pcls', 'pconf', 'pcnt')]
    order = U.sweep_order(_np(store['enms']), X_L)
    for kw in (dict(), dict(class_balance=False), dict(t_intra=0.2, beta=0.5)):
        picks, stage, amb = U.select_float64(order, *tensors, n_cls, BUDGET, **kw)
        assert amb == [], amb
        unc = apis.DivProto_uncertainty(cfg, model, _loader(ds, BS), X_L=X_L, budget=BUDGET, max_obj=K, score_thr=thr, **kw)
        print(f"{pool['kind']} {kw}: sweep {order.tolist()}, picks {picks.tolist()}, stages {stage.tolist()}")
        assert unc.shape == (N_POOL,) and unc.dtype == torch.float32 and not unc.is_cuda
        want = np.zeros(N_POOL, np.float32)
        want[picks] = np.arange(BUDGET, 0, -1)
        assert np.array_equal(unc.numpy(), want) and unc[0] == 0 and unc[9] == 0
    unc = apis.DivProto_uncertainty(cfg, model, _loader(ds, BS), X_L=X_L, budget=BUDGET, max_obj=K, score_thr=thr)
    keep, cfg.uncertainty_pool = cfg.uncertainty_pool, 'DivProto'
    try:
        again = apis.calculate_uncertainty(cfg, model, _loader(ds, BS), X_L=X_L, budget=BUDGET, max_obj=K, score_thr=thr, clsW=False, iou_thr=0.5)
        cfg.uncertainty_pool = 'ENMS'
        enms = apis.calculate_uncertainty(cfg, model, _loader(ds, BS), max_obj=K, score_thr=thr, clsW=False, iou_thr=0.5)
    finally:
        cfg.uncertainty_pool = keep
    assert torch.equal(again, unc) and torch.equal(_bits(enms), _bits(store['enms'].cpu()))
    picks = U.select_float64(order, *tensors, n_cls, BUDGET)[0]
    X_L_next, _ = update_X_L(unc, np.arange(N_POOL), X_L, BUDGET, zeroRate=0)
    assert X_L_next.tolist() == sorted([0, 9] + picks.tolist())


def test_without_its_checks_divproto_is_the_top_budget_by_summed_entropy(pool, monkeypatch):
    from aod_meh_hua_amd import apis
    cfg, model, ds, thr = pool['cfg'], pool['model'], pool['ds'], pool['thr']
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    n_obj = np.array([int((pool['dets'][b, :pool['num'][b], 4] > np.float32(thr)).sum()) for b in range(N_POOL)])
    assert n_obj.max() <= 64
    unc = apis.DivProto_uncertainty(cfg, model, _loader(ds, BS), X_L=[], budget=BUDGET, max_obj=64, score_thr=thr, t_enms=1.0, t_intra=1.0,
                                    class_balance=False)
    post = apis.Posterior_uncertainty(cfg, model, _loader(ds, BS), measure='entropy', aggregate='sum', score_thr=thr).numpy()
    top = np.argsort(-post.astype(np.float64), kind='stable')[:BUDGET + 1]
    assert post[top[BUDGET - 1]] - post[top[BUDGET]] > 1e-5 * post[top[0]]                  # the cut is no near-tie: the sets are comparable
    print(f"{pool['kind']}: summed entropy {post.round(4).tolist()}, top {top[:BUDGET].tolist()}, picks {np.nonzero(unc.numpy())[0].tolist()}")
    assert set(np.nonzero(unc.numpy())[0].tolist()) == set(top[:BUDGET].tolist())
    assert unc.numpy()[top[0]] == BUDGET                                                    # the first pick: the largest summed entropy


def test_ssd_detector_raises():
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_SSD.py'))
    cfg.model.backbone.pop('init_cfg', None)
    model = build_detector(cfg.model).cuda().eval()

    class _L:
        batch_size, dataset, collate_fn = 2, [0] * 4, None
    with pytest.raises(NotImplementedError, match='SSD'):
        apis.DivProto_uncertainty(cfg, model, _L(), X_L=[0], budget=1)
    with pytest.raises(NotImplementedError, match='SSD'):
        apis.ENMS_uncertainty(cfg, model, _L())
