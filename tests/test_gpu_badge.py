"""GPU: the BADGE acquisition -- aod_badge_embedding (scoring.badge_embedding), aod_object_posterior (scoring.object_posterior)
and aod_kmeanspp_seed (scoring.kmeanspp_seed) against the float64 restatements of tests/kmeanspp_util.py, their bit properties, and the pool
pass apis.single_gpu_badge_embeddings / apis.BADGE_uncertainty / apis.KMeansPP_uncertainty (graph replay and eager, evidence head and plain
RetinaNet).

Bounds (derived, not measured):
  embedding   dyadic inputs: bit-equal.  float inputs: |device - float64| <= (K + 2) * 2^-24 * sum_o |a_o[c]| |f_o[j]| per entry, the K-term
              dot-product bound
  seeding     integer descriptors with sum_k (a - a')^2 < 2^24: every fp32 distance and every fp64 sum is exact, so picks, weight and total
              EQUAL the float64 restatement.  float descriptors (N <= 1000, D <= 64): the device's own pick sequence replayed in float64,
              lo64(pick) - tau <= draws[t] * T64 <= hi64(pick) + tau with tau = 4 (D + 4) 2^-24 T64 and |total[t] - T64| <= (D + 4) 2^-24 T64
              (kmeanspp_util.replay_check carries the derivation)"""
import os

import numpy as np
import pytest
import torch

from tests import kmeanspp_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------- embedding
EMB_CASES = [(20, 256, 32), (7, 72, 5), (80, 256, 64)]


@pytest.mark.parametrize('n_cls, Cf, K', EMB_CASES)
def test_embedding_of_dyadic_inputs_is_the_float64_result_bit_for_bit(n_cls, Cf, K):
    from aod_meh_hua_amd import scoring
    feat, post, cls, cnt = U.dyadic_objects(n_cls + K, 4, K, Cf, n_cls + 1, n_cls, cnt=[K, 0, max(K // 2, 1), 1])
    want, _ = U.embedding_float64(feat, post, cls, cnt, n_cls)
    got = scoring.badge_embedding(*(_dev(a) for a in (feat, post, cls, cnt)), n_cls)
    assert got.shape == (4, n_cls * Cf) and got.dtype == torch.float32
    assert np.array_equal(_np(got).astype(np.float64), want) and not _np(got[1]).any() and _np(got[0]).any()


@pytest.mark.parametrize('n_cls, Cf, K', EMB_CASES)
def test_embedding_of_float_inputs_is_within_the_dot_product_bound(n_cls, Cf, K):
    from aod_meh_hua_amd import scoring
    feat, post, cls, cnt = U.float_objects(100 + n_cls, 3, K, Cf, n_cls, n_cls, cnt=[K, max(K // 3, 1), K])
    want, bound = U.embedding_float64(feat, post, cls, cnt, n_cls)
    got = _np(scoring.badge_embedding(*(_dev(a) for a in (feat, post, cls, cnt)), n_cls)).astype(np.float64)
    err = np.abs(got - want)
    print(f'embedding n_cls={n_cls} Cf={Cf} K={K}: max |err| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}')
    assert (err <= bound).all(), float((err - bound).max())


def test_embedding_pads_empty_images_and_batch_places():
    """cnt = 0 writes the zero row and leaves its neighbours alone; a NaN pad column and NaN rows >= cnt change nothing; an image has the
    same bits alone and at every place of a batch of 3"""
    from aod_meh_hua_amd import scoring
    n_cls, Cf, K, W = 20, 256, 32, 21
    feat, post, cls, cnt = U.float_objects(7, 3, K, Cf, W, n_cls, cnt=[5, 0, K])
    args = [_dev(a) for a in (feat, post, cls, cnt)]
    ref = scoring.badge_embedding(*args, n_cls)
    store = torch.full((5, n_cls * Cf + 8), 7.0, device='cuda')
    out = scoring.badge_embedding(*args, n_cls, out=store[1:4, :n_cls * Cf])
    assert out.data_ptr() == store[1].data_ptr() and torch.equal(_bits(store[1:4, :n_cls * Cf]), _bits(ref))
    assert not bool(ref[1].any()) and bool((store[0] == 7).all()) and bool((store[4] == 7).all()) and bool((store[:, n_cls * Cf:] == 7).all())
    feat_p, post_p, cls_p = feat.copy(), post.copy(), cls.copy()
    post_p[:, :, n_cls:] = np.nan
    feat_p[0, 5:], post_p[0, 5:], cls_p[0, 5:] = np.nan, np.nan, 3
    feat_p[1], post_p[1] = np.nan, np.nan
    got = scoring.badge_embedding(_dev(feat_p), _dev(post_p), _dev(cls_p), args[3], n_cls)
    assert torch.equal(_bits(got), _bits(ref)) and bool(torch.isfinite(got).all())
    for b in range(3):
        alone = scoring.badge_embedding(*(a[b:b + 1].contiguous() for a in args), n_cls)
        assert torch.equal(_bits(alone[0]), _bits(ref[b])), b
        for place in range(3):
            order = [(b + k - place) % 3 for k in range(3)]              # image b at index `place`
            moved = scoring.badge_embedding(*(a[order].contiguous() for a in args), n_cls)
            assert torch.equal(_bits(moved[place]), _bits(ref[b])), (b, place)


def test_object_posterior_slots_on_planted_rows():
    from aod_meh_hua_amd import scoring
    g = np.random.default_rng(3)
    B, n, W, max_num, K = 3, 50, 21, 12, 4
    scores = g.random((B, n, W)).astype(np.float32)
    dets = np.zeros((B, max_num, 5), np.float32)
    dets[:, :, 4] = np.sort(g.random((B, max_num)).astype(np.float32), axis=1)[:, ::-1]
    dets[0, :, 4] = np.linspace(0.9, 0.35, max_num)                      # image 0: more than K objects
    dets[1, :, 4] = 0.3                                                  # image 1: none (the gate is strict)
    num = np.array([max_num, max_num, 5], np.int32)
    obj_cand = g.integers(0, n, (B, max_num)).astype(np.int32)
    obj_cand[0, 1] = -1                                                  # a row without a candidate takes no slot
    want, cnt = U.posterior_slots(scores, dets, num, obj_cand, K, 0.3)
    assert cnt[0] == K and cnt[1] == 0
    got = scoring.object_posterior(_dev(scores), _dev(dets), _dev(num), _dev(obj_cand), K, 0.3)
    assert got.shape == (B, K, W) and np.array_equal(_np(got).view(np.int32), want.view(np.int32))      # every word, the zero rows included


# ---------------------------------------------------------------------------------------------------------------- seeding, exact
def _seed(desc, excluded, budget, draws):
    from aod_meh_hua_amd import scoring
    picks, weight, total = scoring.kmeanspp_seed(_dev(desc), excluded, budget, draws=draws)
    assert picks.dtype == torch.int64 and weight.dtype == torch.float32 and total.dtype == torch.float64
    assert picks.shape == weight.shape == total.shape == (budget,)
    return _np(picks), _np(weight), _np(total)


def _exact(desc, excluded, budget, seed=0, draws=None):
    from aod_meh_hua_amd import scoring
    desc = np.ascontiguousarray(desc, np.float32)
    draws = np.random.default_rng(seed).random(budget) if draws is None else np.asarray(draws, np.float64)
    want = U.seed_float64(desc, excluded, budget, draws, scoring.kmeanspp_block())
    got = _seed(desc, excluded, budget, draws)
    assert got[0].tolist() == want[0].tolist(), (got[0][:10], want[0][:10])
    assert np.array_equal(got[1].astype(np.float64), want[1]) and np.array_equal(got[2], want[2])
    assert len(set(got[0].tolist())) == budget and not set(got[0].tolist()) & set(np.asarray(excluded).reshape(-1).tolist())
    return got


def test_seeding_is_exact_at_one_and_seven_columns():
    g = np.random.default_rng(11)
    _exact(g.integers(-20, 21, (200, 1)), [3, 0, 150], 12, seed=1)
    _exact(g.integers(0, 10, (300, 7)), g.permutation(300)[:40], 25, seed=2)      # the scalar path
    _exact(g.integers(0, 10, (33, 5)), [], 3, seed=3)                             # one row past a block


@pytest.mark.parametrize('D', [2048, 2052, 20480])
def test_seeding_is_exact_on_wide_rows(D):
    g = np.random.default_rng(D)
    desc = g.integers(0, 3, (70, D))
    desc[40] = 2                                                                  # the longest row: pick 0
    picks, weight, _ = _exact(desc, [1, 69, 33], 8, seed=D)
    assert picks[0] == 40 and weight[0] == 4.0 * D


def test_seeding_never_samples_a_duplicate_of_a_pick_and_takes_them_in_order_at_zero_total():
    g = np.random.default_rng(5)
    rows = g.integers(0, 6, (4, 4))
    while len({tuple(r) for r in rows.tolist()}) < 4:
        rows = g.integers(0, 6, (4, 4))
    desc = rows[g.integers(0, 4, 90)]                                             # 90 rows, 4 distinct
    excluded = [0, 7, 50, 51, 89]
    picks, weight, total = _exact(desc, excluded, 85, seed=6)                     # the budget: every eligible row
    assert sorted(picks.tolist()) == sorted(set(range(90)) - set(excluded))
    live = total > 0
    assert 1 <= live.sum() <= 3 and (weight[1:][live[1:]] > 0).all() and not weight[1:][~live[1:]].any()
    seen = {tuple(desc[picks[0]])}
    for t in np.flatnonzero(live):                                                # while T > 0 a pick never repeats a picked row
        assert tuple(desc[picks[t]]) not in seen
        seen.add(tuple(desc[picks[t]]))
    tail = picks[1:][~live[1:]]
    assert tail.tolist() == sorted(tail.tolist())                                 # T = 0: the lowest eligible row, one after the other


def test_seeding_ignores_the_order_of_excluded_and_takes_an_empty_set():
    g = np.random.default_rng(8)
    desc = g.integers(-5, 6, (500, 12))
    excluded = g.permutation(500)[:60]
    a = _exact(desc, excluded, 30, seed=9)
    b = _exact(desc, excluded[::-1].copy(), 30, seed=9)
    c = _exact(desc, torch.from_numpy(np.sort(excluded)), 30, seed=9)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    _exact(desc, [], 30, seed=9)
    _exact(desc[:7], [], 7, seed=10)                                              # every row of a pool smaller than a block


def test_integer_weights_are_sampled_in_proportion():
    """N = 5, the draws swept over the grid (k + 1/2) / T: row i is picked exactly w_i times -- the deterministic form of 'probability
    proportional to D^2'"""
    desc = np.array([[0, 6], [0, 5], [1, 5], [2, 4], [0, 2]], np.float32)         # from (0, 6): 1, 2, 8, 16 -> T = 27
    hits = np.zeros(5, int)
    for k in range(27):
        picks, weight, total = _seed(desc, [], 2, [0.0, (k + 0.5) / 27])
        assert picks[0] == 0 and weight[0] == 36 and total.tolist() == [0.0, 27.0]
        hits[picks[1]] += 1
    assert hits.tolist() == [0, 1, 2, 8, 16]


def test_seeding_is_exact_past_one_trip_of_every_workgroup():
    """262 444 rows of 4 columns: more blocks than workgroups, several trips each, the heaviest rows past the first trip"""
    g = np.random.default_rng(12)
    N = 262444
    desc = g.integers(0, 4, (N, 4))
    desc[N - 200:] = g.integers(40, 60, (200, 4))
    desc[N - 3] = 63
    picks, weight, total = _exact(desc, [N - 1, 5, 100000], 5, draws=[0.0, 0.999, 0.5, 0.02, 0.75])
    assert picks[0] == N - 3 and weight[0] == 4 * 63 * 63 and total[1] > 0


# ---------------------------------------------------------------------------------------------------------------- seeding, float
@pytest.mark.parametrize('N, D, n_exc, budget', [(1000, 64, 50, 24), (333, 7, 0, 16), (600, 33, 100, 16)])
def test_float_seeding_replays_in_float64_and_is_deterministic(N, D, n_exc, budget):
    g = np.random.default_rng(N + D)
    desc = g.standard_normal((N, D)).astype(np.float32)
    excluded = g.permutation(N)[:n_exc]
    draws = g.random(budget)
    picks, weight, total = _seed(desc, excluded, budget, draws)
    worst = U.replay_check(desc, excluded, picks, weight, total, draws)
    print(f'float seeding N={N} D={D}: worst margin / tau = {worst:.3f} (inside the pick\'s interval: <= 0)')
    again = _seed(desc, excluded, budget, draws)
    for a, b in zip((picks, weight, total), again):
        assert a.tobytes() == b.tobytes()
    assert len(set(picks.tolist())) == budget and not set(picks.tolist()) & set(excluded.tolist())


@pytest.mark.parametrize('D', [800, 1280])
def test_a_pair_has_the_distance_bits_of_kcenter_greedy(D):
    from aod_meh_hua_amd import scoring
    g = np.random.default_rng(D)
    desc = g.standard_normal((3, D)).astype(np.float32)
    desc[2] = 0
    dev = _dev(desc)
    picks, weight, _ = scoring.kmeanspp_seed(dev, [2], 2, draws=[0.0, 0.5])
    p0, p1 = (int(v) for v in picks)
    assert {p0, p1} == {0, 1} and (desc[p0].astype(np.float64) ** 2).sum() > (desc[p1].astype(np.float64) ** 2).sum()
    pair = torch.from_numpy(desc[:2]).cuda()
    _, radius = scoring.kcenter_greedy(pair, [p0], 1)                              # the two-row pool: d(p1, p0)
    assert torch.equal(_bits(weight[1:2]), _bits(radius))
    _, norm = scoring.kcenter_greedy(dev, [2], 1)                                  # against the all-zero row: the largest norm
    assert torch.equal(_bits(weight[0:1]), _bits(norm))


# ---------------------------------------------------------------------------------------------------------------- the whole pass
N_POOL, SIZE, BUDGET = 6, 128, 3


def _loader(ds, bs):
    from aod_meh_hua_amd.datasets import build_dataloader
    return build_dataloader(ds, samples_per_gpu=bs, workers_per_gpu=0, dist=False, shuffle=False)


def _batches(ds, bs):
    from aod_meh_hua_amd.apis.test import _unwrap
    for data in _loader(ds, bs):
        data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
        yield data['img'][0].cuda(), data['img_metas'][0]


def _build(kind):
    """the small synthetic detectors of tests/test_gpu_ccms.py, on a pool of 6 images of 128 x 128"""
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
        bench.calibrate_head(model, next(_batches(ds, 3))[0])
    return cfg, MMDataParallel(model).eval(), ds


@pytest.fixture(scope='module', params=['SSL_L_RetinaNet', 'MyRetinaNet'])
def pool(request):
    """the model, the pool, and what the model returns eagerly per batch of 3: the padded detections with det_posterior's rows (detPost) --
    the gate is the smallest of the images' top scores (that image has no object: the gate is strict), K one less than the largest object
    count (that image has more than K)"""
    cfg, model, ds = _build(request.param)
    m = model.module
    with torch.no_grad():
        outs = [m.simple_test(img, metas, rescale=True, isEval=True, _padded=True, detPost=True, isUnc=False) for img, metas in _batches(ds, 3)]
    dets, labels, num, dpost = (np.concatenate([_np(o[i]) for o in outs]) for i in range(4))
    top = np.array([dets[b, :num[b], 4].max() if num[b] else 0.0 for b in range(N_POOL)], np.float32)
    thr = float(top.min())
    n_obj = np.array([int((dets[b, :num[b], 4] > np.float32(thr)).sum()) for b in range(N_POOL)])
    assert n_obj.max() >= 2 and n_obj.min() == 0, n_obj
    K = int(min(n_obj.max() - 1, 64))
    return dict(kind=request.param, cfg=cfg, model=model, ds=ds, dets=dets, labels=labels, num=num, dpost=dpost, thr=thr, K=K, n_obj=n_obj)


def test_pool_pass_rows_eager_replayed_batch_sizes_and_the_posterior_slots(pool, monkeypatch):
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis import test as apis_test
    model, ds, thr, K = pool['model'], pool['ds'], pool['thr'], pool['K']
    m = model.module
    n_cls, Cf = int(m.bbox_head.num_classes), int(m.neck.out_channels)
    # what the model returns eagerly: the descriptors and the posterior rows in their slots
    with torch.no_grad():
        outs = [m.simple_test(img, metas, rescale=True, isEval=True, _padded=True, objDesc=K, objPost=True, score_thr=thr, isUnc=False)
                for img, metas in _batches(ds, 3)]
    assert all(len(o) == 10 for o in outs)
    feat, cls, _, cnt, missing, post = (np.concatenate([_np(o[i]) for o in outs]) for i in range(4, 10))
    assert cnt.tolist() == np.minimum(pool['n_obj'], K).tolist() and (cnt == K).any() and (cnt == 0).any() and not missing.any()
    print(f"{pool['kind']}: score_thr {thr:.6f}, K {K}, objects per image {pool['n_obj'].tolist()}")
    # post = det_posterior's rows gathered by the slot rule, bit for bit
    assert post.shape == (N_POOL, K, pool['dpost'].shape[2])
    for b in range(N_POOL):
        rows = [j for j in range(pool['num'][b]) if pool['dets'][b, j, 4] > np.float32(thr)][:K]
        assert np.array_equal(post[b, :len(rows)].view(np.int32), pool['dpost'][b, rows].view(np.int32)), b
        assert not post[b, len(rows):].view(np.int32).any() and cls[b, :len(rows)].tolist() == pool['labels'][b, rows].tolist()
    with torch.no_grad():                                                         # with objUnc too, post comes last
        both = m.simple_test(*next(_batches(ds, 3)), rescale=True, isEval=True, _padded=True, objDesc=K, objUnc=True, objPost=True, score_thr=thr,
                             isUnc=False)
    assert len(both) == 11 and both[9].shape == (3, K) and torch.equal(_bits(both[10]), _bits(outs[0][9]))
    want, bound = U.embedding_float64(feat, post, cls, cnt, n_cls)
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    ref = apis.single_gpu_badge_embeddings(model, _loader(ds, 3), max_obj=K, score_thr=thr)
    assert set(ref) == {'emb', 'cnt', 'missing'} and ref['emb'].shape == (N_POOL, n_cls * Cf) and ref['emb'].dtype == torch.float32
    assert _np(ref['cnt']).tolist() == cnt.tolist() and not _np(ref['missing']).any()
    err = np.abs(_np(ref['emb']).astype(np.float64) - want)
    assert (err <= bound).all(), float((err - bound).max())
    assert not bool(ref['emb'][int(np.flatnonzero(cnt == 0)[0])].any()) and bool(ref['emb'][int(np.flatnonzero(cnt == K)[0])].any())
    same = lambda a: all(torch.equal(_bits(a[k]), _bits(ref[k])) for k in ref)
    for bs in (1, 2):
        assert same(apis.single_gpu_badge_embeddings(model, _loader(ds, bs), max_obj=K, score_thr=thr)), bs
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    for bs in (3, 2, 1):
        assert same(apis.single_gpu_badge_embeddings(model, _loader(ds, bs), max_obj=K, score_thr=thr)), bs
    gs = [v for k, v in apis_test._GSCORE.get(model).items() if k[0] == 'badge']
    assert len(gs) == 1 and len(gs[0].cache) == 3


def test_the_two_pools_mark_exactly_the_budget_and_update_X_L_takes_the_picks(pool, monkeypatch):
    from aod_meh_hua_amd import apis, scoring
    from aod_meh_hua_amd.utils.active_datasets import update_X_L
    cfg, model, ds, thr, K = pool['cfg'], pool['model'], pool['ds'], pool['thr'], pool['K']
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    X_L = np.array([4, 1])
    keep = cfg.uncertainty_pool
    try:
        for name, fn, own in (('BADGE', apis.BADGE_uncertainty, dict(max_obj=K, score_thr=thr)), ('KMeansPP', apis.KMeansPP_uncertainty, dict())):
            unc = fn(cfg, model, _loader(ds, 3), X_L=X_L, budget=BUDGET, seed=5, **own)
            assert unc.shape == (N_POOL,) and unc.dtype == torch.float32 and not unc.is_cuda
            assert sorted(unc.tolist()) == [0.0] * (N_POOL - BUDGET) + list(range(1, BUDGET + 1)) and unc[4] == 0 and unc[1] == 0
            picks = np.argsort(-unc.numpy(), kind='stable')[:BUDGET]
            # the picks are the seeding's on the store
            desc = (apis.single_gpu_badge_embeddings(model, _loader(ds, 3), max_obj=K, score_thr=thr)['emb'] if name == 'BADGE'
                    else apis.single_gpu_descriptors(model, _loader(ds, 3)))
            assert _np(scoring.kmeanspp_seed(desc, X_L, BUDGET, seed=5)[0]).tolist() == picks.tolist()
            X_L_next, _ = update_X_L(unc, np.arange(N_POOL), X_L, BUDGET, zeroRate=0)
            assert X_L_next.tolist() == sorted([1, 4] + picks.tolist())
            assert torch.equal(fn(cfg, model, _loader(ds, 3), X_L=X_L[::-1].copy(), budget=BUDGET, seed=5, **own), unc)      # the same seed: the same vector
            cfg.uncertainty_pool = name
            again = apis.calculate_uncertainty(cfg, model, _loader(ds, 3), X_L=X_L, budget=BUDGET, seed=5, max_obj=K, score_thr=thr, clsW=False,
                                               iou_thr=0.5)
            assert torch.equal(again, unc)
            print(f"{pool['kind']} {name}: picks {picks.tolist()}")
    finally:
        cfg.uncertainty_pool = keep


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
        apis.BADGE_uncertainty(cfg, model, _L(), X_L=[0], budget=1)
    with pytest.raises(NotImplementedError, match='SSD'):
        apis.KMeansPP_uncertainty(cfg, model, _L(), X_L=[0], budget=1)
