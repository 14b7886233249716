"""GPU: the consistency pool -- aod_flip_images against torch.flip, aod_det_posterior on hand-built candidates,
aod_det_consistency against the float64 restatement on integer-coordinate boxes (every IoU operand exact, so the match is asserted equal),
the pool pass apis.single_gpu_consistency on the three detector families (eager, replayed, batch sizes 1 / 2 / 3) and the hand-over to
update_X_L.

Tolerances (tests/consistency_util.py, derived in the issue): absolute (4 T + 4 V + 32) * 2^-24 per object value, T the number of column
terms of a Jensen-Shannon value; 16 * 2^-24 more for an image's max and mean, `count` times that for its sum; an entry whose float64
value is exactly 0 must be exactly 0."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests import consistency_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THR = 0.3
VIEWS3 = ('hflip', 'vflip', 'hvflip')
ORDERS = ([0], [1], [2], [1, 0, 2], [2, 1, 0], [0, 2, 1])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- flip
DIMS = {'hflip': (2,), 'vflip': (1,), 'hvflip': (1, 2)}


def _flip(src, hw, view):
    from aod_meh_hua_amd import hipops as ho
    dst = torch.full_like(src, float('nan'))
    out = ho.flip_images(src, dst, torch.tensor(hw, dtype=torch.int32, device='cuda'), view)
    assert out is dst
    return dst


def _flip_want(src, hw, view):
    want = src.clone()
    for b, (h, w) in enumerate(hw):
        want[b, :, :h, :w] = torch.flip(src[b, :, :h, :w], DIMS[view])
    return want


def _unaligned(t):
    """a contiguous view of t's shape whose base is 4-B but not 16-B aligned, holding t's bits"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    off = next(o for o in range(1, 5) if (buf.data_ptr() + 4 * o) % 16 == 4)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize('case', ['aligned', 'odd_width_unaligned_base'])
def test_flip_matches_torch_flip_keeps_the_pad_and_is_an_involution(case):
    # the pad keeps its random values, so that every pad pixel differs from the one a mirrored row or column would bring there -- to the
    # right of the window (rows y < h, columns x >= w: (5, 7) in Wp = 16 has a quad that straddles w) as well as below it; a NaN with its
    # own payload per (image, channel, row) and a -0 are planted in both parts
    g = torch.Generator().manual_seed(11)
    if case == 'aligned':
        src, hw = torch.randn(3, 3, 8, 16, generator=g).cuda(), [(8, 16), (5, 7), (1, 1)]
        assert src.data_ptr() % 16 == 0
    else:
        src, hw = torch.randn(2, 3, 5, 7, generator=g).cuda(), [(5, 7), (3, 4)]
    B, C, Hp, Wp = src.shape
    payload = (0x7fc00001 + torch.arange(B * C * Hp, dtype=torch.int32, device='cuda')).view(B, C, Hp)
    for b, (h, w) in enumerate(hw):
        if w < Wp:
            src.view(torch.int32)[b, :, :, Wp - 1] = payload[b]                    # the last column: right of the window in every row
            src[b, :, ::2, w] = -0.0                                               # the first pad column, every second row
        if h < Hp:
            src.view(torch.int32)[b, :, h:, 0] = payload[b, :, h:]                 # below the window
            src[b, :, h, 1:w] = -0.0
    if case != 'aligned':
        src = _unaligned(src)
    for b, (h, w) in enumerate(hw):                                                # the data can tell a mirrored pad from an untouched one
        if w < Wp and h > 1:
            right = _bits(src[b, :, :h, w:])
            assert not torch.equal(right, torch.flip(right, (1,)))
    for view in VIEWS3:
        got = _flip(src, hw, view)
        assert torch.equal(_bits(got), _bits(_flip_want(src, hw, view))), view                      # the window mirrored, the pad src's bits
        for b, (h, w) in enumerate(hw):
            pad = torch.ones(src.shape[1:], dtype=torch.bool, device='cuda')
            pad[:, :h, :w] = False
            assert torch.equal(_bits(got[b])[pad], _bits(src[b])[pad]), (view, b)
        assert torch.equal(_bits(_flip(got, hw, view)), _bits(src)), view                           # twice: src's bits
        assert torch.equal(_bits(_flip(src, hw, U.VIEWS[view])), _bits(got))                        # a code names the same view
        # the scalar path (an unaligned base) and the 16-B path give the same bits
        assert torch.equal(_bits(_flip(_unaligned(src), hw, view)), _bits(got)), view
        order = [2, 0, 1][:len(hw)] if len(hw) == 3 else [1, 0]
        moved = _flip(src[order].contiguous(), [hw[i] for i in order], view)
        for pos, i in enumerate(order):
            assert torch.equal(_bits(moved[pos]), _bits(got[i])), (view, i)                         # no dependence on the batch position
        alone = _flip(src[1:2].contiguous(), hw[1:2], view)
        assert torch.equal(_bits(alone[0]), _bits(got[1]))
    assert not torch.equal(_bits(_flip(src, hw, 'hflip')), _bits(_flip(src, hw, 'vflip')))


# ---------------------------------------------------------------------------------------------------------------- posterior gather
def test_posterior_gather_copies_the_candidate_rows_and_counts_the_missing():
    from aod_meh_hua_amd import scoring
    g = torch.Generator().manual_seed(5)
    B, n, W, max_num = 2, 2300, 21, 7                                      # (two candidate tiles of the lookup)
    boxes = (torch.rand(B, n, 4, generator=g) * 100).cuda()
    scores = torch.rand(B, n, W, generator=g).cuda()
    ks = [[2299, 0, 17, 2048, 2047], [5, 1111, 3]]
    ls = [[0, 19, 7, 3, 20], [4, 4, 0]]
    dets = torch.full((B, max_num, 5), float('nan'), device='cuda')
    labels = torch.full((B, max_num), 10 ** 12, dtype=torch.int64, device='cuda')
    for b in range(B):
        for j, (k, l) in enumerate(zip(ks[b], ls[b])):
            dets[b, j, :4], dets[b, j, 4], labels[b, j] = boxes[b, k], scores[b, k, l], l
    # a row >= num that IS a candidate's: still a zero row
    dets[1, 3, :4], dets[1, 3, 4], labels[1, 3] = boxes[1, 9], scores[1, 9, 2], 2
    num = torch.tensor([5, 3], dtype=torch.int32, device='cuda')
    cand = scoring.Candidates(boxes, scores, None, None, None, None, None)
    post, missing = scoring.det_posterior(cand, dets, labels, num)
    assert post.shape == (B, max_num, W) and post.dtype == torch.float32 and missing.dtype == torch.int32
    for b in range(B):
        for j, k in enumerate(ks[b]):
            assert torch.equal(_bits(post[b, j]), _bits(scores[b, k])), (b, j)
        assert bool((_bits(post[b, len(ks[b]):]) == 0).all())
    assert missing.tolist() == [0, 0]
    # one planted row without a candidate: a zero row, missing 1; the other rows as before
    dets2 = dets.clone()
    dets2[0, 2, 0] += 0.5
    post2, missing2 = scoring.det_posterior(cand, dets2, labels, num)
    assert missing2.tolist() == [1, 0] and bool((_bits(post2[0, 2]) == 0).all())
    keep = torch.ones(B, max_num, dtype=torch.bool, device='cuda')
    keep[0, 2] = False
    assert torch.equal(_bits(post2)[keep], _bits(post)[keep])
    # num = 0: nothing but zero rows
    post0, missing0 = scoring.det_posterior(cand, dets, labels, torch.zeros(2, dtype=torch.int32, device='cuda'))
    assert bool((_bits(post0) == 0).all()) and missing0.tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------- consistency kernel, exact
EXT = np.array([[160, 140], [150, 150], [128, 200]], np.float32)


def _mirror(box, code, ew, eh):
    """[n, 4] integer boxes mirrored in an (ew, eh) frame (exact in float32)"""
    b = np.array(box, np.float32, copy=True)
    if code & 1:
        b[:, 0], b[:, 2] = ew - box[:, 2], ew - box[:, 0]
    if code & 2:
        b[:, 1], b[:, 3] = eh - box[:, 3], eh - box[:, 1]
    return b


def _rows(g, n, W):
    """n posterior rows: Dirichlet draws of mixed concentration, some entries exactly 0"""
    conc = g.choice([0.05, 0.5, 5.0], (n, 1))
    p = g.gamma(np.broadcast_to(conc, (n, W)) + 1e-3)
    p = p / np.maximum(p.sum(1, keepdims=True), 1e-300)
    p[g.random((n, W)) < 0.1] = 0.0
    return p.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _exact_case(max_num, V, W, seed=0):
    """B = 3 stacks on integer coordinates.  Image 0: every clean row live (num = max_num), a score exactly at the threshold, scores on both
    sides of it, every view populated.  Image 1: view 0 is empty.  Image 2: every score <= the threshold (row 0 exactly at it): no object.
    View boxes are mirrored copies of clean boxes shifted by 2..4 px with a +-1 size change, a fifth of their labels changed; a third of
    their posterior rows equal the clean row's.  Rows >= num hold NaN boxes, garbage labels and NaN posteriors."""
    g = np.random.default_rng(1000 * max_num + 10 * V + W + seed)
    B = 3
    codes = [U.VIEWS[v] for v in VIEWS3[:V]]
    dets = np.full((V + 1, B, max_num, 5), np.nan, np.float32)
    labels = np.full((V + 1, B, max_num), 10 ** 12, np.int64)
    num = np.zeros((V + 1, B), np.int32)
    post = np.full((V + 1, B, max_num, W), np.nan, np.float32)
    num[0] = [max_num, max(1, max_num // 2), max(1, max_num // 3)]
    for b in range(B):
        n0 = int(num[0, b])
        seen, xy, wh = set(), np.zeros((n0, 2), np.int64), np.zeros((n0, 2), np.int64)
        for j in range(n0):                                               # distinct boxes: a box's only IoU-1 partner is its own copy
            while True:
                c = tuple(g.integers(0, 100, 2)) + tuple(g.integers(6, 25, 2))
                if c not in seen:
                    break
            seen.add(c)
            xy[j], wh[j] = c[:2], c[2:]
        dets[0, b, :n0, :2], dets[0, b, :n0, 2:4] = xy, xy + wh
        s = g.uniform(0.05, 1.0, n0).astype(np.float32)
        s[:1] = 0.9
        if b == 0 and n0 >= 2:
            s[1] = np.float32(THR)
        if b == 2:
            s = np.minimum(s, np.float32(THR) * g.uniform(0.2, 1.0, n0).astype(np.float32))
            s[0] = np.float32(THR)
        dets[0, b, :n0, 4] = s
        labels[0, b, :n0] = g.integers(0, 4, n0)
        post[0, b, :n0] = _rows(g, n0, W)
        for v in range(V):
            nv = 0 if (b == 1 and v == 0) else int(g.integers(max(1, max_num // 2), max_num + 1))
            num[v + 1, b] = nv
            src = g.integers(0, n0, nv)
            src[:min(nv, n0)] = g.permutation(n0)[:min(nv, n0)]
            base = dets[0, b, src, :4]
            shift = g.integers(2, 5, (nv, 1)) * g.choice([-1, 1], (nv, 1)) * np.array([[1, 0]]) + g.integers(-2, 3, (nv, 1)) * np.array([[0, 1]])
            grow = g.integers(-1, 2, (nv, 2))
            box = np.concatenate([base[:, :2] + shift, base[:, 2:] + shift + grow], 1).astype(np.float32)
            dets[v + 1, b, :nv, :4] = _mirror(box, codes[v], EXT[b, 0], EXT[b, 1])
            dets[v + 1, b, :nv, 4] = g.uniform(0.05, 1.0, nv)
            labels[v + 1, b, :nv] = labels[0, b, src]
            change = g.random(nv) < 0.2
            labels[v + 1, b, :nv][change] = (labels[v + 1, b, :nv][change] + 1) % 4
            rows = _rows(g, nv, W)
            same = g.random(nv) < 0.33
            rows[same] = post[0, b, src[same]]
            post[v + 1, b, :nv] = rows
    live = np.isfinite(dets[..., :4])
    assert np.array_equal(dets[..., :4][live], np.round(dets[..., :4][live]))
    return dets, labels, num, post


def _run(stack, views, ext, layout, **kw):
    from aod_meh_hua_amd import scoring
    return scoring.det_consistency(*(torch.from_numpy(x).cuda() for x in stack), views, torch.from_numpy(ext).cuda(), layout, **kw)


WORST = {}


@pytest.mark.parametrize('max_num', [1, 5, 100, 300, 1024])
@pytest.mark.parametrize('V', [1, 3])
def test_consistency_matches_float64_on_exact_boxes(max_num, V):
    views = VIEWS3[:V]
    worst = 0.0
    for layout, W in (('cat', 21), ('cat_bg', 21), ('sigmoid', 21), ('cat', 3)):
        stack = _exact_case(max_num, V, W)
        A = U.bound_obj(W, layout, V)
        for same_class in (False, True):
            pt = U.parts(*stack, views, EXT, layout, THR, same_class)
            assert pt['count'][0] >= 1 and pt['count'][2] == 0
            for mode in U.MODES:
                for aggregate in U.AGGREGATES:
                    want = U.combine(pt, mode, aggregate)
                    unc, obj, iou, js, match = _run(stack, views, EXT, layout, mode=mode, aggregate=aggregate, score_thr=THR,
                                                    same_class=same_class, want_objects=True, want_parts=True)
                    alone = _run(stack, views, EXT, layout, mode=mode, aggregate=aggregate, score_thr=THR, same_class=same_class)
                    assert unc.dtype == torch.float32 and unc.shape == (3,) and obj.shape == (3, max_num) and match.dtype == torch.int32
                    assert iou.shape == js.shape == match.shape == (V, 3, max_num)
                    assert np.array_equal(_np(match), want['match'])                              # equal, not close: the IoU operands are exact
                    for got, key in ((obj, 'obj'), (iou, 'iou'), (js, 'js')):
                        assert np.array_equal(np.isnan(_np(got)), np.isnan(want[key])), key       # NaN exactly on the rows that are no object
                    fr = dict(unc=U.fraction_of_bound(_np(unc), want['unc'], U.bound_unc(W, layout, V, aggregate, want['count'])),
                              obj=U.fraction_of_bound(_np(obj), want['obj'], A), iou=U.fraction_of_bound(_np(iou), want['iou'], A),
                              js=U.fraction_of_bound(_np(js), want['js'], A))
                    worst = max(worst, *fr.values())
                    assert all(f <= 1.0 for f in fr.values()), (layout, W, same_class, mode, aggregate, fr)
                    assert torch.equal(_bits(alone), _bits(unc))                                  # the nullable outputs change nothing
                    assert _np(unc)[2] == 0.0
            if max_num >= 2:
                assert np.isnan(want['obj'][0, 1])                                                # the score exactly at the threshold
            assert (want['match'][0, 1][np.isfinite(want['iou'][0, 1])] == -1).all()              # image 1: view 0 is empty
        print(f'max_num {max_num} V {V} {layout} W {W}: objects {pt["count"].tolist()}, largest fraction of the bound so far {worst:.3f}')
    WORST[(max_num, V)] = worst
    print(f'largest observed fraction of the bound at max_num {max_num}, V {V}: {worst:.3f}')


@pytest.mark.parametrize('max_num, V', [(1, 1), (5, 3), (300, 3), (1024, 1)])
def test_mirror_slots_score_exactly_zero(max_num, V):
    views = VIEWS3[:V]
    for layout, W in (('cat', 21), ('sigmoid', 21), ('cat_bg', 21)):
        dets, labels, num, post = (x.copy() for x in _exact_case(max_num, V, W))
        for v, name in enumerate(views):
            dets[v + 1], labels[v + 1], num[v + 1], post[v + 1] = dets[0], labels[0], num[0], post[0]
            for b in range(3):
                n0 = int(num[0, b])
                dets[v + 1, b, :n0, :4] = _mirror(dets[0, b, :n0, :4], U.VIEWS[name], EXT[b, 0], EXT[b, 1])
        for same_class in (False, True):
            for mode in U.MODES:
                unc, obj, iou, js, match = _run((dets, labels, num, post), views, EXT, layout, mode=mode, score_thr=THR, same_class=same_class,
                                                want_objects=True, want_parts=True)
                live = np.isfinite(_np(obj))
                assert live.sum() >= 2 - (max_num == 1) and _np(unc).tolist() == [0.0, 0.0, 0.0] and (_np(obj)[live] == 0.0).all()
                for v in range(V):
                    assert (_np(iou)[v][live] == 1.0).all() and (_np(js)[v][live] == 0.0).all()
                    assert np.array_equal(_np(match)[v][live], np.broadcast_to(np.arange(max_num), live.shape)[live])
                    assert (_np(match)[v][~live] == -1).all()


def test_the_smallest_denormal_against_zero_stays_finite():
    """m = (2^-149 + 0) / 2 rounds to 0 in fp32: the term (2^-149 ln 2 in float64) is taken as 0, not as 2^-149 (ln a + inf)"""
    tiny = np.float32(2.0 ** -149)
    dets = np.zeros((2, 1, 1, 5), np.float32)
    dets[0, 0, 0], dets[1, 0, 0] = [10, 10, 30, 30, .9], [34, 10, 54, 30, .9]            # the hflip of the same box in a 64-wide frame
    labels, num = np.zeros((2, 1, 1), np.int64), np.ones((2, 1), np.int32)
    post = np.array([[[[.5, tiny, 0, tiny, .25]]], [[[.5, 0, tiny, tiny, .5]]]], np.float32)
    ext = np.array([[64, 48]], np.float32)
    for layout in U.LAYOUTS:
        want = U.reference(dets, labels, num, post, ('hflip',), ext, layout, 'cls')
        unc, iou, js, match = _run((dets, labels, num, post), ('hflip',), ext, layout, mode='cls', want_parts=True)
        assert _np(match).ravel().tolist() == [0] and _np(iou).ravel().tolist() == [1.0] and np.isfinite(_np(js)).all()
        assert U.fraction_of_bound(_np(js), want['js'], U.bound_obj(5, layout, 1)) <= 1.0
        assert U.fraction_of_bound(_np(unc), want['unc'], U.bound_unc(5, layout, 1, 'max', want['count'])) <= 1.0


def test_an_image_has_the_same_bits_alone_and_anywhere_in_a_batch():
    for max_num, V in ((5, 3), (100, 3), (1024, 1)):
        stack = _exact_case(max_num, V, 21)
        views = VIEWS3[:V]
        for layout, aggregate in (('cat', 'max'), ('sigmoid', 'mean'), ('cat_bg', 'sum')):
            ref = _run(stack, views, EXT, layout, aggregate=aggregate, score_thr=THR, want_objects=True, want_parts=True)
            for order in ORDERS:
                got = _run(tuple(np.ascontiguousarray(x[:, order]) for x in stack), views, np.ascontiguousarray(EXT[order]), layout,
                           aggregate=aggregate, score_thr=THR, want_objects=True, want_parts=True)
                for row, i in enumerate(order):
                    assert torch.equal(_bits(got[0][row]), _bits(ref[0][i])) and torch.equal(_bits(got[1][row]), _bits(ref[1][i])), (max_num, order)
                    for a, r in zip(got[2:], ref[2:]):
                        assert torch.equal(_bits(a[:, row]), _bits(r[:, i])), (max_num, order)


# ---------------------------------------------------------------------------------------------------------------- the pool pass
def _loader(ds, bs):
    from aod_meh_hua_amd.datasets import build_dataloader
    return build_dataloader(ds, samples_per_gpu=bs, workers_per_gpu=0, dist=False, shuffle=False)


def _dataset(size):
    from aod_meh_hua_amd.datasets import SyntheticVOCDataset

    class Resized(SyntheticVOCDataset):
        """the synthetic images, every second one with the metas a keep-ratio resize and the collate's pad leave: a window smaller than
        the tensor and a scale factor, so that the mirrored window and the rescaled frame differ from the tensor's"""

        def __getitem__(self, i):
            d = super().__getitem__(i)
            if i % 2:
                H, W = self.size
                d['img_metas'].update(img_shape=(H - 8, W - 12, 3), scale_factor=np.array([0.8, 0.75, 0.8, 0.75], np.float32))
            return d
    return Resized(num_images=6, size=size, test_mode=True)


def _batches(ds, bs):
    from aod_meh_hua_amd.apis.test import _unwrap
    for data in _loader(ds, bs):
        data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
        yield data['img'][0].cuda(), data['img_metas'][0]


def _detect(model, img, metas, **kw):
    with torch.no_grad():
        out = model(return_loss=False, rescale=True, isEval=True, _padded=True, isUnc=False, img=[img], img_metas=[metas], **kw)
    return tuple(t.clone() for t in out)


@functools.lru_cache(maxsize=None)
def _build(kind):
    """the small synthetic detectors of the posterior / localization-stability GPU tests, their classification heads calibrated so that
    detections pass the default 0.3 gate, their regressors scaled so that boxes keep an area"""
    from aod_meh_hua_amd.mmcv_lite import Config, MMDataParallel
    from aod_meh_hua_amd.models import build_detector
    from oracle import model as om
    from oracle import model_ssd as ossd
    from tests import plain_retina_util as PU
    config, sd, size = {'SSL_L_RetinaNet': ('configs/_base_/Config_RetinaNet.py', lambda: om.seeded_state_dict(cls_bias=-2.0), (128, 128)),
                        'MyRetinaNet': ('configs/_base_/Config_RetinaNet_plain.py', lambda: PU.plain_state_dict(cls_bias=-0.5), (128, 128)),
                        'SSD_L_SingleStageDetector': ('configs/_base_/Config_SSD.py', lambda: ossd.seeded_state_dict(), (300, 300))}[kind]
    cfg = Config.fromfile(os.path.join(ROOT, config))
    cfg.model.backbone.pop('init_cfg', None)
    model = build_detector(cfg.model)
    assert type(model).__name__ == kind
    model.load_state_dict(sd(), strict=True)
    model = model.cuda().eval()
    ds = _dataset(size)
    cal = torch.cat([img for img, _ in _batches(ds, 3)])[:4]
    if kind == 'SSL_L_RetinaNet':
        import bench
        bench.calibrate_head(model, cal)
    if kind != 'SSD_L_SingleStageDetector':
        # a trained-like regressor: the seeded one throws most boxes out of the image, where clipping leaves them no area, and a box without
        # area has IoU 0 with everything (the union is clamped).  Scale the last conv until no delta of the calibration batch exceeds 0.2
        with torch.no_grad():
            reg = model.bbox_head.forward(model.extract_feat(cal))[1]
            top = max(float(r.abs().max()) for r in reg)
            model.bbox_head.retina_reg.weight.mul_(0.2 / top), model.bbox_head.retina_reg.bias.mul_(0.2 / top)
    else:
        metas = next(_batches(ds, 3))[1]
        for _ in range(12):
            dets, _, num = _detect(model, cal[:3], metas)
            if int((dets[..., 4] > THR).sum()) >= 6:
                break
            with torch.no_grad():
                for c in model.bbox_head.cls_convs:
                    c[0].weight.mul_(2.0), c[0].bias.mul_(2.0)
    return cfg, MMDataParallel(model).eval(), ds


def _extent(metas):
    """(w / scale_x, h / scale_y) per image in Python floats, cast to fp32: the frame of the rescaled detections"""
    out = []
    for m in metas:
        sf = np.asarray(m['scale_factor'], np.float64).reshape(-1)
        out.append((float(m['img_shape'][1]) / float(sf[0]), float(m['img_shape'][0]) / float(sf[1])))
    return torch.tensor(out, dtype=torch.float32).cuda()


def _chain(model, ds, views, layout, **kw):
    """the pool pass restated eagerly: hipops.flip_images -> model(..., detPost=True) -> scoring.det_consistency, batches of 3; returns the
    scores, the stacked outputs of every batch with their extents, and det_consistency's parts"""
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd import scoring
    scores, stacks, pieces = [], [], []
    for img, metas in _batches(ds, 3):
        hw = torch.tensor([m['img_shape'][:2] for m in metas], dtype=torch.int32, device='cuda')
        slots = [_detect(model, img, metas, detPost=True)]
        for view in views:
            slots.append(_detect(model, ho.flip_images(img, torch.empty_like(img), hw, view), metas, detPost=True))
        stack = tuple(torch.stack([sl[i] for sl in slots]) for i in range(5))
        ext = _extent(metas)
        out = scoring.det_consistency(*stack[:4], views, ext, layout, score_thr=THR, want_objects=True, want_parts=True, **kw)
        scores.append(out[0]), stacks.append((stack, ext)), pieces.append(out[1:])
    return torch.cat(scores).cpu(), stacks, pieces


@pytest.mark.parametrize('kind', ['SSL_L_RetinaNet', 'MyRetinaNet', 'SSD_L_SingleStageDetector'])
def test_pool_pass_eager_replayed_and_batch_sizes(kind, monkeypatch):
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis import test as apis_test
    from aod_meh_hua_amd.scoring import ACTIVATION_LAYOUT
    cfg, model, ds = _build(kind)
    layout = ACTIVATION_LAYOUT[getattr(model, 'module', model).bbox_head.last_activation]
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    stats = {}
    eager = apis.single_gpu_consistency(model, _loader(ds, 3), _stats=stats).cpu()
    assert eager.shape == (6,) and eager.dtype == torch.float32 and bool(torch.isfinite(eager).all()) and bool((eager >= 0).all())
    assert stats['missing'].tolist() == [0.0] * 6
    assert torch.equal(_bits(apis.Consistency_uncertainty(cfg, model, _loader(ds, 3))), _bits(eager))
    for bs in (2, 1):
        assert torch.equal(_bits(apis.Consistency_uncertainty(cfg, model, _loader(ds, bs))), _bits(eager)), bs
    # the chain this test runs itself: the same bits
    chain, stacks, pieces = _chain(model, ds, ('hflip',), layout)
    assert torch.equal(_bits(chain), _bits(eager))
    counts = [int(np.isfinite(_np(p[0][b])).sum()) for p in pieces for b in range(3)]
    W, max_num = int(stacks[0][0][3].shape[-1]), int(stacks[0][0][0].shape[2])
    best = max(float(np.nanmax(np.where(np.isfinite(_np(p[1])), _np(p[1]), -1.0))) for p in pieces)
    print(f'{kind}: layout {layout}, W {W}, max_num {max_num}, objects per image {counts}, scores {eager.tolist()}, best matched IoU {best:.3f}')
    assert sum(1 for n in counts if n > 0) >= 1, counts                            # not vacuous: the calibrated head finds objects,
    assert bool((eager > 0).any())                                                 # ... an image scores,
    assert best > 0 and any(int((_np(p[3]) >= 0).sum()) > 0 for p in pieces)       # ... an object is matched with iou > 0,
    assert all(int(st[0][4].sum()) == 0 for st in stacks)                          # ... and every detection has its posterior row
    # box and cls against the restatement fed the device's own stacked outputs (its match is decided in float32, like the kernel's)
    # (... and their mean under `mean`: the seeded SSD keeps some detection without a partner in every image, so its `max` is exactly 1)
    for mode, aggregate in (('box', 'max'), ('cls', 'max'), ('both', 'mean')):
        got = apis.Consistency_uncertainty(cfg, model, _loader(ds, 3), mode=mode, aggregate=aggregate)
        assert torch.equal(_bits(_chain(model, ds, ('hflip',), layout, mode=mode, aggregate=aggregate)[0]), _bits(got))
        want = [U.reference(*(_np(t) for t in stack[:4]), ('hflip',), _np(ext), layout, mode, aggregate, THR) for stack, ext in stacks]
        frac = U.fraction_of_bound(got.numpy(), np.concatenate([w['unc'] for w in want]),
                                   np.concatenate([U.bound_unc(W, layout, 1, aggregate, w['count']) for w in want]))
        print(f'{kind} mode {mode} {aggregate}: scores {got.tolist()}, fraction of the bound {frac:.3f}')
        assert frac <= 1.0
        assert aggregate != 'mean' or bool(((got > 0) & (got < 1)).any())
    two = apis.Consistency_uncertainty(cfg, model, _loader(ds, 3), views=('hflip', 'vflip'))
    assert not torch.equal(two, eager)
    assert torch.equal(_bits(_chain(model, ds, ('hflip', 'vflip'), layout)[0]), _bits(two))
    # replayed: the V + 1 forwards of a batch are replays of one captured graph under its own key; the same bits
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    for bs in (3, 2, 1):
        assert torch.equal(_bits(apis.Consistency_uncertainty(cfg, model, _loader(ds, bs))), _bits(eager)), bs
    assert torch.equal(_bits(apis.Consistency_uncertainty(cfg, model, _loader(ds, 3), views=('hflip', 'vflip'))), _bits(two))
    keys = list(apis_test._GSCORE.get(model, {}))
    assert len(keys) == 1 and keys[0][0] == 'eval_post'
    gs = apis_test._GSCORE[model][keys[0]]
    assert len(gs.cache) == 3
    # a shape seen for the first time runs eagerly: batches of 4 and 2 -- the 4 is new and is not captured, the 2 replays; the same bits
    assert torch.equal(_bits(apis.Consistency_uncertainty(cfg, model, _loader(ds, 4))), _bits(eager))
    assert len(gs.cache) == 3 and all(k[0][0] in (1, 2, 3) for k in gs.cache)


def test_calculate_uncertainty_hands_the_scores_to_update_X_L():
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.utils.active_datasets import update_X_L
    cfg, model, ds = _build('MyRetinaNet')
    cfg.uncertainty_pool = 'Consistency'
    hua = dict(return_box=False, showNMS=False, saveUnc=False, saveMaxConf=False, clsW=False, scaleUnc=False, score_thr=0.3, iou_thr=0.9)
    unc = apis.calculate_uncertainty(cfg, model, _loader(ds, 3), **hua)
    assert torch.is_tensor(unc) and unc.shape == (6,) and unc.dtype == torch.float32 and not unc.is_cuda and bool((unc >= 0).all())
    assert torch.equal(_bits(unc), _bits(apis.Consistency_uncertainty(cfg, model, _loader(ds, 3))))
    mean = apis.calculate_uncertainty(cfg, model, _loader(ds, 3), unc_aggregate='mean', mode='box', views=('vflip',), **hua)
    assert torch.equal(_bits(mean), _bits(apis.Consistency_uncertainty(cfg, model, _loader(ds, 3), aggregate='mean', mode='box', views=('vflip',))))
    assert not torch.equal(mean, unc)
    np.random.seed(20)
    X_L = np.array([0, 3])
    X_L_next, X_U_next = update_X_L(unc.numpy(), np.arange(6), X_L, 2, zeroRate=0.15)
    order = np.argsort(unc.numpy()[[1, 2, 4, 5]])
    assert X_L_next.tolist() == sorted([0, 3] + np.array([1, 2, 4, 5])[order[-2:]].tolist())


@pytest.mark.parametrize('kind', ['SSL_L_RetinaNet', 'MyRetinaNet', 'SSD_L_SingleStageDetector'])
def test_det_post_leaves_the_padded_triple_alone(kind):
    cfg, model, ds = _build(kind)
    img, metas = next(_batches(ds, 3))
    plain = _detect(model, img, metas)
    with_post = _detect(model, img, metas, detPost=True)
    assert len(plain) == 3 and len(with_post) == 5
    for a, b in zip(plain, with_post):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    dets, labels, num, post, missing = with_post
    assert post.shape[:2] == dets.shape[:2] and post.dtype == torch.float32 and missing.tolist() == [0, 0, 0]
    for b in range(3):
        n = int(num[b])
        assert bool((post[b, n:] == 0).all())
        # the detection's score is the posterior row's entry at its label
        assert torch.equal(post[b, :n].gather(1, labels[b, :n, None])[:, 0], dets[b, :n, 4])
    with pytest.raises(ValueError):
        _detect(model, img, metas, detPost=True, detUnc=True)
    if kind != 'SSD_L_SingleStageDetector':                                  # (SSD refuses objDesc itself)
        with pytest.raises(ValueError, match='detPost'):
            _detect(model, img, metas, detPost=True, objDesc=8)
