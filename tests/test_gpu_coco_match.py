"""GPU: aod_coco_match (csrc/cocomatch.hip) against the host's coco_eval.match_image called per image and class: the uint8 states are
equal, for every area range and IoU threshold of one launch, on shapes up to the kernel's documented limits, on the quantised draw with
score ties and exact-threshold IoUs, and at the edges (no detections, no gts, crowds only, 80 mostly empty classes)."""
import ctypes as C

import numpy as np
import pytest
import torch

from aod_meh_hua_amd.core import coco_eval as CE
from aod_meh_hua_amd.core.coco_eval_device import coco_match, pack_eval_infos
from tests.coco_util import naive_states, padded_batch, quantised_draw, tie_case

pytestmark = pytest.mark.gpu
THRS = CE.default_iou_thrs()


def host_states(dets, labels, num, infos, thrs=THRS, ranges=CE.AREA_RANGES):
    B, M = labels.shape
    out = np.zeros((len(ranges), len(thrs), B, M), np.uint8)
    for b in range(B):
        lab = labels[b, :num[b]]
        for c in np.unique(lab):
            rows = np.flatnonzero(lab == c)
            sel = infos[b]['labels'] == c
            box, area, _, order = CE.rank_detections(dets[b, rows], M)
            out[:, :, b, rows[order]] = CE.match_image(box, area, infos[b]['boxes'][sel], infos[b]['area'][sel], infos[b]['iscrowd'][sel],
                                                       thrs, ranges)
    return out


def device_states(dets, labels, num, infos, thrs=THRS, ranges=CE.AREA_RANGES):
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    gb, ga, gl, gc, gn = pack_eval_infos(infos)
    # poison the padding: rows >= num[b] and gts >= gt_num[b] must never be read
    dets, labels = dets.copy(), labels.copy()
    for b in range(len(num)):
        dets[b, num[b]:] = [0, 0, 1e4, 1e4, 2.0]
        labels[b, num[b]:] = infos[b]['labels'][0] if len(infos[b]['labels']) else 0
        gb[b, gn[b]:], gl[b, gn[b]:], ga[b, gn[b]:] = [0, 0, 1e4, 1e4], 0, 500.0
    st = coco_match(cu(dets), cu(labels), cu(num), cu(gb), cu(ga), cu(gl), cu(gc), cu(gn), thrs, ranges)
    torch.cuda.synchronize()
    return st.cpu().numpy()


def random_case(B, M, G, num_classes, seed, size=512):
    """quarter-pixel boxes; image 0 holds M detections and G gts, the others random counts; detections are copies / halves / shifts of gts
    or free boxes, scores in 1/64 steps"""
    rng = np.random.RandomState(seed)
    infos = []
    dets, labels, num = np.zeros((B, M, 5), np.float32), np.zeros((B, M), np.int64), np.zeros((B,), np.int32)
    for b in range(B):
        g = G if b == 0 else int(rng.randint(0, G + 1))
        wh = rng.choice([8, 16, 24, 32, 48, 64, 96, 128], size=(g, 2)).astype(np.float64)
        xy = np.floor(rng.rand(g, 2) * (size - wh) * 4) / 4
        gl = rng.randint(0, num_classes, g).astype(np.int64)
        infos.append(dict(boxes=np.concatenate([xy, wh], 1).reshape(-1, 4), area=wh[:, 0] * wh[:, 1] * rng.choice([1.0, 0.5], size=g),
                          iscrowd=(rng.rand(g) < 0.1).astype(np.uint8), labels=gl))
        n = M if b == 0 else int(rng.randint(0, M + 1))
        for m in range(n):
            if g and rng.rand() < 0.7:
                k = int(rng.randint(g))
                x, y, w, h = xy[k, 0], xy[k, 1], wh[k, 0] * rng.choice([1.0, 0.5, 0.75]), wh[k, 1]
                x += wh[k, 0] * rng.choice([0.0, 0.0, 0.25])
                c = gl[k]
            else:
                w, h = rng.choice([8, 16, 32, 64, 128], size=2).astype(np.float64)
                x, y = np.floor(rng.rand(2) * (size - np.array([w, h])) * 4) / 4
                c = rng.randint(num_classes)
            dets[b, m], labels[b, m] = [x, y, x + w, y + h, rng.randint(1, 65) / 64.0], c
        num[b] = n
    if B > 1 and M >= 2 and G >= 2:
        # image 1 starts with tie_case, far from everything else and with scores above every other: equal IoUs decide its states
        rows, gts, area = tie_case(1000.0, 1000.0, scores=(1.5, 1.25))
        i = infos[1]
        keep = slice(0, G - 2)
        infos[1] = dict(boxes=np.concatenate([gts, i['boxes'][keep]]), area=np.concatenate([area, i['area'][keep]]),
                        iscrowd=np.concatenate([np.zeros(2, np.uint8), i['iscrowd'][keep]]),
                        labels=np.concatenate([np.zeros(2, np.int64), i['labels'][keep]]))
        dets[1, :2], labels[1, :2], num[1] = rows, 0, max(num[1], 2)
    return dets, labels, num, infos


def rule_sensitive(dets, labels, num, infos, b, c, states, thrs=THRS):
    """number of states of (image b, class c) that taking the EARLIER of two equal IoUs would change"""
    rows = np.flatnonzero(labels[b, :num[b]] == c)
    sel = infos[b]['labels'] == c
    wrong, order = naive_states(dets[b, rows], infos[b]['boxes'][sel], infos[b]['area'][sel], infos[b]['iscrowd'][sel], thrs, tie='earlier')
    return int((np.asarray(wrong, np.uint8) != states[:, :, b, rows[order]]).sum())


@pytest.mark.parametrize('M', [1, 100, 256])
@pytest.mark.parametrize('G', [0, 1, 70, 512])
def test_states_equal_match_image(M, G):
    dets, labels, num, infos = random_case(5, M, G, 4 if G < 512 else 12, seed=100 * M + G)
    want = host_states(dets, labels, num, infos)
    got = device_states(dets, labels, num, infos)
    assert got.shape == (4, 10, 5, M) and torch.equal(torch.from_numpy(got), torch.from_numpy(want))
    if G >= 70 and M >= 100:
        assert all((want == v).any() for v in (0, 1, 2))          # every state occurs
    if G >= 2 and M >= 2:                                         # the replacement rule shows in image 1's states, in both sweeps
        assert want[0, 0, 1, :2].tolist() == [1, 1] and want[2, 0, 1, :2].tolist() == [2, 2]
        assert rule_sensitive(dets, labels, num, infos, 1, 0, got) >= 3


def test_quantised_draw_in_batches_of_eight():
    results, infos = quantised_draw()
    assert len(results) == 204                                   # 200 random images + coco_util.tie_images
    rng = np.random.RandomState(11)
    seen = np.zeros(3, np.int64)
    rule = 0
    for s in range(0, 204, 8):
        d, l, n = padded_batch(results[s:s + 8], 16, rng)
        want = host_states(d, l, n, infos[s:s + 8])
        got = device_states(d, l, n, infos[s:s + 8])
        assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)), s
        for b in range(len(n)):
            seen += np.bincount(want[:, :, b, :n[b]].reshape(-1), minlength=3)
            rule += sum(rule_sensitive(d, l, n, infos[s:s + 8], b, c, got) for c in np.unique(l[b, :n[b]]))
    assert (seen > 1000).all() and rule >= 8                     # the draw tells `later gt on equal IoUs` from `earlier gt`


def test_one_threshold_one_range():
    dets, labels, num, infos = random_case(5, 100, 70, 4, seed=5)
    for thrs, ranges in (([0.5], ((0.0, 1e10),)), ([0.75], (CE.AREA_RANGES[2],)), (list(np.linspace(.05, .8, 16)), CE.AREA_RANGES[:3])):
        want = host_states(dets, labels, num, infos, thrs, ranges)
        got = device_states(dets, labels, num, infos, thrs, ranges)
        assert got.shape == (len(ranges), len(thrs), 5, 100) and torch.equal(torch.from_numpy(got), torch.from_numpy(want))


def test_edges_empty_images_crowds_only_and_eighty_classes():
    dets, labels, num, infos = random_case(6, 100, 70, 80, seed=9)
    num[1] = 0                                                   # no detections
    infos[2] = {k: v[:0] for k, v in infos[2].items()}            # no gts
    infos[3] = dict(infos[3], iscrowd=np.ones_like(infos[3]['iscrowd']))          # crowds only
    num[4], infos[4] = 0, {k: v[:0] for k, v in infos[4].items()}                 # neither
    want = host_states(dets, labels, num, infos)
    got = device_states(dets, labels, num, infos)
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(want))
    assert not got[:, :, 1].any() and not got[:, :, 4].any() and not (got[:, :, 3, :num[3]] == 1).any()
    assert (got[0, :, 2, :num[2]] == 0).all()                    # range `all`, no gts: every detection is a counted false positive
    # a batch without any gt at all: G is padded to one row that is never read
    none = [{k: v[:0] for k, v in i.items()} for i in infos]
    assert torch.equal(torch.from_numpy(device_states(dets, labels, num, none)), torch.from_numpy(host_states(dets, labels, num, none)))


def test_an_image_has_the_same_states_alone_and_at_any_batch_position():
    dets, labels, num, infos = random_case(8, 100, 70, 4, seed=21)
    whole = device_states(dets, labels, num, infos)
    for b in (0, 3, 7):
        alone = device_states(dets[b:b + 1], labels[b:b + 1], num[b:b + 1], infos[b:b + 1])
        assert np.array_equal(alone[:, :, 0], whole[:, :, b])
    perm = [5, 0, 7, 2, 1, 6, 3, 4]
    moved = device_states(dets[perm], labels[perm], num[perm], [infos[i] for i in perm])
    assert np.array_equal(moved, whole[:, :, perm])


def test_nan_scores_leave_no_uninitialised_state():
    # a NaN score has no rank: the rows the kernel then never visits read 0, not whatever the allocator left (states start zeroed)
    dets, labels, num, infos = random_case(2, 100, 70, 4, seed=33)
    dets[0, :num[0]:3, 4] = np.nan
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    gb, ga, gl, gc, gn = pack_eval_infos(infos)
    junk = torch.full((4, 10, 2, 100), 77, dtype=torch.uint8, device='cuda')       # (recycled by the allocator for the next same-size request)
    del junk
    st = coco_match(cu(dets), cu(labels), cu(num), cu(gb), cu(ga), cu(gl), cu(gc), cu(gn), THRS).cpu().numpy()
    assert st.max() <= 2
    want = host_states(dets[1:], labels[1:], num[1:], infos[1:])
    assert np.array_equal(st[:, :, 1:], want)                    # the image without NaN is untouched by its neighbour


def test_entry_refusals():
    from aod_meh_hua_amd import _C
    f = _C.lib.aod_coco_match
    d = torch.zeros(1, 4, 5, device='cuda')
    lab, n = torch.zeros(1, 4, dtype=torch.int64, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    gb, ga = torch.zeros(1, 1, 4, dtype=torch.float64, device='cuda'), torch.zeros(1, 1, dtype=torch.float64, device='cuda')
    gl, gc = torch.zeros(1, 1, dtype=torch.int32, device='cuda'), torch.zeros(1, 1, dtype=torch.uint8, device='cuda')
    out = torch.zeros(4, 16, 1, 4, dtype=torch.uint8, device='cuda')
    rng, thr = (C.c_double * 10)(*([0.0, 1e10] * 5)), (C.c_double * 17)(*([0.5] * 17))
    p = _C.ptr

    def call(dets=d, gt_boxes=gb, M=4, G=1, A=4, T=10, ranges=rng, thrs=thr, states=out):
        return f(p(dets), p(lab), p(n), p(gt_boxes), p(ga), p(gl), p(gc), p(n), 1, M, G, ranges, A, thrs, T, p(states), _C.stream())

    assert call() == 0
    for kw, word in ((dict(T=17), '16 IoU thresholds'), (dict(T=0), '16 IoU thresholds'), (dict(A=5), '4 area ranges'), (dict(A=0), '4 area ranges'),
                     (dict(M=1025), 'at most 1024 detection rows'), (dict(G=513), 'at most 512 gts'), (dict(M=-1), 'bad shape'),
                     (dict(dets=None), 'null pointer'), (dict(states=None), 'null pointer'), (dict(gt_boxes=None), 'null gt pointer'),
                     (dict(thrs=None), 'IoU thresholds'), (dict(ranges=None), 'area ranges')):
        assert call(**kw) == -1, kw
        assert word in _C.lib.aod_last_error().decode(), (kw, _C.lib.aod_last_error().decode())
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match='IoU thresholds'):
        coco_match(d, lab, n, gb, ga, gl, gc, n, [0.5] * 17)
    # the wrapper names the shape itself, with the limits the entry has
    from aod_meh_hua_amd.core import coco_eval_device as CD
    assert (CD.MAX_THRESHOLDS, CD.MAX_RANGES, CD.MAX_DETS, CD.MAX_GTS) == (16, 4, 1024, 512)
    big = torch.zeros(1, CD.MAX_DETS + 1, 5, device='cuda')
    with pytest.raises(ValueError, match='1024 detection rows'):
        coco_match(big, torch.zeros(1, CD.MAX_DETS + 1, dtype=torch.int64, device='cuda'), n, gb, ga, gl, gc, n, [0.5])
    with pytest.raises(ValueError, match='512 gts'):
        coco_match(d, lab, n, torch.zeros(1, 513, 4, dtype=torch.float64, device='cuda'), torch.zeros(1, 513, dtype=torch.float64, device='cuda'),
                   torch.zeros(1, 513, dtype=torch.int32, device='cuda'), torch.zeros(1, 513, dtype=torch.uint8, device='cuda'), n, [0.5])
    with pytest.raises(_C.AodHipError, match='no CPU fallback'):
        coco_match(d.cpu(), lab.cpu(), n.cpu(), gb.cpu(), ga.cpu(), gl.cpu(), gc.cpu(), n.cpu(), [0.5])
