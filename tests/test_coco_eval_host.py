"""CPU tests of the COCO bbox evaluator (core/coco_eval.py): known answers of the matching protocol, the evaluator against the
naive flat-loop restatement of tests/coco_util.py on a seeded draw with score ties and exact-threshold IoUs, and DeviceCocoAccumulator on
'cpu' (store / merge / finalize) against evaluate_bbox."""
import numpy as np
import pytest
import torch

from aod_meh_hua_amd.core import coco_eval as CE
from tests.coco_util import naive_states, naive_summary, padded_batch, quantised_draw, tie_case

THRS = CE.default_iou_thrs()


def info(boxes, labels=None, crowd=None, area=None):
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    G = len(boxes)
    return dict(boxes=boxes, labels=np.zeros(G, np.int64) if labels is None else np.asarray(labels, np.int64),
                iscrowd=np.zeros(G, np.uint8) if crowd is None else np.asarray(crowd, np.uint8),
                area=boxes[:, 2] * boxes[:, 3] if area is None else np.asarray(area, np.float64))


def dets(rows):
    return np.asarray(rows, np.float32).reshape(-1, 5)


def states_of(rows, gi, thrs=THRS):
    box, area, _, _ = CE.rank_detections(dets(rows), 1000)
    return CE.match_image(box, area, gi['boxes'], gi['area'], gi['iscrowd'], thrs)


def test_perfect_detections_score_one_and_empty_ranges_minus_one():
    # 40 x 40 gts: medium only
    infos = [info([[10, 10, 40, 40], [60, 60, 40, 40]], labels=[0, 1]), info([[5, 5, 40, 40]], labels=[1])]
    results = [[dets([[10, 10, 50, 50, .9]]), dets([[60, 60, 100, 100, .8]])], [dets([]), dets([[5, 5, 45, 45, .7]])]]
    out = CE.evaluate_bbox(results, infos, ('a', 'b'), logger='silent')
    assert out['bbox_mAP'] == 1.0 and out['bbox_mAP_50'] == 1.0 and out['bbox_mAP_75'] == 1.0 and out['bbox_mAP_m'] == 1.0
    assert out['bbox_mAP_s'] == -1.0 and out['bbox_mAP_l'] == -1.0
    assert out['bbox_mAP_copypaste'] == '1.000 1.000 1.000 -1.000 1.000 -1.000'
    assert list(out) == ['bbox_mAP', 'bbox_mAP_50', 'bbox_mAP_75', 'bbox_mAP_s', 'bbox_mAP_m', 'bbox_mAP_l', 'bbox_mAP_copypaste']


def test_analytic_tp_fp_tp():
    gi = info([[0, 0, 40, 40], [100, 100, 40, 40]])
    res = [[dets([[0, 0, 40, 40, .9], [200, 200, 240, 240, .8], [100, 100, 140, 140, .7]])]]
    assert states_of(res[0][0], gi)[0].tolist() == [[1, 0, 1]] * 10
    prec = CE.accumulate(np.array([.9, .8, .7]), np.zeros(3, np.int64), states_of(res[0][0], gi), CE.count_npig([gi], 1), 1)
    want = (51 + 50 * 2 / (3 + np.spacing(1))) / 101
    # recall 0 .. 0.5 reads precision 1 (51 points), above it 2 / 3 (50 points)
    for t in range(10):
        assert np.mean(prec[t, :, 0, 0]) == pytest.approx(want, rel=1e-12)
    assert prec[0, :51, 0, 0].tolist() == [1 / (1 + np.spacing(1))] * 51 and prec[0, 51:, 0, 0].tolist() == [2 / (3 + np.spacing(1))] * 50
    assert CE.summarize(prec, THRS)['mAP'] == pytest.approx(want, rel=1e-12)


def test_crowd_absorbs_detections_as_ignored_and_is_never_tp():
    gi = info([[0, 0, 64, 64]], crowd=[1])
    rows = [[0, 0, 64, 64, .9], [8, 8, 40, 40, .8], [16, 16, 48, 48, .7], [300, 300, 364, 364, .6]]
    st = states_of(rows, gi)
    assert st[0].tolist() == [[2, 2, 2, 0]] * 10               # union = the detection's own area: inside boxes have IoU 1
    assert CE.count_npig([gi], 1).tolist() == [[0, 0, 0, 0]]
    assert CE.evaluate_bbox([[dets(rows)]], [gi], ('a',), logger='silent')['bbox_mAP'] == -1.0


def test_counted_gt_wins_over_ignored_gt_even_at_lower_iou():
    # the crowd coincides with the detection (IoU 1), the plain gt overlaps it with IoU 0.6
    gi = info([[0, 0, 40, 40], [10, 0, 40, 40]], crowd=[1, 0])
    st = states_of([[0, 0, 40, 40, .9], [0, 0, 40, 40, .8]], gi, [0.5])
    assert st[0, 0].tolist() == [1, 2]                          # first takes the plain gt; the second finds it taken and falls to the crowd


def test_equal_ious_go_to_the_later_gt():
    # detection A overlaps both gts with the same IoU 28 / 52; B coincides with gt 0 (tests/coco_util.tie_case).  A must take gt 1.
    rows, gts, area = tie_case()
    gi = info(gts, area=area)                                   # area 100: counted by all / small, ignored by medium
    box, darea, _, _ = CE.rank_detections(rows, 1000)
    iou = CE.iou_matrix(box, darea, gts, gi['iscrowd'])
    assert iou[0, 0] == iou[0, 1] == 896 / 1664 and iou[1].tolist() == [1.0, 0.25]
    st = states_of(rows, gi, [0.5])
    assert st[:, 0, :].tolist() == [[1, 1], [1, 1], [2, 2], [2, 2]]
    # first sweep (range all): the earlier gt would leave B without a partner; second sweep (medium, both gts ignored by their area): too
    wrong, _ = naive_states(rows, gts, area, gi['iscrowd'], [0.5], tie='earlier')
    assert [w[0] for w in wrong] == [[1, 0], [1, 2], [2, 0], [2, 2]]
    right, _ = naive_states(rows, gts, area, gi['iscrowd'], [0.5])
    assert [r[0] for r in right] == st[:, 0, :].tolist()
    # at t = 0.55 A matches nothing and B takes gt 0 under either rule
    assert states_of(rows, gi, [0.55])[0, 0].tolist() == [0, 1]
    # the same with the two detections tied in score: the earlier row (A) ranks first
    rows2 = tie_case(scores=(.5, .5))[0]
    assert states_of(rows2, gi, [0.5])[:, 0, :].tolist() == [[1, 1], [1, 1], [2, 2], [2, 2]]
    # coincident gts: every one of them is taken once, whatever the order
    same = info([[0, 0, 32, 32]] * 3, area=[100, 100, 5000])
    assert states_of([[0, 0, 32, 32, .9], [0, 0, 32, 32, .8], [0, 0, 32, 32, .7]], same, [0.5])[0, 0].tolist() == [1, 1, 1]


def test_iou_exactly_at_the_threshold_matches():
    gi = info([[0, 0, 64, 32]])
    half = [[0, 0, 32, 32, .9]]                                  # inter 1024, union 2048: exactly 0.5
    assert CE.iou_matrix(*CE.rank_detections(dets(half), 10)[:2], gi['boxes'], gi['iscrowd'])[0, 0] == 0.5
    assert states_of(half, gi, [0.5])[0, 0].tolist() == [1]
    assert states_of(half, gi, [np.nextafter(0.5, 1)])[0, 0].tolist() == [0]
    three = [[0, 0, 48, 32, .9]]                                 # exactly 0.75, the sixth default threshold
    assert THRS[5] == 0.75 and states_of(three, gi)[0, :, 0].tolist() == [1] * 6 + [0] * 4
    # an IoU of 1 still matches at t = 1 (the bound is min(t, 1 - 1e-10))
    assert states_of([[0, 0, 64, 32, .9]], gi, [1.0])[0, 0].tolist() == [1]


def test_area_32_squared_is_small_and_medium():
    gi = info([[0, 0, 32, 32], [100, 100, 96, 96]])
    assert CE.count_npig([gi], 1).tolist() == [[2, 1, 2, 1]]
    st = states_of([[0, 0, 32, 32, .9], [100, 100, 196, 196, .8]], gi, [0.5])
    assert st[:, 0, :].tolist() == [[1, 1], [1, 2], [1, 1], [2, 1]]


def test_unmatched_detection_outside_the_range_is_ignored_a_matched_one_is_not():
    # a 16 x 16 gt (small) matched by a 20 x 20 detection; a free 100 x 100 detection (large), a free 8 x 8 one (small)
    gi = info([[0, 0, 16, 16]])
    st = states_of([[0, 0, 20, 20, .9], [200, 200, 300, 300, .8], [400, 400, 408, 408, .7]], gi, [0.5])
    assert st[:, 0, :].tolist() == [[1, 0, 0], [1, 2, 0], [2, 2, 2], [2, 0, 2]]
    # a detection of large area matched to a small gt stays a tp of `small`
    big = info([[0, 0, 30, 30]], area=[100.0])
    assert states_of([[0, 0, 40, 40, .9]], big, [0.5])[1, 0].tolist() == [1]


def test_score_ties_across_images_keep_dataset_order():
    # image 0: a false positive, image 1: a true positive, equal scores -> fp first: AP = precision 1/2 everywhere
    infos = [info([]), info([[0, 0, 40, 40]])]
    results = [[dets([[0, 0, 40, 40, .5]])], [dets([[0, 0, 40, 40, .5]])]]
    out = CE.evaluate_bbox(results, infos, ('a',), logger='silent')
    assert out['bbox_mAP'] == 0.5
    out = CE.evaluate_bbox(results[::-1], infos[::-1], ('a',), logger='silent')
    assert out['bbox_mAP'] == 1.0
    # inside one image the earlier row ranks first
    box, _, _, order = CE.rank_detections(dets([[0, 0, 1, 1, .5], [0, 0, 2, 2, .7], [0, 0, 3, 3, .5]]), 1000)
    assert order.tolist() == [1, 0, 2]
    assert CE.rank_detections(dets([[0, 0, 1, 1, .5], [0, 0, 2, 2, .7], [0, 0, 3, 3, .5]]), 2)[3].tolist() == [1, 0]


def test_metric_items_classwise_thresholds():
    infos = [info([[10, 10, 40, 40], [60, 60, 40, 40]], labels=[0, 1])]
    results = [[dets([[10, 10, 50, 50, .9]]), dets([[200, 200, 240, 240, .8]])]]
    out = CE.evaluate_bbox(results, infos, ('a', 'b'), metric_items=['mAP_50', 'mAP'], logger='silent')
    assert list(out) == ['bbox_mAP_50', 'bbox_mAP', 'bbox_mAP_copypaste'] and out['bbox_mAP'] == 0.5
    with pytest.raises(KeyError, match='mAP_xl'):
        CE.evaluate_bbox(results, infos, ('a', 'b'), metric_items=['mAP_xl'], logger='silent')
    out = CE.evaluate_bbox(results, infos, ('a', 'b'), classwise=True, logger='silent')
    assert out['bbox_AP_a'] == 1.0 and out['bbox_AP_b'] == 0.0 and list(out)[:2] == ['bbox_AP_a', 'bbox_AP_b']
    # thresholds without 0.5 / 0.75: selected by index, -1 when absent
    out = CE.evaluate_bbox(results, infos, ('a', 'b'), iou_thrs=[0.6, 0.75 + 1e-12], logger='silent')
    assert out['bbox_mAP_50'] == -1.0 and out['bbox_mAP_75'] == 0.5
    for m in CE.UNSUPPORTED:
        with pytest.raises(KeyError, match='is not supported'):
            CE.check_metric(m)


@pytest.fixture(scope='module')
def draw():
    results, infos = quantised_draw()
    return results, infos


def test_the_draw_has_ties_and_exact_threshold_ious(draw):
    results, infos = draw
    ties = exact = 0
    for res, gi in zip(results, infos):
        for c, rows in enumerate(res):
            s = np.sort(rows[:, 4])
            ties += int((s[1:] == s[:-1]).sum())
            sel = gi['labels'] == c
            if len(rows) and sel.any():
                box, area, _, _ = CE.rank_detections(rows, 1000)
                iou = CE.iou_matrix(box, area, gi['boxes'][sel], gi['iscrowd'][sel])
                exact += int(np.isin(iou, THRS).sum())
    print('tied score pairs', ties, 'exact-threshold pairs', exact)
    assert ties >= 20 and exact >= 5


def test_evaluator_equals_the_naive_restatement(draw):
    results, infos = draw
    assert len(results) == 204
    n = rule = 0
    for res, gi in zip(results, infos):
        for c, rows in enumerate(res):
            if not len(rows):
                continue
            sel = gi['labels'] == c
            box, area, _, order = CE.rank_detections(rows, 1000)
            got = CE.match_image(box, area, gi['boxes'][sel], gi['area'][sel], gi['iscrowd'][sel], THRS)
            want, worder = naive_states(rows, gi['boxes'][sel], gi['area'][sel], gi['iscrowd'][sel], THRS)
            assert order.tolist() == worder and got.tolist() == want
            n += got.size
            rule += int((np.asarray(naive_states(rows, gi['boxes'][sel], gi['area'][sel], gi['iscrowd'][sel], THRS, tie='earlier')[0],
                                    np.uint8) != got).sum())
    print('states that taking the earlier of two equal IoUs would change:', rule)
    assert n > 10000 and rule >= 8           # the comparison pins the replacement rule (tie_images: first and second sweep)
    K = len(results[0])
    out = CE.evaluate_bbox(results, infos, [str(c) for c in range(K)], logger='silent')
    want = naive_summary(results, infos, K, THRS)
    assert all(v > 0 for v in want.values())
    for k, v in want.items():
        assert out[f'bbox_{k}'] == float(f'{v:.3f}') or abs(out[f'bbox_{k}'] - v) <= 0.0005 + 1e-12 * abs(v)
    # the unrounded summary
    parts = [CE.image_states(r, i, THRS, 1000) for r, i in zip(results, infos)]
    prec = CE.accumulate(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts], 2),
                         CE.count_npig(infos, K), K)
    for k, v in CE.summarize(prec, THRS).items():
        assert v == pytest.approx(want[k], rel=1e-12), k
    # max_det truncates per (image, class)
    few = CE.evaluate_bbox(results, infos, [str(c) for c in range(K)], proposal_nums=(1, 2), logger='silent')
    wfew = naive_summary(results, infos, K, THRS, max_det=2)
    assert few['bbox_mAP'] == float(f"{wfew['mAP']:.3f}") and few['bbox_mAP'] != out['bbox_mAP']


def _fill(acc, results, infos, picks, M, rng=None):
    from aod_meh_hua_amd.core.coco_eval_device import pack_eval_infos          # noqa: F401  (importable without a GPU)
    d, l, n = padded_batch([results[i] for i in picks], M, rng)
    states = np.zeros((4, len(THRS), len(picks), M), np.uint8)
    for b, i in enumerate(picks):
        for c in range(len(results[i])):
            rows = np.flatnonzero((l[b, :n[b]] == c))
            if not len(rows):
                continue
            sel = infos[i]['labels'] == c
            box, area, _, order = CE.rank_detections(d[b, rows], 1000)
            st = CE.match_image(box, area, infos[i]['boxes'][sel], infos[i]['area'][sel], infos[i]['iscrowd'][sel], THRS)
            states[:, :, b, rows[order]] = st
    acc.store(torch.tensor(picks, dtype=torch.int64), torch.from_numpy(d[:, :, 4].copy()), torch.from_numpy(l), torch.from_numpy(states),
              torch.from_numpy(n), [infos[i] for i in picks])


def test_device_accumulator_on_cpu_reproduces_evaluate_and_merges(draw):
    from aod_meh_hua_amd.core.coco_eval_device import DeviceCocoAccumulator
    results, infos = draw
    results, infos = results[:60], infos[:60]
    K, M = len(results[0]), 16
    names = [str(c) for c in range(K)]
    want = CE.evaluate_bbox(results, infos, names, classwise=True, logger='silent')
    rng = np.random.RandomState(3)
    full = DeviceCocoAccumulator(K, None, M, 60, 'cpu')
    for s in range(0, 60, 7):
        _fill(full, results, infos, list(range(s, min(s + 7, 60))), M, rng)
    got = full.finalize(names, classwise=True, logger='silent')
    assert got == want and list(got) == list(want)
    # two half-filled accumulators (interleaved rows) merge into the full one
    a, b = DeviceCocoAccumulator(K, None, M, 60, 'cpu'), DeviceCocoAccumulator(K, None, M, 60, 'cpu')
    _fill(a, results, infos, list(range(0, 60, 2)), M)
    _fill(b, results, infos, list(range(1, 60, 2)), M)
    assert a.finalize(names, logger='silent') != want
    merged = a.merge(b)
    assert bool(merged.owned.all()) and np.array_equal(merged.npig, full.npig)
    assert merged.finalize(names, classwise=True, logger='silent') == want
    assert np.array_equal(merged.precision(), full.precision())
    with pytest.raises(ValueError, match='max_per_img'):
        DeviceCocoAccumulator(K, None, 1001, 4, 'cpu')
    with pytest.raises(ValueError, match='IoU thresholds'):
        DeviceCocoAccumulator(K, np.linspace(.1, .9, 17), 16, 4, 'cpu')
