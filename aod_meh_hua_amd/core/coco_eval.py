"""COCO bbox evaluation on the host, numpy float64, without pycocotools: the protocol of COCOeval's bbox mode as mmdet's
CocoDataset.evaluate drives it (maxDets = proposal_nums, AP read at the last of them), restated from its description.  Unpinned at the
pycocotools boundary: pycocotools is neither installed nor part of the reference tree, so no test compares against it.

Three stages, split so that the device path (core/coco_eval_device.py) reuses the tail:
    match_image   one (image, class): ranked detections x gts -> states [A, T, k]   (aod_coco_match does this for a whole batch)
    accumulate    (score, label, state) rows of the whole set -> precision [T, 101, K, A]
    summarize     precision -> mAP, mAP_50, mAP_75, mAP_s, mAP_m, mAP_l
States: 1 matched to a counted gt (tp), 0 unmatched and counted (fp), 2 ignored."""
from collections import OrderedDict

import numpy as np

AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # all, small, medium, large; inclusive bounds
AREA_NAMES = ('all', 'small', 'medium', 'large')
REC_THRS = np.linspace(0, 1, 101)
METRIC_ITEMS = ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l')
UNSUPPORTED = ('segm', 'proposal', 'proposal_fast')


def default_iou_thrs():
    return np.linspace(.5, .95, 10)


def check_metric(metric):
    """the one metric of this evaluator; the reference's other three raise like an unknown one"""
    metrics = [metric] if isinstance(metric, str) else list(metric)
    for m in metrics:
        if m != 'bbox':
            raise KeyError(f'metric {m} is not supported')
    return metrics


def rank_detections(rows, max_det):
    """rows [k, 5] (xyxy + score, any float dtype) -> (boxes [k', 4] float64 xywh, area [k'], score [k'] float64, order [k']): the rows
    promoted to float64, ranked by score descending (stable: the earlier row first on a tie), the first max_det kept."""
    d = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    order = np.argsort(-d[:, 4], kind='mergesort')[:max_det]
    d = d[order]
    w, h = d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]
    return np.stack([d[:, 0], d[:, 1], w, h], 1), w * h, d[:, 4], order


def iou_matrix(det_xywh, det_area, gt_xywh, gt_crowd):
    """[k, G] float64.  iw = min(dx + dw, gx + gw) - max(dx, gx), ih likewise; 0 unless both are positive; inter = iw * ih;
    union = d_area for a crowd gt, else (d_area + gw * gh) - inter.  The kernel repeats these operations in this order."""
    d, g = np.asarray(det_xywh, np.float64).reshape(-1, 4), np.asarray(gt_xywh, np.float64).reshape(-1, 4)
    dx, dy, dw, dh = (d[:, i][:, None] for i in range(4))
    gx, gy, gw, gh = (g[:, i][None, :] for i in range(4))
    iw = np.minimum(dx + dw, gx + gw) - np.maximum(dx, gx)
    ih = np.minimum(dy + dh, gy + gh) - np.maximum(dy, gy)
    hit = (iw > 0) & (ih > 0)
    inter = iw * ih
    da = np.asarray(det_area, np.float64).reshape(-1, 1)
    union = np.where(np.asarray(gt_crowd).reshape(1, -1).astype(bool), da + np.zeros_like(inter), (da + gw * gh) - inter)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(hit, inter / np.where(hit, union, 1.0), 0.0)


def match_image(det_xywh, det_area, gt_xywh, gt_area, gt_crowd, iou_thrs, area_ranges=AREA_RANGES):
    """One (image, class): detections in rank order against the class's gts in file order -> states [A, T, k] uint8.
    Per (range, threshold), per detection: the best countable gt that is still free and reaches min(t, 1 - 1e-10) -- the LAST one among
    equal IoUs -- else the best ignored gt (a crowd may be taken again); a match takes the gt's ignore flag; an unmatched detection whose
    own area lies outside the range is ignored."""
    k, G = len(det_area), len(gt_area)
    A, T = len(area_ranges), len(iou_thrs)
    states = np.zeros((A, T, k), np.uint8)
    det_area = np.asarray(det_area, np.float64)
    gt_area, crowd = np.asarray(gt_area, np.float64), np.asarray(gt_crowd).astype(bool)
    ious = iou_matrix(det_xywh, det_area, gt_xywh, crowd) if k and G else np.zeros((k, G))
    rev = np.arange(G)[::-1]
    for a, (lo, hi) in enumerate(area_ranges):
        ign = crowd | (gt_area < lo) | (gt_area > hi)
        out = (det_area < lo) | (det_area > hi)
        for t, thr in enumerate(iou_thrs):
            b0 = min(float(thr), 1 - 1e-10)
            taken = np.zeros(G, bool)
            for d in range(k):
                row, m = ious[d], -1
                for cand in (~ign & ~taken, ign & (~taken | crowd)):
                    cand = cand & (row >= b0)
                    if cand.any():
                        best = row[cand].max()
                        m = int(rev[(cand & (row == best))[::-1]][0])          # the last gt that holds the maximum
                        break
                if m >= 0:
                    taken[m] = True
                    states[a, t, d] = 2 if ign[m] else 1
                elif out[d]:
                    states[a, t, d] = 2
    return states


def count_npig(eval_infos, num_classes, area_ranges=AREA_RANGES):
    """[K, A] int64: gts a range counts (not a crowd, the file's area inside the inclusive bounds), over all images"""
    npig = np.zeros((num_classes, len(area_ranges)), np.int64)
    for info in eval_infos:
        lb, ar, cr = np.asarray(info['labels']).reshape(-1), np.asarray(info['area'], np.float64).reshape(-1), np.asarray(info['iscrowd']).reshape(-1)
        ok = (lb >= 0) & (lb < num_classes)
        for a, (lo, hi) in enumerate(area_ranges):
            keep = ok & (cr == 0) & ~(ar < lo) & ~(ar > hi)
            npig[:, a] += np.bincount(lb[keep].astype(np.int64), minlength=num_classes)
    return npig


def accumulate(scores, labels, states, npig, num_classes=None, rec_thrs=REC_THRS):
    """scores [n] / labels [n] / states [A, T, n]: the detection rows of the whole set, images in dataset order; npig [K, A].
    -> precision [T, R, K, A] float64, -1 where a (class, range) has no counted gt.  Per class: stable sort by score descending, cumulative
    tp / fp over the counted rows, precision made non-increasing from the end, read at the first recall >= each of the R thresholds."""
    scores, labels, states = np.asarray(scores), np.asarray(labels), np.asarray(states)
    npig = np.asarray(npig)
    K = npig.shape[0] if num_classes is None else num_classes
    A, T, R = states.shape[0], states.shape[1], len(rec_thrs)
    precision = -np.ones((T, R, K, A))
    for c in range(K):
        sel = np.flatnonzero(labels == c)
        s = scores[sel].astype(np.float64)
        order = np.argsort(-s, kind='mergesort')
        rows = sel[order]
        for a in range(A):
            if npig[c, a] == 0:
                continue
            st = states[a][:, rows]
            for t in range(T):
                counted = st[t][st[t] != 2]
                tp = np.cumsum(counted == 1).astype(np.float64)
                fp = np.cumsum(counted == 0).astype(np.float64)
                nd = len(tp)
                rc = tp / npig[c, a]
                pr = tp / (fp + tp + np.spacing(1))
                pr = np.maximum.accumulate(pr[::-1])[::-1]
                inds = np.searchsorted(rc, rec_thrs, side='left')
                q = np.zeros(R)
                ok = inds < nd
                q[ok] = pr[inds[ok]]
                precision[t, :, c, a] = q
    return precision


def _mean(x):
    x = x[x > -1]
    return float(np.mean(x)) if x.size else -1.0


def _thr_index(iou_thrs, value):
    """index of the threshold nearest `value` when it is within 1e-9 of it, else None"""
    d = np.abs(np.asarray(iou_thrs, np.float64) - value)
    i = int(np.argmin(d))
    return i if d[i] <= 1e-9 else None


def summarize(precision, iou_thrs):
    """precision [T, R, K, A] (A = 4: all, small, medium, large) -> OrderedDict of the six COCO AP numbers (floats, -1 without data)"""
    out = OrderedDict()
    out['mAP'] = _mean(precision[:, :, :, 0])
    for name, v in (('mAP_50', 0.5), ('mAP_75', 0.75)):
        i = _thr_index(iou_thrs, v)
        out[name] = -1.0 if i is None else _mean(precision[i:i + 1, :, :, 0])
    for a, name in ((1, 'mAP_s'), (2, 'mAP_m'), (3, 'mAP_l')):
        out[name] = _mean(precision[:, :, :, a])
    return out


def class_aps(precision):
    """per-class AP at range `all`: [K] floats, -1 for a class without counted gts (as the summary numbers; mmdet prints nan there, which
    would make two result dicts compare unequal)"""
    return [_mean(precision[:, :, c, 0]) for c in range(precision.shape[2])]


def format_eval(precision, iou_thrs, classes=None, classwise=False, metric_items=None, logger=None, max_det=1000):
    """the tail shared by both paths: precision -> mmdet's dict (bbox_<item> rounded to three digits, bbox_mAP_copypaste)"""
    from ..mmcv_lite import print_log
    stats = summarize(precision, iou_thrs)
    if metric_items is not None:
        for item in metric_items:
            if item not in METRIC_ITEMS:
                raise KeyError(f'metric item {item} is not supported')
    eval_results = OrderedDict()
    span = f'{float(iou_thrs[0]):0.2f}:{float(iou_thrs[-1]):0.2f}'
    lines = [f' Average Precision  (AP) @[ IoU={lab:<9s} | area={ar:>6s} | maxDets={max_det:>4d} ] = {stats[key]:0.3f}'
             for key, lab, ar in (('mAP', span, 'all'), ('mAP_50', '0.50', 'all'), ('mAP_75', '0.75', 'all'), ('mAP_s', span, 'small'),
                                  ('mAP_m', span, 'medium'), ('mAP_l', span, 'large'))]
    print_log('\n'.join(lines), logger=logger)
    if classwise:
        names = list(classes) if classes is not None else [str(c) for c in range(precision.shape[2])]
        aps = class_aps(precision)
        print_log('\n'.join(['| category | AP |'] + [f'| {n} | {ap:0.3f} |' for n, ap in zip(names, aps)]), logger=logger)
        for n, ap in zip(names, aps):
            eval_results[f'bbox_AP_{n}'] = float(f'{ap:.3f}')
    for item in (metric_items if metric_items is not None else METRIC_ITEMS):
        eval_results[f'bbox_{item}'] = float(f'{stats[item]:.3f}')
    eval_results['bbox_mAP_copypaste'] = ' '.join(f'{stats[k]:.3f}' for k in METRIC_ITEMS)
    print_log(f"bbox_mAP_copypaste: {eval_results['bbox_mAP_copypaste']}", logger=logger)
    return eval_results


def image_states(result, info, iou_thrs, max_det, area_ranges=AREA_RANGES):
    """One image: result[c] = [k, 5] rows per class, info = the dataset's get_eval_info -> (scores [n] float64, labels [n], states
    [A, T, n]) with the classes in order and each class's rows in rank order."""
    gl = np.asarray(info['labels']).reshape(-1)
    gb, ga, gc = np.asarray(info['boxes'], np.float64).reshape(-1, 4), np.asarray(info['area'], np.float64).reshape(-1), np.asarray(info['iscrowd']).reshape(-1)
    sc, lb, st = [], [], []
    for c, rows in enumerate(result):
        if len(rows) == 0:
            continue
        box, area, score, _ = rank_detections(rows, max_det)
        sel = gl == c
        st.append(match_image(box, area, gb[sel], ga[sel], gc[sel], iou_thrs, area_ranges))
        sc.append(score)
        lb.append(np.full(len(score), c, np.int64))
    A, T = len(area_ranges), len(iou_thrs)
    if not sc:
        return np.zeros(0), np.zeros(0, np.int64), np.zeros((A, T, 0), np.uint8)
    return np.concatenate(sc), np.concatenate(lb), np.concatenate(st, 2)


def evaluate_bbox(results, eval_infos, classes, iou_thrs=None, proposal_nums=(100, 300, 1000), classwise=False, metric_items=None,
                  logger=None):
    """results[i][c]: [k, 5] float32 xyxy + score (single_gpu_test's); eval_infos[i]: CocoDataset.get_eval_info(i) -> mmdet's bbox dict."""
    assert len(results) == len(eval_infos), f'{len(results)} results for {len(eval_infos)} images'
    iou_thrs = default_iou_thrs() if iou_thrs is None else np.asarray(iou_thrs, np.float64).reshape(-1)
    K, max_det = len(classes), int(proposal_nums[-1])
    parts = [image_states(res[:K], info, iou_thrs, max_det) for res, info in zip(results, eval_infos)]
    scores = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0)
    labels = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.int64)
    states = np.concatenate([p[2] for p in parts], 2) if parts else np.zeros((len(AREA_RANGES), len(iou_thrs), 0), np.uint8)
    precision = accumulate(scores, labels, states, count_npig(eval_infos, K), K)
    return format_eval(precision, iou_thrs, classes, classwise, metric_items, logger, max_det)
