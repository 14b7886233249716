"""Helpers of the COCO tests: a writer of small COCO annotation files, an independent and deliberately naive float64 restatement of the
bbox matching protocol as one flat loop -- it imports nothing from core/coco_eval.py --, and the seeded, quantised random draw
the host and the GPU tests share."""
import json

import numpy as np

AREA_RANGES = ((0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10))
VOC_NAMES = ('aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog', 'horse',
             'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')


def category_ids(n, gaps=True):
    """n category ids; with gaps they are not contiguous (1, 2, 4, 5, 7, ...) as COCO's are not"""
    return [1 + i + i // 2 for i in range(n)] if gaps else list(range(1, n + 1))


def write_coco_json(path, source, names=VOC_NAMES, size=None, gaps=True, crowd=(), area_scale=None, extra=(), shuffle_categories=False):
    """COCO annotation file at `path`.  `source`: a dataset with get_ann_info (xyxy boxes, labels; e.g. SyntheticVOCDataset) or a list of
    per-image lists of dict(bbox=[x, y, w, h], label=int, and optionally iscrowd, area, ignore, category_id).  size: (h, w) of every image
    (default the dataset's); a list of (h, w) gives one per image.  gaps: non-contiguous category ids.  crowd: (image, k) pairs whose k-th
    annotation becomes a crowd.  area_scale: area = w * h * area_scale instead of w * h.  extra: (image, annotation dict) pairs appended
    behind the image's own.  Image ids are 1000 + 7 * i, file names img_<i>.png.  Returns the image ids."""
    ids = category_ids(len(names), gaps)
    cats = [dict(id=cid, name=n) for cid, n in zip(ids, names)]
    if shuffle_categories:
        cats = cats[::-1]
    if hasattr(source, 'get_ann_info'):
        per_image = []
        for i in range(len(source)):
            ann = source.get_ann_info(i)
            per_image.append([dict(bbox=[float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])], label=int(l))
                              for b, l in zip(ann['bboxes'], ann['labels'])])
        if size is None:
            size = tuple(source.size)
    else:
        per_image = [list(a) for a in source]
    for i, ann in extra:
        per_image[i].append(dict(ann))
    for i, k in crowd:
        per_image[i][k] = dict(per_image[i][k], iscrowd=1)
    images, annotations = [], []
    for i, anns in enumerate(per_image):
        h, w = size[i] if isinstance(size[0], (tuple, list)) else size
        images.append(dict(id=1000 + 7 * i, file_name=f'img_{i}.png', width=int(w), height=int(h)))
        for a in anns:
            x, y, bw, bh = (float(v) for v in a['bbox'])
            rec = dict(id=len(annotations) + 1, image_id=1000 + 7 * i, category_id=a.get('category_id', ids[a['label']] if 'label' in a else None),
                       bbox=[x, y, bw, bh], area=float(a['area']) if 'area' in a else bw * bh * (area_scale or 1.0), iscrowd=int(a.get('iscrowd', 0)))
            if a.get('ignore'):
                rec['ignore'] = 1
            annotations.append(rec)
    with open(path, 'w') as f:
        json.dump(dict(images=images, annotations=annotations, categories=cats), f)
    return [im['id'] for im in images]


def write_coco_images(folder, source):
    """img_<i>.png for every sample of a SyntheticVOCDataset: its N(0, 1) tensor as 8-bit noise around the ImageNet mean (what the configs'
    Normalize step maps back to about N(0, 1))"""
    import os
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i in range(len(source)):
        px = (source[i]['img'].permute(1, 2, 0).numpy() * 57.0 + 114.0).clip(0, 255).astype(np.uint8)
        Image.fromarray(px).save(os.path.join(folder, f'img_{i}.png'))


def naive_states(det_rows, gt_xywh, gt_area, gt_crowd, iou_thrs, max_det=1000, area_ranges=AREA_RANGES, tie='later'):
    """One (image, class), following the text of DESIGN 3n line by line.  det_rows [k, 5] xyxy + score in row order.
    -> (states [A][T][k'] nested lists in rank order, order: the row of every rank).
    tie='earlier' is the WRONG rule (a gt is replaced only by a strictly greater IoU): the tests use it to show that their data tell the
    two rules apart."""
    assert tie in ('later', 'earlier')
    keep_first = tie == 'earlier'
    rows = [[float(np.float64(v)) for v in r] for r in np.asarray(det_rows).reshape(-1, 5)]
    order = sorted(range(len(rows)), key=lambda i: (-rows[i][4], i))[:max_det]
    dets = []
    for i in order:
        x1, y1, x2, y2, _ = rows[i]
        w, h = x2 - x1, y2 - y1
        dets.append((x1, y1, w, h, w * h))
    gts = [tuple(float(v) for v in g) for g in np.asarray(gt_xywh, np.float64).reshape(-1, 4)]
    gt_area = [float(a) for a in np.asarray(gt_area, np.float64).reshape(-1)]
    gt_crowd = [bool(c) for c in np.asarray(gt_crowd).reshape(-1)]

    def iou(d, g, crowd):
        dx, dy, dw, dh, da = d
        gx, gy, gw, gh = g
        iw = min(dx + dw, gx + gw) - max(dx, gx)
        ih = min(dy + dh, gy + gh) - max(dy, gy)
        if iw <= 0 or ih <= 0:
            return 0.0
        inter = iw * ih
        union = da if crowd else da + gw * gh - inter
        return inter / union

    states = []
    for lo, hi in area_ranges:
        ignore = [gt_crowd[g] or gt_area[g] < lo or gt_area[g] > hi for g in range(len(gts))]
        per_t = []
        for t in iou_thrs:
            matched = [False] * len(gts)
            out = []
            for d in dets:
                b, m = min(float(t), 1 - 1e-10), None
                for g in range(len(gts)):
                    if ignore[g] or matched[g]:
                        continue
                    v = iou(d, gts[g], gt_crowd[g])
                    if v < b or (keep_first and m is not None and v <= b):
                        continue
                    b, m = v, g
                if m is None:
                    for g in range(len(gts)):
                        if not ignore[g]:
                            continue
                        if matched[g] and not gt_crowd[g]:
                            continue
                        v = iou(d, gts[g], gt_crowd[g])
                        if v < b or (keep_first and m is not None and v <= b):
                            continue
                        b, m = v, g
                if m is not None:
                    matched[m] = True
                    out.append(2 if ignore[m] else 1)
                elif d[4] < lo or d[4] > hi:
                    out.append(2)
                else:
                    out.append(0)
            per_t.append(out)
        states.append(per_t)
    return states, order


def naive_summary(results, infos, num_classes, iou_thrs, max_det=1000, area_ranges=AREA_RANGES):
    """the six summary numbers from naive_states, accumulated with plain loops"""
    T, A = len(iou_thrs), len(area_ranges)
    rec = list(np.linspace(0, 1, 101))
    cells = {}
    for c in range(num_classes):
        pool = []          # (score, image, rank, states[a][t])
        npig = [0] * A
        for i, (res, info) in enumerate(zip(results, infos)):
            sel = [g for g in range(len(info['labels'])) if int(info['labels'][g]) == c]
            for a, (lo, hi) in enumerate(area_ranges):
                npig[a] += sum(1 for g in sel if not info['iscrowd'][g] and not (info['area'][g] < lo or info['area'][g] > hi))
            rows = np.asarray(res[c]).reshape(-1, 5)
            if not len(rows):
                continue
            st, order = naive_states(rows, np.asarray(info['boxes']).reshape(-1, 4)[sel], np.asarray(info['area'])[sel],
                                     np.asarray(info['iscrowd'])[sel], iou_thrs, max_det, area_ranges)
            for r, row in enumerate(order):
                pool.append((float(np.float64(rows[row, 4])), i, r, [[st[a][t][r] for t in range(T)] for a in range(A)]))
        pool.sort(key=lambda p: (-p[0], p[1], p[2]))
        for a in range(A):
            if npig[a] == 0:
                continue
            for t in range(T):
                tp = fp = 0
                rc, pr = [], []
                for p in pool:
                    s = p[3][a][t]
                    if s == 2:
                        continue
                    tp, fp = tp + (s == 1), fp + (s == 0)
                    rc.append(tp / npig[a])
                    pr.append(tp / (fp + tp + np.spacing(1)))
                for k in range(len(pr) - 1, 0, -1):
                    if pr[k] > pr[k - 1]:
                        pr[k - 1] = pr[k]
                q = []
                for r in rec:
                    k = 0
                    while k < len(rc) and rc[k] < r:
                        k += 1
                    q.append(pr[k] if k < len(rc) else 0.0)
                cells[(t, c, a)] = q
    def mean(keys):
        v = [x for k in keys if k in cells for x in cells[k]]
        return float(np.mean(v)) if v else -1.0
    K = range(num_classes)
    out = dict(mAP=mean([(t, c, 0) for t in range(T) for c in K]))
    for name, val in (('mAP_50', 0.5), ('mAP_75', 0.75)):
        near = [t for t in range(T) if abs(float(iou_thrs[t]) - val) <= 1e-9]
        out[name] = mean([(near[0], c, 0) for c in K]) if near else -1.0
    for a, name in ((1, 'mAP_s'), (2, 'mAP_m'), (3, 'mAP_l')):
        out[name] = mean([(t, c, a) for t in range(T) for c in K])
    return out


def tie_case(x0=0.0, y0=0.0, area=100.0, scores=(.9, .8)):
    """Two gts and two detections of one class on which the replacement rule shows in the states.  gts (xywh) [x0, y0, 40, 32] and
    [x0 + 24, y0, 40, 32]; detection A = [x0 + 12, y0, x0 + 52, y0 + 32] overlaps both with the same IoU 896 / 1664 = 28 / 52 (the same
    float64 operations on both sides); detection B coincides with gt 0 and has IoU 1 / 4 with gt 1.  At t = 0.5 A takes the LATER gt 1 and
    leaves gt 0 to B; under the wrong rule A takes gt 0 and B goes empty.  With the file's `area` = 100 the gts are counted by the ranges
    all and small (first sweep: states [1, 1], wrong rule [1, 0] / [1, 2]) and ignored by medium (second sweep: [2, 2], wrong rule [2, 0],
    B's own area 1280 lies inside medium).  -> (det rows [2, 5] float32 xyxy + score, gt boxes [2, 4], gt area [2])"""
    gts = np.array([[x0, y0, 40.0, 32.0], [x0 + 24.0, y0, 40.0, 32.0]])
    rows = np.array([[x0 + 12.0, y0, x0 + 52.0, y0 + 32.0, scores[0]], [x0, y0, x0 + 40.0, y0 + 32.0, scores[1]]], np.float32)
    return rows, gts, np.array([area, area])


def tie_images(num_classes):
    """four images built around tie_case: alone; behind other gts and detections of another class; twice in one image (two classes); with a
    crowd of the same class in front -> (results, infos) in quantised_draw's form"""
    results, infos = [], []

    def image(parts):
        rows = [[] for _ in range(num_classes)]
        boxes, area, crowd, labels = [], [], [], []
        for c, r, g, a, cr in parts:
            rows[c].extend(r.tolist())
            boxes.extend(g.tolist()), area.extend(a.tolist()), crowd.extend(cr), labels.extend([c] * len(g))
        results.append([np.asarray(r, np.float32).reshape(-1, 5) for r in rows])
        infos.append(dict(boxes=np.asarray(boxes, np.float64).reshape(-1, 4), area=np.asarray(area, np.float64),
                          iscrowd=np.asarray(crowd, np.uint8), labels=np.asarray(labels, np.int64)))

    r, g, a = tie_case()
    image([(0, r, g, a, [0, 0])])
    other = (1, np.array([[4, 4, 36, 36, .95]], np.float32), np.array([[4.0, 4.0, 32.0, 32.0]]), np.array([1024.0]), [0])
    r, g, a = tie_case(16.0, 64.0, scores=(.5, .5))              # a score tie on top: A is the earlier row
    image([other, (2, r, g, a, [0, 0])])
    r2, g2, a2 = tie_case(8.25, 40.5)
    image([(1, r, g, a, [0, 0]), (3, r2, g2, a2, [0, 0])])
    r, g, a = tie_case(0.0, 0.0)
    far = np.array([[0.0, 80.0, 16.0, 16.0]])                     # a crowd that overlaps nothing, first in file order
    image([(0, r[:0], far, np.array([256.0]), [1]), (0, r, g, a, [0, 0])])
    return results, infos


def quantised_draw(num_images=200, num_classes=6, seed=7, size=128, max_gt=6, max_det=14):
    """Seeded random images whose coordinates are multiples of 1/4 pixel and whose scores are multiples of 1/64, so that score ties and
    IoUs exactly equal to a threshold occur.  Detections are copies of gts, shifted copies (power-of-two overlaps) and free boxes.
    Behind the num_images random images come the four of tie_images, on which equal IoUs decide the states.
    -> (results[i][c] = [k, 5] float32, infos[i] = dict(boxes xywh f64, area, iscrowd, labels))."""
    rng = np.random.RandomState(seed)
    results, infos = [], []
    for _ in range(num_images):
        G = int(rng.randint(0, max_gt + 1))
        wh = rng.choice([8, 16, 24, 32, 48, 64, 96], size=(G, 2)).astype(np.float64)
        xy = np.floor(rng.rand(G, 2) * (size - wh) * 4) / 4
        labels = rng.randint(0, num_classes, G).astype(np.int64)
        crowd = (rng.rand(G) < 0.15).astype(np.uint8)
        area = wh[:, 0] * wh[:, 1] * rng.choice([1.0, 0.5, 1.0, 0.75], size=G)
        infos.append(dict(boxes=np.concatenate([xy, wh], 1).reshape(-1, 4), area=area, iscrowd=crowd, labels=labels))
        D = int(rng.randint(0, max_det + 1))
        rows = [[] for _ in range(num_classes)]
        for _ in range(D):
            kind = rng.rand()
            if G and kind < 0.75:
                g = int(rng.randint(G))
                x, y, w, h = xy[g, 0], xy[g, 1], wh[g, 0], wh[g, 1]
                if kind < 0.3:              # shifted by a fraction f of the width: IoU (1 - f) / (1 + f), 3/5 or 1/3
                    x = x + w * rng.choice([0.25, 0.5])
                elif kind < 0.5:            # half the box, same corner: IoU exactly 1/2; three quarters: exactly 3/4
                    w = w * rng.choice([0.5, 0.75])
                c = int(labels[g]) if rng.rand() < 0.9 else int(rng.randint(num_classes))
            else:
                w, h = rng.choice([8, 16, 32, 64], size=2).astype(np.float64)
                x, y = np.floor(rng.rand(2) * (size - np.array([w, h])) * 4) / 4
                c = int(rng.randint(num_classes))
            score = float(rng.randint(1, 65)) / 64.0
            rows[c].append([x, y, x + w, y + h, score])
        results.append([np.asarray(r, np.float32).reshape(-1, 5) for r in rows])
    tr, ti = tie_images(num_classes)
    return results + tr, infos + ti


def padded_batch(results, max_per_img, rng=None):
    """results[i][c] of a batch -> (dets [B,M,5] float32, labels [B,M] int64, num [B] int32) as aod_multiclass_nms leaves them: the rows of
    all classes in one list (shuffled when rng is given: the kernel must not need them sorted), zero padding"""
    B = len(results)
    dets, labels, num = np.zeros((B, max_per_img, 5), np.float32), np.zeros((B, max_per_img), np.int64), np.zeros((B,), np.int32)
    for b, res in enumerate(results):
        rows = np.concatenate([np.asarray(r, np.float32).reshape(-1, 5) for r in res]) if len(res) else np.zeros((0, 5), np.float32)
        lab = np.concatenate([np.full(len(r), c, np.int64) for c, r in enumerate(res)]) if len(res) else np.zeros(0, np.int64)
        if rng is not None:
            # interleave the classes at random; the rows of one class keep their relative order (it breaks score ties)
            keys = rng.rand(len(rows))
            for c in np.unique(lab):
                keys[lab == c] = np.sort(keys[lab == c])
            order = np.argsort(keys, kind='stable')
            rows, lab = rows[order], lab[order]
        n = min(len(rows), max_per_img)
        dets[b, :n], labels[b, :n], num[b] = rows[:n], lab[:n], n
    return dets, labels, num
