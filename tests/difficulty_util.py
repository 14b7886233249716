"""Shared by tests/test_difficulty_host.py and tests/test_gpu_difficulty.py: the numpy float64 restatement of the class difficulty of DESIGN 3p
(PPAL's Difficulty-Calibrated Uncertainty Sampling) -- the class probability of both loss forms, the box quality from the deltas alone, the
per-sample difficulty q, the batch statistic (S, n), the EMA and the class weights -- evaluated on the fp32 inputs; a second, independent
IoU path that decodes both deltas against real anchors; and the seeded input maker of the kernel tests.

Tolerance (ATOL = 1e-5 on S[c] / n[c] and on the updated d, derived in the issue): q <= 1; expf / division / powf contribute a few ulp of 1
each, below 1e-6 per sample; a mean over at most 64 positives per class adds at most 64 * 2^-24 ~ 4e-6.  The input maker keeps the
positives per class at 64 or fewer."""
import math

import numpy as np

ATOL = 1e-5
MAX_POS_PER_CLASS = 64
WH_RATIO_CLIP = 16 / 1000
XI, MOMENTUM, ALPHA, BETA = 0.6, 0.99, 0.3, 0.2
FORMS = ('edl', 'sigmoid')


def class_prob64(x, c, form):
    """P of the target class c from one row of fp32 logits x: 'edl' softmax (maximum subtracted), 'sigmoid' 1 / (1 + exp(-x[c]))"""
    x = np.asarray(x, np.float32).astype(np.float64)
    if form == 'edl':
        e = np.exp(x - x.max())
        return float(e[c] / e.sum())
    if form == 'sigmoid':
        with np.errstate(over='ignore'):
            return float(1.0 / (1.0 + np.exp(-x[c])))
    raise ValueError(form)


def _frame_box(delta, means, stds, clip):
    t = np.asarray(delta, np.float32).astype(np.float64) * np.asarray(stds, np.float64) + np.asarray(means, np.float64)
    mr = abs(math.log(clip))
    w, h = math.exp(min(max(t[2], -mr), mr)), math.exp(min(max(t[3], -mr), mr))
    return np.array([t[0] - 0.5 * w, t[1] - 0.5 * h, t[0] + 0.5 * w, t[1] + 0.5 * h])


def iou64(a, b):
    """ov / max(un, 1e-6) of two (x1, y1, x2, y2) boxes: aod_loc_stability's form"""
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    ov = iw * ih
    un = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - ov
    return ov / max(un, 1e-6)


def delta_iou64(dp, dt, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), clip=WH_RATIO_CLIP):
    """the box quality from the deltas alone, in the anchor-normalised frame (centre (t0, t1), size (exp t2, exp t3))"""
    return iou64(_frame_box(dp, means, stds, clip), _frame_box(dt, means, stds, clip))


def anchor_iou64(anchor, dp, dt, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), clip=WH_RATIO_CLIP):
    """the independent path: both deltas decoded against the anchor (x1, y1, x2, y2) as delta2bbox does (no image clipping), then the plain
    IoU of the two pixel boxes (no floor on the union: the boxes have positive areas)"""
    a = np.asarray(anchor, np.float64)
    aw, ah = a[2] - a[0], a[3] - a[1]
    ax, ay = 0.5 * (a[0] + a[2]), 0.5 * (a[1] + a[3])
    mr = abs(math.log(clip))
    out = []
    for d in (dp, dt):
        t = np.asarray(d, np.float32).astype(np.float64) * np.asarray(stds, np.float64) + np.asarray(means, np.float64)
        w, h = aw * math.exp(np.clip(t[2], -mr, mr)), ah * math.exp(np.clip(t[3], -mr, mr))
        cx, cy = ax + aw * t[0], ay + ah * t[1]
        out.append((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2))
    p, g = out
    iw, ih = max(min(p[2], g[2]) - max(p[0], g[0]), 0.0), max(min(p[3], g[3]) - max(p[1], g[1]), 0.0)
    ov = iw * ih
    return ov / ((p[2] - p[0]) * (p[3] - p[1]) + (g[2] - g[0]) * (g[3] - g[1]) - ov)


def difficulty64(P, iou, xi=XI):
    if not P > 0 or not iou > 0:
        return 1.0
    return float(min(max(1.0 - P ** xi * iou ** (1.0 - xi), 0.0), 1.0))


def positives(labels, label_w, C):
    labels, label_w = np.asarray(labels), np.asarray(label_w, np.float32)
    return np.nonzero((labels >= 0) & (labels < C) & (label_w > 0))[0]


def batch_stat64(cls, labels, label_w, bbox_pred, bbox_tgt, form, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), xi=XI, clip=WH_RATIO_CLIP):
    """(S [C] float64, n [C] int64, q per positive row {row: q}) of one batch's loss operands; only the positives' rows are read"""
    C = cls.shape[1]
    S, n, qs = np.zeros(C), np.zeros(C, np.int64), {}
    for r in positives(labels, label_w, C):
        c = int(labels[r])
        q = difficulty64(class_prob64(cls[r], c, form), delta_iou64(bbox_pred[r], bbox_tgt[r], means, stds, clip), xi)
        S[c] += q
        n[c] += 1
        qs[int(r)] = q
    return S, n, qs


def ema64(d, S, n, momentum=MOMENTUM):
    """d [C] (fp32 values) after one update: classes with n > 0 move, the others keep their value"""
    d = np.asarray(d, np.float32).astype(np.float64).copy()
    has = np.asarray(n) > 0
    d[has] = momentum * d[has] + (1.0 - momentum) * (np.asarray(S, np.float64)[has] / np.asarray(n)[has])
    return d


def class_weight64(d, alpha=ALPHA, beta=BETA):
    """w = 1 + alpha beta ln(1 + gamma d), gamma = e^(1 / alpha) - 1: 1 at d = 0, 1 + beta at d = 1"""
    return 1.0 + alpha * beta * np.log1p(math.expm1(1.0 / alpha) * np.asarray(d, np.float64))


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_inputs(nrows, C, seed, n_pos=None, nan_fill=True, pos_rows=None):
    """dict of fp32 / int64 numpy arrays: cls [nrows, C], labels, label_w, bbox_pred, bbox_tgt [nrows, 4].  Background rows carry the label C
    (a few -1), a few foreground labels carry label_w = 0 (skipped).  The positives -- n_pos of them (default: about nrows / 8, at least
    one if nrows >= 1) at seeded rows or at pos_rows -- number at most 64 per class; the last row is a positive.  With nan_fill every row
    that is no positive holds NaN in cls and bbox_pred: the kernel must not read them."""
    g = np.random.default_rng(seed)
    cls = g.uniform(-4, 4, (nrows, C)).astype(np.float32)
    bp = (0.3 * g.standard_normal((nrows, 4))).astype(np.float32)
    bt = (0.3 * g.standard_normal((nrows, 4))).astype(np.float32)
    labels = np.full(nrows, C, np.int64)
    labels[g.random(nrows) < 0.05] = -1
    lw = np.ones(nrows, np.float32)
    if pos_rows is None:
        n_pos = max(1, nrows // 8) if n_pos is None else n_pos
        n_pos = min(n_pos, nrows, C * MAX_POS_PER_CLASS)
        pos_rows = np.sort(g.choice(nrows, n_pos, replace=False)) if n_pos else np.zeros(0, np.int64)
        if n_pos and pos_rows[-1] != nrows - 1:
            pos_rows[-1] = nrows - 1
    pos_rows = np.asarray(pos_rows, np.int64)
    count = np.zeros(C, np.int64)
    for r in pos_rows:
        c = int(g.integers(C))
        while count[c] >= MAX_POS_PER_CLASS:
            c = (c + 1) % C
        count[c] += 1
        labels[r] = c
    # foreground labels the assigner gave no weight: skipped
    free = np.setdiff1d(np.arange(nrows), pos_rows)
    skipped = free[g.random(len(free)) < 0.03]
    labels[skipped] = g.integers(0, C, len(skipped))
    lw[skipped] = 0.0
    lw[pos_rows] = g.uniform(0.5, 1.5, len(pos_rows)).astype(np.float32)
    if nan_fill:
        no = np.ones(nrows, bool)
        no[pos_rows] = False
        cls[no] = np.nan
        bp[no] = np.nan
    assert len(positives(labels, lw, C)) == len(pos_rows) and count.max(initial=0) <= MAX_POS_PER_CLASS
    return dict(cls=cls, labels=labels, label_w=lw, bbox_pred=bp, bbox_tgt=bt)
