"""Shared by tests/test_consistency_host.py and tests/test_gpu_consistency.py: the float64 restatement of the consistency pool (DESIGN 3q;
Elezi et al., CVPR 2022; CALD, Yu et al., CVPR Workshops 2022).

  reference    the score from the same fp32 detections and posterior rows.  The un-flip and the IoU are restated in numpy float32, operation
               for operation (every numpy float32 operation rounds once, to nearest even: the kernel's __f*_rn), so the match is the
               kernel's match; everything behind the match -- the Jensen-Shannon term, 1 - iou, the view mean, the aggregate -- is float64.

Bound (absolute errors, derived in the issue): with T the number of column terms of one Jensen-Shannon value (`used` for the categorical
layouts, 2 * used for sigmoid) a per-object value lies within A_obj = (4 T + 4 V + 32) * 2^-24 -- each column term carries a few ulp of
a |ln a| <= 0.37, an IoU of integer boxes is correctly rounded, V view terms; an image's max and mean within A_obj + 16 * 2^-24 (the tree
adds log2 roundings of values <= 1), its sum within `count` times that.  An entry whose float64 value is exactly 0 must be exactly 0."""
import numpy as np

VIEWS = {'hflip': 1, 'vflip': 2, 'hvflip': 3}
LAYOUTS = ('cat', 'cat_bg', 'sigmoid')
MODES = ('box', 'cls', 'both')
AGGREGATES = ('max', 'mean', 'sum')
F = np.float32


def unflip32(boxes, code, ext_w, ext_h):
    """[n, 4] float32 boxes of a view mapped back: one float32 subtraction per coordinate (mmdet's bbox_flip)"""
    b = np.array(boxes, F, copy=True).reshape(-1, 4)
    ew, eh = F(ext_w), F(ext_h)
    if code & 1:
        x1, x2 = ew - b[:, 2], ew - b[:, 0]
        b[:, 0], b[:, 2] = x1, x2
    if code & 2:
        y1, y2 = eh - b[:, 3], eh - b[:, 1]
        b[:, 1], b[:, 3] = y1, y2
    return b


def iou32(a, b):
    """float32 IoU of every row of a [m, 4] with every row of b [n, 4] -> [m, n], in the kernel's form, operation for operation: no +1, the
    union clamped at 1e-6"""
    a, b = np.asarray(a, F).reshape(-1, 4)[:, None, :], np.asarray(b, F).reshape(-1, 4)[None, :, :]
    aa = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    ab = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    iw = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), F(0))
    ih = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), F(0))
    ov = iw * ih
    un = (aa + ab) - ov
    out = ov / np.maximum(un, F(1e-6))
    assert out.dtype == F
    return out


def term64(a, b):
    """[a > 0] a (ln a - ln m) + [b > 0] b (ln b - ln m), m = (a + b) / 2, elementwise in float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = 0.5 * (a + b)
    with np.errstate(divide='ignore', invalid='ignore'):
        ta = np.where(a > 0, a * (np.log(np.where(a > 0, a, 1.0)) - np.log(np.where(a > 0, m, 1.0))), 0.0)
        tb = np.where(b > 0, b * (np.log(np.where(b > 0, b, 1.0)) - np.log(np.where(b > 0, m, 1.0))), 0.0)
    return ta + tb


def used_columns(W, layout):
    return W if layout == 'cat_bg' else W - 1


def js64(p, q, layout):
    """Jensen-Shannon divergence in bits of the fp32 posterior rows p, q [..., W] under `layout`, float64 [...]"""
    p, q = np.asarray(p), np.asarray(q)
    used = used_columns(p.shape[-1], layout)
    p, q = p[..., :used].astype(np.float64), q[..., :used].astype(np.float64)
    if layout == 'sigmoid':
        return np.sum(0.5 * (term64(p, q) + term64(1.0 - p, 1.0 - q)), axis=-1) / used / np.log(2.0)
    return 0.5 * np.sum(term64(p, q), axis=-1) / np.log(2.0)


def parts(dets, labels, num, post, views, ext, layout, score_thr=0.3, same_class=False):
    """What does not depend on mode and aggregate: dict(iou / js [V, B, max_num] float64 (NaN where the row is no object), match [V, B,
    max_num] int32 (-1 where unmatched or no object), count [B]).  The match is decided in float32; rows >= num are never read."""
    assert layout in LAYOUTS
    dets, labels, num, post, ext = np.asarray(dets), np.asarray(labels), np.asarray(num), np.asarray(post), np.asarray(ext)
    assert dets.dtype == F and post.dtype == F and ext.dtype == F
    V1, B, max_num, _ = dets.shape
    V = V1 - 1
    assert V == len(views) and 1 <= V <= 3 and len(set(views)) == V
    codes = [VIEWS[v] for v in views]
    thr = F(score_thr)
    count = np.zeros(B, np.int64)
    iou, js = np.full((V, B, max_num), np.nan), np.full((V, B, max_num), np.nan)
    match = np.full((V, B, max_num), -1, np.int32)
    for b in range(B):
        n0 = max(0, min(int(num[0, b]), max_num))
        rows = np.nonzero(dets[0, b, :n0, 4] > thr)[0]                 # rows >= num are not even sliced
        count[b] = rows.size
        if rows.size == 0:
            continue
        for v in range(V):
            nv = max(0, min(int(num[v + 1, b]), max_num))
            iou[v, b, rows], js[v, b, rows] = 0.0, 1.0
            if nv == 0:
                continue
            back = unflip32(dets[v + 1, b, :nv, :4], codes[v], ext[b, 0], ext[b, 1])
            cand = iou32(dets[0, b, rows, :4], back)                   # [rows, nv] float32
            if same_class:
                cand = np.where(labels[0, b, rows][:, None] == labels[v + 1, b, :nv][None, :], cand, F(0))
            cand = np.where(cand > 0, cand, F(0))                      # (a NaN is never larger: the kernel's `iou > m`)
            k = np.argmax(cand, axis=1)                                # the lowest index of the maximum
            m = cand[np.arange(rows.size), k]
            hit = m > 0
            iou[v, b, rows[hit]] = m[hit].astype(np.float64)
            match[v, b, rows[hit]] = k[hit]
            if hit.any():
                js[v, b, rows[hit]] = js64(post[0, b, rows[hit]], post[v + 1, b, k[hit]], layout)
    return dict(iou=iou, js=js, match=match, count=count)


def combine(pt, mode='both', aggregate='max'):
    """parts -> dict(unc [B], obj [B, max_num] (NaN where the row is no object), iou, js, match, count) in float64"""
    assert mode in MODES and aggregate in AGGREGATES
    iou, js = pt['iou'], pt['js']
    V, B, max_num = iou.shape
    u = {'box': 1.0 - iou, 'cls': js, 'both': 0.5 * ((1.0 - iou) + js)}[mode]
    obj = u[0].copy()
    for v in range(1, V):
        obj = obj + u[v]                                               # the views in order
    obj = obj / V
    unc = np.zeros(B)
    for b in range(B):
        vals = obj[b][np.isfinite(obj[b])]
        if vals.size:
            unc[b] = {'max': max(0.0, float(vals.max())), 'mean': float(vals.sum()) / vals.size, 'sum': float(vals.sum())}[aggregate]
    return dict(pt, unc=unc, obj=obj)


def reference(dets, labels, num, post, views, ext, layout, mode='both', aggregate='max', score_thr=0.3, same_class=False):
    """dets [V+1, B, max_num, 5] fp32, labels [V+1, B, max_num] int64, num [V+1, B], post [V+1, B, max_num, W] fp32, views: V names,
    ext [B, 2] fp32 (w, h) -> dict(unc [B], obj [B, max_num], iou / js [V, B, max_num] (NaN where the row is no object), match [V, B,
    max_num] int32 (-1 where unmatched or no object), count [B]); float64 but for the match."""
    return combine(parts(dets, labels, num, post, views, ext, layout, score_thr, same_class), mode, aggregate)


def bound_obj(W, layout, V):
    T = used_columns(W, layout) * (2 if layout == 'sigmoid' else 1)
    return (4 * T + 4 * V + 32) * 2.0 ** -24


def bound_unc(W, layout, V, aggregate, count):
    """[B]: the bound of the image score for `count` [B] objects"""
    per = bound_obj(W, layout, V) + 16 * 2.0 ** -24
    count = np.asarray(count, np.float64)
    return per * count if aggregate == 'sum' else np.full(count.shape, per)


def fraction_of_bound(got, want, bound):
    """max over the finite entries of |got - want| / bound (bound: a scalar or an array of want's shape); entries whose float64 value is
    exactly 0 must be exactly 0 (inf else)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    keep = np.isfinite(want)
    got, want, bound = got[keep], want[keep], bound[keep]
    if got.size == 0:
        return 0.0
    zero = want == 0
    worst = np.inf if (got[zero] != 0).any() else 0.0
    if (~zero).any():
        err = np.abs(got[~zero] - want[~zero])
        if not np.isfinite(err).all() or (bound[~zero] <= 0).any():
            return np.inf
        worst = max(worst, float((err / bound[~zero]).max()))
    return worst
