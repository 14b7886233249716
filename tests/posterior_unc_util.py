"""Shared by tests/test_posterior_unc_host.py and tests/test_gpu_posterior_unc.py: the numpy float64 restatement of the posterior
uncertainty pools -- lookup of a detection's score row by its box and score bits, the object gate, three row layouts x three
measures x three aggregates -- evaluated on the fp32 tensors the device path produced, the seeded input maker of the kernel tests, and the
tolerances the issue derives.

Tolerances: every entropy term is non-negative and carries a few ulp of relative error (logf / log1pf, one product), so a sum of up to
96 terms and up to 100 objects stays within ~1e-5 relative: entropy values and every sum / mean aggregate rtol 2e-5, atol 1e-7 (the loss
rows' tolerances); margin / least confidence per object and their max are two fp32 roundings of values <= 1: atol 4 * 2^-24."""
import numpy as np
import torch

LAYOUTS = ('cat', 'cat_bg', 'sigmoid')
MEASURES = ('entropy', 'margin', 'leastconf')
AGGREGATES = ('max', 'mean', 'sum')
RTOL, ATOL = 2e-5, 1e-7
ATOL_CONF = 4 * 2.0 ** -24
A = 9
LEVELS = ((8, 8), (4, 4), (2, 2), (1, 1), (1, 1))          # 64 x 64 images, strides 8 .. 128: 1 152 / 288 / 72 / 18 / 18 rows for two images
NMS_PRE = 100


def used_columns(W, layout):
    return W if layout == 'cat_bg' else W - 1


def _xlogx(p):
    p = np.asarray(p, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(p > 0, -p * np.log(np.where(p > 0, p, 1.0)), 0.0)


def measure64(s, layout, measure):
    """the measure of score rows s [..., used] (float64 evaluation of fp32 values): [...]"""
    s = np.asarray(s, np.float64)
    if measure == 'entropy':
        h = _xlogx(s)
        if layout == 'sigmoid':
            h = h + _xlogx(1.0 - s)
        return h.sum(-1)
    top = np.sort(s, axis=-1)
    if measure == 'margin':
        if s.shape[-1] < 2:
            raise ValueError('margin needs two used columns')
        return 1.0 - (top[..., -1] - top[..., -2])
    if measure == 'leastconf':
        return 1.0 - top[..., -1]
    raise ValueError(measure)


def _u32(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def lookup(boxes, scores, dets, labels, num, thr):
    """rows [B, max_num] int64: the candidate row of every object (lowest index whose box and score at the label match bit for bit), -1 for
    a row that is no object, -2 for an object without a candidate row.  Rows j >= num[b] are never read."""
    bb, ss, dd = _u32(boxes), _u32(scores), _u32(dets)
    dets, labels, num = np.asarray(dets, np.float32), np.asarray(labels), np.asarray(num)
    B, max_num = dets.shape[:2]
    W = ss.shape[2]
    rows = np.full((B, max_num), -1, np.int64)
    for b in range(B):
        for j in range(min(int(num[b]), max_num)):
            if not dets[b, j, 4] > np.float32(thr):
                continue
            lab = int(labels[b, j])
            rows[b, j] = -2
            if not 0 <= lab < W:
                continue
            hit = np.nonzero((bb[b] == dd[b, j, :4]).all(-1) & (ss[b, :, lab] == dd[b, j, 4]))[0]
            if len(hit):
                rows[b, j] = hit[0]
    return rows


def reference(boxes, scores, dets, labels, num, layout, measure='entropy', aggregate='max', thr=0.3):
    """dict(unc [B] float64, obj [B, max_num] float64 (NaN where the row is no object), missing [B] int, rows [B, max_num], count [B])"""
    scores = np.asarray(scores, np.float32)
    rows = lookup(boxes, scores, dets, labels, num, thr)
    B, max_num = rows.shape
    used = used_columns(scores.shape[2], layout)
    obj = np.full((B, max_num), np.nan)
    unc, missing, count = np.zeros(B), np.zeros(B, np.int64), np.zeros(B, np.int64)
    for b in range(B):
        j = np.nonzero(rows[b] >= 0)[0]
        missing[b] = int((rows[b] == -2).sum())
        count[b] = len(j)
        if len(j):
            v = measure64(scores[b, rows[b, j], :used], layout, measure)
            obj[b, j] = v
            unc[b] = dict(max=v.max(), mean=v.sum() / len(j), sum=v.sum())[aggregate]
    return dict(unc=unc, obj=obj, missing=missing, rows=rows, count=count)


def tolerances(measure, aggregate):
    """((rtol, atol) of the per-object values, (rtol, atol) of the image score)"""
    per_obj = (RTOL, ATOL) if measure == 'entropy' else (0.0, ATOL_CONF)
    return per_obj, ((RTOL, ATOL) if measure == 'entropy' or aggregate != 'max' else (0.0, ATOL_CONF))


def close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.isnan(got) == np.isnan(want)).all() and (np.abs(got - want)[~np.isnan(want)] <= tol[1] + tol[0] * np.abs(want[~np.isnan(want)])).all())


# ---------------------------------------------------------------------------------------------------------------- inputs
PUSHED = ((0, 5), (0, 130), (0, 262), (0, 401), (0, 533), (1, 10), (1, 97), (2, 20))     # (level, row): spread over the map, distinct anchors


def make_maps(B, C_, seed, quiet_scale=0.1, sigmoid=False, has_bg=False):
    """(cls maps, box maps): per level [B, A*C_, h, w] / [B, A*4, h, w] float32.  Logits lie in [-5, 5]: softmax rows are uniform in
    [-5, 5] times a per-row factor in [0.2, 1] (row maxima on both sides of 0.3), sigmoid rows uniform in [-5, -1] (scores below 0.27: the
    NMS kernel keeps them, the object gate does not) -- so a detection list mixes objects and rows below the gate.  In every image but
    the last, the PUSHED rows are made confident -- uniform in [-5, -2] with one class (a different one per row and image) at 5 - small
    and a runner-up at 3 - small -- so that they survive the top-k and the NMS as objects; the LAST image is quiet (no object): its logits
    are quiet_scale * uniform[-5, 5] (softmax rows: near-uniform posteriors) or, for sigmoid rows, uniform in [-3, -1.5] (scores below 0.19)."""
    g = np.random.default_rng(seed)
    n_fg = C_ - 1 if has_bg else C_                            # (SSD rows: the last column is background, never the pushed class)
    cls, reg = [], []
    for l, (h, w) in enumerate(LEVELS):
        n = h * w * A
        rows = g.uniform(-5, -1, (B, n, C_)) if sigmoid else g.uniform(-5, 5, (B, n, C_)) * g.uniform(0.2, 1.0, (B, n, 1))
        rows[B - 1] = g.uniform(-3, -1.5, rows[B - 1].shape) if sigmoid else quiet_scale * rows[B - 1]
        for b in range(B - 1):
            for i, (lv, r) in enumerate(PUSHED):
                if lv != l:
                    continue
                row = g.uniform(-5, -2, C_)
                c = (3 * i + 7 * b) % n_fg
                row[c] = 5 - g.uniform(0, 0.5)
                row[(c + 1) % n_fg] = 3 - g.uniform(0, 0.5)
                rows[b, r] = row
        assert np.abs(rows).max() <= 5
        cls.append(torch.from_numpy(rows.astype(np.float32)).view(B, h, w, A * C_).permute(0, 3, 1, 2).contiguous())
        reg.append(torch.from_numpy((0.1 * g.standard_normal((B, A * 4, h, w))).astype(np.float32)))
    return cls, reg


def check_case(boxes, scores, dets, labels, num, thr):
    """the properties the kernel tests rely on, asserted on host copies of the device path's tensors: no two candidates of an image share
    (box, score at any class) bits; at least one image has >= 2 objects; every image but the last has an object, the last has none"""
    bb, ss = _u32(boxes), _u32(scores)[:, :, :-1]          # the columns a label can name (the last one is the zero pad / the background)
    B = bb.shape[0]
    for b in range(B):
        _, inv, cnt = np.unique(bb[b], axis=0, return_inverse=True, return_counts=True)
        for grp in np.nonzero(cnt > 1)[0]:
            k = np.nonzero(inv.reshape(-1) == grp)[0]
            for i in range(len(k)):
                for j in range(i + 1, len(k)):
                    assert not (ss[b, k[i]] == ss[b, k[j]]).any(), (b, k[i], k[j])
    rows = lookup(boxes, scores, dets, labels, num, thr)
    n_obj = (rows >= 0).sum(1)
    assert (rows != -2).all()
    assert n_obj.max() >= 2 and (n_obj[:-1] >= 1).all() and n_obj[-1] == 0, n_obj
    return n_obj
