"""Shared by tests/test_loc_stability_host.py and tests/test_gpu_loc_stability.py: the float64 restatements of the localization-stability
pool (Kao, Lee, Sen, Liu, ACCV 2018).

  noise_z64 / noisy64     the pixel noise of aod_pixel_noise from oracle.hua.philox4x32 / _u01 (imported, not edited): z is element x & 3 of
                          the four Box-Muller normals of the Philox block at counter ((y << 16) | (x >> 2), 0x80000000 | (level << 8) | c,
                          id & 0xffffffff, id >> 32) under key (seed & 0xffffffff, seed >> 32)
  reference               the stability score in float64 from the same fp32 detections

Tolerance of the score (derived in the issue): relative (max_num + K + 32) * 2^-23 -- a sum of at most max_num non-negative weighted
terms, K non-negative level terms, at most 16 roundings inside one IoU."""
import numpy as np

from oracle.hua import _u01, philox4x32

COMBINES = ('ls', 'ls+c')
SIGMAS = (8, 16, 24, 32, 40, 48)


def noise_z64(seed, level, image_id, c, H, W):
    """float64 [H, W]: z of channel c of the image with global id `image_id` at noise level `level`, for every (y, x) of an H x W window
    (the values do not depend on the padded size)"""
    y = np.arange(H, dtype=np.uint32)[:, None]
    xq = np.arange((W + 3) // 4, dtype=np.uint32)[None, :]
    c0 = (y << np.uint32(16)) | xq
    c1 = np.uint32(0x80000000 | (int(level) << 8) | int(c))
    r = philox4x32(c0, c1, np.uint32(image_id & 0xffffffff), np.uint32((image_id >> 32) & 0xffffffff), seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    u = [_u01(x).astype(np.float64) for x in r]
    ra, rb = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    quad = np.stack([ra * np.cos(2 * np.pi * u[1]), ra * np.sin(2 * np.pi * u[1]), rb * np.cos(2 * np.pi * u[3]), rb * np.sin(2 * np.pi * u[3])], -1)
    return quad.reshape(H, -1)[:, :W]


def noisy64(src, hw, std, sigma, level, seed, image_ids):
    """float64 [B, C, Hp, Wp]: src + (sigma / std_c) z inside every image's (h, w), src itself outside; `live` marks the noisy pixels"""
    src = np.asarray(src)
    B, C, Hp, Wp = src.shape
    out = src.astype(np.float64)
    live = np.zeros(src.shape, bool)
    for b in range(B):
        h, w = int(hw[b][0]), int(hw[b][1])
        for c in range(C):
            out[b, c, :h, :w] += (float(sigma) / float(std[c])) * noise_z64(seed, level, int(image_ids[b]), c, h, w)
            live[b, c, :h, :w] = True
    return out, live


def iou64(a, b):
    """float64 IoU of fp32 boxes in the kernel's form: no +1, the union clamped at 1e-6"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    ov = iw * ih
    un = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - ov
    return ov / max(un, 1e-6)


def iou_matrix64(a, b):
    """iou64 of every row of a [n, 4] with every row of b [m, 4] (float64 in, float64 out)"""
    iw = np.maximum(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0.0)
    ih = np.maximum(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0.0)
    ov = iw * ih
    un = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] + ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :] - ov
    return ov / np.maximum(un, 1e-6)


def reference(dets, labels, num, score_thr=0.3, same_class=False, combine='ls'):
    """dets [K+1, B, max_num, 5] fp32, labels [K+1, B, max_num] int64, num [K+1, B] -> dict(unc [B], stab [B, max_num] (NaN where the row is
    no object), count [B]) in float64.  Rows >= num are never read."""
    assert combine in COMBINES
    dets, labels, num = np.asarray(dets), np.asarray(labels), np.asarray(num)
    assert dets.dtype == np.float32
    K1, B, max_num, _ = dets.shape
    K = K1 - 1
    thr = np.float32(score_thr)
    unc, stab, count = np.zeros(B), np.full((B, max_num), np.nan), np.zeros(B, np.int64)
    for b in range(B):
        n0 = min(int(num[0, b]), max_num)
        rows = np.nonzero(dets[0, b, :n0, 4] > thr)[0]                 # rows >= num are not even sliced
        if rows.size == 0:
            continue
        a = dets[0, b, rows, :4].astype(np.float64)
        w = dets[0, b, rows, 4].astype(np.float64)
        s = np.zeros(rows.size)
        for k in range(K):
            nk = min(int(num[k + 1, b]), max_num)
            m = np.zeros(rows.size)
            if nk:
                m = iou_matrix64(a, dets[k + 1, b, :nk, :4].astype(np.float64))
                if same_class:
                    m = np.where(labels[0, b, rows][:, None] == labels[k + 1, b, :nk][None, :], m, 0.0)
                m = m.max(1)
            s = s + m                                                  # the levels in order
        s = s / K
        stab[b, rows] = s
        count[b] = rows.size
        unc[b] = 1.0 - float(np.sum(w * s)) / float(np.sum(w))
        if combine == 'ls+c':
            unc[b] += 1.0 - float(w.max())
    return dict(unc=unc, stab=stab, count=count)


def bound(max_num, K):
    return (max_num + K + 32) * 2.0 ** -23


def fraction_of_bound(got, want, max_num, K):
    """max over the finite entries of |got - want| / (bound * |want|); entries whose float64 value is exactly 0 must be exactly 0 (inf else)"""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    keep = np.isfinite(want)
    got, want = got[keep], want[keep]
    if got.size == 0:
        return 0.0
    zero = want == 0
    worst = np.inf if (got[zero] != 0).any() else 0.0
    if (~zero).any():
        worst = max(worst, float((np.abs(got[~zero] - want[~zero]) / (bound(max_num, K) * np.abs(want[~zero]))).max()))
    return worst
