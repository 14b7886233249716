"""Float64 numpy restatements of the CCMS acquisition the tests compare the kernels against: the object descriptors of an
image, the directed category-conditioned matching similarity and the distance built from it, and the exact k-center greedy on a given
distance matrix with the lowest-index tie-break."""
import numpy as np

from tests.coreset_util import greedy


def object_descriptors_float64(levels, num_anchors, cand_anchor, dets, labels, num, obj_cand, max_obj, score_thr):
    """levels: per-level float64 values [B, h * w, C] of the neck outputs; num_anchors: anchors per cell of every level; cand_anchor [B, n],
    dets [B, max_num, 5] fp32, labels [B, max_num], num [B], obj_cand [B, max_num].  The objects of image b: rows j < num[b] with a score
    > score_thr (compared in fp32, strict) in row order; one without a candidate row (obj_cand outside [0, n) or an anchor outside every
    level) is skipped and counted in missing; the first max_obj of the others are kept.
    -> feat [B, max_obj, C] float64, cls [B, max_obj] (-1 pad), w [B, max_obj] float64 (0 pad), cnt [B], missing [B]"""
    B, C = levels[0].shape[0], levels[0].shape[2]
    n = cand_anchor.shape[1]
    a0 = np.concatenate([[0], np.cumsum([lv.shape[1] * na for lv, na in zip(levels, num_anchors)])])
    feat = np.zeros((B, max_obj, C))
    cls = np.full((B, max_obj), -1, np.int64)
    w = np.zeros((B, max_obj))
    cnt, missing = np.zeros(B, np.int64), np.zeros(B, np.int64)
    thr = np.float32(score_thr)
    for b in range(B):
        for j in range(min(max(int(num[b]), 0), dets.shape[1])):
            if not np.float32(dets[b, j, 4]) > thr:
                continue
            k = int(obj_cand[b, j])
            level = None
            if 0 <= k < n:
                g = int(cand_anchor[b, k])
                for l in range(len(levels)):
                    if a0[l] <= g < a0[l + 1]:
                        level, cell = l, (g - a0[l]) // num_anchors[l]
            if level is None:
                missing[b] += 1
                continue
            if cnt[b] == max_obj:
                continue
            v = np.asarray(levels[level][b, cell], np.float64)
            ss = float((v * v).sum())
            s = cnt[b]
            feat[b, s] = v / np.sqrt(ss) if ss > 0 else 0.0
            cls[b, s], w[b, s] = int(labels[b, j]), float(dets[b, j, 4])
            cnt[b] += 1
    return feat, cls, w, cnt, missing


def directed_similarity(fa, ca, wa, fb, cb):
    """S(a -> b) = sum_i w_i m_i / sum_i w_i over a's objects, m_i = max(0, max over b's objects j of the same class of <f_i, f_j>)
    (0 if b has none); 0 if a has no object.  fa [na, C], ca [na], wa [na]; fb [nb, C], cb [nb] -- the objects only, no padding."""
    fa, fb, wa = np.asarray(fa, np.float64), np.asarray(fb, np.float64), np.asarray(wa, np.float64)
    if len(ca) == 0:
        return 0.0
    num = 0.0
    for i in range(len(ca)):
        same = [j for j in range(len(cb)) if cb[j] == ca[i]]
        m = max([0.0] + [float(fa[i] @ fb[j]) for j in same])
        num += wa[i] * m
    return num / float(wa.sum())


def distance_matrix(feat, cls, w, cnt):
    """d(a, b) = max(0, 1 - (S(a -> b) + S(b -> a)) / 2) for a != b, d(a, a) = 0, from the padded [M, max_obj, ...] arrays -> [M, M] float64"""
    M = feat.shape[0]
    obj = [(feat[a, :cnt[a]], cls[a, :cnt[a]], w[a, :cnt[a]]) for a in range(M)]
    D = np.zeros((M, M))
    for a in range(M):
        for b in range(a + 1, M):
            s = directed_similarity(*obj[a], obj[b][0], obj[b][1]) + directed_similarity(*obj[b], obj[a][0], obj[a][1])
            D[a, b] = D[b, a] = max(0.0, 1.0 - s / 2.0)
    return D


def greedy_matrix(D, labelled, budget):
    """k-center greedy on a distance matrix, in D's dtype: mind = min over the labelled rows of D[c] (+inf without one), labelled rows
    selected; each step picks the unselected row with the largest mind -- np.argmax returns the LOWEST index of a tie --, records that mind
    as the radius, selects the row and lowers every mind to D[pick].  Returns (picks [budget] int64, radius [budget], ties) with ties = the
    number of steps at which more than one unselected row held the maximum."""
    D = np.asarray(D)
    return greedy(D, labelled, budget, dtype=D.dtype, dist=lambda D, c: D[c])
