"""Float64 restatements of the ENMS + DivProto acquisition: the entropy-NMS of one image, its class prototypes and the
progressive selection, each with the list of its *ambiguous* decisions -- a product within DOT_EPS of the threshold it is compared with, or
two measures of one image closer than H_EPS relative that are not bit-equal (bit-equal values are a defined tie: the lowest index wins).
A test asserts that this list is empty for its seeds: then the fp32 device path has to take the same decisions exactly."""
import math

import numpy as np

DOT_EPS = 1e-5
H_EPS = 1e-6
U32 = 2.0 ** -24          # unit roundoff of fp32


def _f32(x):
    return float(np.float32(x))


def enms_float64(feat, cls, h, cnt, t_enms=0.5):
    """one image: feat [K, C], cls [K], h [K] (fp32 values), cnt.  Returns (E, kept, picks, ambiguous)."""
    n = int(cnt)
    f = np.asarray(feat, np.float64)[:n]
    c = np.asarray(cls)[:n]
    hv = np.asarray(h, np.float32)[:n]
    thr = _f32(t_enms)
    amb = []
    for i in range(n):
        for j in range(i + 1, n):
            a, b = float(hv[i]), float(hv[j])
            if hv[i].tobytes() != hv[j].tobytes() and abs(a - b) < H_EPS * max(abs(a), abs(b)):
                amb.append(('h', i, j, a, b))
    alive = np.ones(n, bool)
    E, picks = 0.0, []
    while alive.any():
        idx = np.nonzero(alive)[0]
        k = int(idx[np.argmax(hv[idx].astype(np.float64))])           # (argmax: the first, so the lowest index, of equal values)
        E += float(hv[k])
        picks.append(k)
        alive[k] = False
        for j in np.nonzero(alive)[0]:
            if c[j] == c[k]:
                d = float(f[j] @ f[k])
                if thr < 1 and abs(d - thr) <= DOT_EPS:
                    amb.append(('dot', k, int(j), d))
                if thr < 1 and d > thr:                               # (a threshold >= 1 switches the suppression off: a cosine cannot exceed 1)
                    alive[j] = False
    return E, len(picks), picks, amb


def prototypes_float64(feat, cls, w, h, cnt):
    """one image -> (proto [K, C] float64, pcls [K] int32 (-1 pad), pconf [K] float32 (0 pad), pcnt, bound [K, C]): bound is the fp32
    error bound of every prototype element, from the operation count alone (see proto_bound)"""
    K, C = np.asarray(feat).shape
    n = int(cnt)
    f = np.asarray(feat, np.float64)[:n]
    c = np.asarray(cls)[:n]
    hv = np.asarray(h, np.float32)[:n].astype(np.float64)
    wv = np.asarray(w, np.float32)[:n]
    proto = np.zeros((K, C))
    bound = np.zeros((K, C))
    pcls = np.full(K, -1, np.int32)
    pconf = np.zeros(K, np.float32)
    classes = sorted(set(int(v) for v in c))
    for r, cc in enumerate(classes):
        ks = [k for k in range(n) if c[k] == cc]
        wt = np.array([hv[k] + 2.0 ** -10 for k in ks])
        v = (wt[:, None] * f[ks]).sum(axis=0)
        A = (np.abs(wt)[:, None] * np.abs(f[ks])).sum(axis=0)
        nv = math.sqrt(float(v @ v))
        proto[r] = v / nv if nv > 0 else 0.0
        bound[r] = proto_bound(len(ks), C, A, proto[r], nv)
        pcls[r] = cc
        pconf[r] = wv[ks].max()
    return proto, pcls, pconf, len(classes), bound


def proto_bound(n, C, A, p, nv):
    """|device - float64| per element of p = v / ||v||, v = sum of n terms (h_k + 2^-10) f_k, all in fp32 with unit roundoff u = 2^-24:
    every term takes one rounding for the weight and one for the product, the running sum at most n - 1 more: |dv| <= (n + 1) u A with
    A = sum |w_k f_k| (elementwise); ||v|| from C squares (one rounding each, C - 1 additions in any order: relative (C + 1) u / 2 after the
    square root, plus the root's own rounding) inherits ||dv|| <= (n + 1) u ||A||; the division adds one rounding.  To first order
      |dp| <= (n + 1) u (A + |p| ||A||) / ||v|| + (C / 2 + 3) u |p|;  a factor 1.01 covers the second-order terms (n, C <= 256)."""
    if nv == 0:
        return np.zeros_like(A)
    return 1.01 * ((n + 1) * U32 * (A + np.abs(p) * math.sqrt(float(A @ A))) / nv + (C / 2 + 3) * U32 * np.abs(p))


def quotas(n_cls, budget, alpha=0.5, beta=0.75):
    n_minor = int(math.ceil(alpha * n_cls))
    reserved = min(budget, int(math.ceil(beta * budget)))
    return n_minor, -(-reserved // n_minor), budget - reserved


def select_float64(order, proto, pcls, pconf, pcnt, n_cls, budget, t_intra=0.7, t_inter=0.3, alpha=0.5, beta=0.75, class_balance=True):
    """the progressive selection over the sweep `order` (pool indices) -> (picks [budget] int64, stage [budget] int32, ambiguous)"""
    order = [int(i) for i in order]
    n_minor, quota, free = quotas(n_cls, budget, alpha, beta)
    ti, te = _f32(t_intra), np.float32(t_inter)
    P = np.asarray(proto, np.float64)
    lists = {c: [] for c in range(n_cls)}
    n_c = [0] * n_cls
    free_used = 0
    picks, stage, deferred, redundant, amb = [], [], [], [], []
    for I in order:
        if len(picks) == budget:
            break
        slots = [(s, int(pcls[I, s])) for s in range(int(pcnt[I])) if 0 <= int(pcls[I, s]) < n_cls]
        if slots:
            m = min(max((float(P[I, s] @ P[J, sj]) for J, sj in lists[c]), default=0.0) for s, c in slots)
            if ti < 1 and abs(m - ti) <= DOT_EPS:
                amb.append(('intra', I, m))
            if ti < 1 and m > ti:                                     # (likewise: t_intra >= 1 makes no image redundant)
                redundant.append(I)
                continue
        st = 1
        if class_balance:
            serves = False
            for s, c in slots:
                rank = sum(1 for cc in range(n_cls) if n_c[cc] < n_c[c] or (n_c[cc] == n_c[c] and cc < c))
                if rank < n_minor and np.float32(pconf[I, s]) > te and n_c[c] < quota:
                    serves = True
            if not serves:
                if free_used < free:
                    free_used += 1
                    st = 2
                else:
                    deferred.append(I)
                    continue
        picks.append(I)
        stage.append(st)
        for s, c in slots:
            lists[c].append((I, s))
            if np.float32(pconf[I, s]) > te:
                n_c[c] += 1
    for I in deferred + redundant:
        if len(picks) == budget:
            break
        picks.append(I)
        stage.append(3)
    assert len(picks) == budget, (len(picks), budget)
    return np.array(picks, np.int64), np.array(stage, np.int32), amb


def sweep_order(enms, X_L):
    """the unlabelled images by enms descending, ties by ascending index"""
    u = np.asarray(enms, np.float64)
    idx = np.array([i for i in range(u.size) if i not in set(int(v) for v in X_L)], np.int64)
    return idx[np.argsort(-u[idx], kind='stable')]


# ------------------------------------------------------------------------------------------------------------------ planted inputs
def centres(g, C, groups):
    """`groups` orthonormal rows of C columns"""
    q, _ = np.linalg.qr(g.standard_normal((C, groups)))
    return q.T


def planted_rows(g, cen, group):
    """unit rows: the centre of each row's group plus 0.25 * N(0, 1 / C) noise, renormalised, rounded to fp32"""
    C = cen.shape[1]
    v = cen[np.asarray(group)] + 0.25 * g.standard_normal((len(group), C)) / math.sqrt(C)
    return (v / np.sqrt((v * v).sum(axis=1, keepdims=True))).astype(np.float32)


def planted_images(seed, B, K, C, groups, n_cls, cnt=None):
    """B images of up to K objects: random classes and groups, features planted_rows, h in (0.05, 2), w in (0.31, 1).  Pad rows hold NaN
    features, a valid-looking class and non-zero h / w: none of them may be read."""
    g = np.random.default_rng(seed)
    cen = centres(g, C, groups)
    cnt = g.integers(0, K + 1, B).astype(np.int32) if cnt is None else np.asarray(cnt, np.int32)
    feat = np.full((B, K, C), np.nan, np.float32)
    cls = np.ones((B, K), np.int32)
    h = np.full((B, K), 9.0, np.float32)
    w = np.full((B, K), 5.0, np.float32)
    for b in range(B):
        n = int(cnt[b])
        feat[b, :n] = planted_rows(g, cen, g.integers(0, groups, n))
        cls[b, :n] = g.integers(0, n_cls, n)
        h[b, :n] = g.uniform(0.05, 2.0, n)
        w[b, :n] = g.uniform(0.31, 1.0, n)
    return feat, cls, w, h, cnt


def planted_pool(seed, N, K, C, groups, n_cls, empty=()):
    """pool tensors for the selection: per image up to min(K, n_cls) distinct classes, each prototype a planted row of one group (so that
    two prototypes of a class have a cosine near 0.94 or near 0), conf in (0.05, 1); images in `empty` have no class"""
    g = np.random.default_rng(seed)
    cen = centres(g, C, groups)
    proto = np.zeros((N, K, C), np.float32)
    pcls = np.full((N, K), -1, np.int32)
    pconf = np.zeros((N, K), np.float32)
    pcnt = np.zeros(N, np.int32)
    for i in range(N):
        if i in empty:
            continue
        n = int(g.integers(1, min(K, n_cls) + 1))
        cs = np.sort(g.choice(n_cls, n, replace=False))
        proto[i, :n] = planted_rows(g, cen, g.integers(0, groups, n))
        pcls[i, :n] = cs
        pconf[i, :n] = g.uniform(0.05, 1.0, n)
        pcnt[i] = n
    return proto, pcls, pconf, pcnt


# ------------------------------------------------------------------------------------------------------------------ hand cases
def unit_at(cos, axis, C=8):
    """the fp32 unit vector cos * e_0 + sqrt(1 - cos^2) * e_axis"""
    v = np.zeros(C)
    v[0] = cos
    v[axis] += math.sqrt(1.0 - cos * cos)
    return v.astype(np.float32)


def hand_enms_case(K=4, C=8):
    """four objects, classes (0, 0, 1, 0), h = (0.5, 0.7, 0.7, 0.2): objects 1 and 2 tie bit for bit -> 1 first; it suppresses 0 (same
    class, cosine 0.9) but not 3 (cosine 0) nor 2 (another class, though its feature equals object 0's).  Picks 1, 2, 3; kept 3;
    E = 0.7 + 0.7 + 0.2."""
    feat = np.zeros((K, C), np.float32)
    feat[0] = unit_at(1.0, 1, C)
    feat[1] = unit_at(0.9, 1, C)
    feat[2] = unit_at(1.0, 1, C)
    feat[3] = np.eye(C, dtype=np.float32)[3]
    return dict(feat=feat, cls=np.array([0, 0, 1, 0], np.int32), h=np.array([0.5, 0.7, 0.7, 0.2], np.float32),
                w=np.array([0.9, 0.8, 0.6, 0.4], np.float32), cnt=4, picks=[1, 2, 3], kept=3,
                E=float(np.float32(0.7)) * 2 + float(np.float32(0.2)))


def hand_pool(C=8, K=2):
    """seven images, three classes, swept in index order; a = e_0, a9 / a5 at cosine 0.9 / 0.5 to it, z = e_3 at cosine 0.
      0: class 0 (a)            1: class 0 (a9)          2: class 0 (a5)        3: class 0 (z)
      4: class 0 (a), class 1 (e_1, conf 0.2)            5: class 1 (e_1)       6: no class
    every other conf 0.9.  With n_cls = 3, alpha = 0.5 (n_minor 2), beta = 0.75:
      0 serves class 0 (stage 1; then the minor classes are 1, 2); 1 is redundant (0.9 > 0.7); 2 passes (0.5), serves nothing and takes
      the one free slot when there is one (stage 2), else is deferred; 3 passes (0), deferred; 4 passes (class 1 has no entry: min(1, 0)
      = 0), its minor class 1 has conf 0.2 <= 0.3: deferred; 5 serves class 1 (stage 1); 6 has no class: passes, deferred.
      budget 7 (free 1): picks 0 2 5 | 3 4 6 | 1, stages 1 2 1 3 3 3 3      -- both fill tiers
      budget 4 (free 1): picks 0 2 5 | 3,         stages 1 2 1 3
      budget 2 (free 0): picks 0 5,               stages 1 1                 (2 is deferred: no free slot)"""
    e = np.eye(C, dtype=np.float32)
    proto = np.zeros((7, K, C), np.float32)
    pcls = np.full((7, K), -1, np.int32)
    pconf = np.zeros((7, K), np.float32)
    pcnt = np.array([1, 1, 1, 1, 2, 1, 0], np.int32)
    for i, v in enumerate((e[0], unit_at(0.9, 1, C), unit_at(0.5, 2, C), e[3], e[0])):
        proto[i, 0], pcls[i, 0], pconf[i, 0] = v, 0, 0.9
    proto[4, 1], pcls[4, 1], pconf[4, 1] = e[1], 1, 0.2
    proto[5, 0], pcls[5, 0], pconf[5, 0] = e[1], 1, 0.9
    answers = {7: ([0, 2, 5, 3, 4, 6, 1], [1, 2, 1, 3, 3, 3, 3]), 4: ([0, 2, 5, 3], [1, 2, 1, 3]), 2: ([0, 5], [1, 1])}
    return dict(proto=proto, pcls=pcls, pconf=pconf, pcnt=pcnt, n_cls=3, answers=answers)
