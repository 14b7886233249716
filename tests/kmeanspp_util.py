"""float64 restatements for the BADGE tests, written for the tests: the gradient embedding with its rounding bound, the slot rule
of the posterior rows, the k-means++ seeding in the association DESIGN 3t fixes, and the replay checker for float descriptors."""
import numpy as np

U24 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- embedding
def embedding_float64(feat, post, cls, cnt, n_cls):
    """G [B, n_cls * Cf] float64 and the per-entry bound (K + 2) * 2^-24 * sum_o |a_o[c]| |f_o[j]|, K = the slots per image: the standard
    K-term dot-product bound (one rounding for a = post - 1, one for the product, at most K - 1 for the running sum, second order in the 2)"""
    feat, post = np.asarray(feat, np.float64), np.asarray(post, np.float64)
    B, K, Cf = feat.shape
    G = np.zeros((B, n_cls, Cf))
    bound = np.zeros((B, n_cls, Cf))
    for b in range(B):
        n = int(cnt[b])
        if n == 0:
            continue
        a = post[b, :n, :n_cls].copy()
        for o in range(n):
            if 0 <= cls[b, o] < n_cls:
                a[o, cls[b, o]] -= 1.0
        G[b] = a.T @ feat[b, :n]
        bound[b] = (K + 2) * U24 * (np.abs(a).T @ np.abs(feat[b, :n]))
    return G.reshape(B, -1), bound.reshape(B, -1)


def dyadic_objects(seed, B, K, Cf, W, n_cls, cnt=None):
    """objects whose embedding sums are exact in fp32: post in multiples of 1/16 within [0, 1], feat in multiples of 1/8 within [-1, 1]:
    a product is a multiple of 2^-7 below 2, a sum of <= 64 of them a multiple of 2^-7 below 2^7 -- 14 bits"""
    g = np.random.default_rng(seed)
    feat = (g.integers(-8, 9, (B, K, Cf)) / 8).astype(np.float32)
    post = (g.integers(0, 17, (B, K, W)) / 16).astype(np.float32)
    cls = g.integers(0, n_cls, (B, K)).astype(np.int32)
    cnt = np.asarray(g.integers(0, K + 1, B) if cnt is None else cnt, np.int32)
    return feat, post, cls, cnt


def float_objects(seed, B, K, Cf, W, n_cls, cnt=None):
    g = np.random.default_rng(seed)
    feat = g.standard_normal((B, K, Cf)).astype(np.float32)
    feat /= np.linalg.norm(feat, axis=2, keepdims=True)
    post = g.dirichlet(np.ones(W), (B, K)).astype(np.float32)
    cls = g.integers(0, n_cls, (B, K)).astype(np.int32)
    cnt = np.asarray(g.integers(1, K + 1, B) if cnt is None else cnt, np.int32)
    return feat, post, cls, cnt


# ---------------------------------------------------------------------------------------------------------------- posterior slots
def posterior_slots(scores, dets, num, obj_cand, K, thr):
    """post [B, K, W]: scores[b, obj_cand[b, j]] at the rows j < num[b] with dets[b, j, 4] > thr (strict) that have a candidate row, the first
    K in row order; zero rows behind them.  Also cnt [B]."""
    B, n, W = scores.shape
    post = np.zeros((B, K, W), np.float32)
    cnt = np.zeros(B, np.int32)
    for b in range(B):
        rows = [j for j in range(int(num[b])) if dets[b, j, 4] > np.float32(thr) and 0 <= obj_cand[b, j] < n][:K]
        cnt[b] = len(rows)
        for s, j in enumerate(rows):
            post[b, s] = scores[b, obj_cand[b, j]]
    return post, cnt


# ---------------------------------------------------------------------------------------------------------------- seeding
def sqdist64(x, c):
    d = np.asarray(x, np.float64) - np.asarray(c, np.float64)
    return (d * d).sum(-1)


def _sample(w, target, block):
    """the first row with w > 0 whose running sum -- the blocks before it in order, then the rows of its block in order, every add a
    float64 add -- exceeds target; None when no row does.  np.cumsum adds sequentially."""
    N = w.size
    NB = -(-N // block)
    wp = np.zeros(NB * block)
    wp[:N] = w
    wp = wp.reshape(NB, block)
    S = np.cumsum(wp, axis=1)[:, -1]                                   # S_b: the rows of block b in order, from 0
    P = np.concatenate([[0.0], np.cumsum(S)[:-1]])                     # the blocks before b, in order
    R = np.cumsum(np.concatenate([P[:, None], wp], axis=1), axis=1)[:, 1:]
    hit = np.flatnonzero(((R > target) & (wp > 0)).reshape(-1))
    return int(hit[0]) if hit.size else None


def total64(w, block):
    N = w.size
    NB = -(-N // block)
    wp = np.zeros(NB * block)
    wp[:N] = w
    return float(np.cumsum(np.cumsum(wp.reshape(NB, block), axis=1)[:, -1])[-1]) if N else 0.0


def seed_float64(desc, excluded, budget, draws, block):
    """DESIGN 3t's seeding in float64 -> (picks int64, weight float64, total float64).  With integer-valued descriptors every value is
    exact, so the device must return exactly this."""
    x = np.asarray(desc, np.float64)
    N = x.shape[0]
    elig = np.ones(N, bool)
    elig[np.asarray(excluded, np.int64).reshape(-1)] = False
    picks, weight, total = [], [], []
    norms = (x * x).sum(1)
    p = int(np.argmax(np.where(elig, norms, -1.0)))                    # the first maximum: the lowest index on a tie
    picks.append(p), weight.append(norms[p]), total.append(0.0)
    mind = np.full(N, np.inf)
    for t in range(1, budget + 1):
        elig[p] = False
        mind = np.minimum(mind, sqdist64(x, x[p]))
        if t == budget:
            break
        w = np.where(elig, mind, 0.0)
        T = total64(w, block)
        if T == 0.0:
            p = int(np.flatnonzero(elig)[0])
        else:
            p = _sample(w, draws[t] * T, block)
            if p is None:
                p = int(np.flatnonzero(w > 0)[-1])
        picks.append(p), weight.append(w[p]), total.append(T)
    return np.array(picks, np.int64), np.array(weight), np.array(total)


def replay_check(desc, excluded, picks, weight, total, draws):
    """The device's own pick sequence replayed in float64 on the stored fp32 rows.  At every step t >= 1:
         lo64(pick) - tau <= draws[t] * T64 <= hi64(pick) + tau, tau = 4 (D + 4) 2^-24 T64, and |total[t] - T64| <= (D + 4) 2^-24 T64,
       lo64 / hi64 the pick's exclusive / inclusive cumulative sum of w64 in row order (DESIGN 3i bounds a distance's relative error by
       (D + 4) 2^-24; a running sum of non-negative terms and T inherit it: 2 (D + 4) 2^-24 T between them, doubled as 3i doubles its own).
       Returns the largest |violation margin| / tau seen (<= 1 means inside), for printing."""
    x = np.asarray(desc, np.float64)
    N, D = x.shape
    elig = np.ones(N, bool)
    elig[np.asarray(excluded, np.int64).reshape(-1)] = False
    norms = (x * x).sum(1)
    p = int(picks[0])
    assert elig[p] and norms[p] >= (1 - 2 * (D + 4) * U24) * np.where(elig, norms, 0).max(), 'pick 0 is not the longest eligible row'
    assert abs(weight[0] - norms[p]) <= (D + 4) * U24 * norms[p] and total[0] == 0
    mind = np.full(N, np.inf)
    worst = 0.0
    for t in range(1, len(picks)):
        elig[p] = False
        mind = np.minimum(mind, sqdist64(x, x[p]))
        w = np.where(elig, mind, 0.0)
        T = float(w.sum())
        p = int(picks[t])
        assert elig[p], (t, p)
        assert abs(total[t] - T) <= (D + 4) * U24 * T, (t, total[t], T)
        assert abs(weight[t] - w[p]) <= (D + 4) * U24 * w[p], (t, weight[t], w[p])
        tau = 4 * (D + 4) * U24 * T
        lo = float(w[:p].sum())
        hi = lo + float(w[p])
        tgt = draws[t] * T
        assert lo - tau <= tgt <= hi + tau, (t, p, lo, tgt, hi, tau)
        if tau > 0:
            worst = max(worst, (lo - tgt) / tau, (tgt - hi) / tau)
    return worst
