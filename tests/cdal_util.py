"""Float64 numpy restatements of the CDAL acquisition the tests compare the kernels against: the class-mixture descriptor
[P | ln P] with its region counts and its ambiguous rows, the symmetrised KL distance, and tests/coreset_util.py's exact greedy and replay
checker with the distance as an argument."""
import numpy as np

from tests import coreset_util

EPS = 2.0 ** -10            # the entropy weight's floor and the smoothing share
AMBIGUOUS = 1e-6


def softmax_float64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def entropy_float64(p):
    """H = -sum p ln p with 0 ln 0 = 0"""
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(p > 0, p * np.log(p), 0.0)
    return -t.sum(axis=-1)


def descriptor_float64(levels, C, thr):
    """levels: per-level logit arrays [B, rows, C] (any float dtype; the values are taken as they are).  Returns (P [B, C, C], ln P,
    R [B, C] region counts, ambiguous): ambiguous = the list of (level, image, row) whose decision a rounding could flip -- |max p - thr| <=
    1e-6 or a gap of the two largest probabilities <= 1e-6."""
    B = levels[0].shape[0]
    num = np.zeros((B, C, C))
    den = np.zeros((B, C))
    R = np.zeros((B, C), np.int64)
    ambiguous = []
    for l, x in enumerate(levels):
        assert x.shape[0] == B and x.shape[2] == C
        p = softmax_float64(x)                                     # [B, rows, C]
        top = np.sort(p, axis=-1)
        pm = top[..., -1]
        gap = pm - top[..., -2] if C > 1 else np.ones_like(pm)
        amb = (np.abs(pm - thr) <= AMBIGUOUS) | (gap <= AMBIGUOUS)
        ambiguous += [(l, int(b), int(r)) for b, r in zip(*np.nonzero(amb))]
        region = pm > thr
        cls = p.argmax(axis=-1)                                    # (the lowest index on a tie)
        w = entropy_float64(p) + EPS
        for b in range(B):
            rr = np.nonzero(region[b])[0]
            np.add.at(num[b], cls[b, rr], w[b, rr, None] * p[b, rr])
            np.add.at(den[b], cls[b, rr], w[b, rr])
            R[b] += np.bincount(cls[b, rr], minlength=C)
    M = np.where(den[..., None] > 0, num / np.where(den > 0, den, 1.0)[..., None], 1.0 / C)
    P = (1.0 - EPS) * M + EPS / C
    return P, np.log(P), R, ambiguous


def rows_float64(levels, C, thr):
    """the descriptor rows [B, 2 C^2] = [P | ln P] (and R, ambiguous)"""
    P, lnP, R, amb = descriptor_float64(levels, C, thr)
    B = P.shape[0]
    return np.concatenate([P.reshape(B, -1), lnP.reshape(B, -1)], axis=1), R, amb


def bound(want_rows, R, C):
    """|device - float64| allowed per descriptor column (derived in tests/test_gpu_cdal.py): P within relative (R_max(b) + 8 C + 64) 2^-23,
    ln P within that amount plus 4 * 2^-24 |ln P|"""
    B = want_rows.shape[0]
    rel = (R.max(axis=1) + 8 * C + 64)[:, None] * 2.0 ** -23
    P, lnP = want_rows[:, :C * C], want_rows[:, C * C:]
    return np.concatenate([rel * P, rel + 4 * 2.0 ** -24 * np.abs(lnP)], axis=1).reshape(B, -1)


def symkl(X, c):
    """d(i, c) = 1/2 sum_k max((P_ik - P_ck)(ln P_ik - ln P_ck), 0) over the rows [P | ln P] of X, in X's dtype"""
    H = X.shape[1] // 2
    assert X.shape[1] == 2 * H
    return (np.maximum((X[:, :H] - X[c, :H]) * (X[:, H:] - X[c, H:]), 0) * X.dtype.type(0.5)).sum(axis=1)


def greedy(X, labelled, budget, dist=symkl, dtype=np.float64):
    return coreset_util.greedy(X, labelled, budget, dtype, dist)


def replay_ratios(X, labelled, picks, dist=symkl, return_radius=False):
    return coreset_util.replay_ratios(X, labelled, picks, return_radius=return_radius, dist=dist)
