"""Float64 restatement of the ensemble mutual-information score (apis.test.single_gpu_ensemble / scoring.ensemble_mi) and the tolerance the
tests of that feature share.  Written from the formula, not from the reference's text:

    p_k = sigmoid(x_k),  avg = mean_k p_k
    level score = sum over ALL elements of [ -avg ln avg + (1/K) sum_k p_k ln p_k ] / rows,   rows = elements / n_cls
    score[b]    = mean over levels,        0 ln 0 = 0
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ensemble_mi.npz')
CASES = ('prior_k3', 'prior_k5', 'saturated_k3')
LEVELS = ((4, 6), (2, 3), (1, 2))


def _xlogx(p):
    return np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)


def _sigmoid64(x):
    x = np.asarray(x, np.float64)
    t = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0, t) / (1.0 + t)


def mi_float64(members, n_cls):
    """members: K lists of L arrays [B, ...] -> (score [B] float64, total_mean: the float64 mean, over images and levels, of the `total`
    term's per-row mean -- the magnitude of the two means whose difference the score is)"""
    K, L = len(members), len(members[0])
    B = np.asarray(members[0][0]).shape[0]
    score, total = np.zeros(B), np.zeros(B)
    for l in range(L):
        p = np.stack([_sigmoid64(np.asarray(m[l])).reshape(B, -1) for m in members])          # [K, B, n]
        rows = p.shape[2] // n_cls
        assert rows * n_cls == p.shape[2]
        tot = -_xlogx(p.mean(0)).sum(1) / rows
        ale = -_xlogx(p).sum(2).mean(0) / rows
        score += (tot - ale) / L
        total += tot / L
    return score, float(total.mean())


def load_case(z, name):
    """-> (members: K lists of L float32 arrays [B, A*C, h, w], ref [B], e_ref, total_mean)"""
    xs = [z[f'{name}_x{l}'] for l in range(len(LEVELS))]                  # each [K, B, A*C, h, w]
    K = xs[0].shape[0]
    return [[x[k] for x in xs] for k in range(K)], z[f'{name}_ref'], float(z[f'{name}_e_ref']), float(z[f'{name}_total_mean'])


def bound(e_ref, total_mean):
    """|x - float64| <= 8 e_ref + 2^-23 total_mean: 8 x the reference's own fp32 error (another, fixed, association of the sums and other
    transcendental implementations) + one fp32 ulp at the magnitude of the two means whose difference is the result"""
    return 8.0 * e_ref + 2.0 ** -23 * total_mean


def mi_fp32_torch(members, n_cls):
    """the score in fp32 torch ops on the tensors' device, per (level, image), from the formula above: what the baseline costs and errs
    when it is written with library ops.  members: K lists of L tensors [B, A*C, h, w].  -> [B] fp32 tensor"""
    import torch
    L, B = len(members[0]), members[0][0].shape[0]
    buf = torch.zeros(B, L, device=members[0][0].device)
    for l in range(L):
        for b in range(B):
            p = torch.stack([torch.sigmoid(m[l][b]).permute(1, 2, 0).reshape(-1, n_cls) for m in members])
            avg = p.mean(0)
            total = -(avg * avg.log()).sum(1)
            aleatoric = -(p * p.log()).sum(2).mean(0)
            buf[b, l] = (total - aleatoric).mean()
    return buf.mean(1)
