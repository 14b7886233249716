"""Float64 numpy restatements of the Core-set acquisition the tests compare the kernels against: the pooled pyramid
descriptor, the exact k-center greedy with the lowest-index tie-break, and a replay checker for inexact (float) descriptors.  The greedy
and the checker take the distance as an argument: tests/cdal_util.py (symmetrised KL) and tests/ccms_util.py (a matrix row) call them."""
import numpy as np


def descriptor_float64(levels):
    """levels: per-level value arrays [B, h * w, C] (any float dtype) -> [B, sum C] float64: the mean over the rows, levels side by side"""
    return np.concatenate([np.asarray(v, np.float64).mean(axis=1) for v in levels], axis=1)


def sqdist(X, c):
    """d(i, c) = sum_k (x_ik - x_ck)^2 in the direct difference form, in X's dtype"""
    diff = X - X[c]
    return (diff * diff).sum(axis=1)


def greedy(X, labelled, budget, dtype=np.float64, dist=sqdist):
    """k-center greedy (Sener & Savarese, Algorithm 1) under the distance dist(X, c) -> [N] (X already in `dtype`): mind = min over
    labelled centers (+inf without one), labelled rows selected; each step picks the unselected row with the largest mind -- np.argmax
    returns the LOWEST index of a tie --, records that mind as the radius, selects the row and lowers every mind to the distance to it.
    Returns (picks [budget] int64, radius [budget] dtype, ties) with ties = the number of steps at which more than one unselected row
    held the maximum."""
    X = np.asarray(X, dtype)
    N = X.shape[0]
    mind = np.full(N, np.inf, dtype)
    sel = np.zeros(N, bool)
    for c in labelled:
        mind = np.minimum(mind, dist(X, int(c)))
        sel[int(c)] = True
    picks, radius, ties = [], [], 0
    for _ in range(budget):
        cand = np.where(sel, -np.inf, mind)
        p = int(np.argmax(cand))
        assert not sel[p], 'budget exceeds the unselected rows'
        ties += int((cand == cand[p]).sum() > 1)
        picks.append(p)
        radius.append(mind[p])
        sel[p] = True
        mind = np.minimum(mind, dist(X, p))
    return np.array(picks, np.int64), np.array(radius, dtype), ties


def replay_ratios(X, labelled, picks, return_radius=False, dist=sqdist):
    """Given a device's own pick sequence: mind recomputed in float64 (under dist(X, c)) along it; per step mind64[pick] / max over
    unselected of mind64 (1.0 where the device took the exact float64 maximum, or where that maximum is 0 or inf and the pick holds it too).  A pick that was
    already selected gives -1.  return_radius: also mind64[pick] per step."""
    X = np.asarray(X, np.float64)
    N = X.shape[0]
    mind = np.full(N, np.inf)
    sel = np.zeros(N, bool)
    for c in labelled:
        mind = np.minimum(mind, dist(X, int(c)))
        sel[int(c)] = True
    out, rad = [], []
    for p in picks:
        p = int(p)
        rad.append(mind[p])
        if sel[p]:
            out.append(-1.0)
            continue
        best = np.where(sel, -np.inf, mind).max()
        out.append(1.0 if mind[p] == best else float(mind[p] / best))
        sel[p] = True
        mind = np.minimum(mind, dist(X, p))
    return (np.array(out), np.array(rad)) if return_radius else np.array(out)


def x_layout_rows(values):
    """fp32 values [M, C] -> (X-layout rows [M, 2 * ceil32(C)], a bf16 torch tensor with ZERO pad; the float64 values head + tail the rows
    represent, [M, C]): [h(0..31) | l(0..31) | h(32..63) | l(32..63) | ...], head = bf16_rne(v), tail = bf16_rne(v - head)"""
    import torch
    v = torch.as_tensor(np.ascontiguousarray(values), dtype=torch.float32)
    M, C = v.shape
    Cp = (C + 31) // 32 * 32
    h = v.to(torch.bfloat16)
    l = (v - h.float()).to(torch.bfloat16)
    rows = torch.zeros(M, Cp // 32, 2, 32, dtype=torch.bfloat16)
    hp, lp = torch.zeros(M, Cp, dtype=torch.bfloat16), torch.zeros(M, Cp, dtype=torch.bfloat16)
    hp[:, :C], lp[:, :C] = h, l
    rows[:, :, 0, :] = hp.view(M, Cp // 32, 32)
    rows[:, :, 1, :] = lp.view(M, Cp // 32, 32)
    return rows.view(M, 2 * Cp), (h.double() + l.double()).numpy()


def pad_mask(C):
    """bool [2 * ceil32(C)]: the pad columns of an X-layout row of C channels"""
    Cp = (C + 31) // 32 * 32
    m = np.zeros((Cp // 32, 2, 32), bool)
    ch = np.arange(Cp).reshape(Cp // 32, 32)
    m[:, 0, :] = ch >= C
    m[:, 1, :] = ch >= C
    return m.reshape(-1)
