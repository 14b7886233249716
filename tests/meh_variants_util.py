"""Restatements for the MEH ablation heads (Lambda_L1Net / Lambda_MSLENet / Lambda_L2Net_ablation / Lambda_L2Net_NoL): the three MEH loss
forms with their gradients in float64, and ComputeAvgUnc + AggregateAvgUnc (Entropy_Avg) on the Philox sampler restatement of oracle/hua.py.
Shared by tools/golden/make_golden_meh_variants.py (which records the reference next to them) and the tests."""
import numpy as np

from oracle import hua as ohua

FORMS = ('l2', 'l1', 'msle')
LOSS_B, LOSS_A = 2, 9
LOSS_LEVELS = ((8, 8), (2, 3), (1, 2))          # 1152 + 108 + 36 rows: several 256-thread blocks, level boundaries inside a block
# (head, score_thr, iou_thr, pool) of the recorded scoring cases
SCORING_CASES = (('nol_030_050', 'Lambda_L2Net_NoL', 0.3, 0.5, 'Entropy_NMS'), ('nol_030_090', 'Lambda_L2Net_NoL', 0.3, 0.9, 'Entropy_NMS'),
                 ('abl_030_090', 'Lambda_L2Net_ablation', 0.3, 0.9, 'Entropy_NMS'), ('abl_050_050', 'Lambda_L2Net_ablation', 0.5, 0.5, 'Entropy_NMS'),
                 ('nol_avg', 'Lambda_L2Net_NoL', 0.3, 0.9, 'Entropy_Avg'))


def meh_loss_float64(form, L_score, loss, w):
    """loss_single_L of the three heads (Lambda_L2.py / Lambda_L1.py / Lambda_MSLE.py :235-242) and its gradient w.r.t. L_score, in float64.
    L_score [B, A, h, w] float32, loss [B*h*w*A], w [B*h*w*A] (= bbox_weights[..., 0]).  The FIRST operation, L_score + 1e-9, is taken in
    float32 as every implementation takes it (1e-9 is below half an ulp of any L_score >= 2^-6: whether a row is an exact tie, and with it
    the sign of the L1 gradient, is a float32 fact of the inputs and not a matter of precision); everything after it is float64.
    Returns (value, grad [B, A, h, w])."""
    B, A, h, ww = L_score.shape
    x = (np.transpose(L_score, (0, 2, 3, 1)).reshape(-1).astype(np.float32) + np.float32(1e-9)).astype(np.float64)
    loss, w = loss.astype(np.float64), w.astype(np.float64)
    n = x.size
    if form == 'l2':
        d = x - loss
        val = ((np.abs(d) * w) ** 2).mean() * 5
        g = 5.0 / n * 2 * (np.abs(d) * w) * w * np.sign(d)
    elif form == 'l1':
        d = x - loss
        val = np.abs(np.abs(d) * w).mean() * 5
        g = 5.0 / n * np.sign(np.abs(d) * w) * w * np.sign(d)
    elif form == 'msle':
        d = np.log(x + 1) - np.log(loss + 1)
        val = ((np.abs(d) * w) ** 2).mean() * 5
        g = 5.0 / n * 2 * (np.abs(d) * w) * w * np.sign(d) / (x + 1)
    else:
        raise ValueError(form)
    return float(val), np.transpose(g.reshape(B, h, ww, A), (0, 3, 1, 2))


def softmax_rows(cls_map, C):
    """[B, A*C, h, w] float32 logits -> [B, h*w*A, C] float32 softmax, the row order of the head (permute(0, 2, 3, 1).reshape)."""
    import torch
    t = torch.as_tensor(np.asarray(cls_map, np.float32))
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, C).softmax(dim=2).numpy()


def avg_unc_philox(mlvl_cls, C, seed=20, image_ids=None, num_samples=50, fg_thr=0.3):
    """ComputeAvgUnc + AggregateAvgUnc (Lambda_L2_noL.py:552-572, 631-640) on the Philox sampler: per (image, level) the rows whose softmax
    maximum exceeds 0.3, alpha = the softmax row, key (seed, image id, global anchor id, pseudo object 0); level value = float32 mean of the
    rows' epistemic values; image score = mean over the levels that HAVE such a row, 0 when none has (the two places where this project
    departs from the reference's NaN / dropped exact-zero level).  Returns (scores [B], fg_counts [B, L], per-level values [B, L] NaN = none)."""
    alphas = [softmax_rows(c, C) for c in mlvl_cls]
    B, L = alphas[0].shape[0], len(alphas)
    offs = np.concatenate([[0], np.cumsum([a.shape[1] for a in alphas])[:-1]])
    counts = np.zeros((B, L), np.int64)
    vals = np.full((B, L), np.nan, np.float64)
    for l in range(L):
        for b in range(B):
            a = alphas[l][b]
            idx = np.nonzero(a.max(1) > np.float32(fg_thr))[0]
            counts[b, l] = len(idx)
            if len(idx) == 0:
                continue
            img = b if image_ids is None else int(image_ids[b])
            _, epi = ohua.philox_dirichlet_stats(a[idx], img, idx + offs[l], np.zeros(len(idx), np.int64), seed, num_samples)
            vals[b, l] = float(np.mean(epi.astype(np.float64)))
    scores = np.array([np.nanmean(vals[b]) if counts[b].any() else 0.0 for b in range(B)])
    return scores, counts, vals
