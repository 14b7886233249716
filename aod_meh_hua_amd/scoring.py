"""HUA scoring pass on the HIP kernels: Lambda_L2Net._get_bboxes (Lambda_L2.py:254-384) +
ComputeObjUnc / AggregateObjScaleUnc (:489-619) for a whole batch without a host sync.

    per level   aod_softmax_rowmax  -> row max of the normalised scores, level gate
                aod_topk_stable     -> per-image top-nms_pre anchors (levels with more than nms_pre anchors)
                aod_gather_decode   -> candidates: boxes / scores(+bg) / lambda / anchor id
                (all levels in two launches: aod_pre_nms_levels)
    per batch   aod_multiclass_nms  -> dets [B,max,5], labels, keep, num_det
                aod_hua_score       -> one epistemic-uncertainty score per image

`unc` stays on the device ([B] fp32 tensor): the pool loop (apis/test.py single_gpu_uncertainty) concatenates
tensors and only syncs once per pool, instead of the reference's `.item()` per (object, level, class) bin."""
import ctypes as C
import os

import numpy as np
import torch

from . import _C
from ._C import call, ptr, stream

AGG_CODE = {'Sum': 0, 'Avg': 1, 'Max': 2}
_F4 = C.c_float * 4


def extract_agg_codes(type_str):
    """mmdet/utils/functions.py:425-436 ExtractAggFunc -> (class, scale, object) kernel codes."""
    out = {}
    for name in ('object', 'scale', 'class'):
        for part in type_str.split('_'):
            if name in part:
                out[name] = AGG_CODE[part.replace(name, '')]
    return out['class'], out.get('scale', 2), out.get('object', 0)


def nhwc_view(x, c):
    """[B, A*c, h, w] channels_last fp32 -> [B, h*w*A, c] view."""
    B = x.shape[0]
    xr = x.permute(0, 2, 3, 1)
    if not xr.is_contiguous():
        xr = xr.contiguous()
    return xr.reshape(B, -1, c)


_META = {}
_META_STATIC = None      # (hw [B,2], sc [B,4]) static device buffers of a captured scoring graph (graphs.GraphedScore refreshes them per batch)


class static_meta:
    """inside this context the image sizes / scale factors of a scoring batch are read from the given STATIC device buffers instead of
    value-keyed cached tensors: a captured scoring graph then serves every batch of its tensor shape, whatever the per-image sizes are"""

    def __init__(self, hw, sc):
        self.new = (hw, sc)

    def __enter__(self):
        global _META_STATIC
        self.prev, _META_STATIC = _META_STATIC, self.new

    def __exit__(self, *exc):
        global _META_STATIC
        _META_STATIC = self.prev
        return False


def meta_values(img_shapes, scale_factors):
    """host rows ([B,2] sizes, [B,4] scale factors) as float32 tensors: what a static-meta graph copies into its buffers"""
    hw = torch.tensor([[float(s[0]), float(s[1])] for s in img_shapes], dtype=torch.float32)
    sc = torch.tensor(np.stack([np.asarray(s, np.float32).reshape(-1)[:4] for s in scale_factors]), dtype=torch.float32)
    return hw, sc


def _meta_tensors(img_shapes, scale_factors, dev):
    """[B,2] image sizes and [B,4] scale factors on the device, cached by value: the pool loop re-uses a handful of shapes, and an
    H2D copy per batch would also break HIP-graph capture of the scoring pass."""
    if _META_STATIC is not None:
        return _META_STATIC[0], (_META_STATIC[1] if scale_factors is not None else None)
    key = (tuple((float(s[0]), float(s[1])) for s in img_shapes),
           None if scale_factors is None else tuple(tuple(float(v) for v in np.asarray(s, np.float32).reshape(-1)[:4]) for s in scale_factors), str(dev))
    hit = _META.get(key)
    if hit is None:
        if len(_META) > 256:
            _META.clear()
        hw = torch.tensor(key[0], dtype=torch.float32).to(dev)
        sc = torch.tensor(key[1], dtype=torch.float32).to(dev) if key[1] is not None else None
        hit = _META[key] = (hw, sc)
    return hit


class Candidates:
    """Outputs of the pre-NMS stage for a batch (concatenated levels)."""

    def __init__(self, boxes, scores, lam, cand_anchor, level_start, any_fg, topk_idx, rowmax=None):
        self.boxes, self.scores, self.lam, self.cand_anchor = boxes, scores, lam, cand_anchor
        self.level_start, self.any_fg, self.topk_idx = level_start, any_fg, topk_idx
        self.rowmax = rowmax              # per level [B, A_l]: max normalised class score of every anchor (before top-k)

    def max_conf(self):
        """getMaxConf (mmdet/utils/functions.py:467-476): per image, the largest class probability over all levels / anchors."""
        return torch.stack([r.amax(dim=1) for r in self.rowmax], dim=1).amax(dim=1)


def pre_nms(mlvl_cls, mlvl_reg, mlvl_L, mlvl_anchors, img_shapes, scale_factors, nms_pre, C_, means, stds, rescale=True,
            fg_thr=0.3, wh_ratio_clip=16 / 1000, normalize=True, has_bg=False, activation=None):
    """activation='sigmoid' (the plain RetinaNet baseline, anchor_head.py:535-553): mode 3 of the kernels -- s_c = 1 / (1 + exp(-x_c)) per
    class, the row key is the maximum over all C columns, C score columns (+ the zero background column) are written."""
    assert activation in (None, 'sigmoid') and not (activation == 'sigmoid' and has_bg)
    mode = 3 if activation == 'sigmoid' else (2 if has_bg else int(bool(normalize)))
    row_mode = 2 if activation == 'sigmoid' else int(has_bg)      # the row-max kernels: 0 EDL-normalised, 1 last column is background, 2 sigmoid
    dev = mlvl_cls[0].device
    B = mlvl_cls[0].shape[0]
    L = len(mlvl_cls)
    cls = [nhwc_view(c.float(), C_) for c in mlvl_cls]
    reg = [nhwc_view(r.float(), 4) for r in mlvl_reg]
    lam = [nhwc_view(l.float(), 1).reshape(B, -1) for l in mlvl_L]
    A = [c.shape[1] for c in cls]
    ks = [nms_pre if 0 < nms_pre < a else a for a in A]
    n = sum(ks)
    any_fg = torch.zeros(L, B, dtype=torch.int32, device=dev)
    boxes = torch.empty(B, n, 4, device=dev)
    scores = torch.empty(B, n, C_ if has_bg else C_ + 1, device=dev)
    lam_o = torch.empty(B, n, device=dev)
    cand_anchor = torch.empty(B, n, dtype=torch.int32, device=dev)
    img_hw, sc4 = _meta_tensors(img_shapes, scale_factors if rescale else None, dev)
    level_start = [0]
    for l in range(L):
        level_start.append(level_start[-1] + ks[l])
    if L <= 8 and max(ks) <= 1024 and os.environ.get('AOD_PRE_NMS_MERGED', '1') != '0':
        # all levels in two launches (aod_pre_nms_levels): one [sum B*A] row-max buffer and one index buffer, handed out as per-level views
        rm = torch.empty(B * sum(A), device=dev)
        tk = [l for l in range(L) if ks[l] < A[l]]
        ix = torch.empty(max(B * sum(ks[l] for l in tk), 1), dtype=torch.int32, device=dev)
        anch = [a.contiguous() for a in mlvl_anchors]
        PA = C.c_void_p * L
        call('aod_pre_nms_levels', L, PA(*[ptr(t).value for t in cls]), PA(*[ptr(t).value for t in reg]), PA(*[ptr(t).value for t in lam]),
             PA(*[ptr(t).value for t in anch]), (C.c_int64 * L)(*A), (C.c_int32 * L)(*ks), B, C_, fg_thr, int(has_bg),
             mode, ptr(img_hw), ptr(sc4), _F4(*means), _F4(*stds), float(wh_ratio_clip), ptr(rm), ptr(any_fg),
             ptr(ix), ptr(boxes), ptr(scores), ptr(lam_o), ptr(cand_anchor), n, stream())
        rowmaxes, idxs, r0, i0 = [], [], 0, 0
        for l in range(L):
            rowmaxes.append(rm[r0:r0 + B * A[l]].view(B, A[l]))
            r0 += B * A[l]
            if ks[l] < A[l]:
                idxs.append(ix[i0:i0 + B * ks[l]].view(B, ks[l]))
                i0 += B * ks[l]
            else:
                idxs.append(None)
        return Candidates(boxes, scores, lam_o, cand_anchor, level_start, any_fg, idxs, rowmaxes)
    c0 = a0 = 0
    idxs, rowmaxes = [], []
    for l in range(L):
        rowmax = torch.empty(B, A[l], device=dev)
        from .hipops import prof_bytes
        prof_bytes('softmax_rowmax', B * A[l] * (C_ * 4 + 4),
                   lambda: call('aod_softmax_rowmax', ptr(cls[l]), B, A[l], C_, fg_thr, ptr(rowmax), ptr(any_fg[l]), row_mode, stream()))
        idx = None
        if ks[l] < A[l]:
            idx = torch.empty(B, ks[l], dtype=torch.int32, device=dev)
            call('aod_topk_stable', ptr(rowmax), B, A[l], ks[l], ptr(idx), ks[l], stream())
        idxs.append(idx)
        rowmaxes.append(rowmax)
        call('aod_gather_decode', ptr(cls[l]), ptr(reg[l]), ptr(lam[l]), ptr(mlvl_anchors[l].contiguous()), ptr(idx), B, A[l], ks[l], C_,
             ks[l], ptr(img_hw), ptr(sc4), _F4(*means), _F4(*stds), float(wh_ratio_clip), ptr(boxes), ptr(scores), ptr(lam_o),
             ptr(cand_anchor), n, c0, a0, mode, stream())
        c0 += ks[l]
        a0 += A[l]
    return Candidates(boxes, scores, lam_o, cand_anchor, level_start, any_fg, idxs, rowmaxes)


def multiclass_nms_batch(boxes, scores, score_thr, iou_thr, max_num):
    B, n, C1 = scores.shape
    dev = boxes.device
    dets = torch.empty(B, max_num, 5, device=dev)
    labels = torch.empty(B, max_num, dtype=torch.int64, device=dev)
    keep = torch.empty(B, max_num, dtype=torch.int64, device=dev)
    num = torch.empty(B, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(_C.lib.aod_nms_ws_bytes(B, n, C1 - 1)), 8), dtype=torch.uint8, device=dev)
    call('aod_multiclass_nms', ptr(boxes), ptr(scores), B, n, C1 - 1, float(score_thr), float(iou_thr), int(max_num), ptr(dets),
         ptr(labels), ptr(keep), ptr(num), ptr(ws), stream())
    return dets, labels, keep, num


HUA_ESTIMATORS = {'mc': 0, 'closed': 1}
HUA_LAM_MODES = {'scaled': 0, 'none': 1}


def hua_score(cand, dets, num_det, image_ids, max_num, agg=(0, 2, 0), clsW=False, num_samples=500, seed=20, obj_score_thr=0.3,
              obj_iou_thr=0.5, fg_thr=0.3, want_pairs=False, max_pairs=None, scale_mode=False, dirichlet_cols=0, estimator='mc',
              want_objects=False, lam_mode='scaled'):
    """estimator: 'mc' (num_samples Dirichlet draws, seeded) or 'closed' (the closed form of the Monte-Carlo limit: no seed, no sample count).
    The closed form is the n -> infinity limit; it is NOT the expectation of a finite-sample run (the `total` term of the Monte-Carlo
    estimator, the entropy of the mean of n samples, is biased downwards at finite n), so 'closed' and 'mc' with 50 samples (Entropy_Avg) differ by more than sampling noise.
    lam_mode: 'scaled' (alpha = score * mean(lambda) / (lambda + 1e-7) * 25, Lambda_L2.py:513-516) or 'none' (alpha = score: Lambda_L2Net_NoL,
    Lambda_L2_noL.py:526-532, 586-592).
    scale_mode: False (objects), True (Entropy_ALL: class bins per level) or 'avg' (Entropy_Avg, Lambda_L2_noL.py:552-572, 631-640: mean over
    the levels that own a foreground row of the level's mean per-row epistemic value; `agg` / `clsW` are not read).
    want_objects appends (obj_out [B, max_num, 2] = (aleatoric, epistemic) per detection row, obj_pairs [B, max_num] int32) to the return;
    rows that are no object (score <= obj_score_thr, row >= num_det) or own no pair hold (NaN, NaN, 0)."""
    if estimator not in HUA_ESTIMATORS:
        raise ValueError(f"hua_score: unknown estimator {estimator!r} (expected 'mc' or 'closed')")
    if lam_mode not in HUA_LAM_MODES:
        raise ValueError(f"hua_score: unknown lam_mode {lam_mode!r} (expected 'scaled' or 'none')")
    if scale_mode not in (False, True, 'avg', 0, 1):
        raise ValueError(f"hua_score: unknown scale_mode {scale_mode!r} (expected False, True or 'avg')")
    if want_objects and scale_mode:
        raise ValueError('hua_score: per-object outputs are not offered in scale_mode')
    B, n, C1 = cand.scores.shape
    dev = cand.boxes.device
    L = len(cand.level_start) - 1
    max_pairs = max_pairs or (n if scale_mode else n * max_num)
    unc = torch.empty(B, device=dev)
    pair_count = torch.empty(B, dtype=torch.int32, device=dev)
    pair_out = torch.zeros(B, max_pairs, 4, device=dev) if want_pairs else None
    ws = torch.empty(int(_C.lib.aod_hua_ws_bytes(B, max_pairs)), dtype=torch.uint8, device=dev)
    if lam_mode != 'scaled' or scale_mode == 'avg':
        obj_out = torch.empty(B, int(max_num), 2, device=dev) if want_objects else None
        obj_pairs = torch.empty(B, int(max_num), dtype=torch.int32, device=dev) if want_objects else None
        call('aod_hua_score_ex2', ptr(cand.boxes), ptr(cand.scores), ptr(cand.lam), ptr(cand.cand_anchor), ptr(dets), ptr(num_det),
             (C.c_int32 * (L + 1))(*cand.level_start), ptr(cand.any_fg), ptr(image_ids), B, n, L, C1 - 1, int(max_num), float(obj_score_thr),
             float(obj_iou_thr), float(fg_thr), int(num_samples), int(seed), (C.c_int32 * 3)(*agg), int(bool(clsW)),
             2 if scale_mode == 'avg' else int(bool(scale_mode)), int(dirichlet_cols), ptr(unc), ptr(pair_out), int(max_pairs), ptr(pair_count),
             HUA_ESTIMATORS[estimator], HUA_LAM_MODES[lam_mode], ptr(obj_out), ptr(obj_pairs), ptr(ws), stream())
        out = (unc, pair_count, pair_out) if want_pairs else (unc,)
        out = out + (obj_out, obj_pairs) if want_objects else out
        return out if len(out) > 1 else unc
    if estimator != 'mc' or want_objects:
        obj_out = torch.empty(B, int(max_num), 2, device=dev) if want_objects else None
        obj_pairs = torch.empty(B, int(max_num), dtype=torch.int32, device=dev) if want_objects else None
        call('aod_hua_score_ex', ptr(cand.boxes), ptr(cand.scores), ptr(cand.lam), ptr(cand.cand_anchor), ptr(dets), ptr(num_det),
             (C.c_int32 * (L + 1))(*cand.level_start), ptr(cand.any_fg), ptr(image_ids), B, n, L, C1 - 1, int(max_num), float(obj_score_thr),
             float(obj_iou_thr), float(fg_thr), int(num_samples), int(seed), (C.c_int32 * 3)(*agg), int(bool(clsW)), int(bool(scale_mode)),
             int(dirichlet_cols), ptr(unc), ptr(pair_out), int(max_pairs), ptr(pair_count), HUA_ESTIMATORS[estimator], ptr(obj_out),
             ptr(obj_pairs), ptr(ws), stream())
        out = (unc, pair_count, pair_out) if want_pairs else (unc,)
        out = out + (obj_out, obj_pairs) if want_objects else out
        return out if len(out) > 1 else unc
    call('aod_hua_score', ptr(cand.boxes), ptr(cand.scores), ptr(cand.lam), ptr(cand.cand_anchor), ptr(dets), ptr(num_det),
         (C.c_int32 * (L + 1))(*cand.level_start), ptr(cand.any_fg), ptr(image_ids), B, n, L, C1 - 1, int(max_num), float(obj_score_thr),
         float(obj_iou_thr), float(fg_thr), int(num_samples), int(seed), (C.c_int32 * 3)(*agg), int(bool(clsW)), int(bool(scale_mode)),
         int(dirichlet_cols), ptr(unc), ptr(pair_out),
         int(max_pairs), ptr(pair_count), ptr(ws), stream())
    return (unc, pair_count, pair_out) if want_pairs else unc


def _dense(t):
    return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))


def ensemble_mi(members, n_cls, out=None):
    """Mutual information between K ensemble members' sigmoid classification maps, one score per image: the public form of the reference's
    ComputeMI (mmdet/apis/CalEnsembleUnc.py:164-180, K = 3 models) and ComputeMCDropoutMI (mmdet/apis/CalMCDropoutUnc.py:183-199, K = n
    stochastic outputs of one model) on the aod_ensemble_mi kernel.

    members: K lists (2 <= K <= 32) of L per-level logit maps (1 <= L <= 8), fp32 device tensors [B, ...] of the same shapes in every
    member, dense in memory with the batch outermost (contiguous or channels_last; nothing is copied).  n_cls: classes per anchor row.
    Returns out [B] fp32 on the device (no host sync); a term with p = 0 contributes 0 where the reference turns the image into NaN."""
    members = [list(m) for m in members]
    K = len(members)
    if not 2 <= K <= 32:
        raise ValueError(f'ensemble_mi: 2..32 members are supported, got {K}')
    L = len(members[0])
    if not 1 <= L <= 8:
        raise ValueError(f'ensemble_mi: 1..8 levels are supported, got {L}')
    n_cls = int(n_cls)
    if n_cls < 1:
        raise ValueError(f'ensemble_mi: n_cls must be positive, got {n_cls}')
    first = members[0]
    for k, m in enumerate(members):
        if len(m) != L:
            raise ValueError(f'ensemble_mi: member {k} has {len(m)} levels, member 0 has {L}')
        for l, t in enumerate(m):
            if not torch.is_tensor(t) or t.dtype != torch.float32:
                raise ValueError(f'ensemble_mi: member {k} level {l} is not an fp32 tensor')
            if t.dim() < 1 or tuple(t.shape) != tuple(first[l].shape):
                raise ValueError(f'ensemble_mi: member {k} level {l} has shape {tuple(t.shape)}, member 0 has {tuple(first[l].shape)}')
    B = int(first[0].shape[0])
    n = []
    for l, t in enumerate(first):
        if int(t.shape[0]) != B or B < 1 or t.numel() == 0:
            raise ValueError(f'ensemble_mi: level {l} has shape {tuple(t.shape)}; every level needs the same positive batch size')
        if (t.numel() // B) % n_cls:
            raise ValueError(f'ensemble_mi: level {l} holds {t.numel() // B} elements per image, not a multiple of n_cls = {n_cls}')
        n.append(t.numel() // B)
    dev = first[0].device
    for k, m in enumerate(members):
        for l, t in enumerate(m):
            if not t.is_cuda:
                raise _C.AodHipError('ensemble_mi needs tensors on the MI355X (cuda:N); got a CPU tensor. There is no CPU fallback.')
            if t.device != dev:
                raise ValueError(f'ensemble_mi: member {k} level {l} lives on {t.device}, member 0 on {dev}')
            if not _dense(t):
                raise ValueError(f'ensemble_mi: member {k} level {l} is not dense (contiguous or channels_last); no copy is made here')
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B,) and out.is_contiguous()):
        raise ValueError(f'ensemble_mi: out must be a contiguous fp32 device tensor of shape ({B},)')
    sizes = (C.c_int64 * L)(*n)
    cap = int(_C.lib.aod_ensemble_mi_partials_len(L, sizes, B))
    ws = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
    call('aod_ensemble_mi', (C.c_void_p * (K * L))(*[t.data_ptr() for m in members for t in m]), K, L, sizes, B, n_cls, ptr(out), ptr(ws), cap,
         stream())
    return out


def pool_descriptor(feats, out=None, channels=None, x3=None):
    """Core-set descriptor of every image of a batch (aod_pool_descriptor): the concatenation over pyramid levels of the global average of
    the neck output, [B, D] fp32 with D = L * C (RetinaNet: 5 * 256 = 1280).

    feats: 1..8 per-level maps [B, width, h_l, w_l], bf16 channels_last device tensors as the neck hands them out (views of the pyramid
    buffer; nothing is copied): plain bf16 (width = C) or X-layout rows (width = 2 * ceil32(C); value = head + tail).  x3: the layout,
    default the current precision mode; channels: C of an X-layout map whose width is padded (default width / 2).  C % 8 == 0.
    out: a [B, D] fp32 device view with unit column stride (e.g. rows of the [N, D] pool matrix).  The bits of a row depend on its image
    alone -- not on B or on its place in the batch.  No host sync."""
    from . import hipops as ho
    feats = list(feats)
    L = len(feats)
    if not 1 <= L <= 8:
        raise ValueError(f'pool_descriptor: 1..8 levels are supported, got {L}')
    x3 = bool(ho.X3 if x3 is None else x3)
    for l, t in enumerate(feats):
        if not torch.is_tensor(t) or t.dtype != torch.bfloat16 or t.dim() != 4:
            raise ValueError(f'pool_descriptor: level {l} is not a bf16 [B, width, h, w] tensor')
        if t.shape[0] != feats[0].shape[0] or t.shape[1] != feats[0].shape[1] or t.numel() == 0:
            raise ValueError(f'pool_descriptor: level {l} has shape {tuple(t.shape)}, level 0 has {tuple(feats[0].shape)}: every level needs the '
                             'same positive batch size and width')
        if not t.permute(0, 2, 3, 1).is_contiguous():
            raise ValueError(f'pool_descriptor: level {l} is not channels_last-dense; no copy is made here')
    B, Wd = int(feats[0].shape[0]), int(feats[0].shape[1])
    if x3 and Wd % 64:
        raise ValueError(f'pool_descriptor: X-layout rows are a multiple of 64 columns wide, got {Wd}')
    Cc = int(channels) if channels is not None else (Wd // 2 if x3 else Wd)
    if Cc < 8 or Cc % 8 or (ho.xw(Cc) if x3 else Cc) != Wd:
        raise ValueError(f'pool_descriptor: {Cc} channels (a positive multiple of 8) do not make rows of {Wd} columns')
    D = L * Cc
    for t in feats:
        if not t.is_cuda:
            raise _C.AodHipError('pool_descriptor needs tensors on the MI355X (cuda:N); got a CPU tensor. There is no CPU fallback.')
    dev = feats[0].device
    if out is None:
        out = torch.empty(B, D, dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, D) and out.stride(1) == 1
              and out.stride(0) >= D):
        raise ValueError(f'pool_descriptor: out must be an fp32 device tensor of shape ({B}, {D}) with unit column stride')
    hw = [int(t.shape[2] * t.shape[3]) for t in feats]
    rb = Wd * 2
    base = min(t.data_ptr() for t in feats)
    offs = [t.data_ptr() - base for t in feats]
    if all(o % rb == 0 for o in offs):          # the levels are row ranges of one buffer (functional.pyramid_buffer): one launch
        groups = [(base, list(range(L)), [o // rb for o in offs])]
    else:
        groups = [(t.data_ptr(), [l], [0]) for l, t in enumerate(feats)]
    for p, ls, rows in groups:
        n = len(ls)
        call('aod_pool_descriptor', C.c_void_p(p), n, (C.c_int64 * n)(*rows), (C.c_int32 * n)(*[hw[l] for l in ls]), Cc, int(x3), B,
             C.c_void_p(out.data_ptr() + 4 * ls[0] * Cc), out.stride(0), stream())
    return out


def kcenter_chunk():
    """labelled centers one initialisation launch of kcenter_greedy stages in LDS"""
    return int(_C.lib.aod_kcenter_chunk())


KCENTER_METRICS = {'sqeuclid': 0, 'symkl': 1}


def kcenter_greedy(desc, labelled, budget, metric='sqeuclid'):
    """k-center greedy selection (Sener & Savarese, ICLR 2018, Algorithm 1) on the aod_kcenter_greedy kernels: starting from the labelled
    rows as centers, `budget` times pick the unselected row farthest (squared Euclidean distance, direct difference form, fp32) from its
    nearest center -- the lowest index on a tie -- and make it a center.
    metric: 'sqeuclid' (Core-set) or 'symkl' (CDAL): a row is [P | ln P], two halves of D / 2 columns (D even), and
    d(i, j) = 1/2 sum_k max((P_ik - P_jk)(ln P_ik - ln P_jk), 0), the symmetrised KL divergence summed over the classes.

    desc: [N, D] fp32 contiguous device tensor (D <= 2048); labelled: distinct row indices in [0, N) (sequence, array or tensor; may be
    empty: the first pick is then row 0 with radius inf); 1 <= budget <= number of unlabelled rows.
    Returns (picks [budget] int64, radius [budget] fp32) on the device, radius[t] = the distance of pick t at the time it was picked
    (non-increasing).  All steps are enqueued on the current stream; no host sync.  The result does not depend on the order of `labelled`."""
    if metric not in KCENTER_METRICS:
        raise ValueError(f"kcenter_greedy: unknown metric {metric!r} (expected 'sqeuclid' or 'symkl')")
    if not (torch.is_tensor(desc) and desc.dim() == 2 and desc.dtype == torch.float32 and desc.is_contiguous() and desc.numel() > 0):
        raise ValueError('kcenter_greedy: desc must be a non-empty contiguous 2-D fp32 tensor')
    N, D = int(desc.shape[0]), int(desc.shape[1])
    if D > 2048:
        raise ValueError(f'kcenter_greedy: up to 2048 descriptor columns are supported, got {D}')
    if metric == 'symkl' and D % 2:
        raise ValueError(f"kcenter_greedy: metric 'symkl' reads a row as two halves [P | ln P]; D = {D} is odd")
    if metric == 'sqeuclid':
        return _kcenter_run('kcenter_greedy', 'aod_kcenter_greedy', desc, (N, D), labelled, budget)
    return _kcenter_run('kcenter_greedy', 'aod_kcenter_greedy_ex', desc, (N, D), labelled, budget, KCENTER_METRICS[metric])


def _index_array(name, idx, N, arg='labelled', distinct=True, noun='labelled'):
    """`idx` (tensor, array or sequence of row indices) as a validated int64 array; the messages carry the caller's `name` (and `noun`,
    what the range and duplicate messages call the set)"""
    lab = idx.detach().cpu().numpy() if torch.is_tensor(idx) else np.asarray(idx)
    lab = lab.reshape(-1)
    if lab.size and not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f'{name}: {arg} must hold integer indices, got {lab.dtype}')
    lab = lab.astype(np.int64)
    if lab.size and (lab.min() < 0 or lab.max() >= N):
        raise ValueError(f'{name}: {noun} index outside [0, {N})')
    if distinct and np.unique(lab).size != lab.size:
        raise ValueError(f'{name}: {noun} holds a duplicated index')
    return lab


def _kcenter_run(name, entry, x, dims, labelled, budget, *tail):
    """what kcenter_greedy and kcenter_greedy_matrix share once `x` (desc or dist; dims = the entry's size arguments, N first) is checked:
    the labelled and budget checks, the CPU refusal, the outputs and the workspace, the call of `entry` and the return"""
    N = dims[0]
    lab = _index_array(name, labelled, N)
    budget = int(budget)
    if budget < 1:
        raise ValueError(f'{name}: budget must be at least 1, got {budget}')
    if budget > N - lab.size:
        raise ValueError(f'{name}: budget {budget} exceeds the {N - lab.size} unselected rows')
    if not x.is_cuda:
        raise _cpu_refusal(name)
    dev = x.device
    lab_d = torch.from_numpy(lab).to(dev) if lab.size else None
    picks = torch.empty(budget, dtype=torch.int64, device=dev)
    radius = torch.empty(budget, dtype=torch.float32, device=dev)
    mind = torch.empty(N, dtype=torch.float32, device=dev)
    ws = torch.empty(int(_C.lib.aod_kcenter_ws_len(N)), dtype=torch.uint8, device=dev)
    call(entry, ptr(x), *dims, ptr(lab_d), int(lab.size), budget, ptr(picks), ptr(radius), ptr(mind), ptr(ws), stream(), *tail)
    return picks, radius


CDAL_MAX_CLASSES = 32      # 2 C^2 <= 2048 columns, the k-center kernels' LDS limit


def cdal_descriptor(maps, n_cls, score_thr=0.3, out=None):
    """CDAL class-mixture descriptor of every image of a batch (aod_cdal_descriptor; Agarwal et al., "Contextual Diversity for Active
    Learning", ECCV 2020): [B, 2 * n_cls^2] fp32 = [P | ln P].  Per anchor row p = softmax(logits); a row is a region iff
    max p > score_thr (strict), its class the argmax (lowest index on a tie), its weight H(p) + 2^-10; P[c] = (1 - 2^-10) * (the weighted
    mean of p over the regions of class c, uniform where there is none) + 2^-10 / n_cls.

    maps: 1..8 per-level fp32 device logit maps, either [B, A * n_cls, h, w] channels_last-dense as the head hands them out (the n_cls
    logits of an anchor are then contiguous: nhwc_view's [B, A_l, n_cls] without a copy) or [B, rows, n_cls] contiguous.  n_cls <= 32.
    out: a [B, D] fp32 device view with unit column stride (e.g. rows of the [N, D] pool matrix).  The bits of a row depend on its image
    alone -- not on B or on its place in the batch.  No host sync."""
    maps = list(maps)
    L = len(maps)
    if not 1 <= L <= 8:
        raise ValueError(f'cdal_descriptor: 1..8 levels are supported, got {L}')
    n_cls = int(n_cls)
    if n_cls < 1:
        raise ValueError(f'cdal_descriptor: n_cls must be positive, got {n_cls}')
    if n_cls > CDAL_MAX_CLASSES:
        raise ValueError(f'cdal_descriptor: up to {CDAL_MAX_CLASSES} classes are supported (2 * n_cls^2 <= 2048 descriptor columns, the k-center '
                         f'kernels\' limit), got n_cls = {n_cls}')
    score_thr = float(score_thr)
    if score_thr != score_thr:
        raise ValueError('cdal_descriptor: score_thr is NaN')
    rows = []
    for l, t in enumerate(maps):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() not in (3, 4):
            raise ValueError(f'cdal_descriptor: level {l} is not an fp32 [B, A * n_cls, h, w] or [B, rows, n_cls] tensor')
        if t.shape[0] != maps[0].shape[0] or t.numel() == 0:
            raise ValueError(f'cdal_descriptor: level {l} has shape {tuple(t.shape)}, level 0 has {tuple(maps[0].shape)}: every level needs the '
                             'same positive batch size')
        if t.dim() == 3:
            if t.shape[2] != n_cls:
                raise ValueError(f'cdal_descriptor: level {l} has rows of {t.shape[2]} columns, not n_cls = {n_cls}')
            dense = t.is_contiguous()
        else:
            if t.shape[1] % n_cls:
                raise ValueError(f'cdal_descriptor: level {l} has {t.shape[1]} channels, not a multiple of n_cls = {n_cls}')
            dense = t.permute(0, 2, 3, 1).is_contiguous()
        if not dense:
            raise ValueError(f'cdal_descriptor: level {l} is not dense with the classes of a row contiguous (channels_last for a 4-D map); no '
                             'copy is made here')
        rows.append(t.numel() // int(t.shape[0]) // n_cls)
    B, D = int(maps[0].shape[0]), 2 * n_cls * n_cls
    for t in maps:
        if not t.is_cuda:
            raise _C.AodHipError('cdal_descriptor needs tensors on the MI355X (cuda:N); got a CPU tensor. There is no CPU fallback.')
    dev = maps[0].device
    if out is None:
        out = torch.empty(B, D, dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, D) and out.stride(1) == 1
              and out.stride(0) >= D):
        raise ValueError(f'cdal_descriptor: out must be an fp32 device tensor of shape ({B}, {D}) with unit column stride')
    sizes = (C.c_int64 * L)(*rows)
    cap = int(_C.lib.aod_cdal_ws_len(L, sizes, n_cls, B))
    ws = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
    call('aod_cdal_descriptor', (C.c_void_p * L)(*[t.data_ptr() for t in maps]), L, sizes, n_cls, B, score_thr, ptr(out), out.stride(0), ptr(ws),
         cap, stream())
    return out


POSTERIOR_POOLS = ('Entropy', 'Margin', 'LeastConf')
UNC_LAYOUTS = {'cat': 0, 'cat_bg': 1, 'sigmoid': 2}
UNC_MEASURES = {'entropy': 0, 'margin': 1, 'leastconf': 2}
UNC_AGGREGATES = {'max': 0, 'mean': 1, 'sum': 2}
POOL_MEASURE = {'Entropy': 'entropy', 'Margin': 'margin', 'LeastConf': 'leastconf'}
ACTIVATION_LAYOUT = {'relu': 'cat', 'softmax': 'cat_bg', 'sigmoid': 'sigmoid'}      # head.last_activation -> the posterior's row layout
UNC_MAX_DET = 1024


def det_uncertainty(cand, dets, labels, num, layout, measure='entropy', aggregate='max', score_thr=0.3, want_objects=False, want_cand=False,
                    class_w=None):
    """Posterior uncertainty of every image of a batch (aod_det_uncertainty): entropy, 1-vs-2 margin or least confidence of the
    class posterior of every detection, aggregated over the image's detections by max, mean or sum; an image without an object scores 0.

    cand: the Candidates of pre_nms (boxes [B, n, 4], scores [B, n, W]); dets [B, max_num, 5], labels [B, max_num] int64, num [B] int32: the
    outputs of multiclass_nms_batch on them.  layout: 'cat' (the first W - 1 columns are one categorical distribution: the Lambda_L2Net
    family), 'cat_bg' (all W columns, background last: MyLSSDHead) or 'sigmoid' (the first W - 1 columns are independent Bernoulli
    posteriors: MyRetinaHead).  A detection row j < num[b] with a score > score_thr (strict) is an object; its score row is looked up among
    the candidates by its box and score bits.  Returns unc [B] fp32 on the device (no host sync), or with want_objects
    (unc, obj_out [B, max_num] fp32 -- NaN where the row is no object --, missing [B] int32 -- objects without a candidate row: always 0).
    want_cand (aod_det_uncertainty_ex; the same unc bits) appends obj_cand [B, max_num] int32: the candidate row matched to every object
    row, -1 elsewhere -- what object_descriptors reads.
    class_w (aod_det_uncertainty_w): fp32 [W] device tensor; the measure of an object with label l is multiplied by class_w[l]
    before it is written to obj_out and enters the aggregate.  None: no multiply (all ones give the same bits)."""
    if layout not in UNC_LAYOUTS:
        raise ValueError(f"det_uncertainty: unknown layout {layout!r} (expected 'cat', 'cat_bg' or 'sigmoid')")
    if measure not in UNC_MEASURES:
        raise ValueError(f"det_uncertainty: unknown measure {measure!r} (expected 'entropy', 'margin' or 'leastconf')")
    if aggregate not in UNC_AGGREGATES:
        raise ValueError(f"det_uncertainty: unknown aggregate {aggregate!r} (expected 'max', 'mean' or 'sum')")
    score_thr = float(score_thr)
    if score_thr != score_thr:
        raise ValueError('det_uncertainty: score_thr is NaN')
    boxes, scores = getattr(cand, 'boxes', None), getattr(cand, 'scores', None)
    for name, t, dt, nd in (('cand.boxes', boxes, torch.float32, 3), ('cand.scores', scores, torch.float32, 3), ('dets', dets, torch.float32, 3),
                            ('labels', labels, torch.int64, 2), ('num', num, torch.int32, 1)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != nd:
            raise ValueError(f"det_uncertainty: {name} is not a {nd}-D {str(dt).replace('torch.', '')} tensor")
        if not t.is_contiguous():
            raise ValueError(f'det_uncertainty: {name} is not contiguous; no copy is made here')
    B, n, W = (int(v) for v in scores.shape)
    if B < 1 or n < 1:
        raise ValueError(f'det_uncertainty: cand.scores has shape {tuple(scores.shape)}; a positive batch size and candidate count are needed')
    if tuple(boxes.shape) != (B, n, 4):
        raise ValueError(f'det_uncertainty: cand.boxes has shape {tuple(boxes.shape)}, cand.scores {tuple(scores.shape)}: expected ({B}, {n}, 4)')
    if W < 2:
        raise ValueError(f'det_uncertainty: cand.scores rows of at least 2 columns are needed, got {W}')
    used = W if layout == 'cat_bg' else W - 1
    if measure == 'margin' and used < 2:
        raise ValueError(f"det_uncertainty: measure 'margin' needs two used columns; layout {layout!r} reads {used} of the {W} of cand.scores")
    if dets.shape[0] != B or dets.shape[2] != 5 or not 1 <= dets.shape[1] <= UNC_MAX_DET:
        raise ValueError(f'det_uncertainty: dets has shape {tuple(dets.shape)}: expected ({B}, max_num, 5) with 1 <= max_num <= {UNC_MAX_DET}')
    max_num = int(dets.shape[1])
    if tuple(labels.shape) != (B, max_num):
        raise ValueError(f'det_uncertainty: labels has shape {tuple(labels.shape)}, expected ({B}, {max_num})')
    if tuple(num.shape) != (B,):
        raise ValueError(f'det_uncertainty: num has shape {tuple(num.shape)}, expected ({B},)')
    ts = (boxes, scores, dets, labels, num)
    if class_w is not None:
        if not torch.is_tensor(class_w) or class_w.dtype != torch.float32 or tuple(class_w.shape) != (W,):
            raise ValueError(f'det_uncertainty: class_w must be an fp32 tensor of shape ({W},): one weight per column of cand.scores')
        if not class_w.is_contiguous():
            raise ValueError('det_uncertainty: class_w is not contiguous; no copy is made here')
        ts = ts + (class_w,)
    for t in ts:
        if not t.is_cuda:
            raise _C.AodHipError('det_uncertainty needs tensors on the MI355X (cuda:N); got a CPU tensor. There is no CPU fallback.')
    dev = scores.device
    if any(t.device != dev for t in ts):
        raise ValueError(f'det_uncertainty: the tensors live on different devices ({sorted({str(t.device) for t in ts})})')
    unc = torch.empty(B, dtype=torch.float32, device=dev)
    obj_out = torch.empty(B, max_num, dtype=torch.float32, device=dev) if want_objects else None
    missing = torch.empty(B, dtype=torch.int32, device=dev) if want_objects else None
    if class_w is not None:
        obj_cand = torch.empty(B, max_num, dtype=torch.int32, device=dev) if want_cand else None
        call('aod_det_uncertainty_w', ptr(boxes), ptr(scores), ptr(dets), ptr(labels), ptr(num), B, n, W, max_num, UNC_LAYOUTS[layout],
             UNC_MEASURES[measure], UNC_AGGREGATES[aggregate], score_thr, ptr(unc), ptr(obj_out), ptr(missing), ptr(obj_cand), ptr(class_w), stream())
        out = (unc,) + ((obj_out, missing) if want_objects else ()) + ((obj_cand,) if want_cand else ())
        return out if len(out) > 1 else unc
    if want_cand:
        obj_cand = torch.empty(B, max_num, dtype=torch.int32, device=dev)
        call('aod_det_uncertainty_ex', ptr(boxes), ptr(scores), ptr(dets), ptr(labels), ptr(num), B, n, W, max_num, UNC_LAYOUTS[layout],
             UNC_MEASURES[measure], UNC_AGGREGATES[aggregate], score_thr, ptr(unc), ptr(obj_out), ptr(missing), ptr(obj_cand), stream())
        return (unc, obj_out, missing, obj_cand) if want_objects else (unc, obj_cand)
    call('aod_det_uncertainty', ptr(boxes), ptr(scores), ptr(dets), ptr(labels), ptr(num), B, n, W, max_num, UNC_LAYOUTS[layout],
         UNC_MEASURES[measure], UNC_AGGREGATES[aggregate], score_thr, ptr(unc), ptr(obj_out), ptr(missing), stream())
    return (unc, obj_out, missing) if want_objects else unc


CCMS_MAX_OBJ = 64
CCMS_MAX_CHANNELS = 256
CCMS_MAX_IMAGES = int(_C.lib.aod_ccms_max_images())      # (written once, in csrc/ccms.hip)


def _cpu_refusal(name):
    return _C.AodHipError(f'{name} needs tensors on the MI355X (cuda:N); got a CPU tensor. There is no CPU fallback.')


def object_descriptors(feats, cand, dets, labels, num, obj_cand, num_anchors, max_obj=32, score_thr=0.3, channels=None, x3=None):
    """Object descriptors of every image of a batch (aod_object_descriptors): per detection with a score > score_thr (strict;
    the first max_obj of them in row order) the L2-normalised neck output row of the cell its anchor sits in.

    feats: 1..8 per-level maps [B, width, h_l, w_l], bf16 channels_last device tensors as the neck hands them out (plain bf16 or X-layout
    rows, as pool_descriptor takes them; `channels` / `x3` likewise).  cand: the Candidates of pre_nms (cand_anchor [B, n] int32 is read);
    dets [B, max_num, 5], labels [B, max_num] int64, num [B] int32: the outputs of multiclass_nms_batch; obj_cand [B, max_num] int32: the
    matched candidate rows of det_uncertainty(..., want_cand=True) with the same score_thr.  num_anchors: anchors per cell, one int or one
    per level.  Returns (feat [B, max_obj, C] fp32, cls [B, max_obj] int32 (-1 pad), w [B, max_obj] fp32 (0 pad), cnt [B] int32,
    missing [B] int32: objects without a candidate row, always 0) on the device, no host sync.  An image's rows have the same bits alone
    and inside any batch."""
    from . import hipops as ho
    feats = list(feats)
    L = len(feats)
    if not 1 <= L <= 8:
        raise ValueError(f'object_descriptors: 1..8 levels are supported, got {L}')
    x3 = bool(ho.X3 if x3 is None else x3)
    for l, t in enumerate(feats):
        if not torch.is_tensor(t) or t.dtype != torch.bfloat16 or t.dim() != 4:
            raise ValueError(f'object_descriptors: level {l} is not a bf16 [B, width, h, w] tensor')
        if t.shape[0] != feats[0].shape[0] or t.shape[1] != feats[0].shape[1] or t.numel() == 0:
            raise ValueError(f'object_descriptors: level {l} has shape {tuple(t.shape)}, level 0 has {tuple(feats[0].shape)}: every level needs '
                             'the same positive batch size and width')
        if not t.permute(0, 2, 3, 1).is_contiguous():
            raise ValueError(f'object_descriptors: level {l} is not channels_last-dense; no copy is made here')
    B, Wd = int(feats[0].shape[0]), int(feats[0].shape[1])
    if x3 and Wd % 64:
        raise ValueError(f'object_descriptors: X-layout rows are a multiple of 64 columns wide, got {Wd}')
    Cc = int(channels) if channels is not None else (Wd // 2 if x3 else Wd)
    if Cc < 8 or Cc % 8 or Cc > 1024 or (ho.xw(Cc) if x3 else Cc) != Wd:
        raise ValueError(f'object_descriptors: {Cc} channels (a multiple of 8 in 8..1024) do not make rows of {Wd} columns')
    na = [int(v) for v in num_anchors] if isinstance(num_anchors, (list, tuple)) else [int(num_anchors)] * L
    if len(na) != L or min(na) < 1:
        raise ValueError(f'object_descriptors: num_anchors {num_anchors!r} does not name a positive count for each of the {L} levels')
    max_obj = int(max_obj)
    if not 1 <= max_obj <= CCMS_MAX_OBJ:
        raise ValueError(f'object_descriptors: max_obj must be in 1..{CCMS_MAX_OBJ}, got {max_obj}')
    score_thr = float(score_thr)
    if score_thr != score_thr:
        raise ValueError('object_descriptors: score_thr is NaN')
    anchor = getattr(cand, 'cand_anchor', None)
    for name, t, dt, nd in (('cand.cand_anchor', anchor, torch.int32, 2), ('dets', dets, torch.float32, 3), ('labels', labels, torch.int64, 2),
                            ('num', num, torch.int32, 1), ('obj_cand', obj_cand, torch.int32, 2)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != nd:
            raise ValueError(f"object_descriptors: {name} is not a {nd}-D {str(dt).replace('torch.', '')} tensor")
        if not t.is_contiguous():
            raise ValueError(f'object_descriptors: {name} is not contiguous; no copy is made here')
    n = int(anchor.shape[1])
    if anchor.shape[0] != B or n < 1:
        raise ValueError(f'object_descriptors: cand.cand_anchor has shape {tuple(anchor.shape)}: expected ({B}, n) with n >= 1')
    if dets.shape[0] != B or dets.shape[2] != 5 or not 1 <= dets.shape[1] <= UNC_MAX_DET:
        raise ValueError(f'object_descriptors: dets has shape {tuple(dets.shape)}: expected ({B}, max_num, 5) with 1 <= max_num <= {UNC_MAX_DET}')
    max_num = int(dets.shape[1])
    for name, t in (('labels', labels), ('obj_cand', obj_cand)):
        if tuple(t.shape) != (B, max_num):
            raise ValueError(f'object_descriptors: {name} has shape {tuple(t.shape)}, expected ({B}, {max_num})')
    if tuple(num.shape) != (B,):
        raise ValueError(f'object_descriptors: num has shape {tuple(num.shape)}, expected ({B},)')
    ts = feats + [anchor, dets, labels, num, obj_cand]
    for t in ts:
        if not t.is_cuda:
            raise _cpu_refusal('object_descriptors')
    dev = dets.device
    if any(t.device != dev for t in ts):
        raise ValueError(f'object_descriptors: the tensors live on different devices ({sorted({str(t.device) for t in ts})})')
    feat = torch.empty(B, max_obj, Cc, dtype=torch.float32, device=dev)
    cls = torch.empty(B, max_obj, dtype=torch.int32, device=dev)
    w = torch.empty(B, max_obj, dtype=torch.float32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    missing = torch.empty(B, dtype=torch.int32, device=dev)
    call('aod_object_descriptors', (C.c_void_p * L)(*[t.data_ptr() for t in feats]), L, (C.c_int32 * L)(*[int(t.shape[2] * t.shape[3]) for t in feats]),
         (C.c_int32 * L)(*na), Cc, int(x3), B, ptr(anchor), n, ptr(dets), ptr(labels), ptr(num), ptr(obj_cand), max_num, max_obj, score_thr,
         ptr(feat), ptr(cls), ptr(w), ptr(cnt), ptr(missing), stream())
    return feat, cls, w, cnt, missing


def ccms_distance(feat, cls, w, cnt):
    """Category-conditioned matching distance between the images of a candidate set (aod_ccms_distance; PPAL, Yang et al., CVPR
    2024): d(a, b) = max(0, 1 - (S(a->b) + S(b->a)) / 2), S(a->b) the w-weighted mean over a's objects of the largest non-negative cosine
    to an object of the same class in b.

    feat [M, max_obj, C] fp32, cls [M, max_obj] int32, w [M, max_obj] fp32, cnt [M] int32: contiguous device tensors as object_descriptors
    writes them (rows >= cnt are not used); M <= 32768, max_obj <= 64, C % 8 == 0, C <= 256.  Returns dist [M, M] fp32 on the device, no
    host sync: exactly symmetric, zero diagonal, every entry a function of its two images alone."""
    for name, t, dt, nd in (('feat', feat, torch.float32, 3), ('cls', cls, torch.int32, 2), ('w', w, torch.float32, 2), ('cnt', cnt, torch.int32, 1)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != nd:
            raise ValueError(f"ccms_distance: {name} is not a {nd}-D {str(dt).replace('torch.', '')} tensor")
        if not t.is_contiguous():
            raise ValueError(f'ccms_distance: {name} is not contiguous; no copy is made here')
    M, K, Cc = (int(v) for v in feat.shape)
    if not 1 <= M <= CCMS_MAX_IMAGES:
        raise ValueError(f'ccms_distance: feat has shape {tuple(feat.shape)}: 1..{CCMS_MAX_IMAGES} images are supported')
    if not 1 <= K <= CCMS_MAX_OBJ:
        raise ValueError(f'ccms_distance: feat has shape {tuple(feat.shape)}: 1..{CCMS_MAX_OBJ} objects per image are supported')
    if Cc < 8 or Cc % 8 or Cc > CCMS_MAX_CHANNELS:
        raise ValueError(f'ccms_distance: feat has shape {tuple(feat.shape)}: the channels must be a multiple of 8 in 8..{CCMS_MAX_CHANNELS}')
    for name, t in (('cls', cls), ('w', w)):
        if tuple(t.shape) != (M, K):
            raise ValueError(f'ccms_distance: {name} has shape {tuple(t.shape)}, expected ({M}, {K})')
    if tuple(cnt.shape) != (M,):
        raise ValueError(f'ccms_distance: cnt has shape {tuple(cnt.shape)}, expected ({M},)')
    ts = (feat, cls, w, cnt)
    for t in ts:
        if not t.is_cuda:
            raise _cpu_refusal('ccms_distance')
    dev = feat.device
    if any(t.device != dev for t in ts):
        raise ValueError(f'ccms_distance: the tensors live on different devices ({sorted({str(t.device) for t in ts})})')
    dist = torch.empty(M, M, dtype=torch.float32, device=dev)
    call('aod_ccms_distance', ptr(feat), ptr(cls), ptr(w), ptr(cnt), M, K, Cc, ptr(dist), stream())
    return dist


def kcenter_greedy_matrix(dist, labelled, budget):
    """kcenter_greedy on a precomputed distance matrix (aod_kcenter_greedy_matrix): dist [N, N] fp32 contiguous device tensor with
    non-negative entries; labelled, budget and the returned (picks [budget] int64, radius [budget] fp32) as kcenter_greedy's -- the same
    tie rule (lowest index), the first pick is row 0 with radius inf when `labelled` is empty, no host sync, and the result does not depend
    on the order of `labelled`."""
    if not (torch.is_tensor(dist) and dist.dim() == 2 and dist.dtype == torch.float32 and dist.is_contiguous() and dist.numel() > 0
            and dist.shape[0] == dist.shape[1]):
        raise ValueError('kcenter_greedy_matrix: dist must be a non-empty contiguous square 2-D fp32 tensor'
                         + (f', got shape {tuple(dist.shape)}' if torch.is_tensor(dist) else ''))
    return _kcenter_run('kcenter_greedy_matrix', 'aod_kcenter_greedy_matrix', dist, (int(dist.shape[0]),), labelled, budget)


def ccms_candidates(unc, X_L, budget, factor=4):
    """Stage 1 of the CCMS pick, on the host: the images not in X_L ordered by `unc` descending -- ties by ascending index --
    cut to M = min(ceil(factor * budget), number of unlabelled images).  Returns the int64 index array [M]; row 0 is the most uncertain
    candidate.  M < budget (too few unlabelled images, or factor < 1) and M > 32768 (the distance matrix's limit) raise ValueError."""
    u = unc.detach().cpu().numpy() if torch.is_tensor(unc) else np.asarray(unc)
    u = u.reshape(-1).astype(np.float64)
    N = u.size
    lab = _index_array('ccms_candidates', X_L, N, arg='X_L', distinct=False)
    budget, factor = int(budget), float(factor)
    if budget < 1:
        raise ValueError(f'ccms_candidates: budget must be at least 1, got {budget}')
    if not factor > 0 or factor == float('inf'):
        raise ValueError(f'ccms_candidates: candidate_factor must be positive and finite, got {factor}')
    if np.isnan(u).any():
        raise ValueError('ccms_candidates: the stage-1 scores hold a NaN')
    free = np.ones(N, bool)
    free[lab] = False
    idx = np.nonzero(free)[0]
    M = min(int(np.ceil(factor * budget)), idx.size)
    if M < budget:
        raise ValueError(f'ccms_candidates: {M} candidates (candidate_factor {factor:g}, {idx.size} unlabelled images) are fewer than the '
                         f'budget {budget}')
    if M > CCMS_MAX_IMAGES:
        raise ValueError(f'ccms_candidates: {M} candidates exceed the {CCMS_MAX_IMAGES} images of one distance matrix; lower candidate_factor')
    order = idx[np.argsort(-u[idx], kind='stable')]          # (idx ascends: a stable sort breaks ties by ascending index)
    return order[:M].astype(np.int64)


DIVPROTO_MAX_CLASSES = 128


def divproto_chunk():
    """sweep positions one selection launch of divproto_select handles"""
    return int(_C.lib.aod_divproto_chunk())


def _check_tensors(name, specs):
    """dtype, dim and contiguity of (name, tensor, dtype, ndim) specs: ccms_distance's checks and messages under the caller's `name`"""
    for n, t, dt, nd in specs:
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != nd:
            raise ValueError(f"{name}: {n} is not a {nd}-D {str(dt).replace('torch.', '')} tensor")
        if not t.is_contiguous():
            raise ValueError(f'{name}: {n} is not contiguous; no copy is made here')


def _check_devices(name, ts):
    for t in ts:
        if not t.is_cuda:
            raise _cpu_refusal(name)
    if any(t.device != ts[0].device for t in ts):
        raise ValueError(f'{name}: the tensors live on different devices ({sorted({str(t.device) for t in ts})})')


def _check_obj_shape(name, what, shape):
    N, K, Cc = (int(v) for v in shape)
    if N < 1:
        raise ValueError(f'{name}: {what} has shape {tuple(shape)}: at least one image is needed')
    if not 1 <= K <= CCMS_MAX_OBJ:
        raise ValueError(f'{name}: {what} has shape {tuple(shape)}: 1..{CCMS_MAX_OBJ} objects per image are supported')
    if Cc < 8 or Cc % 8 or Cc > CCMS_MAX_CHANNELS:
        raise ValueError(f'{name}: {what} has shape {tuple(shape)}: the channels must be a multiple of 8 in 8..{CCMS_MAX_CHANNELS}')
    return N, K, Cc


def object_measure(obj_out, dets, num, obj_cand=None, max_obj=32, score_thr=0.3):
    """The per-object posterior measure in object_descriptors' slots (aod_object_measure): h [B, max_obj] fp32 = obj_out
    (det_uncertainty(..., want_objects=True)'s [B, max_num], the class weight included when it ran class-weighted) at the detection rows
    j < num[b] whose score exceeds score_thr (strict), the first max_obj in row order -- object_descriptors' own slot rule, obj_cand (its
    matched candidate rows; a row without one takes no slot) included; 0 behind them.  Device tensors, no host sync."""
    _check_tensors('object_measure', (('obj_out', obj_out, torch.float32, 2), ('dets', dets, torch.float32, 3), ('num', num, torch.int32, 1))
                   + ((('obj_cand', obj_cand, torch.int32, 2),) if obj_cand is not None else ()))
    B, max_num = (int(v) for v in obj_out.shape)
    max_obj, score_thr = int(max_obj), float(score_thr)
    if B < 1 or not 1 <= max_num <= UNC_MAX_DET or tuple(dets.shape) != (B, max_num, 5) or tuple(num.shape) != (B,):
        raise ValueError(f'object_measure: obj_out {tuple(obj_out.shape)}, dets {tuple(dets.shape)}, num {tuple(num.shape)}: expected (B, max_num), '
                         f'(B, max_num, 5), (B,) with 1 <= max_num <= {UNC_MAX_DET}')
    if obj_cand is not None and tuple(obj_cand.shape) != (B, max_num):
        raise ValueError(f'object_measure: obj_cand has shape {tuple(obj_cand.shape)}, expected ({B}, {max_num})')
    if not 1 <= max_obj <= CCMS_MAX_OBJ:
        raise ValueError(f'object_measure: max_obj must be in 1..{CCMS_MAX_OBJ}, got {max_obj}')
    if score_thr != score_thr:
        raise ValueError('object_measure: score_thr is NaN')
    _check_devices('object_measure', [obj_out, dets, num] + ([obj_cand] if obj_cand is not None else []))
    h = torch.empty(B, max_obj, dtype=torch.float32, device=obj_out.device)
    call('aod_object_measure', ptr(obj_out), ptr(dets), ptr(num), ptr(obj_cand), B, max_num, max_obj, score_thr, ptr(h), stream())
    return h


BADGE_MAX_CLASSES = 128
KMEANSPP_MAX_COLUMNS = 32768
KMEANSPP_MAX_ROWS = 1 << 24


def object_posterior(scores, dets, num, obj_cand, max_obj=32, score_thr=0.3):
    """The candidate score row of every object in object_descriptors' slots (aod_object_posterior): post [B, max_obj, W] fp32 =
    scores[b, obj_cand[b, j], :] (scores = cand.scores [B, n, W], W columns as they lie) at the detection rows j < num[b] whose score
    exceeds score_thr (strict) and that have a candidate row, the first max_obj in row order -- object_measure's slot rule; zero rows
    behind them (every word is written: a replayed graph never exposes stale rows).  Device tensors, no host sync."""
    _check_tensors('object_posterior', (('scores', scores, torch.float32, 3), ('dets', dets, torch.float32, 3), ('num', num, torch.int32, 1),
                                        ('obj_cand', obj_cand, torch.int32, 2)))
    B, n, W = (int(v) for v in scores.shape)
    max_num = int(dets.shape[1])
    max_obj, score_thr = int(max_obj), float(score_thr)
    if B < 1 or n < 1 or W < 1 or not 1 <= max_num <= UNC_MAX_DET or tuple(dets.shape) != (B, max_num, 5) or tuple(num.shape) != (B,):
        raise ValueError(f'object_posterior: scores {tuple(scores.shape)}, dets {tuple(dets.shape)}, num {tuple(num.shape)}: expected (B, n, W), '
                         f'(B, max_num, 5), (B,) with 1 <= max_num <= {UNC_MAX_DET}')
    if tuple(obj_cand.shape) != (B, max_num):
        raise ValueError(f'object_posterior: obj_cand has shape {tuple(obj_cand.shape)}, expected ({B}, {max_num})')
    if not 1 <= max_obj <= CCMS_MAX_OBJ:
        raise ValueError(f'object_posterior: max_obj must be in 1..{CCMS_MAX_OBJ}, got {max_obj}')
    if score_thr != score_thr:
        raise ValueError('object_posterior: score_thr is NaN')
    _check_devices('object_posterior', [scores, dets, num, obj_cand])
    post = torch.empty(B, max_obj, W, dtype=torch.float32, device=scores.device)
    call('aod_object_posterior', ptr(scores), ptr(dets), ptr(num), ptr(obj_cand), B, n, W, max_num, max_obj, score_thr, ptr(post), stream())
    return post


def badge_embedding(feat, post, cls, cnt, n_cls, out=None):
    """BADGE gradient embedding of every image of a batch (aod_badge_embedding; Ash et al., ICLR 2020): [B, n_cls * Cf] fp32,
    class-major: G[b][c][j] = sum over the objects o < cnt[b], in ascending order, of (post[b, o, c] - [c == cls[b, o]]) * feat[b, o, j]
    -- per object the gradient of the cross-entropy with respect to the logits under the detection's own label, times its feature row.
    feat [B, K, Cf] fp32, cls [B, K] int32, cnt [B] int32 as object_descriptors writes them, post [B, K, W] fp32 (object_posterior), W >=
    n_cls: a pad or background column >= n_cls is never read, nor is a row >= cnt.  K <= 64, Cf % 8 == 0, 8 <= Cf <= 256, n_cls <= 128.
    out: a [B, n_cls * Cf] fp32 view with unit column stride (rows of the pool matrix) to write into.  A row's bits depend on its image
    alone.  Device tensors, no host sync."""
    _check_tensors('badge_embedding', (('feat', feat, torch.float32, 3), ('post', post, torch.float32, 3), ('cls', cls, torch.int32, 2),
                                       ('cnt', cnt, torch.int32, 1)))
    B, K, Cf = _check_obj_shape('badge_embedding', 'feat', feat.shape)
    n_cls = int(n_cls)
    if not 1 <= n_cls <= BADGE_MAX_CLASSES:
        raise ValueError(f'badge_embedding: n_cls must be in 1..{BADGE_MAX_CLASSES}, got {n_cls}')
    if tuple(post.shape[:2]) != (B, K) or int(post.shape[2]) < n_cls:
        raise ValueError(f'badge_embedding: post has shape {tuple(post.shape)}, expected ({B}, {K}, W) with W >= n_cls = {n_cls}')
    if tuple(cls.shape) != (B, K):
        raise ValueError(f'badge_embedding: cls has shape {tuple(cls.shape)}, expected ({B}, {K})')
    if tuple(cnt.shape) != (B,):
        raise ValueError(f'badge_embedding: cnt has shape {tuple(cnt.shape)}, expected ({B},)')
    D = n_cls * Cf
    if out is not None:
        if not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (B, D) and out.stride(1) == 1
                and (B == 1 or (out.stride(0) >= D and out.stride(0) % 4 == 0)) and out.data_ptr() % 16 == 0):
            raise ValueError(f'badge_embedding: out must be a 16-B aligned [{B}, {D}] fp32 view with unit column stride and a row stride that is '
                             'a multiple of 4')
    _check_devices('badge_embedding', [feat, post, cls, cnt] + ([out] if out is not None else []))
    if out is None:
        out = torch.empty(B, D, dtype=torch.float32, device=feat.device)
    call('aod_badge_embedding', ptr(feat), ptr(post), ptr(cls), ptr(cnt), B, K, Cf, int(post.shape[2]), n_cls, ptr(out),
         int(out.stride(0)) if B > 1 else D, stream())
    return out


def kmeanspp_block():
    """consecutive rows whose weights kmeanspp_seed adds into one fp64 block sum: with N, the one thing the association of its sums depends on"""
    return int(_C.lib.aod_kmeanspp_block())


def kmeanspp_seed(desc, excluded, budget, draws=None, seed=0):
    """k-means++ D^2 seeding (Arthur & Vassilvitskii, SODA 2007) as BADGE uses it (Ash et al., ICLR 2020) on the aod_kmeanspp_seed kernels
    (DESIGN 3t).  A row is eligible iff it is neither in `excluded` nor picked; excluded rows are NOT centres.  Pick 0 is the eligible row
    with the largest squared norm (the lowest index on a tie).  Pick t >= 1 is drawn with probability proportional to w_i = the squared
    Euclidean distance (kcenter_greedy's arithmetic) of eligible row i to its nearest pick: with T the fp64 sum of the w_i (blocks of
    kmeanspp_block() rows in order), the first row with w_i > 0 whose running sum exceeds draws[t] * T; T == 0: the lowest eligible row.

    desc: [N, D] fp32 contiguous device tensor (N <= 2^24, D <= 32768); excluded: distinct row indices in [0, N) (sequence, array or
    tensor; may be empty); 1 <= budget <= number of eligible rows; draws: [budget] float64 in [0, 1) (draws[0] is not read), default
    np.random.default_rng(seed).random(budget) -- a host input, so every rank draws alike.
    Returns (picks [budget] int64, weight [budget] fp32: w of pick t when it was picked, the norm for t = 0; total [budget] fp64: T,
    0 for t = 0) on the device.  All steps are enqueued on the current stream; no host sync.  The result is a function of (desc, the set
    excluded, draws) alone."""
    if not (torch.is_tensor(desc) and desc.dim() == 2 and desc.dtype == torch.float32 and desc.is_contiguous() and desc.numel() > 0):
        raise ValueError('kmeanspp_seed: desc must be a non-empty contiguous 2-D fp32 tensor')
    N, D = int(desc.shape[0]), int(desc.shape[1])
    if D > KMEANSPP_MAX_COLUMNS:
        raise ValueError(f'kmeanspp_seed: up to {KMEANSPP_MAX_COLUMNS} descriptor columns are supported, got {D}')
    if N > KMEANSPP_MAX_ROWS:
        raise ValueError(f'kmeanspp_seed: up to 2^24 rows are supported, got {N}')
    exc = _index_array('kmeanspp_seed', excluded, N, arg='excluded', noun='excluded')
    budget = int(budget)
    if budget < 1:
        raise ValueError(f'kmeanspp_seed: budget must be at least 1, got {budget}')
    if budget > N - exc.size:
        raise ValueError(f'kmeanspp_seed: budget {budget} exceeds the {N - exc.size} eligible rows')
    if draws is None:
        draws = np.random.default_rng(int(seed)).random(budget)
    draws = np.ascontiguousarray(draws.detach().cpu().numpy() if torch.is_tensor(draws) else np.asarray(draws), dtype=np.float64).reshape(-1)
    if draws.size != budget:
        raise ValueError(f'kmeanspp_seed: draws holds {draws.size} values, expected budget = {budget}')
    if not np.all((draws[1:] >= 0.0) & (draws[1:] < 1.0)):
        raise ValueError('kmeanspp_seed: draws must lie in [0, 1)')
    if not desc.is_cuda:
        raise _cpu_refusal('kmeanspp_seed')
    dev = desc.device
    exc_d = torch.from_numpy(exc).to(dev) if exc.size else None
    draws_d = torch.from_numpy(draws).to(dev)
    picks = torch.empty(budget, dtype=torch.int64, device=dev)
    weight = torch.empty(budget, dtype=torch.float32, device=dev)
    total = torch.empty(budget, dtype=torch.float64, device=dev)
    mind = torch.empty(N, dtype=torch.float32, device=dev)
    ws = torch.empty(int(_C.lib.aod_kmeanspp_ws_len(N)), dtype=torch.uint8, device=dev)
    call('aod_kmeanspp_seed', ptr(desc), N, D, ptr(exc_d), int(exc.size), budget, ptr(draws_d), ptr(picks), ptr(weight), ptr(total), ptr(mind),
         ptr(ws), stream())
    return picks, weight, total


def enms_prototypes(feat, cls, w, h, cnt, t_enms=0.5, want_picks=False):
    """ENMS score and class prototypes of every image of a batch (aod_enms_prototypes; Wu et al., CVPR 2022).

    feat [B, max_obj, C] fp32, cls [B, max_obj] int32, w [B, max_obj] fp32, cnt [B] int32 as object_descriptors writes them, h [B, max_obj]
    fp32 the per-object measure in the same slots (object_measure); rows >= cnt are not used.  max_obj <= 64, C % 8 == 0, 8 <= C <= 256.
    ENMS: repeatedly take the alive object with the largest h (lowest slot on a tie), add its h, and drop it and every alive object of its
    class whose cosine to it exceeds t_enms (strict; t_enms >= 1 drops nothing).  Prototypes: per class present among ALL the image's objects, ascending, the
    (h + 2^-10)-weighted sum of its objects' features, L2-normalised, and the class's largest w.
    Returns (enms [B] fp32, kept [B] int32, proto [B, max_obj, C] fp32, pcls [B, max_obj] int32 (-1 pad), pconf [B, max_obj] fp32 (0 pad),
    pcnt [B] int32) on the device, no host sync; want_picks appends pick [B, max_obj] int32: the picked slots in pick order, -1 behind them.
    An image's outputs have the same bits alone and inside any batch."""
    name = 'enms_prototypes'
    _check_tensors(name, (('feat', feat, torch.float32, 3), ('cls', cls, torch.int32, 2), ('w', w, torch.float32, 2), ('h', h, torch.float32, 2),
                          ('cnt', cnt, torch.int32, 1)))
    B, K, Cc = _check_obj_shape(name, 'feat', feat.shape)
    for n, t in (('cls', cls), ('w', w), ('h', h)):
        if tuple(t.shape) != (B, K):
            raise ValueError(f'{name}: {n} has shape {tuple(t.shape)}, expected ({B}, {K})')
    if tuple(cnt.shape) != (B,):
        raise ValueError(f'{name}: cnt has shape {tuple(cnt.shape)}, expected ({B},)')
    t_enms = float(t_enms)
    if t_enms != t_enms:
        raise ValueError(f'{name}: t_enms is NaN')
    _check_devices(name, [feat, cls, w, h, cnt])
    dev = feat.device
    enms = torch.empty(B, dtype=torch.float32, device=dev)
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    proto = torch.empty(B, K, Cc, dtype=torch.float32, device=dev)
    pcls = torch.empty(B, K, dtype=torch.int32, device=dev)
    pconf = torch.empty(B, K, dtype=torch.float32, device=dev)
    pcnt = torch.empty(B, dtype=torch.int32, device=dev)
    pick = torch.empty(B, K, dtype=torch.int32, device=dev) if want_picks else None
    call('aod_enms_prototypes', ptr(feat), ptr(cls), ptr(w), ptr(h), ptr(cnt), B, K, Cc, t_enms, ptr(enms), ptr(kept), ptr(proto), ptr(pcls),
         ptr(pconf), ptr(pcnt), ptr(pick), stream())
    return (enms, kept, proto, pcls, pconf, pcnt) + ((pick,) if want_picks else ())


def divproto_order(enms, X_L):
    """The sweep order of the DivProto pick, on the host: the images not in X_L by `enms` descending, ties by ascending index.
    Returns the int64 index array [M]."""
    u = enms.detach().cpu().numpy() if torch.is_tensor(enms) else np.asarray(enms)
    u = u.reshape(-1).astype(np.float64)
    lab = _index_array('divproto_order', X_L, u.size, arg='X_L', distinct=False)
    if np.isnan(u).any():
        raise ValueError('divproto_order: the ENMS scores hold a NaN')
    free = np.ones(u.size, bool)
    free[lab] = False
    idx = np.nonzero(free)[0]
    return idx[np.argsort(-u[idx], kind='stable')].astype(np.int64)      # (idx ascends: a stable sort breaks ties by ascending index)


def divproto_quotas(n_cls, budget, alpha=0.5, beta=0.75):
    """the integers the selection kernel takes: (n_minor, quota, free) = (ceil(alpha n_cls), ceil(reserved / n_minor),
    budget - reserved) with reserved = min(budget, ceil(beta budget))"""
    n_cls, budget, alpha, beta = int(n_cls), int(budget), float(alpha), float(beta)
    if not 1 <= n_cls <= DIVPROTO_MAX_CLASSES:
        raise ValueError(f'divproto_select: n_cls must be in 1..{DIVPROTO_MAX_CLASSES}, got {n_cls}')
    if budget < 1:
        raise ValueError(f'divproto_select: budget must be at least 1, got {budget}')
    for n, v in (('alpha', alpha), ('beta', beta)):
        if not 0 < v <= 1:
            raise ValueError(f'divproto_select: {n} must lie in (0, 1], got {v}')
    n_minor = int(np.ceil(alpha * n_cls))
    reserved = min(budget, int(np.ceil(beta * budget)))
    return n_minor, -(-reserved // n_minor), budget - reserved


def divproto_select(order, proto, pcls, pconf, pcnt, n_cls, budget, t_intra=0.7, t_inter=0.3, alpha=0.5, beta=0.75, class_balance=True,
                    _chunk=None):
    """The progressive DivProto pick (aod_divproto_select; Wu et al., CVPR 2022) over the images `order` (distinct pool indices
    in sweep order: divproto_order) of the pool tensors proto [N, max_obj, C] fp32, pcls [N, max_obj] int32, pconf [N, max_obj] fp32,
    pcnt [N] int32 (enms_prototypes' outputs, contiguous, on the device).

    An image is skipped as redundant when every one of its classes has a prototype among the picks so far with a cosine above t_intra
    to its own; with class_balance it is accepted when it serves a minority class (one of the ceil(alpha n_cls) classes the picks hold
    least, present with a confidence above t_inter and below its quota) or while the free share (1 - beta) of the budget lasts,
    else deferred.  t_intra >= 1 makes no image redundant.  A sweep that ends short is filled with the deferred, then the redundant images in sweep order.
    Returns (picks [budget] int64, stage [budget] int32: 1 minority / no balance, 2 free share, 3 fill) on the device; all launches are
    enqueued on the current stream, no host sync behind the upload of `order`.  _chunk: sweep positions per launch (tests; the result
    does not depend on it)."""
    name = 'divproto_select'
    _check_tensors(name, (('proto', proto, torch.float32, 3), ('pcls', pcls, torch.int32, 2), ('pconf', pconf, torch.float32, 2),
                          ('pcnt', pcnt, torch.int32, 1)))
    N, K, Cc = _check_obj_shape(name, 'proto', proto.shape)
    for n, t in (('pcls', pcls), ('pconf', pconf)):
        if tuple(t.shape) != (N, K):
            raise ValueError(f'{name}: {n} has shape {tuple(t.shape)}, expected ({N}, {K})')
    if tuple(pcnt.shape) != (N,):
        raise ValueError(f'{name}: pcnt has shape {tuple(pcnt.shape)}, expected ({N},)')
    n_minor, quota, free = divproto_quotas(n_cls, budget, alpha, beta)
    n_cls, budget = int(n_cls), int(budget)
    t_intra, t_inter = float(t_intra), float(t_inter)
    if t_intra != t_intra or t_inter != t_inter:
        raise ValueError(f'{name}: a threshold is NaN (t_intra {t_intra}, t_inter {t_inter})')
    idx = _index_array(name, order, N, arg='order')
    M = int(idx.size)
    if budget > M:
        raise ValueError(f'{name}: budget {budget} exceeds the {M} images of the sweep')
    chunk = 0 if _chunk is None else int(_chunk)
    if chunk < 0:
        raise ValueError(f'{name}: _chunk must be positive, got {chunk}')
    _check_devices(name, [proto, pcls, pconf, pcnt])
    dev = proto.device
    order_d = torch.from_numpy(idx).to(dev)
    picks = torch.empty(budget, dtype=torch.int64, device=dev)
    stage = torch.empty(budget, dtype=torch.int32, device=dev)
    ws = torch.empty(int(_C.lib.aod_divproto_ws_len(M, n_cls, budget)) // 8 + 1, dtype=torch.int64, device=dev)
    call('aod_divproto_select', ptr(order_d), M, N, ptr(proto), ptr(pcls), ptr(pconf), ptr(pcnt), K, Cc, n_cls, budget, t_intra, t_inter, n_minor,
         quota, free, int(bool(class_balance)), chunk, ptr(picks), ptr(stage), ptr(ws), stream())
    return picks, stage


LOCSTAB_COMBINES = {'ls': 0, 'ls+c': 1}
LOCSTAB_MAX_LEVELS = int(_C.lib.aod_loc_stability_max_levels())      # (written once, in csrc/loc_stability.hip)
LOCSTAB_SIGMAS = (8, 16, 24, 32, 40, 48)      # Kao et al.'s noise levels, 0..255 pixel units


def loc_stability(dets, labels, num, score_thr=0.3, same_class=False, combine='ls', want_objects=False):
    """Localization stability of every image of a batch (aod_loc_stability; Kao et al., ACCV 2018): how far the boxes of the
    clean detections move under pixel noise.

    dets [K+1, B, max_num, 5] fp32, labels [K+1, B, max_num] int64, num [K+1, B] int32: the stacked padded detections, slot 0 of the clean
    batch, slot k + 1 of noise level k; 1 <= K <= 16, 1 <= max_num <= 1024.  A row j < num[0][b] of slot 0 with a score > score_thr (strict)
    is an object of weight w_j = its score; m_jk is its largest IoU over the rows < num[k+1][b] of slot k + 1 (same_class: rows of its label
    only), S_j the mean of m_jk over the levels, S_I the w-weighted mean of S_j.  combine 'ls': 1 - S_I; 'ls+c': (1 - S_I) + (1 - max_j w_j);
    an image without an object scores 0.  Returns unc [B] fp32 on the device (no host sync), or with want_objects (unc, stab [B, max_num]
    fp32: S_j, NaN where the row is no object)."""
    if combine not in LOCSTAB_COMBINES:
        raise ValueError(f"loc_stability: unknown combine {combine!r} (expected 'ls' or 'ls+c')")
    score_thr = float(score_thr)
    if score_thr != score_thr:
        raise ValueError('loc_stability: score_thr is NaN')
    for name, t, dt, nd in (('dets', dets, torch.float32, 4), ('labels', labels, torch.int64, 3), ('num', num, torch.int32, 2)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != nd:
            raise ValueError(f"loc_stability: {name} is not a {nd}-D {str(dt).replace('torch.', '')} tensor")
        if not t.is_contiguous():
            raise ValueError(f'loc_stability: {name} is not contiguous; no copy is made here')
    K1, B, max_num, five = (int(v) for v in dets.shape)
    if not 1 <= K1 - 1 <= LOCSTAB_MAX_LEVELS:
        raise ValueError(f'loc_stability: dets holds {K1} slots: the clean one and 1..{LOCSTAB_MAX_LEVELS} noise levels are needed')
    if B < 1 or five != 5 or not 1 <= max_num <= UNC_MAX_DET:
        raise ValueError(f'loc_stability: dets has shape {tuple(dets.shape)}: expected (K + 1, B, max_num, 5) with B >= 1 and '
                         f'1 <= max_num <= {UNC_MAX_DET}')
    if tuple(labels.shape) != (K1, B, max_num):
        raise ValueError(f'loc_stability: labels has shape {tuple(labels.shape)}, expected ({K1}, {B}, {max_num})')
    if tuple(num.shape) != (K1, B):
        raise ValueError(f'loc_stability: num has shape {tuple(num.shape)}, expected ({K1}, {B})')
    ts = (dets, labels, num)
    for t in ts:
        if not t.is_cuda:
            raise _C.AodHipError('loc_stability needs tensors on the MI355X (cuda:N); got a CPU tensor. There is no CPU fallback.')
    dev = dets.device
    if any(t.device != dev for t in ts):
        raise ValueError(f'loc_stability: the tensors live on different devices ({sorted({str(t.device) for t in ts})})')
    unc = torch.empty(B, dtype=torch.float32, device=dev)
    stab = torch.empty(B, max_num, dtype=torch.float32, device=dev) if want_objects else None
    call('aod_loc_stability', ptr(dets), ptr(labels), ptr(num), K1 - 1, B, max_num, score_thr, 1 if same_class else 0,
         LOCSTAB_COMBINES[combine], ptr(unc), ptr(stab), stream())
    return (unc, stab) if want_objects else unc


from .hipops import FLIP_VIEWS as CONSISTENCY_VIEWS      # noqa: E402  ('hflip': 1, 'vflip': 2, 'hvflip': 3: bit 0 horizontal, bit 1 vertical)
CONSISTENCY_MODES = {'box': 0, 'cls': 1, 'both': 2}
CONSISTENCY_MAX_VIEWS = int(_C.lib.aod_consistency_max_views())      # (written once, in csrc/consistency.hip)


def consistency_views(views, who='det_consistency'):
    """the flip codes of `views`, a sequence of 1..CONSISTENCY_MAX_VIEWS distinct view names; ValueError otherwise"""
    if isinstance(views, str) or not hasattr(views, '__iter__'):
        raise ValueError(f"{who}: views must be a sequence of view names, got {views!r}")
    views = tuple(views)
    if not 1 <= len(views) <= CONSISTENCY_MAX_VIEWS:
        raise ValueError(f'{who}: 1..{CONSISTENCY_MAX_VIEWS} views are supported, got {len(views)}')
    for v in views:
        if not isinstance(v, str) or v not in CONSISTENCY_VIEWS:
            raise ValueError(f"{who}: unknown view {v!r} (expected 'hflip', 'vflip' or 'hvflip')")
    if len(set(views)) != len(views):
        raise ValueError(f'{who}: the views must be distinct, got {views}')
    return [CONSISTENCY_VIEWS[v] for v in views]


def det_posterior(cand, dets, labels, num):
    """The class-posterior row of every detection of a batch (aod_det_posterior): post [B, max_num, W] fp32 with
    post[b, j] = cand.scores[b, k] for the candidate row k that detection j < num[b] was made of -- looked up by its box and score bits
    with the one lookup of det_uncertainty (score_thr = -inf: every row j < num) --, zero rows elsewhere (every word is written: a replayed
    graph never exposes stale rows).  Returns (post, missing [B] int32: the rows j < num[b] without a candidate row, always 0 behind
    multiclass_nms_batch).  Two launches, no host sync."""
    _, obj_cand = det_uncertainty(cand, dets, labels, num, 'cat_bg', 'entropy', 'sum', float('-inf'), want_cand=True)
    scores = cand.scores
    B, n, W = (int(v) for v in scores.shape)
    max_num = int(dets.shape[1])
    post = torch.empty(B, max_num, W, dtype=torch.float32, device=scores.device)
    missing = torch.empty(B, dtype=torch.int32, device=scores.device)
    call('aod_det_posterior', ptr(scores), ptr(obj_cand), ptr(num), B, n, W, max_num, ptr(post), ptr(missing), stream())
    return post, missing


def det_consistency(dets, labels, num, post, views, ext, layout, mode='both', aggregate='max', score_thr=0.3, same_class=False,
                    want_objects=False, want_parts=False):
    """Prediction consistency under mirroring of every image of a batch (aod_det_consistency; Elezi et al., CVPR 2022; CALD, Yu
    et al., CVPRW 2022): how much the detections of the image and of its mirrored views disagree, in box position and in class posterior.

    dets [V+1, B, max_num, 5] fp32, labels [V+1, B, max_num] int64, num [V+1, B] int32, post [V+1, B, max_num, W] fp32: the stacked padded
    detections and their posterior rows (det_posterior), slot 0 of the clean batch, slot v + 1 of the view views[v] ('hflip' | 'vflip' |
    'hvflip', distinct, 1 <= V <= 3); 1 <= max_num <= 1024.  ext [B, 2] fp32: the extent (w, h) of the frame the boxes lie in; a view's boxes
    are mapped back into it first.  A row j < num[0][b] of slot 0 with a score > score_thr (strict) is an object; per view it is matched to
    the un-flipped row of largest IoU (same_class: rows of its label only; none, or IoU 0: iou 0, js 1) and js is the Jensen-Shannon
    divergence in bits of the two posterior rows under `layout` ('cat' | 'cat_bg' | 'sigmoid': UNC_LAYOUTS).  mode 'box': u = 1 - iou,
    'cls': js, 'both': their mean; averaged over the views, then max / mean / sum over the image's objects; an image without one scores 0.
    Returns unc [B] fp32 on the device (no host sync); with want_objects also obj [B, max_num] (u_j, NaN where the row is no object); with
    want_parts also (iou, js, match): [V, B, max_num] fp32 / fp32 / int32 (NaN / NaN / -1 where the row is no object)."""
    codes = consistency_views(views)
    if layout not in UNC_LAYOUTS:
        raise ValueError(f"det_consistency: unknown layout {layout!r} (expected 'cat', 'cat_bg' or 'sigmoid')")
    if mode not in CONSISTENCY_MODES:
        raise ValueError(f"det_consistency: unknown mode {mode!r} (expected 'box', 'cls' or 'both')")
    if aggregate not in UNC_AGGREGATES:
        raise ValueError(f"det_consistency: unknown aggregate {aggregate!r} (expected 'max', 'mean' or 'sum')")
    score_thr = float(score_thr)
    if score_thr != score_thr:
        raise ValueError('det_consistency: score_thr is NaN')
    for name, t, dt, nd in (('dets', dets, torch.float32, 4), ('labels', labels, torch.int64, 3), ('num', num, torch.int32, 2),
                            ('post', post, torch.float32, 4), ('ext', ext, torch.float32, 2)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != nd:
            raise ValueError(f"det_consistency: {name} is not a {nd}-D {str(dt).replace('torch.', '')} tensor")
        if not t.is_contiguous():
            raise ValueError(f'det_consistency: {name} is not contiguous; no copy is made here')
    V1, B, max_num, five = (int(v) for v in dets.shape)
    if V1 - 1 != len(codes):
        raise ValueError(f'det_consistency: dets holds {V1} slots, {len(codes)} views need {len(codes) + 1} (the clean one and one per view)')
    if B < 1 or five != 5 or not 1 <= max_num <= UNC_MAX_DET:
        raise ValueError(f'det_consistency: dets has shape {tuple(dets.shape)}: expected (V + 1, B, max_num, 5) with B >= 1 and '
                         f'1 <= max_num <= {UNC_MAX_DET}')
    if tuple(labels.shape) != (V1, B, max_num):
        raise ValueError(f'det_consistency: labels has shape {tuple(labels.shape)}, expected ({V1}, {B}, {max_num})')
    if tuple(num.shape) != (V1, B):
        raise ValueError(f'det_consistency: num has shape {tuple(num.shape)}, expected ({V1}, {B})')
    if tuple(post.shape[:3]) != (V1, B, max_num) or post.shape[3] < 2:
        raise ValueError(f'det_consistency: post has shape {tuple(post.shape)}, expected ({V1}, {B}, {max_num}, W) with W >= 2')
    if tuple(ext.shape) != (B, 2):
        raise ValueError(f'det_consistency: ext has shape {tuple(ext.shape)}, expected ({B}, 2)')
    ts = (dets, labels, num, post, ext)
    for t in ts:
        if not t.is_cuda:
            raise _cpu_refusal('det_consistency')
    dev = dets.device
    if any(t.device != dev for t in ts):
        raise ValueError(f'det_consistency: the tensors live on different devices ({sorted({str(t.device) for t in ts})})')
    V, W = V1 - 1, int(post.shape[3])
    unc = torch.empty(B, dtype=torch.float32, device=dev)
    obj = torch.empty(B, max_num, dtype=torch.float32, device=dev) if want_objects else None
    iou = torch.empty(V, B, max_num, dtype=torch.float32, device=dev) if want_parts else None
    js = torch.empty(V, B, max_num, dtype=torch.float32, device=dev) if want_parts else None
    match = torch.empty(V, B, max_num, dtype=torch.int32, device=dev) if want_parts else None
    call('aod_det_consistency', ptr(dets), ptr(labels), ptr(num), ptr(post), V, (C.c_int32 * V)(*codes), ptr(ext), B, max_num, W,
         UNC_LAYOUTS[layout], CONSISTENCY_MODES[mode], UNC_AGGREGATES[aggregate], score_thr, 1 if same_class else 0, ptr(unc), ptr(obj),
         ptr(iou), ptr(js), ptr(match), stream())
    out = (unc,) + ((obj,) if want_objects else ()) + ((iou, js, match) if want_parts else ())
    return out if len(out) > 1 else unc


HUA_POOLS = ('Entropy_NMS', 'Entropy_ALL', 'Entropy_Avg')


def refuse_hua(head, **kwargs):
    """A head without a Model Evidence Head (MyRetinaHead) has no lambda: HUA -- the Entropy_* pools of a scoring pass (isEval=False) and the
    per-detection uncertainties (detUnc) -- is not defined for it."""
    if (not kwargs.get('isEval') and kwargs.get('uPool') in HUA_POOLS) or kwargs.get('detUnc'):
        what = 'detUnc' if kwargs.get('detUnc') else f"uncertainty_pool={kwargs.get('uPool')}"
        raise ValueError(f'{type(head).__name__} has no lambda (no Model Evidence Head): {what} (HUA) is not defined for it; '
                         'use Random, Coreset, CDAL, or the Ensemble / MC-dropout scores')


def _class_weight(head, cand, kwargs):
    """class_weighted=True: the head's `class_weight` buffer [W] -- refreshed by head.refresh_class_weight() before the pool pass, read
    by the launch at replay time -- or None.  A head without class-difficulty tracking has no such buffer: ValueError."""
    if not kwargs.get('class_weighted'):
        return None
    w = getattr(head, 'class_weight', None)
    if w is None and getattr(head, 'last_activation', None) == 'softmax':
        raise NotImplementedError(f'class_weighted=True: {type(head).__name__} tracks no class difficulty (DESIGN 3p is built for the RetinaNet '
                                  'heads; the SSD heads are a follow-up)')
    if w is None:
        raise ValueError(f"class_weighted=True needs a head that tracks the class difficulty: build {type(head).__name__} with "
                         'bbox_head.class_difficulty=dict(xi=0.6, momentum=0.99, alpha=0.3, beta=0.2) '
                         '(tools/train_RetinaNet.py: --class-difficulty or --uncertainty-pool PPAL)')
    if cand is not None and w.numel() != cand.scores.shape[2]:
        raise ValueError(f'class_weighted=True: the head holds {w.numel()} class weights, the score rows have {cand.scores.shape[2]} columns')
    return w


def score_batch(head, mlvl_cls_scores, mlvl_bbox_preds, mlvl_anchors, img_shapes, scale_factors, cfg, rescale=False, with_nms=True,
                **kwargs):
    """Body of Lambda_L2Net._get_bboxes for `last_activation == 'relu'`.

    isEval=True (detection for mAP)  -> list of (det_bboxes [k,5], det_labels [k]) per image;
                 with _padded=True   -> (dets [B,max,5], labels [B,max] int64, num [B] int32) on the device, no host sync;
                 with _padded=True, detPost=True -> (dets, labels, num, post [B,max,W] fp32, missing [B] int32): the same triple
                                        and det_posterior's outputs, the class-posterior row of every detection (zero rows >= num);
                                        ValueError together with objDesc or detUnc
                 with _padded=True, objDesc=max_obj -> (dets, labels, num, unc, feat, cls, w, cnt, missing): the triple, the
                                        posterior score and object_descriptors' outputs; objUnc=True (with objDesc only)
                                        appends h [B,max_obj] fp32, the per-object measure in the same slots (object_measure);
                                        objPost=True (with objDesc only) appends post [B,max_obj,W] fp32, the candidate score
                                        row of every object in the same slots (object_posterior), behind h when both are asked for
                 with detUnc=True    -> list of (det_bboxes [k,5], det_labels [k], det_unc [k,2]): HUA runs after NMS (it needs L_scores)
                                        and det_unc holds (aleatoric, epistemic) of every detection, NaN for rows that are no HUA object.
    hua_estimator = 'mc' (default) | 'closed' selects the estimator of the Entropy_NMS / Entropy_ALL / Entropy_Avg / detUnc paths.
    isUnc with uPool == 'Entropy_NMS' -> (det_results, unc [B] device tensor).
    isUnc with uPool in POSTERIOR_POOLS ('Entropy' | 'Margin' | 'LeastConf') -> the same pair from det_uncertainty: the measure of
                 the head's own class posterior per detection, aggregated by `unc_aggregate` ('max' | 'mean' | 'sum', default 'max') over the
                 detections whose score exceeds `score_thr` (default 0.3).  No lambda is read: every head offers these pools.
    Two class attributes of the head select the reference's ablations: `_hua_lam` ('scaled' | 'none': whether lambda scales alpha) and
    `_hua_thr_kwargs` (whether the `score_thr` / `iou_thr` kwargs replace the 0.3 / 0.5 of GetObjectIdx, the level gate and the candidate
    filter, Lambda_L2_ablation.py:261-265,355,496-518; a falsy or missing value falls back to 0.3 / 0.5).
    uPool == 'Entropy_Avg' (Lambda_L2Net_NoL only, Lambda_L2_noL.py:367-369,552-572,631-640): per (image, level) the rows are all anchors
    whose softmax maximum exceeds 0.3 (hard-coded there, not score_thr; no top-k), 50 Dirichlet(softmax) samples per row, level value = mean
    of the rows' epistemic values, image score = mean over the levels that have such a row.  Two corner cases of the reference are NOT
    reproduced: an image without a foreground row on any level scores 0 here (there: mean of an empty list = NaN, which update_X_L's
    argsort ranks most uncertain), and a level counts iff it has a foreground row (there `if sUncs:` also drops a level whose mean is
    exactly 0.0)."""
    assert head.last_activation in ('relu', 'softmax', 'sigmoid')
    has_bg = head.last_activation == 'softmax'         # SSD: 21 logits incl. background (My_L_ssd_head.py:331-345)
    # the plain RetinaNet baseline (MyRetinaHead; anchor_head.py:535-596): per-class sigmoid scores, detection paths only -- it has no lambda
    sigmoid = head.last_activation == 'sigmoid'
    C_ = head.cls_out_channels
    na = head.num_anchors if isinstance(head.num_anchors, (list, tuple)) else [head.num_anchors] * len(mlvl_cls_scores)
    isUnc = kwargs.get('isUnc')
    uPool = kwargs.get('uPool')
    if sigmoid:
        refuse_hua(head, **kwargs)
    _class_weight(head, None, kwargs)          # (class_weighted on a head without the option: refused before the first launch)
    if kwargs.get('objUnc') and not kwargs.get('objDesc'):
        raise ValueError('objUnc is offered together with objDesc only: it appends the per-object measure in the descriptors\' slots')
    if kwargs.get('objPost') and not kwargs.get('objDesc'):
        raise ValueError('objPost is offered together with objDesc only: it appends the posterior rows in the descriptors\' slots')
    if isUnc and uPool == 'Entropy_NoNMS':
        raise NotImplementedError('uncertainty_pool=Entropy_NoNMS crashes in the reference too (ComputeScaleUnc with L_scores=None)')
    lam_mode = getattr(head, '_hua_lam', 'scaled')
    obj_thr, iou_thr = 0.3, 0.5
    if getattr(head, '_hua_thr_kwargs', False):
        obj_thr, iou_thr = float(kwargs.get('score_thr') or 0.3), float(kwargs.get('iou_thr') or 0.5)
    if isUnc and uPool == 'Entropy_Avg' and not getattr(head, '_hua_entropy_avg', False):
        raise NotImplementedError(f'uncertainty_pool=Entropy_Avg is offered by Lambda_L2Net_NoL only: the reference of {type(head).__name__} '
                                  'has no such branch')
    if isUnc and uPool in ('Entropy_ALL', 'Entropy_Avg'):
        # Lambda_L2.py:281-283 (no top-k), :354 (no NMS), :364-365 ComputeScaleUnc + AggregateScaleUnc
        # Entropy_Avg (Lambda_L2_noL.py:367-369): the same front end (every anchor a candidate, raw softmax), ComputeAvgUnc + AggregateAvgUnc
        assert not has_bg, f'{uPool} is built for the RetinaNet evidence head'
        cand = pre_nms(mlvl_cls_scores, mlvl_bbox_preds, kwargs['L_scores'], mlvl_anchors, img_shapes, scale_factors, -1, C_,
                       head.bbox_coder.means, head.bbox_coder.stds, rescale=rescale, normalize=False)
        B = cand.boxes.shape[0]
        image_ids = kwargs.get('image_ids')
        if image_ids is None:
            image_ids = torch.arange(B, device=cand.boxes.device, dtype=torch.int64) + int(kwargs.get('batchIdx', 0)) * B
        if uPool == 'Entropy_Avg':
            unc = hua_score(cand, None, None, image_ids.to(torch.int64).contiguous(), 1, (0, 0, 0), False, num_samples=50,
                            seed=kwargs.get('hua_seed', 20), scale_mode='avg', estimator=kwargs.get('hua_estimator') or 'mc', lam_mode=lam_mode)
        else:
            cls_code, scale_code, _ = extract_agg_codes(kwargs['uPool2'] if 'object' in kwargs['uPool2'] else 'objectSum_' + kwargs['uPool2'])
            unc = hua_score(cand, None, None, image_ids.to(torch.int64).contiguous(), 1, (cls_code, scale_code, 0), False,
                            seed=kwargs.get('hua_seed', 20), scale_mode=True, estimator=kwargs.get('hua_estimator') or 'mc', lam_mode=lam_mode)
        det_results = [(cand.boxes[b], cand.scores[b]) for b in range(B)]
        if kwargs.get('_return_internals'):
            return det_results, unc, dict(cand=cand)
        return det_results, unc
    L_scores = kwargs.get('L_scores')
    if L_scores is None:   # plain detection: lambda is not needed, reuse zeros
        L_scores = [torch.zeros(c.shape[0], a, c.shape[2], c.shape[3], device=c.device).contiguous(memory_format=torch.channels_last)
                    for c, a in zip(mlvl_cls_scores, na)]
    nms_pre = cfg.get('nms_pre', -1)
    cand = pre_nms(mlvl_cls_scores, mlvl_bbox_preds, L_scores, mlvl_anchors, img_shapes, scale_factors, nms_pre, C_,
                   head.bbox_coder.means, head.bbox_coder.stds, rescale=rescale, has_bg=has_bg, fg_thr=obj_thr,
                   activation='sigmoid' if sigmoid else None)
    if not with_nms:
        return [(cand.boxes[b], cand.scores[b]) for b in range(cand.boxes.shape[0])]
    max_num = cfg.max_per_img
    dets, labels, keep, num = multiclass_nms_batch(cand.boxes, cand.scores, cfg.score_thr, cfg.nms.get('iou_threshold', 0.5), max_num)
    B = dets.shape[0]
    if kwargs.get('isEval') and kwargs.get('_padded'):
        # device metric (apis/test.py single_gpu_map): the padded triple stays on the device -- no num.cpu(), graph-capturable
        if kwargs.get('detUnc'):
            raise ValueError('detUnc is not offered with the padded evaluation outputs')
        if kwargs.get('detPost'):
            # consistency pool (apis/test.py single_gpu_consistency): the posterior row of every detection behind the NMS kernel
            # -- the lookup of det_uncertainty over every row j < num, then the gather; two launches, no host sync
            if kwargs.get('objDesc'):
                raise ValueError('detPost is not offered together with objDesc: the two options return different tuples')
            return (dets, labels, num) + det_posterior(cand, dets, labels, num)
        if kwargs.get('objDesc'):
            # CCMS object descriptors (apis/test.py single_gpu_object_descriptors): two launches behind the NMS kernel -- the
            # stage-1 posterior score, which also hands out the matched candidate rows, and the gather from the neck outputs; no host sync
            feats = kwargs.get('_feats')
            if feats is None:
                raise ValueError('objDesc needs the neck outputs: the head passes them on as _feats')
            thr = kwargs.get('score_thr')
            thr = 0.3 if thr is None else thr
            if kwargs.get('objUnc'):
                # ENMS / DivProto (apis/test.py single_gpu_enms): the same launches, the score kernel also hands out its per-object
                # values, and one compaction launch puts them into the descriptors' slots
                unc, obj_out, _, obj_cand = det_uncertainty(cand, dets, labels, num, ACTIVATION_LAYOUT[head.last_activation],
                                                            kwargs.get('unc_measure') or 'entropy', kwargs.get('unc_aggregate') or 'sum', thr,
                                                            want_objects=True, want_cand=True, class_w=_class_weight(head, cand, kwargs))
            else:
                unc, obj_cand = det_uncertainty(cand, dets, labels, num, ACTIVATION_LAYOUT[head.last_activation],
                                                kwargs.get('unc_measure') or 'entropy', kwargs.get('unc_aggregate') or 'sum', thr, want_cand=True,
                                                class_w=_class_weight(head, cand, kwargs))
            desc = object_descriptors(feats, cand, dets, labels, num, obj_cand, list(na), int(kwargs['objDesc']), thr,
                                      channels=getattr(head, 'in_channels', None))
            res = (dets, labels, num, unc) + desc
            if kwargs.get('objUnc'):
                res += (object_measure(obj_out, dets, num, obj_cand, int(kwargs['objDesc']), thr),)
            if kwargs.get('objPost'):
                # BADGE (apis/test.py single_gpu_badge_embeddings): one more launch, the objects' posterior rows in the same slots
                res += (object_posterior(cand.scores, dets, num, obj_cand, int(kwargs['objDesc']), thr),)
            return res
        return dets, labels, num
    if isUnc and not kwargs.get('isEval') and uPool in POSTERIOR_POOLS:
        # posterior uncertainty pools: one launch behind the NMS kernel on what it and pre_nms left on the device; no lambda is
        # read (L_scores may be None: every head has these pools, the plain RetinaNet and the SSD heads included), no host sync
        thr = kwargs.get('score_thr')
        unc = det_uncertainty(cand, dets, labels, num, ACTIVATION_LAYOUT[head.last_activation], POOL_MEASURE[uPool],
                              kwargs.get('unc_aggregate') or 'max', 0.3 if thr is None else thr, class_w=_class_weight(head, cand, kwargs))
        det_results = [(dets[b], labels[b]) for b in range(B)]   # zero-padded to max_per_img rows (num rows are valid)
        if kwargs.get('_return_internals'):
            return det_results, unc, dict(cand=cand, dets=dets, labels=labels, keep=keep, num=num)
        return det_results, unc
    if (not isUnc or kwargs.get('isEval')) and not (kwargs.get('isEval') and kwargs.get('detUnc')):
        nh = num.cpu().tolist()           # evaluation path: variable-length results are part of the interface
        return [(dets[b, :nh[b]], labels[b, :nh[b]]) for b in range(B)]
    image_ids = kwargs.get('image_ids')
    if image_ids is None:
        bs = kwargs.get('batchIdx', 0)
        image_ids = torch.arange(B, device=dets.device, dtype=torch.int64) + int(bs) * B
    estimator = kwargs.get('hua_estimator') or 'mc'
    if kwargs.get('isEval'):              # detUnc: the detections of the evaluation path with their own (aleatoric, epistemic)
        if kwargs.get('L_scores') is None:
            raise ValueError('detUnc needs the lambda head outputs (L_scores)')
        agg = extract_agg_codes(kwargs.get('uPool2') or 'objectSum_scaleMax_classSum')
        _, obj_out, _ = hua_score(cand, dets, num, image_ids.to(torch.int64).contiguous(), max_num, agg, False, seed=kwargs.get('hua_seed', 20),
                                  dirichlet_cols=C_ if has_bg else 0, estimator=estimator, want_objects=True, obj_score_thr=obj_thr,
                                  obj_iou_thr=iou_thr, fg_thr=obj_thr, lam_mode=lam_mode)
        nh = num.cpu().tolist()
        return [(dets[b, :nh[b]], labels[b, :nh[b]], obj_out[b, :nh[b]]) for b in range(B)]
    agg = extract_agg_codes(kwargs['uPool2'])
    unc = hua_score(cand, dets, num, image_ids.to(torch.int64).contiguous(), max_num, agg, kwargs.get('clsW', False),
                    seed=kwargs.get('hua_seed', 20), dirichlet_cols=C_ if has_bg else 0, estimator=estimator, obj_score_thr=obj_thr,
                    obj_iou_thr=iou_thr, fg_thr=obj_thr, lam_mode=lam_mode)
    det_results = [(dets[b], labels[b]) for b in range(B)]   # zero-padded to max_per_img rows (num_det rows are valid)
    if kwargs.get('_return_internals'):
        return det_results, unc, dict(cand=cand, dets=dets, labels=labels, keep=keep, num=num)
    if kwargs.get('saveMaxConf'):            # Lambda_L2.py:375-380: third output = per-image max confidence (device tensor here)
        return det_results, unc, cand.max_conf()
    return det_results, unc
