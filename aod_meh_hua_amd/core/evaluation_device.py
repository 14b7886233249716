"""Device form of the fork's mAP (core/evaluation.py eval_map with tpfp_default): the greedy match runs in `aod_eval_match` on the padded
(dets, labels, num) triple that `aod_multiclass_nms` leaves on the device, per batch and without a host sync; the per-detection
(score, label, flag) rows are kept in fixed-size device buffers, ranks own disjoint image rows and all-gather them, and ONE D2H copy per
evaluation feeds the same numpy tail that eval_map runs (evaluation.class_result): the arrays handed to `np.argsort(-scores)`, the cumsums
and `average_precision` are the host path's arrays, so cross-image score ties resolve as they do there and the result is eval_map's bit
for bit.  Score ties inside one (image, class) rank by row (a stable order) in the kernel.

No area ranges and no custom tpfp function: those stay on eval_map."""
import numpy as np
import torch

from .evaluation import class_result, mean_of_aps

MAX_THRESHOLDS = 8


def pack_annotations(anns):
    """Annotations of a batch (dicts with bboxes / labels and optional bboxes_ignore / labels_ignore) -> (boxes [B,G,4] float32,
    labels [B,G] int32, ignore [B,G] uint8, num [B] int32), G = the batch's largest gt count (at least 1).  Per image: the real gts in
    annotation order, then the ignored ones in annotation order -- get_cls_results / tpfp_default stack a class's real gts above its
    ignored ones, and filtering this list by class gives that order.  Padding rows: zero box, label -1."""
    B = len(anns)
    rows = []
    for ann in anns:
        bb = np.asarray(ann['bboxes'], dtype=np.float32).reshape(-1, 4)
        lb = np.asarray(ann['labels']).reshape(-1)
        if ann.get('labels_ignore', None) is not None:
            bi = np.asarray(ann['bboxes_ignore'], dtype=np.float32).reshape(-1, 4)
            li = np.asarray(ann['labels_ignore']).reshape(-1)
        else:
            bi, li = np.zeros((0, 4), np.float32), np.zeros((0,), np.int64)
        assert bb.shape[0] == lb.shape[0] and bi.shape[0] == li.shape[0]
        rows.append((bb, lb, bi, li))
    G = max([1] + [r[0].shape[0] + r[2].shape[0] for r in rows])
    boxes = np.zeros((B, G, 4), np.float32)
    labels = np.full((B, G), -1, np.int32)
    ignore = np.zeros((B, G), np.uint8)
    num = np.zeros((B,), np.int32)
    for b, (bb, lb, bi, li) in enumerate(rows):
        nr, ni = bb.shape[0], bi.shape[0]
        boxes[b, :nr], labels[b, :nr] = bb, lb
        boxes[b, nr:nr + ni], labels[b, nr:nr + ni], ignore[b, nr:nr + ni] = bi, li, 1
        num[b] = nr + ni
    return boxes, labels, ignore, num


def eval_match(dets, labels, num, gt_boxes, gt_labels, gt_ignore, gt_num, iou_thrs):
    """aod_eval_match on device tensors -> flags [T, B, M] uint8 (0 neither, 1 tp, 2 fp)."""
    import ctypes as C
    from .._C import call, ptr, stream
    B, M = int(dets.shape[0]), int(dets.shape[1])
    T = len(iou_thrs)
    if not 1 <= T <= MAX_THRESHOLDS:
        raise ValueError(f'eval_match: 1..{MAX_THRESHOLDS} IoU thresholds, got {T}')
    assert dets.dtype == torch.float32 and labels.dtype == torch.int64 and num.dtype == torch.int32 and dets.shape[2] == 5
    assert gt_boxes.dtype == torch.float32 and gt_labels.dtype == torch.int32 and gt_ignore.dtype == torch.uint8 and gt_num.dtype == torch.int32
    assert gt_boxes.shape[0] == B and gt_labels.shape == gt_ignore.shape == gt_boxes.shape[:2] and labels.shape == (B, M)
    flags = torch.empty(T, B, M, dtype=torch.uint8, device=dets.device)
    call('aod_eval_match', ptr(dets.contiguous()), ptr(labels.contiguous()), ptr(num.contiguous()), ptr(gt_boxes.contiguous()),
         ptr(gt_labels.contiguous()), ptr(gt_ignore.contiguous()), ptr(gt_num.contiguous()), B, M, int(gt_boxes.shape[1]),
         (C.c_float * T)(*[float(np.float32(t)) for t in iou_thrs]), T, ptr(flags), stream())
    return flags


class DeviceMapAccumulator:
    """Per-detection rows of an evaluation pass in [num_images, max_per_img] buffers on `device` (score fp32, label int32, flags
    [T, num_images, max_per_img] uint8, num int32) + per-class gt counts.  update() is called once per batch with the padded NMS outputs;
    finalize() returns what eval_map returns, per IoU threshold."""

    def __init__(self, num_classes, iou_thrs, max_per_img, num_images, device, scale_ranges=None, tpfp_fn=None):
        if scale_ranges is not None:
            raise ValueError('the device metric has no area ranges (scale_ranges); use eval_map')
        if tpfp_fn is not None:
            raise ValueError('the device metric runs tpfp_default only (custom tpfp_fn); use eval_map')
        iou_thrs = [float(iou_thrs)] if isinstance(iou_thrs, (int, float)) else [float(t) for t in iou_thrs]
        if not 1 <= len(iou_thrs) <= MAX_THRESHOLDS:
            raise ValueError(f'the device metric takes 1..{MAX_THRESHOLDS} IoU thresholds per pass, got {len(iou_thrs)}')
        self.num_classes, self.iou_thrs, self.M, self.N = int(num_classes), iou_thrs, int(max_per_img), int(num_images)
        self.device = torch.device(device)
        T = len(iou_thrs)
        self.score = torch.zeros(self.N, self.M, dtype=torch.float32, device=self.device)
        self.label = torch.full((self.N, self.M), -1, dtype=torch.int32, device=self.device)
        self.flags = torch.zeros(T, self.N, self.M, dtype=torch.uint8, device=self.device)
        self.num = torch.zeros(self.N, dtype=torch.int32, device=self.device)
        self.owned = torch.zeros(self.N, dtype=torch.bool, device=self.device)
        self.num_gts = np.zeros(self.num_classes, dtype=np.int64)

    # ------------------------------------------------------------------ filling
    def _count_gts(self, annotations):
        for ann in annotations:
            lb = np.asarray(ann['labels']).reshape(-1).astype(np.int64)
            self.num_gts += np.bincount(lb[(lb >= 0) & (lb < self.num_classes)], minlength=self.num_classes)

    def store(self, rows, score, label, flags, num, annotations):
        """Write a batch whose flags are already known: rows [B] int64 global image rows (on the buffers' device), score [B,M] fp32,
        label [B,M] integer, flags [T,B,M] uint8, num [B] int32.  No host sync.  (update() ends here; the CPU tests start here.)"""
        self.score.index_copy_(0, rows, score.to(torch.float32))
        self.label.index_copy_(0, rows, label.to(torch.int32))
        self.flags.index_copy_(1, rows, flags)
        self.num.index_copy_(0, rows, num.to(torch.int32).clamp(0, self.M))
        self.owned.index_fill_(0, rows, True)
        self._count_gts(annotations)

    def update(self, image_indices, dets, labels, num, annotations):
        """dets [B,M,5] fp32 / labels [B,M] int64 / num [B] int32: the padded device outputs of scoring.multiclass_nms_batch for the images
        `image_indices` (global rows) with their `annotations`.  One H2D copy (packed gts + rows), one launch, no host sync."""
        B, M = int(dets.shape[0]), int(dets.shape[1])
        assert M == self.M and len(image_indices) == B == len(annotations), (M, self.M, B, len(image_indices), len(annotations))
        gb, gl, gi, gn = pack_annotations(annotations)
        G = gb.shape[1]
        # one host buffer: rows int64 | boxes fp32 | labels int32 | num int32 | ignore uint8 (every section starts 8-byte aligned or better)
        parts = [np.asarray(image_indices, np.int64), gb, gl, gn, gi]
        offs, tot = [], 0
        for p in parts:
            offs.append(tot)
            tot += (p.nbytes + 7) // 8 * 8
        host = torch.empty(tot, dtype=torch.uint8)
        if dets.is_cuda:
            host = host.pin_memory()
        hv = host.numpy()
        for p, o in zip(parts, offs):
            hv[o:o + p.nbytes] = p.reshape(-1).view(np.uint8)
        dev = host.to(dets.device, non_blocking=True)
        sec = lambda k, dt, shape: dev[offs[k]:offs[k] + parts[k].nbytes].view(dt).view(shape)
        rows = sec(0, torch.int64, (B,))
        flags = eval_match(dets, labels, num, sec(1, torch.float32, (B, G, 4)), sec(2, torch.int32, (B, G)), sec(4, torch.uint8, (B, G)),
                           sec(3, torch.int32, (B,)), self.iou_thrs)
        self.store(rows, dets[:, :, 4], labels, flags, num, annotations)

    # ------------------------------------------------------------------ combining
    def merge(self, other):
        """Take over the image rows `other` owns (ranks / shards own disjoint rows) and add its gt counts."""
        assert (other.N, other.M, other.num_classes, other.iou_thrs) == (self.N, self.M, self.num_classes, self.iou_thrs)
        m = other.owned.to(self.device)
        self.score = torch.where(m[:, None], other.score.to(self.device), self.score)
        self.label = torch.where(m[:, None], other.label.to(self.device), self.label)
        self.flags = torch.where(m[None, :, None], other.flags.to(self.device), self.flags)
        self.num = torch.where(m, other.num.to(self.device), self.num)
        self.owned = self.owned | m
        self.num_gts = self.num_gts + other.num_gts
        return self

    def gather(self):
        """All ranks' rows on every rank (parallel.gather_rows; gt counts are summed).  No process group: nothing to do."""
        from ..parallel import gather_rows, get_dist_info
        if get_dist_info()[1] == 1:
            return self
        import torch.distributed as dist
        owned = self.owned
        self.score, _ = gather_rows(self.score, owned)
        self.label, _ = gather_rows(self.label, owned)
        self.flags = gather_rows(self.flags.transpose(0, 1).contiguous(), owned)[0].transpose(0, 1).contiguous()
        self.num, self.owned = gather_rows(self.num, owned)
        cnt = torch.from_numpy(self.num_gts).to(self.device)
        dist.all_reduce(cnt)
        self.num_gts = cnt.cpu().numpy()
        return self

    # ------------------------------------------------------------------ the metric
    def finalize(self, dataset=None):
        """-> list over the IoU thresholds of (mean_ap, eval_results), each exactly eval_map(..., iou_thr=thr, dataset=dataset)'s."""
        T, N, M = len(self.iou_thrs), self.N, self.M
        # one D2H copy: the four buffers as one byte vector
        blob = torch.cat([self.score.reshape(-1).view(torch.uint8), self.label.reshape(-1).view(torch.uint8), self.num.view(torch.uint8),
                          self.flags.reshape(-1)]).cpu().numpy()
        o1, o2, o3 = N * M * 4, N * M * 8, N * M * 8 + N * 4
        score = blob[:o1].view(np.float32).reshape(N, M)
        label = blob[o1:o2].view(np.int32).reshape(N, M)
        num = blob[o2:o3].view(np.int32)
        flags = blob[o3:].reshape(T, N, M)
        valid = np.arange(M)[None, :] < num[:, None]
        picks = []
        for c in range(self.num_classes):
            sel = valid & (label == c)                       # row-major boolean pick: image-major, within an image by detection row
            picks.append((sel, np.ascontiguousarray(score[sel])))
        out = []
        for t in range(T):
            eval_results = []
            for c, (sel, sc) in enumerate(picks):
                f = flags[t][sel]
                tp, fp = (f == 1).astype(np.float32)[None, :], (f == 2).astype(np.float32)[None, :]
                num_gts = np.zeros(1, dtype=int)
                num_gts[0] += int(self.num_gts[c])
                eval_results.append(class_result(sc, tp, fp, num_gts, True, dataset))
            out.append((mean_of_aps(eval_results), eval_results))
        return out
