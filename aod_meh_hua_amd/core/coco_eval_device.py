"""Device form of the COCO bbox metric (core/coco_eval.py): the per-image matching -- coco_eval.match_image once per image and
class on the host -- runs in `aod_coco_match` on the padded (dets, labels, num) triple that `aod_multiclass_nms` leaves on the device, per
batch and without a host sync, for the four area ranges and every IoU threshold at once.  The per-detection (score, label, state) rows are
kept in fixed-size device buffers as in evaluation_device.DeviceMapAccumulator, ranks own disjoint image rows and all-gather them, and ONE
D2H copy per evaluation feeds the numpy tail the host path runs (coco_eval.accumulate / summarize): the stable sort there orders equal
scores by (image, row), which is the host path's (image, rank) order, so the dict equals CocoDataset.evaluate's value for value."""
import numpy as np
import torch

from . import coco_eval

# the limits of csrc/cocomatch.hip (CM_MAX_T, CM_MAX_A, CM_MAX_M, CM_MAX_G): checked here so that a caller gets a ValueError that names the
# shape, and by the entry itself (tests/test_gpu_coco_match.py::test_entry_refusals holds the two sides together)
MAX_THRESHOLDS = 16
MAX_RANGES = 4
MAX_DETS = 1024          # rows per image
MAX_GTS = 512            # gts per image


def pack_eval_infos(infos):
    """CocoDataset.get_eval_info dicts of a batch -> (boxes [B,G,4] float64 xywh, area [B,G] float64, labels [B,G] int32, crowd [B,G] uint8,
    num [B] int32), file order kept, G = the batch's largest gt count (at least 1).  Padding rows: zero box, label -1."""
    B = len(infos)
    G = max([1] + [len(i['labels']) for i in infos])
    boxes, area = np.zeros((B, G, 4), np.float64), np.zeros((B, G), np.float64)
    labels, crowd, num = np.full((B, G), -1, np.int32), np.zeros((B, G), np.uint8), np.zeros((B,), np.int32)
    for b, i in enumerate(infos):
        n = len(i['labels'])
        boxes[b, :n], area[b, :n], labels[b, :n], crowd[b, :n], num[b] = np.asarray(i['boxes']).reshape(-1, 4), i['area'], i['labels'], i['iscrowd'], n
    return boxes, area, labels, crowd, num


def coco_match(dets, labels, num, gt_boxes, gt_area, gt_labels, gt_crowd, gt_num, iou_thrs, area_ranges=coco_eval.AREA_RANGES):
    """aod_coco_match on device tensors -> states [A, T, B, M] uint8 (1 tp, 0 fp, 2 ignored; rows >= num[b]: 0)."""
    import ctypes as C
    from .._C import call, ptr, stream
    B, M, G = int(dets.shape[0]), int(dets.shape[1]), int(gt_boxes.shape[1])
    T, A = len(iou_thrs), len(area_ranges)
    if not 1 <= T <= MAX_THRESHOLDS:
        raise ValueError(f'coco_match: 1..{MAX_THRESHOLDS} IoU thresholds, got {T}')
    if not 1 <= A <= MAX_RANGES:
        raise ValueError(f'coco_match: 1..{MAX_RANGES} area ranges, got {A}')
    if M > MAX_DETS:
        raise ValueError(f'coco_match: at most {MAX_DETS} detection rows per image, got {M}')
    if G > MAX_GTS:
        raise ValueError(f'coco_match: at most {MAX_GTS} gts per image, got {G} (use CocoDataset.evaluate for such a set)')
    assert dets.dtype == torch.float32 and labels.dtype == torch.int64 and num.dtype == torch.int32 and dets.shape[2] == 5
    assert gt_boxes.dtype == torch.float64 and gt_area.dtype == torch.float64 and gt_labels.dtype == torch.int32
    assert gt_crowd.dtype == torch.uint8 and gt_num.dtype == torch.int32
    assert gt_boxes.shape == (B, G, 4) and gt_area.shape == gt_labels.shape == gt_crowd.shape == (B, G) and labels.shape == (B, M)
    assert num.shape == gt_num.shape == (B,)
    # zeros, not empty: a row whose score is NaN has no rank, and the kernel then leaves some rows below num[b] unwritten
    states = torch.zeros(A, T, B, M, dtype=torch.uint8, device=dets.device)
    rng = [float(v) for r in area_ranges for v in r]
    call('aod_coco_match', ptr(dets.contiguous()), ptr(labels.contiguous()), ptr(num.contiguous()), ptr(gt_boxes.contiguous()),
         ptr(gt_area.contiguous()), ptr(gt_labels.contiguous()), ptr(gt_crowd.contiguous()), ptr(gt_num.contiguous()), B, M, G,
         (C.c_double * (2 * A))(*rng), A, (C.c_double * T)(*[float(t) for t in iou_thrs]), T, ptr(states), stream())
    return states


class DeviceCocoAccumulator:
    """Per-detection rows of a COCO evaluation pass in [num_images, max_per_img] buffers on `device` (score fp32, label int32, states
    [A, T, num_images, max_per_img] uint8, num int32, owned bool) + the counted gts per (class, range), counted on the host from the
    annotations.  update() is called once per batch with the padded NMS outputs; finalize() returns CocoDataset.evaluate's dict."""

    def __init__(self, num_classes, iou_thrs, max_per_img, num_images, device, proposal_nums=(100, 300, 1000)):
        iou_thrs = coco_eval.default_iou_thrs() if iou_thrs is None else np.asarray(iou_thrs, np.float64).reshape(-1)
        if not 1 <= len(iou_thrs) <= MAX_THRESHOLDS:
            raise ValueError(f'the device COCO metric takes 1..{MAX_THRESHOLDS} IoU thresholds per pass, got {len(iou_thrs)}')
        self.proposal_nums = tuple(int(p) for p in proposal_nums)
        if int(max_per_img) > self.proposal_nums[-1]:
            raise ValueError(f'the device COCO metric keeps every detection row: max_per_img = {max_per_img} exceeds maxDets = '
                             f'proposal_nums[-1] = {self.proposal_nums[-1]}, a truncation only CocoDataset.evaluate performs')
        if int(max_per_img) > MAX_DETS:
            raise ValueError(f'the device COCO metric takes up to {MAX_DETS} detection rows per image, max_per_img = {max_per_img}')
        self.num_classes, self.iou_thrs, self.M, self.N = int(num_classes), iou_thrs, int(max_per_img), int(num_images)
        self.area_ranges = coco_eval.AREA_RANGES
        self.device = torch.device(device)
        A, T = len(self.area_ranges), len(iou_thrs)
        self.score = torch.zeros(self.N, self.M, dtype=torch.float32, device=self.device)
        self.label = torch.full((self.N, self.M), -1, dtype=torch.int32, device=self.device)
        self.states = torch.zeros(A, T, self.N, self.M, dtype=torch.uint8, device=self.device)
        self.num = torch.zeros(self.N, dtype=torch.int32, device=self.device)
        self.owned = torch.zeros(self.N, dtype=torch.bool, device=self.device)
        self.npig = np.zeros((self.num_classes, A), dtype=np.int64)

    def _same(self, other):
        return ((other.N, other.M, other.num_classes, other.proposal_nums) == (self.N, self.M, self.num_classes, self.proposal_nums)
                and np.array_equal(other.iou_thrs, self.iou_thrs))

    # ------------------------------------------------------------------ filling
    def store(self, rows, score, label, states, num, infos):
        """Write a batch whose states are already known: rows [B] int64 global image rows (on the buffers' device), score [B,M] fp32,
        label [B,M] integer, states [A,T,B,M] uint8, num [B] int32, infos: the images' eval infos.  No host sync.  (update() ends here;
        the CPU tests start here.)"""
        self.score.index_copy_(0, rows, score.to(torch.float32))
        self.label.index_copy_(0, rows, label.to(torch.int32))
        self.states.index_copy_(2, rows, states)
        self.num.index_copy_(0, rows, num.to(torch.int32).clamp(0, self.M))
        self.owned.index_fill_(0, rows, True)
        self.npig += coco_eval.count_npig(infos, self.num_classes, self.area_ranges)

    def update(self, image_indices, dets, labels, num, infos):
        """dets [B,M,5] fp32 / labels [B,M] int64 / num [B] int32: the padded device outputs of scoring.multiclass_nms_batch for the images
        `image_indices` (global rows) with their eval infos.  One H2D copy (packed gts + rows), one launch, no host sync."""
        B, M = int(dets.shape[0]), int(dets.shape[1])
        assert M == self.M and len(image_indices) == B == len(infos), (M, self.M, B, len(image_indices), len(infos))
        gb, ga, gl, gc, gn = pack_eval_infos(infos)
        G = gb.shape[1]
        # one host buffer: rows int64 | boxes fp64 | area fp64 | labels int32 | num int32 | crowd uint8 (every section starts 8-byte aligned)
        parts = [np.asarray(image_indices, np.int64), gb, ga, gl, gn, gc]
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
        states = coco_match(dets, labels, num, sec(1, torch.float64, (B, G, 4)), sec(2, torch.float64, (B, G)), sec(3, torch.int32, (B, G)),
                            sec(5, torch.uint8, (B, G)), sec(4, torch.int32, (B,)), self.iou_thrs, self.area_ranges)
        self.store(sec(0, torch.int64, (B,)), dets[:, :, 4], labels, states, num, infos)

    # ------------------------------------------------------------------ combining
    def merge(self, other):
        """Take over the image rows `other` owns (ranks / shards own disjoint rows) and add its gt counts."""
        assert self._same(other)
        m = other.owned.to(self.device)
        self.score = torch.where(m[:, None], other.score.to(self.device), self.score)
        self.label = torch.where(m[:, None], other.label.to(self.device), self.label)
        self.states = torch.where(m[None, None, :, None], other.states.to(self.device), self.states)
        self.num = torch.where(m, other.num.to(self.device), self.num)
        self.owned = self.owned | m
        self.npig = self.npig + other.npig
        return self

    def gather(self):
        """All ranks' rows on every rank (parallel.gather_rows; gt counts are summed).  No process group: nothing to do."""
        from ..parallel import gather_rows, get_dist_info
        if get_dist_info()[1] == 1:
            return self
        import torch.distributed as dist
        owned = self.owned
        A, T = self.states.shape[:2]
        self.score, _ = gather_rows(self.score, owned)
        self.label, _ = gather_rows(self.label, owned)
        st = gather_rows(self.states.permute(2, 0, 1, 3).contiguous(), owned)[0]
        self.states = st.permute(1, 2, 0, 3).contiguous()
        self.num, self.owned = gather_rows(self.num, owned)
        cnt = torch.from_numpy(self.npig).to(self.device)
        dist.all_reduce(cnt)
        self.npig = cnt.cpu().numpy()
        return self

    # ------------------------------------------------------------------ the metric
    def precision(self):
        """one D2H copy -> coco_eval.accumulate's precision [T, 101, K, A]"""
        N, M = self.N, self.M
        A, T = self.states.shape[:2]
        blob = torch.cat([self.score.reshape(-1).view(torch.uint8), self.label.reshape(-1).view(torch.uint8), self.num.view(torch.uint8),
                          self.states.reshape(-1)]).cpu().numpy()
        o1, o2, o3 = N * M * 4, N * M * 8, N * M * 8 + N * 4
        score = blob[:o1].view(np.float32).reshape(N, M)
        label = blob[o1:o2].view(np.int32).reshape(N, M)
        num = blob[o2:o3].view(np.int32)
        states = blob[o3:].reshape(A, T, N, M)
        valid = np.arange(M)[None, :] < num[:, None]          # row-major pick: image-major, within an image by detection row
        return coco_eval.accumulate(score[valid], label[valid], states[:, :, valid], self.npig, self.num_classes)

    def finalize(self, classes=None, classwise=False, metric_items=None, logger=None):
        """-> the dict CocoDataset.evaluate(results, metric='bbox', iou_thrs=..., classwise=..., metric_items=...) returns"""
        return coco_eval.format_eval(self.precision(), self.iou_thrs, classes, classwise, metric_items, logger, self.proposal_nums[-1])
