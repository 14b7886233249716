"""Helpers of the device-metric tests: eval_map-format detections <-> the padded (dets, labels, num) layout of aod_multiclass_nms, and
the expected flags from the host's own tpfp_default, called per image and class."""
import numpy as np

from aod_meh_hua_amd.core import evaluation as ev


def padded_from_results(det_results, M):
    """list[image][class] of (k,5) float32 -> dets [N,M,5] float32, labels [N,M] int64, num [N] int32.  Rows are class-major in the given
    order (NOT sorted by score: the kernel must not assume it), so bbox2result of the padded rows gives `det_results` back."""
    N = len(det_results)
    dets, labels, num = np.zeros((N, M, 5), np.float32), np.zeros((N, M), np.int64), np.zeros((N,), np.int32)
    for i, per_cls in enumerate(det_results):
        rows = np.concatenate(per_cls, 0) if per_cls else np.zeros((0, 5), np.float32)
        lab = np.concatenate([np.full(len(d), c, np.int64) for c, d in enumerate(per_cls)]) if per_cls else np.zeros(0, np.int64)
        assert len(rows) <= M
        dets[i, :len(rows)], labels[i, :len(rows)], num[i] = rows, lab, len(rows)
    return dets, labels, num


def results_from_padded(dets, labels, num, num_classes):
    """bbox2result per image of the valid rows."""
    return [[dets[i, :num[i]][labels[i, :num[i]] == c] for c in range(num_classes)] for i in range(len(num))]


def host_flags(dets, labels, num, anns, thrs, num_classes, stable_ties=False):
    """flags [T,N,M] uint8 (0 neither, 1 tp, 2 fp; rows >= num: 0) from tpfp_default per (image, class, threshold).  stable_ties: the
    host function is fed surrogate scores -stable_rank (rank by descending score, ties by lower row, inside the image's class): only the
    score ORDER enters tpfp_default, so the surrogate is tie-free and order-equivalent and numpy's sort internals do not matter."""
    N, M = labels.shape
    out = np.zeros((len(thrs), N, M), np.uint8)
    for i in range(N):
        n = int(num[i])
        ann = anns[i]
        for c in range(num_classes):
            rows = np.flatnonzero(labels[i, :n] == c)
            if not rows.size:
                continue
            d = dets[i, rows].copy()
            if stable_ties:
                order = np.lexsort((rows, -d[:, 4].astype(np.float64)))          # primary: descending score, then row
                rank = np.empty(len(rows), np.int64)
                rank[order] = np.arange(len(rows))
                d[:, 4] = -rank.astype(np.float32)
            g = ann['bboxes'][ann['labels'] == c]
            gi = ann['bboxes_ignore'][ann['labels_ignore'] == c] if ann.get('labels_ignore', None) is not None else np.zeros((0, 4), np.float32)
            for t, thr in enumerate(thrs):
                tp, fp = ev.tpfp_default(d, g.astype(np.float32).reshape(-1, 4), gi.astype(np.float32).reshape(-1, 4), thr)
                out[t, i, rows] = (tp[0] + 2 * fp[0]).astype(np.uint8)
    return out


def assert_same_eval(got, want):
    """(mean_ap, eval_results) pairs: the same float and np.array_equal on every per-class entry, dtypes included"""
    assert got[0] == want[0] and type(got[0]) is type(want[0]), (got[0], want[0])
    assert len(got[1]) == len(want[1])
    for c, (a, b) in enumerate(zip(got[1], want[1])):
        assert set(a) == set(b) == {'num_gts', 'num_dets', 'recall', 'precision', 'ap'}
        assert a['num_gts'] == b['num_gts'] and type(a['num_gts']) is type(b['num_gts']), c
        assert a['num_dets'] == b['num_dets'] and type(a['num_dets']) is type(b['num_dets']), c
        for k in ('recall', 'precision'):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (c, k)
        assert np.asarray(a['ap']).dtype == np.asarray(b['ap']).dtype and np.array_equal(a['ap'], b['ap']), (c, a['ap'], b['ap'])
