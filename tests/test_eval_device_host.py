"""CPU tests of the device metric's host side (core/evaluation_device.py): gt packing order, the finalize arithmetic against eval_map on
the seeded detection cases behind tests/golden/eval_map.npz (flags from the host's own tpfp_default), merge of disjoint accumulators, the
row gather over gloo at world 2, and the refusals."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from aod_meh_hua_amd.core import evaluation as ev
from aod_meh_hua_amd.core.evaluation_device import DeviceMapAccumulator, pack_annotations
from tests import synth
from tests.eval_device_util import assert_same_eval, host_flags, padded_from_results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'eval_map.npz'))
THRS = [0.5, 0.75]


def test_pack_annotations_orders_real_gts_before_ignored_ones():
    a0 = dict(bboxes=np.array([[0, 0, 10, 10], [5, 5, 20, 20]], np.float64), labels=np.array([3, 1]),
              bboxes_ignore=np.array([[1, 1, 2, 2]], np.float64), labels_ignore=np.array([3]))
    a1 = dict(bboxes=np.zeros((0, 4), np.float32), labels=np.zeros((0,), np.int64))                       # no gts, no ignore keys
    a2 = dict(bboxes=np.array([[7, 7, 9, 9]], np.float32), labels=np.array([0]), bboxes_ignore=np.array([[1, 2, 3, 4], [4, 3, 2, 1]], np.float32),
              labels_ignore=np.array([5, 0]))
    boxes, labels, ignore, num = pack_annotations([a0, a1, a2])
    assert boxes.shape == (3, 3, 4) and boxes.dtype == np.float32 and labels.dtype == np.int32 and ignore.dtype == np.uint8 and num.dtype == np.int32
    assert num.tolist() == [3, 0, 3]
    assert labels.tolist() == [[3, 1, 3], [-1, -1, -1], [0, 5, 0]]
    assert ignore.tolist() == [[0, 0, 1], [0, 0, 0], [0, 1, 1]]
    assert boxes[0].tolist() == [[0, 0, 10, 10], [5, 5, 20, 20], [1, 1, 2, 2]] and boxes[2].tolist() == [[7, 7, 9, 9], [1, 2, 3, 4], [4, 3, 2, 1]]
    assert not boxes[1].any()
    # a batch without any gt still has one (padding) column
    b, l, i, n = pack_annotations([a1])
    assert b.shape == (1, 1, 4) and l.tolist() == [[-1]] and n.tolist() == [0]
    # float64 VOC boxes arrive as their fp32 roundings
    a = dict(bboxes=np.array([[0.1, 0.2, 100.3, 200.7]], np.float64), labels=np.array([2]))
    assert np.array_equal(pack_annotations([a])[0][0, 0], np.array([0.1, 0.2, 100.3, 200.7], np.float64).astype(np.float32))


def _filled(dets, labels, num, anns, rows, M=32, thrs=THRS):
    acc = DeviceMapAccumulator(20, thrs, M, len(anns), 'cpu')
    flags = host_flags(dets, labels, num, anns, thrs, 20)
    for lo in range(0, len(rows), 5):
        r = rows[lo:lo + 5]
        acc.store(torch.tensor(r, dtype=torch.int64), torch.from_numpy(dets[r, :, 4]), torch.from_numpy(labels[r]), torch.from_numpy(flags[:, r]),
                  torch.from_numpy(num[r]), [anns[i] for i in r])
    return acc


@pytest.mark.parametrize('name,seed,ign', [('a', 50, True), ('b', 51, False)])
def test_finalize_reproduces_eval_map(name, seed, ign):
    results, anns = synth.detection_eval_case(seed=seed, with_ignore=ign)
    dets, labels, num = padded_from_results(results, 32)
    # hostile padding: finalize must never read rows >= num
    for i in range(len(num)):
        dets[i, num[i]:, 4], labels[i, num[i]:] = np.inf, 3
    acc = _filled(dets, labels, num, anns, list(range(len(anns))))
    for ds, tag in (('voc07', 'voc07'), (None, 'area')):
        got = acc.finalize(ds)
        assert len(got) == 2
        for thr, g in zip(THRS, got):
            assert_same_eval(g, ev.eval_map(results, anns, iou_thr=thr, dataset=ds, logger='silent'))
        assert got[0][0] == float(G[f'{name}_{tag}_map'])                          # ... which is the reference's number
        assert np.array_equal(np.array([r['ap'] for r in got[0][1]], np.float64), G[f'{name}_{tag}_ap'])


def test_merge_of_even_and_odd_rows_equals_one_accumulator():
    results, anns = synth.detection_eval_case(seed=50)
    dets, labels, num = padded_from_results(results, 32)
    n = len(anns)
    whole = _filled(dets, labels, num, anns, list(range(n)))
    even, odd = _filled(dets, labels, num, anns, list(range(0, n, 2))), _filled(dets, labels, num, anns, list(range(1, n, 2)))
    assert not np.array_equal(even.num_gts, whole.num_gts) and int(even.owned.sum()) == (n + 1) // 2
    merged = even.merge(odd)
    assert bool(merged.owned.all()) and np.array_equal(merged.num_gts, whole.num_gts)
    for a, b in zip(merged.finalize('voc07'), whole.finalize('voc07')):
        assert_same_eval(a, b)
    assert whole.gather() is whole                                                  # no process group: nothing to do


def _gather_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from aod_meh_hua_amd.parallel import gather_rows
    n = 7
    mine = torch.arange(n) % world == rank
    for dt, shape in ((torch.float32, (n, 3)), (torch.uint8, (n, 2, 4)), (torch.int32, (n,))):
        full = (torch.arange(int(np.prod(shape))).reshape(shape) * 3 + 1).to(dt)
        buf = torch.where(mine.view((-1,) + (1,) * (len(shape) - 1)), full, torch.zeros_like(full))
        got, owned = gather_rows(buf, mine)
        assert got.dtype == dt and torch.equal(got, full) and bool(owned.all()), (rank, dt)
    # the accumulator's gather: each rank stores its rows, every rank finalizes the whole set
    results, anns = synth.detection_eval_case(seed=51, with_ignore=False)
    dets, labels, num = padded_from_results(results, 32)
    acc = _filled(dets, labels, num, anns, list(range(rank, len(anns), world)))
    acc.gather()
    m, res = acc.finalize('voc07')[0]
    q.put((rank, m, [float(r['ap']) for r in res], [int(r['num_gts']) for r in res]))
    dist.destroy_process_group()


def test_row_gather_world2():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 977) % 2000
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    results, anns = synth.detection_eval_case(seed=51, with_ignore=False)
    m, er = ev.eval_map(results, anns, iou_thr=0.5, dataset='voc07', logger='silent')
    for rank, gm, aps, ngt in res:
        assert gm == m and aps == [float(r['ap']) for r in er] and ngt == [r['num_gts'] for r in er]


def test_refusals():
    with pytest.raises(ValueError, match='area ranges'):
        DeviceMapAccumulator(20, [0.5], 8, 4, 'cpu', scale_ranges=[(0, 32)])
    with pytest.raises(ValueError, match='tpfp'):
        DeviceMapAccumulator(20, [0.5], 8, 4, 'cpu', tpfp_fn=ev.tpfp_default)
    with pytest.raises(ValueError, match='thresholds'):
        DeviceMapAccumulator(20, [0.1 * i for i in range(1, 10)], 8, 4, 'cpu')
    DeviceMapAccumulator(20, [0.1 * i for i in range(1, 9)], 8, 4, 'cpu')          # 8 is the limit
    from aod_meh_hua_amd.apis.test import single_gpu_map
    with pytest.raises(ValueError, match='detUnc'):
        single_gpu_map(None, None, detUnc=True)
