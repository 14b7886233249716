#!/usr/bin/env python
"""Wall time of one evaluation of a RetinaNet on a SyntheticVOCDataset through the host path (single_gpu_test + dataset.evaluate) and
through the device path (apis.test.single_gpu_map: graph-replayed padded detections -> aod_eval_match -> one D2H copy), each split into
the detection pass and the metric.  --metric bbox times the COCO bbox metric the same way: CocoDataset.evaluate's evaluator
(core/coco_eval.evaluate_bbox) on single_gpu_test's results against apis.single_gpu_coco_map (aod_coco_match), the synthetic annotations
read as COCO ground truth.

    python tools/eval_throughput.py --images 512 --size 512 --rounds 3
    python tools/eval_throughput.py --images 512 --size 512 --rounds 3 --metric bbox

Both paths run in this process on the same model and loader, warmed once (the device path captures its graph there), then interleaved
host / device per round; the medians are reported.  One JSON line per round and a summary line.  A measurement, not a test."""
import argparse
import json
import os.path as osp
import statistics
import sys
import time

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--images', type=int, default=512)
    p.add_argument('--size', type=int, default=512)
    p.add_argument('--samples-per-gpu', type=int, default=16)
    p.add_argument('--workers', type=int, default=8)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--cls-bias', type=float, default=1.0, help='classification bias of the seeded weights (1.0: ~100 detections per image)')
    p.add_argument('--metric', choices=['mAP', 'bbox'], default='mAP', help='mAP: the VOC metric (default); bbox: the COCO bbox metric')
    a = p.parse_args()
    import numpy as np
    import torch

    from aod_meh_hua_amd.apis.test import single_gpu_coco_map, single_gpu_map, single_gpu_test
    from aod_meh_hua_amd.datasets import build_dataloader, build_dataset
    from aod_meh_hua_amd.mmcv_lite import Config, MMDataParallel
    from aod_meh_hua_amd.models import build_detector
    from oracle import model as omodel
    cfg = Config.fromfile(osp.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg.model.backbone.pop('init_cfg', None)
    model = build_detector(cfg.model)
    model.load_state_dict(omodel.seeded_state_dict(cls_bias=a.cls_bias), strict=True)
    model = MMDataParallel(model.cuda())
    ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=a.images, size=(a.size, a.size)), dict(test_mode=True))
    dl = build_dataloader(ds, samples_per_gpu=a.samples_per_gpu, workers_per_gpu=a.workers, dist=False, shuffle=False)

    key = 'mAP' if a.metric == 'mAP' else 'bbox_mAP'
    if a.metric == 'bbox':          # the synthetic annotations as COCO ground truth: xywh boxes, area = w * h, no crowds
        from aod_meh_hua_amd.core.coco_eval import evaluate_bbox
        infos = []
        for i in range(len(ds)):
            ann = ds.get_ann_info(i)
            bb = ann['bboxes'].astype(np.float64)
            wh = bb[:, 2:] - bb[:, :2]
            infos.append(dict(boxes=np.concatenate([bb[:, :2], wh], 1), area=wh[:, 0] * wh[:, 1], iscrowd=np.zeros(len(bb), np.uint8),
                              labels=ann['labels'].astype(np.int64)))

    def host():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        results = single_gpu_test(model, dl, isUnc=False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = ds.evaluate(results, logger='silent') if a.metric == 'mAP' else evaluate_bbox(results, infos, ds.CLASSES, logger='silent')
        return dict(pass_s=t1 - t0, metric_s=time.perf_counter() - t1, mAP=out[key], dets=sum(c.shape[0] for r in results for c in r))

    def device():
        tm = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if a.metric == 'bbox':
            out = single_gpu_coco_map(model, dl, isUnc=False, eval_infos=infos, _timing=tm)
            total = time.perf_counter() - t0
            return dict(pass_s=tm['pass_s'], metric_s=total - tm['pass_s'], mAP=out[key], dets=None)
        mean_ap, res = single_gpu_map(model, dl, iou_thr=0.5, dataset='voc07', isUnc=False, _timing=tm)
        total = time.perf_counter() - t0
        return dict(pass_s=tm['pass_s'], metric_s=total - tm['pass_s'], mAP=mean_ap, dets=sum(r['num_dets'] for r in res))

    h0, d0 = host(), device()                      # warm-up: loader workers, kernels, the eval graph's capture, the annotation cache
    if (h0['mAP'], h0['dets'] if d0['dets'] is not None else None) != (d0['mAP'], d0['dets']):
        raise SystemExit(f'the two paths disagree: host {h0}, device {d0}')
    rounds = []
    for r in range(a.rounds):
        h, d = host(), device()
        rounds.append((h, d))
        print(json.dumps(dict(kind='round', round=r, host=h, device=d)), flush=True)
    med = lambda path, k: round(statistics.median(x[path][k] for x in rounds), 4)
    s = dict(kind='summary', metric=a.metric, images=a.images, size=a.size, samples_per_gpu=a.samples_per_gpu, workers=a.workers, rounds=a.rounds,
             detections=h0['dets'], mAP=h0['mAP'])
    for i, name in enumerate(('host', 'device')):
        s[f'{name}_pass_s'], s[f'{name}_metric_s'] = med(i, 'pass_s'), med(i, 'metric_s')
        s[f'{name}_total_s'] = round(statistics.median(x[i]['pass_s'] + x[i]['metric_s'] for x in rounds), 4)
    s['speedup'] = round(s['host_total_s'] / s['device_total_s'], 2)
    print(json.dumps(s), flush=True)


if __name__ == '__main__':
    main()
