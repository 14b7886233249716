#!/usr/bin/env python
"""What the IoU / GIoU box forms cost: ms per captured training iteration of 16 x 512^2 on SSL_L_RetinaNet (RetinaNet-R50 + MEH)
with loss_bbox = L1Loss (the default: the launches as they always were), IoULoss and GIoULoss (reg_decoded_bbox=True) -- three models built
from one seed, each with its own optimizers, each replayed from its own graph (graphs.GraphedTrainStep).  Only rows with a box weight --
the positives -- evaluate the decode (four exponentials) and the overlap terms, in the lane that formed |d| * w before.  The variants are
interleaved repetition by repetition; medians and the 5th..95th percentile, and the ratios over L1.

    python tools/iou_loss_cost.py [--batch 16] [--size 512] [--reps 20] [--inner 4] [--warmup 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOSSES = dict(L1=(dict(type='L1Loss', loss_weight=1.0), False), IoU=(dict(type='IoULoss', loss_weight=1.0), True),
              GIoU=(dict(type='GIoULoss', loss_weight=1.0), True))


def _build(dev, cd, name, seed=20):
    """bench.build_model's detector, with the box loss written into the head's config"""
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg.model.backbone.pop('init_cfg')
    cfg.model.backbone.depth = cd['depth']
    cfg.model.bbox_head.num_classes = cd['classes']
    cfg.model.bbox_head.loss_cls.num_classes = cd['classes']
    cfg.model.bbox_head.loss_bbox, cfg.model.bbox_head.reg_decoded_bbox = dict(LOSSES[name][0]), LOSSES[name][1]
    torch.manual_seed(seed)
    model = build_detector(cfg.model)
    model.init_weights()
    with torch.no_grad():
        model.bbox_head.retina_L.bias.fill_(0.1)
    return model.to(dev), cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--inner', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    import bench
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd.graphs import GraphedTrainStep
    dev = torch.device('cuda', 0)
    cd = dict(bench.CONFIGS['voc512'], batch=args.batch, H=args.size, W=args.size)
    data = bench.synth_batch(cd['batch'], cd['H'], cd['W'], dev, seed=1021, classes=cd['classes'])
    res = dict(batch=args.batch, size=args.size, reps=args.reps, inner=args.inner, warmup=args.warmup, precision=AF.get_precision(),
               device=torch.cuda.get_device_name(0), timing='inner replayed iterations queued between two device events, variants interleaved')
    fns, last = {}, {}
    for name in LOSSES:
        model, cfg = _build(dev, cd, name)
        model.train()
        opt, opt_L = bench.make_optimizers(model, cfg)
        gs = GraphedTrainStep(model, opt, opt_L, Labeled=True, Pseudo=False)

        def replayed(gs=gs, model=model, name=name):
            model.train()
            for _ in range(args.inner):
                last[name] = gs(data)
        fns[name] = replayed
    for _ in range(args.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.inner)
    for k, t in times.items():
        t = np.asarray(t)
        res[k + '_ms'] = round(float(np.median(t)), 3)
        res[k + '_p5_p95_ms'] = [round(float(np.percentile(t, 5)), 3), round(float(np.percentile(t, 95)), 3)]
        res[k + '_loss_bbox'] = round(float(last[k]['log_vars']['loss_bbox']), 5)
    for k in ('IoU', 'GIoU'):
        res[f'{k}_over_L1'] = round(res[k + '_ms'] / res['L1_ms'], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
