#!/usr/bin/env python
"""What a posterior-uncertainty scoring batch costs: ms per scoring batch of 16 x 512^2 for
    Entropy       the new pool on SSL_L_RetinaNet (cls / reg towers, pre-NMS, NMS, one aod_det_uncertainty launch; no lambda tower)
    Entropy_NMS   the paper's rule on the same detector (three towers, pre-NMS, NMS, pair search, Dirichlet sampler, reduce): the yardstick
    detect        the plain isEval detection pass (padded outputs) on MyRetinaNet
each eager and replayed (graphs.GraphedScore: --inner batches queued with defer=True between two device events, so the two-stream form
overlaps as it does in the pool loop).  The evidence head is calibrated as bench.py calibrates it (a trained-like share of foreground
anchors), the plain head's classification bias is set so that a comparable share of its sigmoid scores passes 0.3.  The variants are
interleaved repetition by repetition; medians and the 5th..95th percentile.

    python tools/posterior_unc_cost.py [--batch 16] [--size 512] [--reps 20] [--inner 8] [--warmup 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _plain(dev):
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet_plain.py'))
    cfg.model.backbone.pop('init_cfg')
    model = build_detector(cfg.model)
    model.init_weights()
    with torch.no_grad():
        model.bbox_head.retina_cls.bias.fill_(-2.5)
    return model.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--inner', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    import bench
    from aod_meh_hua_amd.graphs import GraphedScore
    dev = torch.device('cuda', 0)
    cd = dict(bench.CONFIGS['voc512'], batch=args.batch, H=args.size, W=args.size)
    meh, _ = bench.build_model(dev, cd)
    pool = bench.synth_batch(cd['batch'], cd['H'], cd['W'], dev, seed=1020, classes=cd['classes'])
    img, metas = pool['img'].to(dev), pool['img_metas']
    bench.calibrate_head(meh, img)
    meh.eval()
    plain = _plain(dev)
    ids = torch.arange(args.batch, device=dev, dtype=torch.int64)
    base = dict(rescale=True, isEval=False, isUnc='Epistemic', batchIdx=0)
    variants = {'Entropy': (meh, dict(base, uPool='Entropy', unc_aggregate='max', score_thr=0.3)),
                'Entropy_NMS': (meh, dict(base, uPool='Entropy_NMS', uPool2='objectSum_scaleMax_classSum', clsW=False)),
                'detect': (plain, dict(rescale=True, isEval=True, isUnc=False, _padded=True))}
    fns, res = {}, dict(batch=args.batch, size=args.size, reps=args.reps, inner=args.inner, warmup=args.warmup,
                        timing='inner scoring batches queued between two device events (replayed: defer=True, then sync), variants interleaved')
    for name, (model, kw) in variants.items():
        gs = GraphedScore(model, **kw)

        def eager(model=model, kw=kw):
            with torch.no_grad():
                for _ in range(args.inner):
                    model(img=[img], img_metas=[metas], return_loss=False, image_ids=ids, **kw)

        def replayed(gs=gs):
            for _ in range(args.inner):
                gs(img, metas, ids, defer=True)
            gs.sync()
        fns[name + '_eager'], fns[name + '_replayed'] = eager, replayed
        with torch.no_grad():
            out = model(img=[img], img_metas=[metas], return_loss=False, image_ids=ids, **kw)
        if name != 'detect':
            res[name + '_nonzero_images'] = int((out[1] > 0).sum())
        else:
            res['detect_detections'] = int(out[2].sum())
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
    for mode in ('eager', 'replayed'):
        res[f'Entropy_over_Entropy_NMS_{mode}'] = round(res[f'Entropy_{mode}_ms'] / res[f'Entropy_NMS_{mode}_ms'], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
