#!/usr/bin/env python
"""What the class-difficulty tracking costs: ms per training iteration of 16 x 512^2 on SSL_L_RetinaNet (RetinaNet-R50 + MEH) with
bbox_head.class_difficulty off and on -- two models built from one seed, each with its own optimizers -- eager and replayed
(graphs.GraphedTrainStep), and ms per `Entropy` scoring batch without and with class_weighted, eager and replayed (graphs.GraphedScore).
The yardstick is the same run with the option off: nothing is enqueued there, it is the path of a build without the feature.  On: the
accumulate (block partials + a one-block add) and the EMA update behind the loss forward, three small launches per iteration; a weighted
scoring batch adds one multiply per detection inside the aod_det_uncertainty launch.  The variants are interleaved repetition by
repetition; medians and the 5th..95th percentile.

    python tools/difficulty_cost.py [--batch 16] [--size 512] [--reps 20] [--inner 4] [--warmup 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLASS_DIFFICULTY = dict(xi=0.6, momentum=0.99, alpha=0.3, beta=0.2)


def _build(dev, cd, tracked, seed=20):
    """bench.build_model's detector, with the option written into the head's config"""
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg.model.backbone.pop('init_cfg')
    cfg.model.backbone.depth = cd['depth']
    cfg.model.bbox_head.num_classes = cd['classes']
    cfg.model.bbox_head.loss_cls.num_classes = cd['classes']
    if tracked:
        cfg.model.bbox_head.class_difficulty = dict(CLASS_DIFFICULTY)
    torch.manual_seed(seed)
    model = build_detector(cfg.model)
    model.init_weights()
    with torch.no_grad():
        model.bbox_head.retina_L.bias.fill_(0.1)
    return model.to(dev), cfg


def _eager_iter(model, opt, opt_L, data):
    out, head_out, feat_out, prev = model.train_step(data, Labeled=True, Pseudo=False)
    opt.zero_grad()
    out['loss'].backward()
    lossL = model.train_step_L(prev, head_out, feat_out)
    opt_L.zero_grad()
    lossL['loss'].backward()
    opt.step()
    opt_L.step()


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
    from aod_meh_hua_amd.graphs import GraphedScore, GraphedTrainStep
    dev = torch.device('cuda', 0)
    cd = dict(bench.CONFIGS['voc512'], batch=args.batch, H=args.size, W=args.size)
    data = bench.synth_batch(cd['batch'], cd['H'], cd['W'], dev, seed=1021, classes=cd['classes'])
    fns, res = {}, dict(batch=args.batch, size=args.size, reps=args.reps, inner=args.inner, warmup=args.warmup, precision=AF.get_precision(),
                        timing='inner iterations / scoring batches queued between two device events, variants interleaved')
    models = {}
    for name, tracked in (('off', False), ('on', True)):
        model, cfg = _build(dev, cd, tracked)
        model.train()
        opt, opt_L = bench.make_optimizers(model, cfg)
        gs = GraphedTrainStep(model, opt, opt_L, Labeled=True, Pseudo=False)
        models[name] = model

        def eager(model=model, opt=opt, opt_L=opt_L):
            model.train()
            for _ in range(args.inner):
                _eager_iter(model, opt, opt_L, data)

        def replayed(gs=gs, model=model):
            model.train()
            for _ in range(args.inner):
                gs(data)
        fns[f'train_{name}_eager'], fns[f'train_{name}_replayed'] = eager, replayed
    # the Entropy scoring batch on the tracking model, without and with the class weights
    scorer, _ = _build(dev, cd, True)
    ids = torch.arange(args.batch, device=dev, dtype=torch.int64)
    img, metas = data['img'], data['img_metas']
    bench.calibrate_head(scorer, img)
    scorer.bbox_head.refresh_class_weight()
    base = dict(rescale=True, isEval=False, isUnc='Epistemic', batchIdx=0, uPool='Entropy', unc_aggregate='max', score_thr=0.3)
    for name, kw in (('Entropy', base), ('Entropy_weighted', dict(base, class_weighted=True))):
        scorer.eval()
        gsc = GraphedScore(scorer, **kw)

        def eager(kw=kw):
            scorer.eval()
            with torch.no_grad():
                for _ in range(args.inner):
                    scorer(img=[img], img_metas=[metas], return_loss=False, image_ids=ids, **kw)

        def replayed(gsc=gsc):
            scorer.eval()
            for _ in range(args.inner):
                gsc(img, metas, ids, defer=True)
            gsc.sync()
        fns[name + '_eager'], fns[name + '_replayed'] = eager, replayed
        with torch.no_grad():
            res[name + '_nonzero_images'] = int((scorer(img=[img], img_metas=[metas], return_loss=False, image_ids=ids, **kw)[1] > 0).sum())
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
        res[f'train_on_over_off_{mode}'] = round(res[f'train_on_{mode}_ms'] / res[f'train_off_{mode}_ms'], 4)
        res[f'Entropy_weighted_over_plain_{mode}'] = round(res[f'Entropy_weighted_{mode}_ms'] / res[f'Entropy_{mode}_ms'], 4)
    d = models['on'].bbox_head.class_difficulty
    res['class_difficulty_min_max'] = [round(float(d.min()), 6), round(float(d.max()), 6)]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
