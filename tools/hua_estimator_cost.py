#!/usr/bin/env python
"""What the HUA launch sequence (pairs -> sample | closed -> reduce) costs per scoring batch with each estimator: `mc` (the default, 500
Dirichlet samples per pair), `closed` (closed form of the Monte-Carlo limit) and `closed` + per-object outputs (the reduce kernel's
second instance).  The batch is the bench scoring batch (16 x 512^2 of the synthetic pool, candidates / detections as the scoring pass
produces them with the calibrated head).  Every variant is captured into a graph (no host launch path in the window) and timed with
device events; the variants are INTERLEAVED repetition by repetition so that clock drift hits all of them alike; median and the
5th..95th percentile spread of --reps repetitions after --warmup are reported.

    python tools/hua_estimator_cost.py [--reps 100] [--warmup 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--variants', default='mc,closed,closed_objects,mc_objects',
                    help="comma list; 'mc' alone also runs on a library built from an older commit (AOD_HIP_LIB): the comparison base")
    ap.add_argument('--out')
    args = ap.parse_args()
    assert args.reps >= 50, 'at least 50 timed repetitions'
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    import bench
    from aod_meh_hua_amd import scoring
    dev = torch.device('cuda', 0)
    cd = dict(bench.CONFIGS['voc512'])
    model, _ = bench.build_model(dev, cd)
    pool = bench.synth_batch(cd['batch'], cd['H'], cd['W'], dev, seed=1020, classes=cd['classes'])
    bench.calibrate_head(model, pool['img'])
    head = model.bbox_head
    model.eval()
    with torch.no_grad():
        feats = model.extract_feat(pool['img'])
        outs, Ls = head.forward(feats), head.forward_L(feats)
        kw = {k: v for k, v in bench.SCORE_KW.items() if k not in ('return_loss', 'rescale')}
        _, unc, it = head.get_bboxes(*outs, pool['img_metas'], rescale=True, with_nms=True, L_scores=Ls, _return_internals=True, **kw)
    B = unc.shape[0]
    ids = torch.arange(B, device=dev, dtype=torch.int64)
    hargs = (it['cand'], it['dets'], it['num'], ids, head.test_cfg.max_per_img)
    _, pc, _ = scoring.hua_score(*hargs, want_pairs=True)
    variants = {'mc': dict(), 'closed': dict(estimator='closed'), 'closed_objects': dict(estimator='closed', want_objects=True),
                'mc_objects': dict(want_objects=True)}
    graphs = {k: _capture(lambda v=v: scoring.hua_score(*hargs, **v)) for k, v in variants.items() if k in args.variants.split(',')}
    for _ in range(args.warmup):
        for g in graphs.values():
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(args.reps):
        for k, g in graphs.items():                      # interleaved: one repetition of every variant per round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    res = dict(batch=B, size=[cd['H'], cd['W']], pairs=int(pc.sum()), objects=int((it['dets'][..., 4] > 0.3).sum()), reps=args.reps,
               warmup=args.warmup, timing='device events around graph replays, variants interleaved')
    for k, t in times.items():
        t = np.asarray(t)
        res[k + '_us'] = round(float(np.median(t)), 2)
        res[k + '_p5_p95_us'] = [round(float(np.percentile(t, 5)), 2), round(float(np.percentile(t, 95)), 2)]
    if 'mc' in times:
        res['mc_spread_us'] = round(res['mc_p5_p95_us'][1] - res['mc_p5_p95_us'][0], 2)
    if 'mc' in times and 'closed' in times:
        res['closed_over_mc'] = round(res['closed_us'] / res['mc_us'], 3)
    if 'closed_objects' in times and 'closed' in times:
        res['objects_extra_us'] = round(res['closed_objects_us'] - res['closed_us'], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
