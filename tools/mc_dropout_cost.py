#!/usr/bin/env python
"""What one MC-dropout forward costs beside the plain classification-map forward, at the bench scoring shape (16 x 512^2), as captured HIP
graphs -- the form the pool pass replays:

  plain     model(isEval=True, justOut=True): the default inference path (whole-block fusions, grouped towers: cls + reg + MEH)
  dropout   the same maps with a Dropout2d behind every ReLU that feeds them (functional.mc_dropout): three launches per bottleneck, one
            apply launch behind each ReLU, the cls tower alone -- plus the eager aod_dropout2d_masks launch in front of every replay

One process, both graphs captured and warmed, INTERLEAVED repetition by repetition so that clock drift hits both alike; per form the
median and the 5th..95th percentile of --reps repetitions of the device time between two events around one replay (the mask launch
included for the dropout form).  The mask kernel is also timed alone.

    python tools/mc_dropout_cost.py [--batch 16] [--size 512] [--reps 50] [--warmup 5] [--rate 0.1] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rate', type=float, default=0.1)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd.graphs import GraphedScore
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    from oracle import model as om
    from tests import synth
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg.model.backbone.pop('init_cfg')
    model = build_detector(cfg.model)
    model.load_state_dict(om.seeded_state_dict(cls_bias=-2.0), strict=True)
    model = model.cuda().eval()
    B, S = args.batch, args.size
    img = synth.images(B, S, S).cuda()
    mt = synth.metas(B, S, S)
    ids = torch.arange(B, dtype=torch.int64, device='cuda')
    sites = AF.dropout_sites(model)
    table = torch.ones(B, sites.T, device='cuda')
    offs = sites.offsets(img.device)
    g_plain = GraphedScore(model, rescale=True, isEval=True, justOut=True)
    g_drop = GraphedScore(model, rescale=True, isEval=True, justOut=True, mc_dropout=AF.MCDropoutState(table, sites))
    state = dict(k=0)

    def plain():
        return g_plain(img, mt, ids)

    def masks():
        ho.dropout2d_masks(table, ids, offs, args.rate, 0, state['k'])
        state['k'] += 1

    def dropout():
        masks()
        return g_drop(img, mt, ids)
    forms = dict(plain=plain, dropout=dropout, masks_only=masks)
    for _ in range(args.warmup + 1):                       # (the first call of a GraphedScore captures)
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.reps):
        for name, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    res = dict(batch=B, size=S, rate=args.rate, precision=AF.get_precision(), sites=len(sites), table_columns=sites.T, reps=args.reps,
               warmup=args.warmup, timing='forms interleaved; device time between two events around one graph replay (+ the mask launch)')
    for name, v in times.items():
        v = np.asarray(v)
        res[name + '_us'] = round(float(np.median(v)), 1)
        res[name + '_p5_p95_us'] = [round(float(np.percentile(v, 5)), 1), round(float(np.percentile(v, 95)), 1)]
    res['dropout_over_plain'] = round(res['dropout_us'] / res['plain_us'], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
