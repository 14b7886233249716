#!/usr/bin/env python
"""What one CDAL descriptor launch pair (scoring.cdal_descriptor: aod_cdal_descriptor) costs on the classification maps of one batch:
16 images at 512 x 512 -- five levels of 64^2, 32^2, 16^2, 8^2, 4^2 positions x 9 anchors x 20 classes, fp32, the levels adjacent row
ranges of one buffer as the head hands them out.  The kernel is a streaming read of the maps; the second pass of a chunk walks the rows
that passed the threshold, so the time depends on how many there are: `dense` logits 3 N(0, 1) (almost nine rows in ten are regions, far
more than a trained detector yields) and `sparse` logits N(0, 1) - 2 on all classes but a few (a few rows in a hundred).  One process,
both inputs warmed; every repetition QUEUES `--inner` calls between two events (a single call is a few tens of microseconds: timing one
would measure the timer) and the two inputs alternate.  Per input the median and the 5th..95th percentile of the per-call device time.

    python tools/cdal_cost.py [--batch 16] [--size 512] [--classes 20] [--reps 9] [--inner 50] [--warmup 2] [--out FILE.json]
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
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    from aod_meh_hua_amd import scoring
    dev = torch.device('cuda', 0)
    B, C, A = args.batch, args.classes, 9
    hw = [(args.size // s) for s in (8, 16, 32, 64, 128)]
    rows = [h * h * A for h in hw]
    g = torch.Generator(device=dev).manual_seed(512)

    def maps_of(fill):
        buf = torch.empty(B * sum(rows) * C, device=dev)
        fill(buf.view(-1, C))
        out, o = [], 0
        for h, r in zip(hw, rows):
            out.append(buf[o:o + B * r * C].view(B, h, h, A * C).permute(0, 3, 1, 2))
            o += B * r * C
        return out

    def dense(x):
        x.normal_(generator=g).mul_(3.0)

    def sparse(x):
        x.normal_(generator=g).sub_(2.0)
        hot = torch.rand(x.shape[0], device=dev, generator=g) < 0.03
        x[hot, 0] += 6.0
    inputs = dict(dense=maps_of(dense), sparse=maps_of(sparse))
    out = torch.empty(B, 2 * C * C, device=dev)
    res = dict(batch=B, size=args.size, classes=C, rows_per_image=sum(rows), map_bytes=B * sum(rows) * C * 4, out_bytes=B * 2 * C * C * 4,
               partial_bytes=int(scoring._C.lib.aod_cdal_ws_len(len(rows), (scoring.C.c_int64 * len(rows))(*rows), C, B)) * 4,
               reps=args.reps, inner=args.inner, warmup=args.warmup, timing='inner queued calls between two events, inputs alternating')
    for name, maps in inputs.items():
        d = scoring.cdal_descriptor(maps, C, 0.3, out=out)
        P = d[:, :C * C].view(B, C, C)
        assert bool(torch.isfinite(d).all()) and float((P.sum(dim=2) - 1).abs().max()) < 1e-4
        pm = torch.cat([torch.softmax(scoring.nhwc_view(m, C), dim=2).amax(dim=2) for m in maps], dim=1)
        res[name + '_region_share'] = round(float((pm > 0.3).float().mean()), 4)
    for _ in range(args.warmup):
        for maps in inputs.values():
            for _ in range(args.inner):
                scoring.cdal_descriptor(maps, C, 0.3, out=out)
    torch.cuda.synchronize()
    times = {k: [] for k in inputs}
    for _ in range(args.reps):
        for name, maps in inputs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                scoring.cdal_descriptor(maps, C, 0.3, out=out)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.inner)
    for name, v in times.items():
        v = np.asarray(v)
        res[name + '_us'] = round(float(np.median(v)), 2)
        res[name + '_p5_p95_us'] = [round(float(np.percentile(v, 5)), 2), round(float(np.percentile(v, 95)), 2)]
        res[name + '_read_GBps'] = round(res['map_bytes'] / (res[name + '_us'] * 1e-6) / 1e9, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
