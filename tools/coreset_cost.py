#!/usr/bin/env python
"""What one Core-set selection costs in each form: `kernel` (scoring.kcenter_greedy: aod_kcenter_greedy, one launch per pick, nothing
read back inside the loop) and `torch` (the same algorithm as a torch-on-device loop written here: per center one ((X - X[p])^2).sum(1),
one minimum and -- per pick -- one argmax; the pick stays on the device, so this loop has no host round trip either), on the SAME
descriptor matrix: N = 16 551 rows (VOC07+12 trainval) x D = 1 280 (five pyramid levels x 256), 827 labelled rows, budget 1 000; seeded
standard-normal descriptors.  One process, both forms warmed; every repetition QUEUES a whole run between two events and the two forms
ALTERNATE repetition by repetition so that clock drift hits both alike (a run is ~1 800 dependent sub-40-us launches: timing single
launches would measure the timer).  Per form the median and the 5th..95th percentile spread of --reps whole-run device times.

    python tools/coreset_cost.py [--n 16551] [--d 1280] [--labelled 827] [--budget 1000] [--reps 7] [--warmup 2] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_form(X, lab, budget):
    """k-center greedy with torch ops on the device; returns (picks, radius) device tensors"""
    N = X.shape[0]
    mind = torch.full((N,), float('inf'), device=X.device)
    sel = torch.zeros(N, dtype=torch.bool, device=X.device)
    sel[lab] = True
    for j in range(lab.numel()):
        mind = torch.minimum(mind, ((X - X[lab[j]]) ** 2).sum(1))
    picks = torch.empty(budget, dtype=torch.int64, device=X.device)
    radius = torch.empty(budget, device=X.device)
    neg = torch.full((), -1.0, device=X.device)
    for t in range(budget):
        p = torch.argmax(torch.where(sel, neg, mind))
        picks[t], radius[t] = p, mind[p]
        sel[p] = True
        mind = torch.minimum(mind, ((X - X[p]) ** 2).sum(1))
    return picks, radius


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=16551)
    ap.add_argument('--d', type=int, default=1280)
    ap.add_argument('--labelled', type=int, default=827)
    ap.add_argument('--budget', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    from aod_meh_hua_amd import scoring
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(1280)
    X = torch.randn(args.n, args.d, device=dev, generator=g)
    lab = torch.randperm(args.n, device=dev, generator=g)[:args.labelled].sort().values
    lab_host = lab.cpu().numpy()

    def kernel():
        return scoring.kcenter_greedy(X, lab_host, args.budget)
    kp, kr = kernel()
    tp, tr = torch_form(X, lab, args.budget)
    torch.cuda.synchronize()
    agree = int((kp == tp).sum())
    for _ in range(args.warmup):
        kernel(), torch_form(X, lab, args.budget)
    torch.cuda.synchronize()
    times = dict(kernel=[], torch=[])
    for _ in range(args.reps):                           # alternating: one whole queued run of each form per round
        for name, fn in (('kernel', kernel), ('torch', lambda: torch_form(X, lab, args.budget))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    launches = 3 + -(-args.labelled // scoring.kcenter_chunk()) + args.budget
    res = dict(n=args.n, d=args.d, labelled=args.labelled, budget=args.budget, matrix_bytes=args.n * args.d * 4, reps=args.reps,
               warmup=args.warmup, timing='whole queued runs between two events, forms alternating',
               picks_agreeing_with_torch=agree, radius_first_last=[float(kr[0]), float(kr[-1])], kernel_launches=launches)
    for name, v in times.items():
        v = np.asarray(v)
        res[name + '_ms'] = round(float(np.median(v)), 3)
        res[name + '_p5_p95_ms'] = [round(float(np.percentile(v, 5)), 3), round(float(np.percentile(v, 95)), 3)]
    res['kernel_us_per_launch'] = round(res['kernel_ms'] * 1e3 / launches, 2)
    res['torch_over_kernel'] = round(res['torch_ms'] / res['kernel_ms'], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
