#!/usr/bin/env python
"""What one BADGE selection costs in each form: `kernel` (scoring.kmeanspp_seed: aod_kmeanspp_seed, one launch per pick, nothing read
back inside the loop) and `torch` (the same algorithm as a torch-on-device loop written here: per pick one ((X - X[p])^2).sum(1), one
minimum, one fp64 cumsum over the eligible weights and one searchsorted; the pick stays on the device, so this loop has no host round trip
either), on the SAME matrix: N = 16 551 rows (VOC07+12 trainval) x D = 5 120 (20 classes x 256 channels: a VOC gradient embedding), 827
excluded rows, budget 1 000, the same host draws; seeded standard-normal rows.  One process, both forms warmed; every repetition QUEUES a
whole run between two events and the two forms ALTERNATE repetition by repetition so that clock drift hits both alike.  Per form the
median and the 5th..95th percentile spread of --reps whole-run device times.  Also the embedding launch (scoring.badge_embedding) for one
batch of --batch images x --objects objects, whole queued calls between two events.

    python tools/badge_cost.py [--n 16551] [--d 5120] [--excluded 827] [--budget 1000] [--reps 7] [--warmup 2] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_form(X, exc, budget, draws):
    """k-means++ seeding with torch ops on the device (largest-norm first pick, then D^2 sampling by an fp64 cumulative sum); returns
    (picks, weight, total) device tensors"""
    N = X.shape[0]
    elig = torch.ones(N, dtype=torch.bool, device=X.device)
    elig[exc] = False
    picks = torch.empty(budget, dtype=torch.int64, device=X.device)
    weight = torch.empty(budget, device=X.device)
    total = torch.zeros(budget, dtype=torch.float64, device=X.device)
    norms = (X ** 2).sum(1)
    p = torch.argmax(torch.where(elig, norms, torch.full((), -1.0, device=X.device)))
    picks[0], weight[0] = p, norms[p]
    mind = torch.full((N,), float('inf'), device=X.device)
    zero = torch.zeros((), device=X.device)
    for t in range(1, budget):
        elig[p] = False
        mind = torch.minimum(mind, ((X - X[p]) ** 2).sum(1))
        c = torch.where(elig, mind, zero).double().cumsum(0)
        total[t] = c[-1]
        p = torch.searchsorted(c, draws[t] * c[-1], right=True).clamp_(max=N - 1)
        picks[t], weight[t] = p, mind[p]
    return picks, weight, total


def _stats(v):
    v = np.asarray(v)
    return round(float(np.median(v)), 3), [round(float(np.percentile(v, 5)), 3), round(float(np.percentile(v, 95)), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=16551)
    ap.add_argument('--d', type=int, default=5120)
    ap.add_argument('--excluded', type=int, default=827)
    ap.add_argument('--budget', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--objects', type=int, default=32)
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    from aod_meh_hua_amd import scoring
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(5120)
    X = torch.randn(args.n, args.d, device=dev, generator=g)
    exc = torch.randperm(args.n, device=dev, generator=g)[:args.excluded].sort().values
    exc_host = exc.cpu().numpy()
    draws = np.random.default_rng(0).random(args.budget)
    draws_d = torch.from_numpy(draws).to(dev)

    def kernel():
        return scoring.kmeanspp_seed(X, exc_host, args.budget, draws=draws)

    def loop():
        return torch_form(X, exc, args.budget, draws_d)
    kp, kw, kt = kernel()
    tp, _, tt = loop()
    torch.cuda.synchronize()
    same = (kp == tp).long().cumprod(0)                      # a sampled sequence: after the first difference the two runs are different runs
    agree = int(same.sum())
    for _ in range(args.warmup):
        kernel(), loop()
    torch.cuda.synchronize()
    times = dict(kernel=[], torch=[])
    for _ in range(args.reps):                               # alternating: one whole queued run of each form per round
        for name, fn in (('kernel', kernel), ('torch', loop)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    launches = 3 + args.budget
    res = dict(n=args.n, d=args.d, excluded=args.excluded, budget=args.budget, matrix_bytes=args.n * args.d * 4, reps=args.reps,
               warmup=args.warmup, timing='whole queued runs between two events, forms alternating', block=scoring.kmeanspp_block(),
               leading_picks_agreeing_with_torch=agree, total_rel_diff_at_1=abs(float(kt[1]) - float(tt[1])) / float(tt[1]),
               weight_first_last=[float(kw[0]), float(kw[-1])], kernel_launches=launches)
    for name, v in times.items():
        res[name + '_ms'], res[name + '_p5_p95_ms'] = _stats(v)
    res['kernel_us_per_launch'] = round(res['kernel_ms'] * 1e3 / launches, 2)
    res['kernel_sweep_tb_per_s'] = round(args.n * args.d * 4 / (res['kernel_ms'] * 1e-3 / launches) / 1e12, 2)
    res['torch_over_kernel'] = round(res['torch_ms'] / res['kernel_ms'], 2)
    # the embedding launch of one batch
    B, K, Cf, n_cls = args.batch, args.objects, args.channels, args.classes
    feat = torch.nn.functional.normalize(torch.randn(B, K, Cf, device=dev, generator=g), dim=2)
    post = torch.softmax(torch.randn(B, K, n_cls, device=dev, generator=g), dim=2)
    cls = torch.randint(0, n_cls, (B, K), device=dev, generator=g, dtype=torch.int32)
    cnt = torch.full((B,), K, dtype=torch.int32, device=dev)
    out = torch.zeros(B, n_cls * Cf, device=dev)
    for _ in range(5):
        scoring.badge_embedding(feat, post, cls, cnt, n_cls, out=out)
    torch.cuda.synchronize()
    emb = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        scoring.badge_embedding(feat, post, cls, cnt, n_cls, out=out)
        e1.record()
        e1.synchronize()
        emb.append(e0.elapsed_time(e1) * 1e3)
    res['embedding_us'], res['embedding_p5_p95_us'] = _stats(emb)
    res['embedding_shape'] = [B, K, Cf, n_cls]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
