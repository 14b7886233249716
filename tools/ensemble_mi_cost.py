#!/usr/bin/env python
"""What the ensemble mutual-information score costs per scoring batch in each form: `kernel` (scoring.ensemble_mi: aod_ensemble_mi, two
launches) and `torch` (the baseline as the reference writes it -- a Python loop over levels x images of fp32 torch ops, ending in
.tolist()), on the SAME device maps: K members' classification maps of the bench scoring batch (16 x 512^2, five pyramid levels, 9 x 20
columns; seeded logits ~ N(-4.6, 2^2), channels_last as the head writes them).  One process, both forms warmed, INTERLEAVED repetition by
repetition so that clock drift hits both alike; per form the median and the 5th..95th percentile spread of --reps repetitions: wall time
of the call up to a device synchronise (the torch form ends in a host sync by itself; it is launch-bound, so its wall time IS its cost)
and, for the kernel, the device time between two events as well.

    python tools/ensemble_mi_cost.py [--members 3] [--reps 50] [--warmup 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_form(members, n_cls):
    """per (level, image): sigmoid -> [rows, n_cls] -> total - aleatoric entropy -> mean; .tolist() at the end"""
    L, B = len(members[0]), members[0][0].shape[0]
    buf = torch.zeros(B, L)
    for l in range(L):
        for b in range(B):
            p = torch.stack([torch.sigmoid(m[l][b]).permute(1, 2, 0).reshape(-1, n_cls) for m in members])
            avg = p.mean(0)
            buf[b, l] = (-(avg * avg.log()).sum(1) + (p * p.log()).sum(2).mean(0)).mean()
    return buf.mean(1).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=3)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    from aod_meh_hua_amd import scoring
    dev = torch.device('cuda', 0)
    n_cls, A = 20, 9
    g = torch.Generator(device=dev).manual_seed(1020)
    sizes = [-(-args.size // s) for s in (8, 16, 32, 64, 128)]
    members = [[(torch.randn(args.batch, A * n_cls, h, h, device=dev, generator=g) * 2 - 4.6).contiguous(memory_format=torch.channels_last)
                for h in sizes] for _ in range(args.members)]
    nbytes = sum(t.numel() * 4 for m in members for t in m)

    def kernel():
        return scoring.ensemble_mi(members, n_cls)
    k = kernel().cpu().numpy()
    t = np.asarray(torch_form(members, n_cls))
    for _ in range(args.warmup):
        kernel(), torch_form(members, n_cls)
    torch.cuda.synchronize()
    times = dict(kernel_wall=[], kernel_device=[], torch_wall=[])
    for _ in range(args.reps):                           # interleaved: one repetition of each form per round
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        kernel()
        e1.record()
        torch.cuda.synchronize()
        times['kernel_wall'].append((time.perf_counter() - t0) * 1e6)
        times['kernel_device'].append(e0.elapsed_time(e1) * 1e3)
        t0 = time.perf_counter()
        torch_form(members, n_cls)
        torch.cuda.synchronize()
        times['torch_wall'].append((time.perf_counter() - t0) * 1e6)
    res = dict(members=args.members, batch=args.batch, size=args.size, levels=sizes, map_bytes=nbytes, reps=args.reps, warmup=args.warmup,
               timing='forms interleaved; wall = call + device synchronise, device = events around the two launches',
               max_abs_diff_kernel_vs_torch=float(np.abs(k - t).max()), score_mean=float(k.mean()))
    for name, v in times.items():
        v = np.asarray(v)
        res[name + '_us'] = round(float(np.median(v)), 2)
        res[name + '_p5_p95_us'] = [round(float(np.percentile(v, 5)), 2), round(float(np.percentile(v, 95)), 2)]
    res['kernel_device_gb_per_s'] = round(nbytes / (res['kernel_device_us'] * 1e-6) / 1e9, 1)
    res['torch_wall_over_kernel_wall'] = round(res['torch_wall_us'] / res['kernel_wall_us'], 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
