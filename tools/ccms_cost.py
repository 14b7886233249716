#!/usr/bin/env python
"""What the CCMS acquisition costs, part by part, on one MI355X:

  pool      apis.single_gpu_object_descriptors (detections, the posterior score and the object descriptors of every image) against
            apis.Posterior_uncertainty('entropy', 'sum') -- the `Entropy` pool pass -- on the SAME synthetic pool and detector; whole
            passes on a host clock that ends in a device synchronise, both warmed (their graphs captured), alternating
  distance  scoring.ccms_distance (aod_ccms_distance) against a straightforward torch formulation of the same matrix written here (per
            block of a-images one einsum over the channels, a class mask, two amax, two weighted means), on the SAME seeded descriptors:
            M images x max_obj objects x C channels, once with every image full (`full`: max_obj objects each, what the torch form
            computes anyway) and once with 0..6 objects per image (`sparse`: what a detector leaves above the gate); whole queued runs
            between two events, forms alternating
  kcenter   scoring.kcenter_greedy_matrix: all `budget` picks on the [M, M] matrix, one queued run between two events

Per form the median and the 5th..95th percentile spread of --reps runs.

    python tools/ccms_cost.py [--m 1000,4000] [--max-obj 32] [--channels 256] [--budget 1000] [--pool 96] [--size 320] [--batch 8]
                              [--reps 5] [--warmup 2] [--skip-pool] [--out FILE.json]
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


def torch_form(feat, cls, w, cnt, block=16):
    """the [M, M] CCMS distance with torch ops on the device, `block` a-images at a time (the [block, M, K, K] product is the intermediate)"""
    M, K, _ = feat.shape
    live = torch.arange(K, device=feat.device)[None, :] < cnt[:, None]
    wl = torch.where(live, w, torch.zeros_like(w))
    den = wl.sum(1)
    out = torch.empty(M, M, device=feat.device)
    for a0 in range(0, M, block):
        a1 = min(a0 + block, M)
        P = torch.einsum('aic,bjc->abij', feat[a0:a1], feat)
        mask = (cls[a0:a1, None, :, None] == cls[None, :, None, :]) & live[a0:a1, None, :, None] & live[None, :, None, :]
        P = torch.where(mask, P.clamp_min(0), torch.zeros((), device=feat.device))
        sab = (wl[a0:a1, None, :] * P.amax(3)).sum(2) / den[a0:a1, None]
        sba = (wl[None, :, :] * P.amax(2)).sum(2) / den[None, :]
        s = torch.nan_to_num(sab, nan=0.0) + torch.nan_to_num(sba, nan=0.0)
        out[a0:a1] = (1.0 - s * 0.5).clamp_min(0)
    out.fill_diagonal_(0.0)
    return out


def descriptors(M, K, C, sparse, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    feat = torch.randn(M, K, C, device=dev, generator=g)
    feat = feat + 0.5 * torch.randn(1, 1, C, device=dev, generator=g)          # a shared component: the matched cosines are not all ~ 0
    feat = feat / feat.norm(dim=2, keepdim=True)
    cls = torch.randint(0, 20, (M, K), device=dev, generator=g, dtype=torch.int32)
    w = torch.rand(M, K, device=dev, generator=g) * 0.69 + 0.31
    cnt = (torch.randint(0, 7, (M,), device=dev, generator=g, dtype=torch.int32).clamp_max(K) if sparse
           else torch.full((M,), K, dtype=torch.int32, device=dev))
    live = torch.arange(K, device=dev)[None, :] < cnt[:, None]
    return (feat * live[..., None]).contiguous(), torch.where(live, cls, torch.full_like(cls, -1)), (w * live).contiguous(), cnt


def timed(fns, reps, warmup):
    """fns: name -> callable that queues one whole run; alternating rounds between two events -> name -> list of ms"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return times


def stats(v):
    v = np.asarray(v)
    return round(float(np.median(v)), 3), [round(float(np.percentile(v, 5)), 3), round(float(np.percentile(v, 95)), 3)]


def pool_pass(args, dev):
    import bench
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.datasets import build_dataloader, build_dataset
    from aod_meh_hua_amd.mmcv_lite import Config, MMDataParallel
    from aod_meh_hua_amd.models import build_detector
    from oracle import model as om
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg.model.backbone.pop('init_cfg', None)
    model = build_detector(cfg.model)
    model.load_state_dict(om.seeded_state_dict(cls_bias=-2.0), strict=True)
    model = model.to(dev).eval()
    ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=args.pool, size=(args.size, args.size)), dict(test_mode=True))
    loader = lambda: build_dataloader(ds, samples_per_gpu=args.batch, workers_per_gpu=0, dist=False, shuffle=False)
    first = next(iter(loader()))
    img = first['img']
    while not torch.is_tensor(img):
        img = img[0] if isinstance(img, (list, tuple)) else img.data
    bench.calibrate_head(model, img.to(dev))
    model = MMDataParallel(model).eval()
    forms = dict(ccms=lambda: apis.single_gpu_object_descriptors(model, loader(), max_obj=args.max_obj, score_thr=0.3),
                 entropy=lambda: apis.Posterior_uncertainty(cfg, model, loader(), measure='entropy', aggregate='sum', score_thr=0.3))
    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.reps):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    store = forms['ccms']()
    res = dict(images=args.pool, size=args.size, batch=args.batch, max_obj=args.max_obj,
               timing='whole passes (host loop, synthetic loader, forward, gather) on a host clock behind a device synchronise, alternating',
               objects_per_image_mean=round(float(store['cnt'].float().mean()), 2), missing=int(store['missing'].sum()))
    for name, v in times.items():
        res[name + '_ms'], res[name + '_p5_p95_ms'] = stats(v)
    res['ccms_over_entropy'] = round(res['ccms_ms'] / res['entropy_ms'], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--m', default='1000,4000')
    ap.add_argument('--max-obj', type=int, default=32)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--budget', type=int, default=1000)
    ap.add_argument('--pool', type=int, default=96)
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--skip-pool', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    from aod_meh_hua_amd import scoring
    dev = torch.device('cuda', 0)
    K, C = args.max_obj, args.channels
    res = dict(max_obj=K, channels=C, reps=args.reps, warmup=args.warmup, distance=[], kcenter=[],
               timing='distance / kcenter: whole queued runs between two events, forms alternating')
    for M in (int(v) for v in args.m.split(',')):
        for regime in ('full', 'sparse'):
            d = descriptors(M, K, C, regime == 'sparse', dev, 1000 + M)
            kd, td = scoring.ccms_distance(*d), torch_form(*d)
            torch.cuda.synchronize()
            row = dict(m=M, objects=regime, objects_per_image_mean=round(float(d[3].float().mean()), 2),
                       max_abs_kernel_minus_torch=float((kd - td).abs().max()), symmetric=bool(torch.equal(kd, kd.t())),
                       fma_full_tiles=M * M // 2 * ((K + 31) // 32 * 32) ** 2 * C)
            t = timed(dict(kernel=lambda: scoring.ccms_distance(*d), torch=lambda: torch_form(*d)), args.reps, args.warmup)
            for name, v in t.items():
                row[name + '_ms'], row[name + '_p5_p95_ms'] = stats(v)
            row['torch_over_kernel'] = round(row['torch_ms'] / row['kernel_ms'], 2)
            if regime == 'full':
                row['kernel_tflops_full_tiles'] = round(2 * row['fma_full_tiles'] / (row['kernel_ms'] * 1e-3) / 1e12, 1)
            res['distance'].append(row)
            if regime == 'sparse':
                budget = min(args.budget, M // 4)
                t = timed(dict(kcenter=lambda: scoring.kcenter_greedy_matrix(kd, [], budget)), args.reps, args.warmup)
                ms, spread = stats(t['kcenter'])
                res['kcenter'].append(dict(m=M, budget=budget, launches=2 + budget, ms=ms, p5_p95_ms=spread, us_per_pick=round(ms * 1e3 / budget, 2)))
            del d, kd, td
    if not args.skip_pool:
        res['pool'] = pool_pass(args, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
