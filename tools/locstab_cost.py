#!/usr/bin/env python
"""What the localization-stability pool costs.

  launches   hipops.pixel_noise (aod_pixel_noise) on one 16 x 3 x 512 x 512 batch and scoring.loc_stability (aod_loc_stability) on the
             stacked detections of such a batch (K = 6 levels, max_num = 100, every row live).  `--inner` calls of a launch are captured
             into ONE HIP graph and every repetition times one replay of it between two events: the kernels then run back to back on the
             device, without the host's ctypes call and launch dispatch between them, which would dominate a kernel of a few microseconds.
             Per launch the median and the 5th..95th percentile of replay time / inner -- device time per kernel, the graph's own
             node-to-node gap included.
  pool pass  apis.single_gpu_loc_stability against apis.single_gpu_map on the same model (the evidence RetinaNet of bench.py's voc512
             configuration, its head calibrated as bench.py calibrates it) and the same loader (`--images` synthetic 512 x 512 images kept
             in host memory, batches of 16): wall time of a whole pass behind a device sync, the two passes alternating, the first pair
             (captures) dropped.  A stability pass makes K + 1 detection forwards per batch where the evaluation makes one.

    python tools/locstab_cost.py [--batch 16] [--size 512] [--images 64] [--reps 5] [--inner 50] [--warmup 2] [--out FILE.json]
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


def _stats(v, scale=1.0, digits=2):
    v = np.asarray(v) * scale
    return round(float(np.median(v)), digits), [round(float(np.percentile(v, 5)), digits), round(float(np.percentile(v, 95)), digits)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    import bench
    from aod_meh_hua_amd import apis, scoring
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd.apis.test import single_gpu_map
    from aod_meh_hua_amd.datasets import SyntheticVOCDataset, build_dataloader
    from aod_meh_hua_amd.mmcv_lite import MMDataParallel
    dev = torch.device('cuda', 0)
    B, S, K, max_num = args.batch, args.size, len(scoring.LOCSTAB_SIGMAS), 100
    g = torch.Generator(device=dev).manual_seed(512)
    res = dict(batch=B, size=S, levels=K, max_num=max_num, images=args.images, reps=args.reps, inner=args.inner, warmup=args.warmup,
               launch_timing='one replay of a graph of `inner` captured launches between two events, / inner')

    # ------------------------------------------------------------------ the two launches
    src = torch.randn(B, 3, S, S, device=dev, generator=g)
    dst = torch.empty_like(src)
    hw = torch.tensor([[S, S]] * B, dtype=torch.int32, device=dev)
    ids = torch.arange(B, dtype=torch.int64, device=dev)
    inv_std = [1 / 58.395, 1 / 57.12, 1 / 57.375]
    xy = torch.rand(K + 1, B, max_num, 2, device=dev, generator=g) * (S - 64)
    wh = torch.rand(K + 1, B, max_num, 2, device=dev, generator=g) * 56 + 8
    dets = torch.cat([xy, xy + wh, torch.rand(K + 1, B, max_num, 1, device=dev, generator=g) * 0.7 + 0.3001], dim=3).contiguous()
    labels = torch.randint(0, 20, (K + 1, B, max_num), device=dev, generator=g)
    num = torch.full((K + 1, B), max_num, dtype=torch.int32, device=dev)
    launches = dict(pixel_noise=lambda: ho.pixel_noise(src, dst, hw, inv_std, 24.0, 2, 0, ids),
                    loc_stability=lambda: scoring.loc_stability(dets, labels, num))
    graphs = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for f in launches.values():
            f()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for name, f in launches.items():
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(args.inner):
                f()
    for _ in range(args.warmup):
        for gr in graphs.values():
            gr.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in launches}
    for _ in range(max(args.reps, 9)):
        for name, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.inner)
    for name, v in times.items():
        res[name + '_us'], res[name + '_p5_p95_us'] = _stats(v)
    res['pixel_noise_GBps'] = round(2 * src.numel() * 4 / (res['pixel_noise_us'] * 1e-6) / 1e9, 1)          # read + write

    # ------------------------------------------------------------------ the pool pass against the evaluation pass
    class Kept(SyntheticVOCDataset):
        """the synthetic images drawn once and kept: the host's randn per image would dominate both passes alike"""

        def __getitem__(self, i):
            kept = self.__dict__.setdefault('_kept', {})
            if i not in kept:
                kept[i] = super().__getitem__(i)
            d = kept[i]
            return dict(d, img_metas=dict(d['img_metas']))

    cd = dict(bench.CONFIGS['voc512'], batch=B, H=S, W=S)
    model, _ = bench.build_model(dev, cd)
    ds = Kept(num_images=args.images, size=(S, S), test_mode=True)
    loader = build_dataloader(ds, samples_per_gpu=B, workers_per_gpu=0, dist=False, shuffle=False)
    cal = torch.stack([ds[i]['img'] for i in range(min(4, len(ds)))]).to(dev)
    bench.calibrate_head(model, cal)
    model = MMDataParallel(model).eval()

    def stab_pass():
        return apis.single_gpu_loc_stability(model, loader)

    def map_pass():
        return single_gpu_map(model, loader, iou_thr=0.5)

    passes = dict(loc_stability_pass=stab_pass, map_pass=map_pass)
    walls = {k: [] for k in passes}
    for rep in range(args.reps + 1):
        for name, f in passes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            if rep:                                                   # (the first pair captures the detection graph)
                walls[name].append(time.perf_counter() - t0)
            if name == 'loc_stability_pass':
                res['nonzero_scores'] = int((out > 0).sum())
    for name, v in walls.items():
        res[name + '_s'], res[name + '_p5_p95_s'] = _stats(v, digits=4)
    res['pass_ratio'] = round(res['loc_stability_pass_s'] / res['map_pass_s'], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
