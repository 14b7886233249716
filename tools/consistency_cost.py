#!/usr/bin/env python
"""What the consistency pool costs, in ms per batch.

  launches   hipops.flip_images (aod_flip_images) on one 16 x 3 x 512 x 512 batch; scoring.det_posterior (the candidate-row lookup of
             aod_det_uncertainty_ex under score_thr = -inf plus the aod_det_posterior gather) on `--cand` candidate rows of 21 columns and
             max_num = 100 detections per image, every row live; scoring.det_consistency (aod_det_consistency) on the stacked outputs of
             such a batch (V = 1 and V = 3, every clean row an object).  `--inner` calls of a launch are captured into ONE HIP graph and
             every repetition times one replay of it between two events: the kernels then run back to back on the device, without the
             host's ctypes call and launch dispatch between them.  Per launch the median and the 5th..95th percentile of replay time /
             inner.
  forward    one replay of the captured detection graph of the pool pass (isEval=True, _padded=True, detPost=True) and of
             single_gpu_map's (without detPost) on the evidence RetinaNet of bench.py's voc512 configuration, its head calibrated as
             bench.py calibrates it, between two events.
  pool pass  apis.single_gpu_consistency (views=('hflip',): V + 1 = 2 forwards per batch) against apis.single_gpu_map on the same model
             and loader (`--images` synthetic 512 x 512 images kept in host memory, batches of 16): wall time of a whole pass behind a
             device sync, the two passes alternating, the first pair (captures) dropped.

    python tools/consistency_cost.py [--batch 16] [--size 512] [--images 64] [--cand 4000] [--reps 5] [--inner 50] [--warmup 2] [--out FILE.json]
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


def _stats(v, scale=1.0, digits=4):
    v = np.asarray(v) * scale
    return round(float(np.median(v)), digits), [round(float(np.percentile(v, 5)), digits), round(float(np.percentile(v, 95)), digits)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--cand', type=int, default=4000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    import bench
    from aod_meh_hua_amd import apis, scoring
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd.apis import test as apis_test
    from aod_meh_hua_amd.datasets import SyntheticVOCDataset, build_dataloader
    from aod_meh_hua_amd.mmcv_lite import MMDataParallel
    dev = torch.device('cuda', 0)
    B, S, n, W, max_num = args.batch, args.size, args.cand, 21, 100
    g = torch.Generator(device=dev).manual_seed(512)
    res = dict(batch=B, size=S, cand=n, W=W, max_num=max_num, images=args.images, reps=args.reps, inner=args.inner, warmup=args.warmup,
               launch_timing='one replay of a graph of `inner` captured launches between two events, / inner; ms')

    # ------------------------------------------------------------------ the launches
    src = torch.randn(B, 3, S, S, device=dev, generator=g)
    dst = torch.empty_like(src)
    hw = torch.tensor([[S, S]] * B, dtype=torch.int32, device=dev)
    xy = torch.rand(B, n, 2, device=dev, generator=g) * (S - 64)
    wh = torch.rand(B, n, 2, device=dev, generator=g) * 56 + 8
    boxes = torch.cat([xy, xy + wh], dim=2).contiguous()
    scores = torch.rand(B, n, W, device=dev, generator=g) * 0.7 + 0.3001
    cand = scoring.Candidates(boxes, scores, None, None, None, None, None)
    rows = torch.stack([torch.randperm(n, device=dev, generator=g)[:max_num] for _ in range(B)])
    labels = torch.randint(0, 20, (B, max_num), device=dev, generator=g)
    dets = torch.cat([boxes.gather(1, rows[..., None].expand(-1, -1, 4)),
                      scores.gather(1, rows[..., None].expand(-1, -1, W)).gather(2, labels[..., None])], dim=2).contiguous()
    num = torch.full((B,), max_num, dtype=torch.int32, device=dev)
    post, missing = scoring.det_posterior(cand, dets, labels, num)
    assert int(missing.sum()) == 0
    ext = torch.tensor([[S, S]] * B, dtype=torch.float32, device=dev)

    def stacked(V):
        jit = (torch.rand(V + 1, B, max_num, 4, device=dev, generator=g) - 0.5) * 6
        jit[0] = 0
        d = dets[None].repeat(V + 1, 1, 1, 1)
        d[..., :4] += jit
        for v in range(V):                                  # the views' boxes lie in their own mirrored frames
            code = v + 1
            x1, y1, x2, y2 = d[v + 1, ..., 0].clone(), d[v + 1, ..., 1].clone(), d[v + 1, ..., 2].clone(), d[v + 1, ..., 3].clone()
            if code & 1:
                d[v + 1, ..., 0], d[v + 1, ..., 2] = S - x2, S - x1
            if code & 2:
                d[v + 1, ..., 1], d[v + 1, ..., 3] = S - y2, S - y1
        p = post[None].repeat(V + 1, 1, 1, 1)
        p[1:] = (p[1:] + torch.rand(V, B, max_num, W, device=dev, generator=g) * 0.2).clamp_(0, 1)
        return (d.contiguous(), labels[None].repeat(V + 1, 1, 1).contiguous(), num[None].repeat(V + 1, 1).contiguous(), p.contiguous())

    st1, st3 = stacked(1), stacked(3)
    launches = dict(flip_images=lambda: ho.flip_images(src, dst, hw, 'hflip'),
                    det_posterior=lambda: scoring.det_posterior(cand, dets, labels, num),
                    det_consistency_v1=lambda: scoring.det_consistency(*st1, ('hflip',), ext, 'cat'),
                    det_consistency_v3=lambda: scoring.det_consistency(*st3, ('hflip', 'vflip', 'hvflip'), ext, 'cat'))
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
            times[name].append(e0.elapsed_time(e1) / args.inner)
    for name, v in times.items():
        res[name + '_ms'], res[name + '_p5_p95_ms'] = _stats(v)
    res['flip_images_GBps'] = round(2 * src.numel() * 4 / (res['flip_images_ms'] * 1e-3) / 1e9, 1)          # read + write
    res['matched_rows_v1'] = int((scoring.det_consistency(*st1, ('hflip',), ext, 'cat', want_parts=True)[3] >= 0).sum())

    # ------------------------------------------------------------------ the forward and the pool pass
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

    passes = dict(consistency_pass=lambda: apis.single_gpu_consistency(model, loader),
                  map_pass=lambda: apis_test.single_gpu_map(model, loader, iou_thr=0.5))
    walls = {k: [] for k in passes}
    for rep in range(args.reps + 1):
        for name, f in passes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            if rep:                                                   # (the first pair captures the detection graphs)
                walls[name].append(time.perf_counter() - t0)
            if name == 'consistency_pass':
                res['nonzero_scores'] = int((out > 0).sum())
    for name, v in walls.items():
        res[name + '_s'], res[name + '_p5_p95_s'] = _stats(v)
    res['pass_ratio'] = round(res['consistency_pass_s'] / res['map_pass_s'], 2)
    res['batches_per_pass'] = -(-args.images // B)
    res['consistency_pass_ms_per_batch'] = round(1e3 * res['consistency_pass_s'] / res['batches_per_pass'], 3)

    # one replay of each captured detection graph (the passes above captured them for this batch shape)
    img = torch.stack([ds[i]['img'] for i in range(B)]).to(dev)
    metas = [dict(ds[i]['img_metas']) for i in range(B)]
    ids = torch.arange(B, dtype=torch.int64, device=dev)
    for name, prefix, ctor in (('forward_post', ('eval_post',), dict(isEval=True, _padded=True, detPost=True)),
                               ('forward_plain', ('eval_padded',), dict(isEval=True, _padded=True))):
        gs = apis_test._graphed(model, dev, prefix, dict(isUnc=False), **ctor)
        v = []
        for rep in range(args.warmup + max(args.reps, 9)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gs(img, metas, ids)
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                v.append(e0.elapsed_time(e1))
        res[name + '_ms'], res[name + '_p5_p95_ms'] = _stats(v)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
