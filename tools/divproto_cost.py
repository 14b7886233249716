#!/usr/bin/env python
"""What the ENMS + DivProto acquisition costs, part by part, on one MI355X, on synthetic pool tensors:

  enms      scoring.enms_prototypes (aod_enms_prototypes) on one batch of --batch images x max_obj objects x C channels, every image full
            (`full`) and with 0..6 objects per image (`sparse`: what a detector leaves above the gate); whole queued runs between two events
  select    scoring.divproto_select (aod_divproto_select): the whole progressive pick -- the upload of the sweep order, the init launch,
            ceil(M / chunk) one-workgroup sweep launches, the fill launch -- between two events, at a VOC-sized pool (16 551 images, 20
            classes, budget 1 000) and a COCO-sized one (118 287 images, 80 classes, budget 2 345).  Every image has 1..6 class prototypes,
            each a noisy copy of one of --groups centres of its class, so that the sweep meets redundant images as a real pool does.
            Reported with the number of sweep launches that did work (the launches behind the one that met the budget exit at once), the
            mean time of one of them, and the stages of the picks.
  pool      apis.single_gpu_enms against apis.single_gpu_object_descriptors (the CCMS pass) on the SAME synthetic pool and detector; whole
            passes on a host clock that ends in a device synchronise, both warmed (their graphs captured), alternating

Per form the median and the 5th..95th percentile spread of --reps runs.

    python tools/divproto_cost.py [--sizes voc,coco] [--max-obj 32] [--channels 256] [--groups 64] [--batch 16] [--pool 96] [--size 320]
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
from tools.ccms_cost import descriptors, stats, timed  # noqa: E402

SIZES = dict(voc=(16551, 20, 1000), coco=(118287, 80, 2345))


def pool_tensors(N, K, C, n_cls, groups, dev, seed):
    """proto [N, K, C], pcls, pconf [N, K], pcnt [N], enms [N]: 1..6 distinct classes per image in ascending order"""
    g = torch.Generator(device=dev).manual_seed(seed)
    cen = torch.randn(n_cls, groups, C, device=dev, generator=g)
    cen = cen / cen.norm(dim=2, keepdim=True)
    most = min(6, K, n_cls)
    pcnt = torch.randint(1, most + 1, (N,), device=dev, generator=g, dtype=torch.int32)
    cls = torch.rand(N, n_cls, device=dev, generator=g).argsort(dim=1)[:, :most].sort(dim=1).values.to(torch.int32)   # distinct, ascending
    if cls.shape[1] < K:
        cls = torch.cat([cls, torch.full((N, K - cls.shape[1]), -1, dtype=torch.int32, device=dev)], 1)
    live = torch.arange(K, device=dev)[None, :] < pcnt[:, None]
    # (the first pcnt of K sorted distinct classes are ascending too)
    grp = torch.randint(0, groups, (N, K), device=dev, generator=g)
    proto = torch.empty(N, K, C, device=dev)
    for i0 in range(0, N, 8192):                              # in pieces: the noise of the COCO-sized pool is 3.9 GB
        sl = slice(i0, min(i0 + 8192, N))
        v = cen[cls[sl].clamp_min(0).long(), grp[sl]] + 0.25 * torch.randn(proto[sl].shape, device=dev, generator=g) / C ** 0.5
        proto[sl] = v / v.norm(dim=2, keepdim=True) * live[sl, :, None]
    pcls = torch.where(live, cls, torch.full_like(cls, -1))
    pconf = (torch.rand(N, K, device=dev, generator=g) * 0.95 + 0.05) * live
    enms = torch.rand(N, device=dev, generator=g) * 4
    return proto.contiguous(), pcls.contiguous(), pconf.contiguous(), pcnt, enms


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
    img = next(iter(loader()))['img']
    while not torch.is_tensor(img):
        img = img[0] if isinstance(img, (list, tuple)) else img.data
    bench.calibrate_head(model, img.to(dev))
    model = MMDataParallel(model).eval()
    forms = dict(enms=lambda: apis.single_gpu_enms(model, loader(), max_obj=args.max_obj, score_thr=0.3),
                 ccms=lambda: apis.single_gpu_object_descriptors(model, loader(), max_obj=args.max_obj, score_thr=0.3))
    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.reps):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    store = forms['enms']()
    res = dict(images=args.pool, size=args.size, batch=args.batch, max_obj=args.max_obj,
               timing='whole passes (host loop, synthetic loader, forward, gather) on a host clock behind a device synchronise, alternating',
               kept_per_image_mean=round(float(store['kept'].float().mean()), 2), classes_per_image_mean=round(float(store['pcnt'].float().mean()), 2))
    for name, v in times.items():
        res[name + '_ms'], res[name + '_p5_p95_ms'] = stats(v)
    res['enms_over_ccms'] = round(res['enms_ms'] / res['ccms_ms'], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='voc,coco')
    ap.add_argument('--max-obj', type=int, default=32)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--groups', type=int, default=64)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--pool', type=int, default=96)
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--skip-pool', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    from aod_meh_hua_amd import scoring
    dev = torch.device('cuda', 0)
    K, C = args.max_obj, args.channels
    res = dict(max_obj=K, channels=C, groups=args.groups, reps=args.reps, warmup=args.warmup, chunk=scoring.divproto_chunk(), enms=[], select=[],
               timing='enms / select: whole queued runs between two events')
    for regime in ('full', 'sparse'):
        feat, cls, w, cnt = descriptors(args.batch, K, C, regime == 'sparse', dev, 77)
        h = torch.rand(args.batch, K, device=dev) * 2
        t = timed(dict(enms=lambda: scoring.enms_prototypes(feat, cls, w, h, cnt)), max(args.reps, 20), args.warmup)
        ms, spread = stats(t['enms'])
        res['enms'].append(dict(batch=args.batch, objects=regime, objects_per_image_mean=round(float(cnt.float().mean()), 2), us=round(ms * 1e3, 1),
                                p5_p95_us=[round(v * 1e3, 1) for v in spread]))
    for name in (s for s in args.sizes.split(',') if s):
        N, n_cls, budget = SIZES[name]
        proto, pcls, pconf, pcnt, enms = pool_tensors(N, K, C, n_cls, args.groups, dev, 1000 + N)
        order = scoring.divproto_order(enms, np.arange(0, N, 10))          # a tenth of the pool is labelled
        M = len(order)
        run = lambda: scoring.divproto_select(order, proto, pcls, pconf, pcnt, n_cls, budget)
        picks, stage = run()
        torch.cuda.synchronize()
        pos = {int(i): p for p, i in enumerate(order)}
        swept = [pos[int(i)] for i, s in zip(picks.tolist(), stage.tolist()) if s != 3]
        filled = int((stage == 3).sum())
        active = -(-M // res['chunk']) if filled else -(-(max(swept) + 1) // res['chunk'])
        t = timed(dict(select=run), args.reps, args.warmup)
        ms, spread = stats(t['select'])
        res['select'].append(dict(pool=name, images=N, candidates=M, classes=n_cls, budget=budget, store_mb=round(proto.numel() * 4 / 2 ** 20),
                                  launches=2 + -(-M // res['chunk']), sweep_launches_with_work=active, ms=ms, p5_p95_ms=spread,
                                  ms_per_working_launch_mean=round(ms / active, 3), us_per_swept_candidate=round(ms * 1e3 / min(active * res['chunk'], M), 2),
                                  stages=[int((stage == s).sum()) for s in (1, 2, 3)]))
        del proto, pcls, pconf, pcnt, enms
        torch.cuda.empty_cache()
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
