#!/usr/bin/env python
"""What the plain RetinaNet baseline costs next to the MEH detector: ms per training iteration of MyRetinaNet (one optimizer: train_step ->
backward -> step) beside SSL_L_RetinaNet (main + MEH step) at 16 x 512^2, eager and replayed from the captured graph, in both precision
modes; and the fused loss launches (all levels, forward and backward) of the sigmoid form beside the EDL form on the same rows.  Device
events around --reps iterations after --warmup, medians.  The plain iteration launches a strict subset of the MEH iteration's convs.

    python tools/plain_retina_cost.py [--batch 16] [--size 512] [--reps 30] [--warmup 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _batch(B, size, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, size, size, generator=g).cuda()
    boxes, labels = [], []
    for _ in range(B):
        n = int(torch.randint(1, 6, (1,), generator=g))
        wh = torch.rand(n, 2, generator=g) * size * 0.6 + size / 16.0
        xy = torch.rand(n, 2, generator=g) * (size - wh)
        boxes.append(torch.cat([xy, xy + wh], 1))
        labels.append(torch.randint(0, 20, (n,), generator=g))
    metas = [dict(img_shape=(size, size, 3), pad_shape=(size, size, 3), ori_shape=(size, size, 3), scale_factor=np.ones(4, np.float32), flip=False) for _ in range(B)]
    return dict(img=img, img_metas=metas, gt_bboxes=boxes, gt_labels=labels)


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return round(statistics.median(times), 3)


def _iteration_ms(config, batches, reps, warmup):
    from aod_meh_hua_amd.apis.train_Lambda import build_optimizers
    from aod_meh_hua_amd.graphs import GraphedTrainStep
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, config))
    cfg.model.backbone.pop('init_cfg')
    model = build_detector(cfg.model)
    model.init_weights()
    model = model.cuda().train()
    opt, opt_L = build_optimizers(model, cfg)
    state = dict(i=0)

    def eager():
        d = batches[state['i'] % len(batches)]
        state['i'] += 1
        out, head_out, feat_out, prev = model.train_step(d, Labeled=True, Pseudo=False)
        opt.zero_grad()
        out['loss'].backward()
        if opt_L is not None:
            loss_L = model.train_step_L(prev, head_out, feat_out)
            opt_L.zero_grad()
            loss_L['loss'].backward()
        opt.step()
        if opt_L is not None:
            opt_L.step()
    gs = GraphedTrainStep(model, opt, opt_L, warmup=2, Labeled=True, Pseudo=False)

    def replayed():
        d = batches[state['i'] % len(batches)]
        state['i'] += 1
        gs(d)
    res = dict(eager_ms=_median_ms(eager, reps, warmup), replayed_ms=_median_ms(replayed, reps, warmup))
    del gs, model, opt, opt_L
    torch.cuda.empty_cache()
    return res


def _loss_us(B, size, reps, warmup):
    """the level-fused loss launches alone on the rows of a B x size^2 batch (C = 20, 9 anchors), forward + backward, both forms"""
    from aod_meh_hua_amd import hipops as ho
    g = torch.Generator().manual_seed(7)
    level_rows = [B * 9 * max(size // s, 1) ** 2 for s in (8, 16, 32, 64, 128)]
    rows, L = sum(level_rows), 5
    x = (torch.randn(rows, 20, generator=g) * 2 - 3).cuda()
    lab = torch.randint(0, 21, (rows,), generator=g)
    lab[torch.rand(rows, generator=g) < 0.99] = 20
    lab = lab.cuda()
    lw = torch.ones(rows, device='cuda')
    bp, bt = torch.randn(rows, 4, generator=g).cuda(), torch.randn(rows, 4, generator=g).cuda()
    bw = (lab < 20).float()[:, None].expand(rows, 4).contiguous()
    num_pos = torch.full((B,), 40, dtype=torch.int32, device='cuda')
    g_sums = torch.ones(3, L, device='cuda')
    gc, gb = torch.empty(rows // 9, 180, device='cuda'), torch.empty(rows // 9, 36, device='cuda')
    out = dict(rows=rows)
    for form in ('edl', 'sigmoid'):
        div = ho.edl_focal_l1_levels_fwd(x, lab, lw, bp, bt, bw, level_rows, num_pos=num_pos, form=form)[2]
        fwd = lambda: ho.edl_focal_l1_levels_fwd(x, lab, lw, bp, bt, bw, level_rows, num_pos=num_pos, form=form)
        bwd = lambda: ho.edl_focal_l1_levels_bwd(x, lab, lw, bp, bt, bw, level_rows, g_sums, None, gc, gb, 9, divisors=div, form=form)
        out[form + '_fwd_us'] = round(_median_ms(fwd, reps * 4, warmup) * 1e3, 1)
        out[form + '_bwd_us'] = round(_median_ms(bwd, reps * 4, warmup) * 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    from aod_meh_hua_amd import functional as AF
    batches = [_batch(args.batch, args.size, 100 + i) for i in range(2)]
    res = dict(device=torch.cuda.get_device_name(0), batch=args.batch, size=args.size, reps=args.reps, warmup=args.warmup)
    for prec in ('bf16x3', 'bf16'):
        AF.set_precision(prec)
        res[prec] = dict(MyRetinaNet=_iteration_ms('configs/_base_/Config_RetinaNet_plain.py', batches, args.reps, args.warmup),
                         SSL_L_RetinaNet=_iteration_ms('configs/_base_/Config_RetinaNet.py', batches, args.reps, args.warmup))
    res['loss_launches'] = _loss_us(args.batch, args.size, args.reps, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
