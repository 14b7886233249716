#!/usr/bin/env python
"""What gradient-norm clipping costs per training step: the norm launches (grad_sqsum_multi_kernel per <= 48 tensors +
grad_clip_finalize_kernel) beside the sgd_multi launches, over the two parameter sets of the real RetinaNet-R50 + MEH model (main and MEH
optimizer, ~38.9 M parameters), timed with device events around captured-graph replays (no host launch path in the window), median of
--reps repetitions after --warmup.  The norm pass reads 4 B per parameter, the SGD launches move 20.

    python tools/grad_clip_cost.py [--reps 100] [--warmup 20] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_us(graph, reps, warmup):
    for _ in range(warmup):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times), min(times), max(times)


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert args.reps >= 50, 'at least 50 timed repetitions'
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    from aod_meh_hua_amd.apis.train_Lambda import build_optimizers
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg.model.backbone.pop('init_cfg')
    model = build_detector(cfg.model).cuda().train()
    cfg.optimizer_config = dict(grad_clip=dict(max_norm=35, norm_type=2))
    clipped = build_optimizers(model, cfg)
    cfg.optimizer_config = dict(grad_clip=None)
    plain = build_optimizers(model, cfg)
    gen = torch.Generator(device='cuda').manual_seed(0)
    nparam = 0
    for opt in clipped:
        for p in opt.param_groups[0]['params']:
            p.grad = torch.randn(p.shape, device='cuda', generator=gen) * 1e-3
            nparam += p.numel()
    for opt in clipped + plain:
        opt.param_groups[0]['lr'] = 0.0          # (the timed steps move nothing)
        opt.device_lr()
        opt.step()                               # momentum buffers exist: the steady-state launches

    def norm_only():
        for opt in clipped:
            ps = [p for p in opt.param_groups[0]['params'] if p.grad is not None]
            opt._grad_norm([p.grad.data_ptr() for p in ps], [p.numel() for p in ps], ps[0].device)

    def sgd_only():
        for opt in plain:
            opt.step()

    def clipped_step():
        for opt in clipped:
            opt.step()
    res = dict(parameters=nparam, tensors=[len(o.param_groups[0]['params']) for o in clipped], reps=args.reps, warmup=args.warmup)
    for name, fn in (('norm_us', norm_only), ('sgd_us', sgd_only), ('clipped_step_us', clipped_step)):
        med, lo, hi = _median_us(_capture(fn), args.reps, args.warmup)
        res[name] = round(med, 2)
        res[name + '_min_max'] = [round(lo, 2), round(hi, 2)]
    res['norm_over_sgd'] = round(res['norm_us'] / res['sgd_us'], 3)
    res['norm_GBps'] = round(nparam * 4 / res['norm_us'] / 1e3, 1)
    res['sgd_GBps'] = round(nparam * 20 / res['sgd_us'] / 1e3, 1)
    res['norms'] = [float(o.clip_state()[0]) for o in clipped]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
