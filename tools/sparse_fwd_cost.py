#!/usr/bin/env python
"""What the sparse forward of the reg / MEH towers can skip, counted on the bench's own batches.

For each of the rotating train batches of bench.py (voc512: 16 x 512^2, seeds as in bench.py) the assigner runs once and
hipops.fwd_row_maps builds the chain m0, D(m0), ..., D^5(m0).  Printed per batch:

  blocks / tiles   live 64-row blocks and live 256-row tiles of a mapped member, per launch: the four paired forward launches (tower layer k
                   needs its output on F_k = D^(5 - k)(m0)) and the four paired dgrad launches (the dX of layer k's dgrad is live on D^(6 - k)(m0))
  per class        live workgroups per blockIdx % 8 class (one XCD of 32 CUs each, one 256 x 256 workgroup per CU) under the OLD order of that
                   launch and under the even deal (aod_conv2d_grouped_deal, mapped = 1).  Old forward: every tile of the three members is
                   computed, member-major over xcd_swizzle.  Old dgrad: (tile, member)-interleaved over xcd_swizzle.
  rounds           ceil(largest class / 32): the launch lasts as long as its fullest XCD

    python tools/sparse_fwd_cost.py [--batch 16] [--size 512] [--rotate 4] [--out FILE.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUS_PER_XCD = 32


def xcd_swizzle(bid, nwg):
    q, r, xcd, j = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + j


def deal(lib, nwg, ng, mapped):
    n = nwg * ng
    tile, group = (C.c_int32 * n)(), (C.c_int32 * n)()
    assert lib.aod_conv2d_grouped_deal(nwg, ng, mapped, tile, group) == 0
    return list(tile), list(group)


def per_class(tile, group, live):
    """live[g]: bool array over tiles (None: a dense member) -> live workgroups per blockIdx % 8 class"""
    per = np.zeros(8, np.int64)
    for b, (t, g) in enumerate(zip(tile, group)):
        per[b % 8] += 1 if live[g] is None else int(live[g][t])
    return per


def rounds(per):
    return int(-(-per.max() // CUS_PER_XCD))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--rotate', type=int, default=4)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the assigner runs on the MI355X'
    import bench
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd._C import lib
    dev = torch.device('cuda', 0)
    AF.set_precision('bf16x3')
    B, S = args.batch, args.size
    cd = dict(bench.CONFIGS['voc512'], batch=B, H=S, W=S)
    model, _ = bench.build_model(dev, cd)
    head = model.bbox_head
    sizes = [(-(-S // s), -(-S // s)) for s in head.anchor_generator.strides] if not isinstance(head.anchor_generator.strides[0], tuple) \
        else [(-(-S // s[1]), -(-S // s[0])) for s in head.anchor_generator.strides]
    segs = AF.dense_segs([ho.Seg(B, h, w, 0) for h, w in sizes])
    M = sum(s.rows for s in segs)
    nt = (M + 255) // 256
    lines = [f'{B} x {S}^2, levels {sizes}: {M} pyramid rows = {(M + 63) // 64} blocks of 64 = {nt} tiles of 256; {CUS_PER_XCD} CUs per XCD, '
             f'one workgroup per CU']

    def tiles_of(m):
        pad = np.zeros(nt * 4, np.uint8)
        pad[:len(m)] = m
        return pad.reshape(nt, 4).any(1)

    # old orders
    fwd_old = ([xcd_swizzle(b, nt * 3) % nt for b in range(nt * 3)], [xcd_swizzle(b, nt * 3) // nt for b in range(nt * 3)])
    dg_old = ([xcd_swizzle(b, nt * 2) // 2 for b in range(nt * 2)], [xcd_swizzle(b, nt * 2) % 2 for b in range(nt * 2)])
    fwd_new, dg_new = deal(lib, nt, 3, 1), deal(lib, nt, 2, 1)
    rider_new = deal(lib, nt, 2, 1)
    tot = dict(fwd_old=0, fwd_new=0, dg_old=0, dg_new=0)
    for k in range(args.rotate):
        d = bench.synth_batch(B, S, S, dev, seed=20 + 1000 * k, classes=cd['classes'])
        gtb, gtl = [b.to(dev) for b in d['gt_bboxes']], [l.to(dev) for l in d['gt_labels']]
        t = head.get_targets_batch(sizes, d['img_metas'], gtb, gtl, dev, raw_num_pos=True)
        bw = AF.dense_concat([x.reshape(-1, 4) for x in t[3]])
        npos = int((bw.abs().sum(1) != 0).sum())
        maps = [m.cpu().numpy() for m in ho.fwd_row_maps(bw, segs, head.num_anchors, ho.width(256), 256, 3, 3, 1, 1, 6)]
        lines.append(f'\nbatch {k} (seed {20 + 1000 * k}): {npos} positive anchors of {bw.shape[0]} ({100.0 * npos / bw.shape[0]:.2f} %), '
                     f'm0 {int(maps[0].sum())} blocks')
        for layer in (1, 2, 3, 4):
            live = tiles_of(maps[5 - layer])
            old = per_class(*fwd_old, [None, None, None])
            new = per_class(*fwd_new, [None, live, live])
            lines.append(f'  forward layer {layer}: F_{layer} {int(maps[5 - layer].sum()):4d} blocks {int(live.sum()):3d} tiles per mapped member; live workgroups '
                         f'{3 * nt} -> {int(new.sum())}; per class old {old.tolist()} ({rounds(old)} rounds) new {new.tolist()} ({rounds(new)} rounds)')
            tot['fwd_old'] += rounds(old)
            tot['fwd_new'] += rounds(new)
            if layer == 1:       # the variant: cls + reg in one launch, the MEH tower mapped alone
                pair = per_class(*rider_new, [None, live])
                lines.append(f'      (rider in a launch of its own: cls + reg {pair.tolist()} ({rounds(pair)} rounds) + MEH alone '
                             f'{int(live.sum())} tiles ({int(-(-live.sum() // 256))} round))')
        for layer in (4, 3, 2, 1):
            live = tiles_of(maps[6 - layer])
            old = per_class(*dg_old, [None, live])
            new = per_class(*dg_new, [None, live])
            lines.append(f'  dgrad layer {layer}:   dX map {int(maps[6 - layer].sum()):4d} blocks {int(live.sum()):3d} tiles; live workgroups {int(new.sum())} of {2 * nt}; '
                         f'per class old {old.tolist()} ({rounds(old)} rounds) new {new.tolist()} ({rounds(new)} rounds)')
            tot['dg_old'] += rounds(old)
            tot['dg_new'] += rounds(new)
    n = 4 * args.rotate
    lines.append(f'\nmean rounds per launch over {args.rotate} batches: forward {tot["fwd_old"] / n:.2f} -> {tot["fwd_new"] / n:.2f}, '
                 f'paired dgrad {tot["dg_old"] / n:.2f} -> {tot["dg_new"] / n:.2f}')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
