"""The towers' grouped 256 x 256 launches, isolated, at the bench shape (16 x 512^2 pyramid: 87 296 rows = 341 tiles of 256 per member; mapped
members live on the last 85 tiles): dense, mapped and zero-map forms of the three-member forward and of the paired dgrad, each under
AOD_TILE_ORDER=0 (the fixed deal) and with the device-built list (docs/LAB_NOTES.md section 23).
  launches   device time per launch by the method of LAB_NOTES 22: ten launches captured into one graph, one replay between two events,
             median and p5 / p95 of 15 replays (the small launch that builds the list is part of the mapped forms)
  stamps     one launch of each mapped form under per-block stamps (needs the -DAOD_TILE_TIMING build: python tools/dbg/tile_timing.py build,
             then AOD_HIP_LIB=tools/dbg/_build/libaodhip_dbg.so): start and end of every block, its XCD / CU, member, live or dead
    [PROBE_ROOT=<another checkout of this project, e.g. the parent commit>] python tools/dbg/tile_order_probe.py launches|stamps LABEL OUTFILE"""
import ctypes as C
import os
import sys

ROOT = os.environ.get('PROBE_ROOT') or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from aod_meh_hua_amd import functional as AF
from aod_meh_hua_amd import hipops as ho
from aod_meh_hua_amd._C import lib

mode, label, outfile = sys.argv[1], sys.argv[2], sys.argv[3]
AF.set_precision('bf16x3')
ho.SPLITK = False
Bn, CH = 16, 256
sizes = [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)]
segs, M = [], 0
for h, w in sizes:
    segs.append(ho.Seg(Bn, h, w, M))
    M += Bn * h * w
NT, NBLK = (M + 255) // 256, (M + 63) // 64
gen = torch.Generator(device='cuda').manual_seed(7)
rnd = lambda *sh: torch.randn(*sh, device='cuda', generator=gen)
x = [ho.x3_split(rnd(M, CH)) for _ in range(3)]
w = [ho.x3_split((rnd(CH * 9, CH) / (9 * CH / 2) ** 0.5)).reshape(CH, 9 * ho.xw(CH)) for _ in range(3)]
bias = [rnd(CH) for _ in range(3)]
mask = [ho.x3_split(rnd(M, CH)) for _ in range(2)]
outs3 = [torch.empty(M, ho.xw(CH), device='cuda', dtype=torch.bfloat16) for _ in range(3)]
cs = [torch.zeros(CH, device='cuda') for _ in range(2)]
last85 = torch.zeros(NBLK, dtype=torch.uint8, device='cuda')
last85[(NT - 85) * 4:] = 1
# the dgrad's IN map: its dilation must come out as the last 85 tiles -> mark from one tile further in (the dilation reaches < 1 tile back)
in85 = torch.zeros(NBLK, dtype=torch.uint8, device='cuda')
in85[(NT - 84) * 4:] = 1
zero = torch.zeros(NBLK, dtype=torch.uint8, device='cuda')
dz_mapped = x[1] * in85.bool().repeat_interleave(64)[:M, None].to(torch.bfloat16)
dz_zero = torch.zeros_like(x[1])


def fwd(m):
    return lambda: ho.conv2d_rows_grouped(x, segs, w, CH, 3, 3, 1, 1, 1, pre_shifts=bias, relu=True, outs=outs3,
                                          omaps=[None, m, m] if m is not None else None)


def dgrad(m, dz):
    return lambda: ho.conv2d_dgrad_rows_grouped([x[0], dz], segs, segs, w[:2], CH, 3, 3, 1, 1, 1, masks=mask, colsums=cs,
                                                in_maps=[None, m] if m is not None else None, outs=outs3[:2])


CASES = [('forward, dense', fwd(None), 3), ('forward, reg / MEH mapped (85 + 85 live)', fwd(last85), 3), ('forward, both maps zero', fwd(zero), 3),
         ('paired dgrad, dense', dgrad(None, x[1]), 2), ('paired dgrad, reg mapped', dgrad(in85, dz_mapped), 2), ('paired dgrad, zero map', dgrad(zero, dz_zero), 2)]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(f):
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(10):
            f()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(15):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); g.replay(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 100.0)          # us per launch
    return np.median(ts), np.percentile(ts, 5), np.percentile(ts, 95)


def stamps(name, f, ng):
    nb = ng * NT
    for _ in range(20):
        f()
    st = torch.zeros(nb * 16, dtype=torch.int64, device='cuda')
    lib.aod_dbg_set_tile_stamps.argtypes = [C.c_void_p]
    assert lib.aod_dbg_set_tile_stamps(st.data_ptr()) == 0
    torch.cuda.synchronize()
    f()
    torch.cuda.synchronize()
    assert lib.aod_dbg_set_tile_stamps(None) == 0
    s = st.cpu().numpy().reshape(nb, 16)
    t = s.astype(np.float64) * 0.01
    t0 = t[:, 0].min()
    start, end = t[:, 0] - t0, t[:, 15] - t0
    dead = s[:, 11] == 1
    member, tile = (s[:, 14] >> 32) & 0xff, s[:, 14] & 0xffffffff
    hw = s[:, 7]
    cu = (hw & 0xffffffff) >> 8 & 0xf; se = (hw & 0xffffffff) >> 13 & 0x7; sh = (hw & 0xffffffff) >> 12 & 1; xcc = (hw >> 32) & 0xf
    key = xcc * 1000 + se * 100 + sh * 50 + cu
    live = ~dead
    say(f'  {name}: {nb} blocks, {int(live.sum())} live, {int(dead.sum())} dead; span {end.max():.1f} us; block -> XCD: xcc == blockIdx % 8 for '
        f'{int((xcc == np.arange(nb) % 8).sum())} of {nb}')
    lk = key[live]
    cnt = np.array([(lk == k).sum() for k in np.unique(key)])
    say(f'    CUs seen {len(np.unique(key))}; live tiles per CU (rounds): ' + ', '.join(f'{v}: {int((cnt == v).sum())} CUs' for v in np.unique(cnt)))
    per_x = [int((live & (xcc == c)).sum()) for c in range(8)]
    say(f'    live tiles per XCD {per_x}; XCD finish times (us) {[round(float(end[xcc == c].max()), 1) for c in range(8)]}')
    dur = end - start
    for g in range(ng):
        sel = live & (member == g)
        if sel.any():
            d = dur[sel]
            kl = (t[sel, 3] - t[sel, 2]); ep = (t[sel, 6] - t[sel, 3]); tail = (t[sel, 15] - t[sel, 6]); pro = (t[sel, 2] - t[sel, 0])
            say(f'    live tile, member {g}: n {int(sel.sum())} total median {np.median(d):.1f} p10 {np.percentile(d, 10):.1f} p90 {np.percentile(d, 90):.1f} us; '
                f'prologue {np.median(pro):.1f}, K loop {np.median(kl):.1f}, epilogue to stores acknowledged {np.median(ep):.1f}, column sums {np.median(tail):.1f}')
            ss = np.sort(start[sel])
            say(f'      start times p0/25/50/75/100: {[round(float(np.percentile(ss, q)), 1) for q in (0, 25, 50, 75, 100)]}; '
                f'end times p50/100: {[round(float(np.percentile(end[sel], q)), 1) for q in (50, 100)]}')
    # live tile time against the number of different members live on its XCD at its midpoint
    mid = (start + end) / 2
    nm = np.zeros(nb, np.int64)
    nco = np.zeros(nb, np.int64)
    for b in np.nonzero(live)[0]:
        co = live & (xcc == xcc[b]) & (start <= mid[b]) & (end >= mid[b])
        nm[b] = len(np.unique(member[co])); nco[b] = int(co.sum())
    for k in np.unique(nm[live]):
        sel = live & (nm == k)
        say(f'    live tile with {k} member(s) running on its XCD: n {int(sel.sum())} median {np.median(dur[sel]):.1f} us (K loop {np.median(t[sel, 3] - t[sel, 2]):.1f}), '
            f'co-resident live tiles median {np.median(nco[sel]):.0f}')
    first = live & (start < 20.0)
    later = live & ~first
    if later.any():
        say(f'    live tiles that start in the first 20 us: {int(first.sum())}, median {np.median(dur[first]):.1f} us; later ones: {int(later.sum())}, '
            f'median {np.median(dur[later]):.1f} us, start median {np.median(start[later]):.1f}')
    if dead.any():
        d = dur[dead]
        say(f'    dead block: holds its slot median {np.median(d):.2f} p90 {np.percentile(d, 90):.2f} max {d.max():.2f} us; sum {d.sum():.0f} us; '
            f'start times p0/50/100 {[round(float(np.percentile(start[dead], q)), 1) for q in (0, 50, 100)]}')
        # dead blocks that run while live tiles hold every other CU of their XCD: do they delay anything?
        say(f'    dead blocks started before 20 us: {int((dead & (start < 20)).sum())}; between 20 us and the last live start '
            f'({start[live].max():.1f}): {int((dead & (start >= 20) & (start < start[live].max())).sum())}; after: {int((dead & (start >= start[live].max())).sum())}')


has_switch = hasattr(ho, 'tile_order_list')
say(f'# {label}: {mode}; {M} rows, {NT} tiles per member, library {os.environ.get("AOD_HIP_LIB", "default")}')
for sw in (['0', None] if has_switch else [None]):
    if sw is None:
        os.environ.pop('AOD_TILE_ORDER', None)
    else:
        os.environ['AOD_TILE_ORDER'] = sw
    say(f'## AOD_TILE_ORDER={"unset (list)" if sw is None and has_switch else ("0 (fixed deal)" if sw == "0" else "n/a (parent: fixed deal)")}')
    for name, f, ng in CASES:
        if mode == 'launches':
            md, p5, p95 = timed(f)
            say(f'{name:45s}: median {md:7.1f} us  p5 {p5:7.1f}  p95 {p95:7.1f}')
        elif 'dense' not in name:
            stamps(name, f, ng)
os.makedirs(os.path.dirname(os.path.abspath(outfile)), exist_ok=True)
with open(outfile, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
