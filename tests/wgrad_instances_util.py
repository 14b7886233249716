"""One launch per tile instance of the weight gradient (csrc/conv_wgrad.hip WGRAD_INSTANCES), single and grouped: the cases of
tests/test_gpu_wgrad_instances.py, their operands and the recorded digests of their slabs.

Every case is a 1x1 conv (K = one tap) at the smallest shape whose plan names the instance.  Operands come from a CPU generator, so they are the
same bits on every commit; the slab form is bit-reproducible run to run, so the SHA-256 of the slab bytes is a property of the kernel, the
split plan and the launch parameters together.  DIGESTS were recorded with `python -m tests.wgrad_instances_util record` on an MI355X from the
library of commit 11f5e1a (the parent of the change that moved the dispatch to a plan and an instance table); this module uses only what
hipops had at that commit.  The test never records: a missing digest fails."""
import hashlib
import sys
import zlib

import torch

from tests import synth

# (wide, waves, tile, x3, sparse): tests/test_wgrad_plan.py
W4, W8, W8B = (0, 4, 1, 0, 0), (0, 8, 1, 0, 0), (0, 8, 2, 0, 0)
X4, X4S, X8B = (0, 4, 1, 1, 0), (0, 4, 1, 1, 1), (0, 8, 2, 1, 0)
XW4, XW4S, XW8, XW8S = (1, 4, 2, 1, 0), (1, 4, 2, 1, 1), (1, 8, 4, 1, 0), (1, 8, 4, 1, 1)

BIG, GBIG, SMALL, RAGGED = 12 * 64 * 64, 4 * 64 * 64, 4096, 16384      # rows: the big forms alone / in a group, a small launch, the ragged form
TAIL = 30                                                              # M % 64 = 30 with the last block active on the sparse cases
# name: (mode, members, cin, cout, rows, members with a map, atomic, instance, once-per-process switch the case needs)
CASES = {
    's_w8': ('bf16', 1, 64, 64, SMALL + TAIL, (), False, W8, None),
    's_w8_atomic': ('bf16', 1, 64, 64, SMALL + TAIL, (), True, W8, None),
    's_w8b': ('bf16', 1, 256, 256, BIG, (), False, W8B, None),
    's_x4': ('bf16x3', 1, 128, 32, SMALL + TAIL, (), False, X4, None),
    's_x4s': ('bf16x3', 1, 128, 32, SMALL + TAIL, (0,), False, X4S, None),
    's_xw4': ('bf16x3', 1, 128, 128, SMALL + TAIL, (), False, XW4, None),
    's_xw4s': ('bf16x3', 1, 128, 128, SMALL + TAIL, (0,), False, XW4S, None),
    's_xw4s_ragged': ('bf16x3', 1, 128, 64, RAGGED + TAIL, (0,), False, XW4S, None),
    's_xw8': ('bf16x3', 1, 256, 256, BIG, (), False, XW8, None),
    's_xw8s': ('bf16x3', 1, 256, 256, BIG + TAIL, (0,), False, XW8S, None),
    'g_w8': ('bf16', 2, 64, 64, SMALL + TAIL, (), False, W8, None),
    'g_w8b': ('bf16', 2, 256, 256, GBIG, (), False, W8B, None),
    'g_x4': ('bf16x3', 2, 128, 32, SMALL + TAIL, (), False, X4, None),
    'g_x4s': ('bf16x3', 2, 128, 32, SMALL + TAIL, (0,), False, X4S, None),            # (member 1 passes a null map to the sparse instance)
    'g_xw4': ('bf16x3', 2, 128, 128, SMALL + TAIL, (), False, XW4, None),
    'g_xw4s': ('bf16x3', 2, 128, 128, SMALL + TAIL, (0,), False, XW4S, None),
    'g_xw8': ('bf16x3', 2, 256, 256, GBIG, (), False, XW8, None),
    'g_xw8s': ('bf16x3', 2, 256, 256, GBIG + TAIL, (0, 1), False, XW8S, None),
    # the three instances no default plan reaches
    's_w4': ('bf16', 1, 64, 64, SMALL + TAIL, (), False, W4, 'AOD_WGRAD_W8'),
    's_x8b': ('bf16x3', 1, 256, 256, BIG, (0,), False, X8B, 'AOD_WGRAD_X3_WIDE'),      # (this form ignores the map)
    'g_x8b': ('bf16x3', 2, 256, 256, GBIG, (), False, X8B, 'AOD_WGRAD_X3_WIDE'),
}

PARENT = '11f5e1a'
DIGESTS = {
    's_w8': 'e1e74afa27b875de2bbf1ad0a5a52790337b92dddc477fb579e2d14778241080',
    's_w8b': '676d5f14abdafd2d1ad6049566335e2e6b0dd3ce28b2d97cec6fd87ca7a4c364',
    's_x4': 'd1286c4e632602e9236d882a8a1211627b211379851b3adc5dc3a38056dda7bd',
    's_x4s': 'aceb1cf9a5158bf50925dec1e466f8b1be9050ddfee87d813c2858d396cac604',
    's_xw4': '1805c9b72797f98098276f08914398aee5595049f09e39b1c7893a1444afa75d',
    's_xw4s': 'd38c556bf9dc893259d4079206dc970a82313e3203e155a4eb94265c0ef2295a',
    's_xw4s_ragged': '07645393da63aea417202f7c5c74a78a6db64aa2812a42de651a575245e615f6',
    's_xw8': '1d164936c8864bdb9f2fdeb8e73829604996a4aaacb3c2cb29def630fdcd8e5e',
    's_xw8s': 'c6287f0e3181db96135d42a29a9cf1102e35d2cbfd814020df5fc717c636cce0',
    'g_w8': '70403d3c34f2b754e9888cae48d0e74de8091c73ed99447aecb2e63a0615e7a5',
    'g_w8b': 'f29cd590487f94f534a886af7be8802e47b4cff96126d3234210108ae51b46ca',
    'g_x4': 'bd7fc04c48abbe275fc16eeac7e199da9970fb65eab3024050af6aec3682d1bd',
    'g_x4s': '83ed23e4ea3b7229c24d0d0e170253795e9272623f9547109a646a5085eefbd6',
    'g_xw4': '4e168c98c8c114f01562d3390316d0d5ef5756c63f2734ef4b14f92909e437f6',
    'g_xw4s': '211259487d2a0d78b2732b8044572e1700247f73d9b66d0ba9efadb6d4ba485f',
    'g_xw8': 'd975431f84505321bd4374837be17a0d8b6dd0dcd4d612046754fbbd5deebbcf',
    'g_xw8s': '25cd33477f074d5890530a1ceb5c3624dc581bdfcad03a9626289152ceae5c1b',
    's_w4': '3c49032e0a9710f3d15ab78650ca7b97000cbc30989b9384f11d8fd01d46b71c',
    's_x8b': '3149b282c1fc5a3bb18c7f4555d2fbc01074e65cb5eb1a229f24b5dc82ac21d7',
    'g_x8b': 'b51190f16bd41c54e4d6c6b64000ac646b02051553ec2e4709869cb0c5513a45',
}


def _operands(mode, cin, cout, rows, mapped, seed):
    """-> x fp32 [rows, cin], dZ fp32 [rows, cout] (bf16 mode: bf16-representable values), map or None.  A mapped dZ is zero outside its active
    64-row blocks: every third block and the ragged last one"""
    g = synth.gen(seed)
    x, dz = torch.randn(rows, cin, generator=g), torch.randn(rows, cout, generator=g)
    zmap = None
    if mapped:
        nb = (rows + 63) // 64
        zmap = torch.zeros(nb, dtype=torch.uint8)
        zmap[1::3] = 1
        zmap[nb - 1] = 1
        dz = dz * zmap.repeat_interleave(64)[:rows, None].float()
    if mode == 'bf16':
        x, dz = x.bfloat16().float(), dz.bfloat16().float()
    return x.cuda(), dz.cuda(), (zmap.cuda() if mapped else None)


def descs(name):
    """the members' descriptors and the flags of aod_conv2d_wgrad_plan_ex (the caller has set the case's precision mode)"""
    from aod_meh_hua_amd import hipops as ho
    mode, n, cin, cout, rows, maps, atomic, _, _ = CASES[name]
    segs = [ho.Seg(1, 1, rows, 0)]
    pad8 = lambda c: (c + 7) // 8 * 8
    d = ho.make_desc(ho.width(pad8(cin)), ho.width(pad8(cout)), 1, 1, 1, 0, 1, segs, segs, False, False, False)
    flags = (1 if atomic else 0) | (2 if n > 1 else 0)
    for g in maps:
        flags |= 16 << g
    return [d] * n, flags


def run(name):
    """launches the case in its precision mode -> (gradients [cout, cin] per member, fp64 references, SHA-256 of the slab bytes or None)"""
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    mode, n, cin, cout, rows, maps, atomic, _, _ = CASES[name]
    prev = AF.get_precision()
    AF.set_precision(mode)
    try:
        x3 = mode == 'bf16x3'
        segs = [ho.Seg(1, 1, rows, 0)]
        ops = [_operands(mode, cin, cout, rows, g in maps, zlib.crc32(name.encode()) % 100000 + g) for g in range(n)]
        rows_of = (lambda t: ho.x3_split(t)) if x3 else (lambda t: t.bfloat16())
        xs, dzs = [rows_of(o[0]) for o in ops], [rows_of(o[1]) for o in ops]
        refs = [o[1].double().T @ o[0].double() for o in ops]
        if n == 1 and atomic:
            dw = torch.zeros(cout, 1, 1, cin, device='cuda')
            ho.conv2d_wgrad_rows(xs[0], segs, dzs[0], segs, 1, 1, 1, 0, 1, dw=dw)
            torch.cuda.synchronize()
            return [dw.view(cout, cin)], refs, None
        if n == 1:
            slabs = ho.conv2d_wgrad_rows(xs[0], segs, dzs[0], segs, 1, 1, 1, 0, 1, zmap=ops[0][2])
            torch.cuda.synchronize()
            grads = [slabs.double().sum(0).view(slabs.shape[1], slabs.shape[4])[:cout, :cin].float()]
        else:
            gws = [torch.full((cout, cin, 1, 1), float('nan'), device='cuda') for _ in range(n)]
            jobs = [ho.WgradJob(xs[g], segs, dzs[g], segs, 1, 1, 1, 0, 1, (cin, cout), cout, cin, gws[g], zmap=ops[g][2]) for g in range(n)]
            splits = ho.wgrad_group_splits(jobs)
            assert splits is not None, f'{name}: the members do not share a grid'
            ho.wgrad_unpack_group(jobs)
            torch.cuda.synchronize()
            lg = 2 if x3 else 1
            tot = sum(sp * (j.dz.shape[1] // lg) * (j.x_rows.shape[1] // lg) for sp, j in zip(splits, jobs))
            # the scratch the launch just wrote.  This leans on hipops internals: _slab_scratch caches one buffer per (device, stream) and `tot` is
            # recomputed the way wgrad_unpack_group computes it -- a change of that scratch policy breaks this digest without any kernel change
            slabs = ho._slab_scratch(tot, xs[0].device)
            grads = [g.view(cout, cin) for g in gws]
        return grads, refs, hashlib.sha256(slabs.cpu().numpy().tobytes()).hexdigest()
    finally:
        AF.set_precision(prev)


def record(names):
    for name in names:
        grads, refs, digest = run(name)
        err = max(float((g.double() - r).abs().max() / r.abs().max()) for g, r in zip(grads, refs))
        print(f"    '{name}': '{digest}',      # max error {err:.2e}" if digest else f'    # {name}: max error {err:.2e}', flush=True)


if __name__ == '__main__':
    if sys.argv[1] == 'record':          # record [SWITCH]: the cases of that once-per-process switch, which the caller has set to 0
        record([k for k, c in CASES.items() if c[8] == (sys.argv[2] if len(sys.argv) > 2 else None)])
