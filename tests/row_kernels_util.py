"""Cases and helpers of tests/test_gpu_row_kernels.py: the row kernels under and around the FPN neck (csrc/elementwise.hip, csrc/ssd_ops.hip
and csrc/x3_ops.hip; max-pool and upsample-add are one template each over the row layout of csrc/row_layout.h) at the shapes where an
index or a grid-stride loop goes wrong -- 1x1 maps, one-column maps, H = 2h - 1, and one case each beyond the grid cap of 2048 blocks x 256 threads (CAP work items: the loop's second trip).

Most expectations are bit for bit and carry no figure.  The adjoint of the upsample is bounded element by element on the scale
S = the sum of the absolute values folded into the element (at most four, plus the old value when accumulating):
    x3         |got - ref| <= 2^-16 S   (the 16-bit split of an fp32 sum of at most four, whose three adds cost 2^-22)
    fast mode  |got - ref| <= 2^-8 S    (one bf16 rounding of an fp32 sum)
The trailing comment of an adjoint case is the largest |got - ref| / S measured on an MI355X over the bound (`python -m tests.row_kernels_util
record`): x3 set / fast set / fast accumulate."""
import sys

import torch
import torch.nn.functional as F

CAP = 2048 * 256
# ---- max-pool 3x3 / stride 2 / pad 1: (B, C, H, W)
POOL_SHAPES = [(1, 64, 1, 1), (2, 64, 2, 3), (1, 64, 7, 1), (2, 64, 13, 11),
               (4, 256, 129, 131)]          # 4 * 65 * 66 octets * 32 = 549 120 work items > CAP
# ---- upsample + add: ((h, w), (H, W)) at B = 2, C = 64; the last at B = 4, C = 256 (4 * 66 * 79 * 32 = 667 392 work items > CAP)
UPSAMPLE_PAIRS = [((1, 1), (1, 1)), ((1, 2), (2, 3)), ((4, 5), (7, 10)), ((7, 10), (13, 19)), ((33, 40), (66, 79))]
UPSAMPLE_CASES = [(2, 64) + p for p in UPSAMPLE_PAIRS[:-1]] + [(4, 256) + UPSAMPLE_PAIRS[-1]]
# ---- its adjoint: one work item per SOURCE element, so the last pair again at B = 13 (13 * 33 * 40 * 32 = 549 120 > CAP)
ADJOINT_CASES = [
    (2, 64, (1, 1), (1, 1)),            # 0.00 / 0.00 / 0.99   (a copy; the accumulate form is one add)
    (2, 64, (1, 2), (2, 3)),            # 0.50 / 0.94 / 0.82
    (2, 64, (4, 5), (7, 10)),           # 0.49 / 1.00 / 0.99
    (2, 64, (7, 10), (13, 19)),         # 0.50 / 1.00 / 1.00
    (4, 256, (33, 40), (66, 79)),       # 0.50 / 1.00 / 1.00
    (13, 256, (33, 40), (66, 79)),      # 0.50 / 1.00 / 1.00
]
X3_ADJ_BOUND, FAST_ADJ_BOUND = 2.0 ** -16, 2.0 ** -8
# ---- layout: (B, H, W); the last of each list is one past the cap in the kernel's own unit of work (pixels; space-to-depth pixels)
ROWS_SIZES = [(1, 2, 2), (2, 6, 10), (1, 727, 723)]          # 525 621 pixels
S2D_SIZES = [(1, 2, 2), (2, 6, 10), (2, 1026, 1024)]         # 2 * 513 * 512 = 525 312 space-to-depth pixels
ROWS_CHANNELS = [(3, 8), (8, 8), (3, 16), (16, 16)]          # (C, cpad): cpad 8 the vector store, cpad 16 the scalar loop
# ---- element-wise: bf16 elements; the smallest legal size and one legal size past the cap (x3_add: n % 64 == 0, 16 per work item; add_relu: 8)
X3_ADD_SIZES = [64, 16 * (CAP + 4)]
ADD_RELU_SIZES = [8, 8 * (CAP + 1)]
SPLIT_CHANNELS = [1, 31, 32, 33, 180]
SPLIT_ROWS = 21846          # x 24 octets (C = 180) = 524 304 work items > CAP


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(seed, *shape):
    """CPU generator -> device fp32"""
    return torch.randn(*shape, generator=gen(seed)).cuda()


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def rows_of(t_nhwc, x3):
    """fp32 [B, H, W, C] -> (the rows a kernel is given, their values fp32 [B, H, W, C])"""
    from aod_meh_hua_amd import hipops as ho
    C = t_nhwc.shape[-1]
    flat = t_nhwc.reshape(-1, C).contiguous()
    if x3:
        r = ho.x3_split(flat)
        return r, ho.x3_merge(r, C).view(t_nhwc.shape)
    r = flat.bfloat16()
    return r, r.float().view(t_nhwc.shape)


def values_of(rows, shape, x3):
    from aod_meh_hua_amd import hipops as ho
    return (ho.x3_merge(rows, shape[-1]) if x3 else rows.float()).view(shape)


def heads_tails(xrows):
    """X rows [M, 64 * bands] -> (heads, tails) as bf16 [M, 32 * bands] in logical channel order"""
    M, Wd = xrows.shape
    assert Wd % 64 == 0 and xrows.dtype == torch.bfloat16
    v = xrows.view(M, Wd // 64, 2, 32)
    return v[:, :, 0].reshape(M, Wd // 2), v[:, :, 1].reshape(M, Wd // 2)


def split_in_torch(t):
    """x3_split written out: head = bf16(v), tail = bf16(v - head), channels padded to whole bands of 32 with +0"""
    M, C = t.shape
    Cp = (C + 31) // 32 * 32
    v = F.pad(t.float(), (0, Cp - C))
    h = v.bfloat16()
    l = (v - h.float()).bfloat16()
    return torch.stack([h.view(M, Cp // 32, 32), l.view(M, Cp // 32, 32)], 2).reshape(M, 2 * Cp)


def canonical(xrows):
    """An X-layout result is canonical when the head is a nearest bf16 of the value and the tail the rounding of the remainder, i.e. when
    splitting its merged values again gives it back.  One exception is in the format itself: a tail of exactly half the head's spacing (the
    remainder rounded up to it, about one value in a thousand) leaves the merged value halfway between two heads, and the second split
    takes the even one -- x3_split(x3_merge(x3_split(t))) differs from x3_split(t) there too.  Both pairs are nearest-head pairs of the same
    value.  -> (whether every element is either given back or such a tie with the same merged value, how many are ties)"""
    from aod_meh_hua_amd import hipops as ho
    v = ho.x3_merge(xrows)
    again = ho.x3_split(v)
    if not torch.equal(ho.x3_merge(again), v):
        return False, -1
    (h, l), (h2, l2) = heads_tails(xrows), heads_tails(again)
    h, l, h2, l2 = h.float(), l.float(), h2.float(), l2.float()
    back = (h2 == h) & (l2 == l)
    tie = (h2 != h) & ((v - h).abs() == (v - h2).abs())
    return bool((back | tie).all()), int((~back).sum())


def up_nearest(t_nhwc, H, W):
    return F.interpolate(t_nhwc.permute(0, 3, 1, 2), size=(H, W), mode='nearest').permute(0, 2, 3, 1)


def adjoint64(g_nhwc, h, w):
    """fp64 adjoint of the nearest upsample by autograd -> [B, h, w, C]"""
    B, H, W, C = g_nhwc.shape
    t = torch.zeros(B, C, h, w, dtype=torch.float64, device=g_nhwc.device, requires_grad=True)
    F.interpolate(t, size=(H, W), mode='nearest').backward(g_nhwc.double().permute(0, 3, 1, 2))
    return t.grad.permute(0, 2, 3, 1)


def adjoint_set(g_rows, B, h, w, H, W):
    """the set form into a destination pre-filled with NaN (hipops.upsample_add_bwd allocates its own: the same launch on our buffer)"""
    from aod_meh_hua_amd import hipops as ho
    out = torch.full((B * h * w, g_rows.shape[1]), float('nan'), dtype=torch.bfloat16, device=g_rows.device)
    ho.call('aod_x3_upsample2x_add_bwd_set' if ho.X3 else 'aod_upsample2x_add_bwd_set', ho.ptr(g_rows), ho.ptr(out), B, h, w, g_rows.shape[1], H, W,
            ho.stream())
    return out


def adjoint_figures(case, x3, seed=0):
    """-> (largest |got - ref| / S of the set form, of the accumulate form or None, the set form's rows, the wrapper's rows)"""
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd.hipops import Seg
    B, C, (h, w), (H, W) = case
    g_rows, g = rows_of(randn(seed + 1, B, H, W, C), x3)
    ref, S = adjoint64(g, h, w), adjoint64(g.abs(), h, w)
    got_rows = adjoint_set(g_rows, B, h, w, H, W)
    wrapped = ho.upsample_add_bwd(g_rows, Seg(B, H, W), Seg(B, h, w))
    got = values_of(got_rows, (B, h, w, C), x3).double()
    assert bool(torch.isfinite(got).all()), 'a source element was not written'
    fig = float(((got - ref).abs() / S).max())
    acc = None
    if not x3:
        old_rows, old = rows_of(randn(seed + 2, B, h, w, C), False)
        before = old_rows.clone()
        ho.upsample_add_bwd_(old_rows, Seg(B, h, w), g_rows, Seg(B, H, W))
        assert not torch.equal(old_rows, before)
        acc = float(((old_rows.double().view(B, h, w, C) - (old.double() + ref)).abs() / (S + old.double().abs())).max())
    return fig, acc, got_rows, wrapped


def record():
    from aod_meh_hua_amd import functional as AF
    for case in ADJOINT_CASES:
        AF.set_precision('bf16x3')
        fx = adjoint_figures(case, True)[0]
        AF.set_precision('bf16')
        fb, fa, _, _ = adjoint_figures(case, False)
        print(f'{case}: {fx / X3_ADJ_BOUND:.2f} / {fb / FAST_ADJ_BOUND:.2f} / {fa / FAST_ADJ_BOUND:.2f}', flush=True)


if __name__ == '__main__':
    if sys.argv[1] == 'record':
        record()
