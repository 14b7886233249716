"""CPU-only case builders and references of the pre-NMS edge tests (tests/test_gpu_pre_nms_edges.py on the device,
tests/test_pre_nms_cases_host.py for the preconditions of the committed seeds).  Nothing here touches the GPU.

Section 1 (aod_topk_stable): score rows of the named distributions at the shapes that reach each path of topk_block, a host restatement of
the kernel's u64 key and of its 8-pass radix select (which pass takes the `whole_bin` exit, how many distinct digits one wave meets).
Section 2 (scoring.pre_nms): head outputs built directly as NCHW lists, the float32 / float64 row references (softmax, normalisation, row
max, level gate) and the full decode of every anchor with its edge flags (clamped dw / dh, clipped at 0, clipped at the image border)."""
import functools

import numpy as np
import torch

from oracle import geometry as ogeo
from oracle.detect import stable_topk
from oracle.model import nhwc_flat
from tests import synth

# ---------------------------------------------------------------- section 1: score rows for aod_topk_stable
TOPK_B = 3                       # b = 1, 2 start unaligned when A is odd
CACHE_N = 36864                  # floats of one row that topk_block keeps in LDS
TOPK_SHAPES = [(65, 1), (65, 64), (1025, 1000), (1025, 1024), (2304, 1000), (4099, 1000), (36864, 1000), (37893, 1000)]
TOPK_DISTS = ('const', 'two_level', 'quantised', 'uniform', 'ulp_cluster', 'ramp_up', 'ramp_down', 'edges')
TIE_FREE_DISTS = ('uniform', 'ramp_up', 'ramp_down')       # every other distribution holds exact ties on purpose
FLT_MIN = float(np.finfo(np.float32).tiny)
DENORMAL = 1e-42                 # a float32 subnormal (score bits 0x000002ca)
# (pass, A, k): rows built so that radix_select_kth leaves through `whole_bin` at exactly that pass.  Passes 7..4 read the score bytes,
# 3..0 the bytes of ~index.  Pass 1 is met by `const` at k = 1024 and pass 0 by `const` at k = 1000.  Pass 2 needs a tie group that reaches
# past index 65 535, hence the one row longer than the sizes above.  Pass 3 would need a tie group that reaches past index 2^24 (a level of
# a 119-megapixel image): no such row is built.
EXIT_CASES = [(7, 1025, 1000), (6, 4099, 1000), (5, 1025, 1000), (4, 4099, 1000), (2, 65600, 1000)]


def _stratified_uniform(B, A, g):
    """U(0,1)-like float32 rows WITHOUT exact ties: element i = (perm(i) + U(0, 0.5)) / A, so two scores differ by at least 0.5 / A
    (1.3e-5 at the longest row, 200 float32 ulps below 1.0).  torch.rand itself has 24 random bits: a row of 37 893 draws holds about 40
    colliding pairs, which would make `uniform` a tie case."""
    perm = torch.stack([torch.randperm(A, generator=g) for _ in range(B)]).double()
    return ((perm + 0.5 * torch.rand(B, A, generator=g, dtype=torch.float64)) / A).float()


def topk_seed(dist, A, k):
    return 7000 + 131 * TOPK_DISTS.index(dist) + 17 * (A % 1009) + k


def topk_scores(dist, A, k, B=TOPK_B):
    """float32 [B, A] CPU score rows; all values are non-negative and finite"""
    g = synth.gen(topk_seed(dist, A, k))
    if dist == 'const':
        return torch.full((B, A), 0.05)
    if dist == 'two_level':
        x = torch.full((B, A), 0.25)
        for b in range(B):
            x[b, torch.randperm(A, generator=g)[:k // 3]] = 0.9
        return x
    if dist == 'quantised':
        return (torch.rand(B, A, generator=g) * 8).round() / 8
    if dist == 'uniform':
        return _stratified_uniform(B, A, g)
    if dist == 'ulp_cluster':
        bits = 0x3f000000 + torch.randint(0, 256, (B, A), generator=g, dtype=torch.int32)
        return bits.view(torch.float32)
    if dist == 'ramp_up':
        return (torch.arange(A, dtype=torch.float32) / A).expand(B, A).contiguous()
    if dist == 'ramp_down':
        return (torch.arange(A, dtype=torch.float32) / A).flip(0).expand(B, A).contiguous()
    if dist == 'edges':
        x = _stratified_uniform(B, A, g)
        for b in range(B):
            pos = torch.randperm(A, generator=g)[:8]
            x[b, pos] = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0, FLT_MIN, DENORMAL], dtype=torch.float32)
        return x
    raise ValueError(dist)


def exit_scores(p, A, k, B=TOPK_B):
    """float32 [B, A] rows on which the radix select takes the whole_bin exit at pass p (see EXIT_CASES)"""
    g = synth.gen(7900 + 10 * p + A % 7)
    if p >= 4:
        byte = p - 4                                                   # the score byte that pass p reads
        shared = (0x3e404040 >> (8 * (byte + 1))) << (8 * (byte + 1))   # the bytes above it: the same in the whole row (p = 7: none)
        low = torch.randint(0, 1 << (8 * byte), (B, A), generator=g, dtype=torch.int64) if byte else torch.zeros(B, A, dtype=torch.int64)
        # digit of that byte: losers below the winners; the top byte (p = 7) is sign + exponent, 0x30..0x3e are scores below 0.5, 0x3f is
        # [0.5, 2); the lower bytes take 0x00..0x7f against 0x80..0xff
        lose, win = ((0x30, 0x3f), (0x3f, 0x40)) if p == 7 else ((0x00, 0x80), (0x80, 0x100))
        dig = torch.randint(*lose, (B, A), generator=g, dtype=torch.int64)
        win = torch.randint(*win, (B, A), generator=g, dtype=torch.int64)
        for b in range(B):
            pos = torch.randperm(A, generator=g)[:k]
            dig[b, pos] = win[b, pos]
        bits = shared | (dig << (8 * byte)) | low
        return bits.to(torch.int32).view(torch.float32)
    if p == 2:
        assert A > 65536 + 16 and k > 8
        x = torch.full((B, A), 0.1)
        x[:, 65536:] = 0.25                                            # tied with the winners below, but behind them in index order
        for b in range(B):
            pos = torch.randperm(65536, generator=g)[:k]
            x[b, pos[:k // 2]] = 0.9
            x[b, pos[k // 2:]] = 0.25
        return x
    raise ValueError(p)


def topk_keys(row, tie='low'):
    """the kernel's key of every element of one float32 row, as numpy uint64: (score bits << 32) | (0xffffffff - index).
    tie='high' is the flipped rule (`| index`) that a broken kernel would use."""
    bits = row.contiguous().numpy().view(np.uint32).astype(np.uint64)
    i = np.arange(bits.shape[0], dtype=np.uint64)
    return (bits << np.uint64(32)) | (i if tie == 'high' else np.uint64(0xffffffff) - i)


def host_topk(row, k, tie='low', ncache=None):
    """indices of the k largest keys in descending key order.  ncache: a broken key that reads the LDS cache past its end is modelled by
    a score of 0 for every index >= ncache (whatever such a read returns, it is not the element's score)."""
    if ncache is not None:
        row = row.clone()
        row[ncache:] = 0.0
    keys = topk_keys(row, tie)
    top = np.sort(keys)[::-1][:k]
    low = (top & np.uint64(0xffffffff)).astype(np.int64)
    return low if tie == 'high' else 0xffffffff - low


def radix_trace(row, k):
    """host restatement of radix_select_kth on one row: (threshold key, pass of the whole_bin exit, per pass the largest number of
    distinct digits that the active lanes of one 64-lane wave hold)"""
    keys = topk_keys(row)
    n = keys.shape[0]
    prefix, mask, remaining = np.uint64(0), np.uint64(0), int(k)
    wave_digits = {}
    for p in range(7, -1, -1):
        shift = np.uint64(8 * p)
        act = (keys & mask) == prefix
        dig = ((keys >> shift) & np.uint64(0xff)).astype(np.int64)
        hist = np.bincount(dig[act], minlength=256)
        incl = np.cumsum(hist[::-1])[::-1]
        excl = incl - hist
        d = int(np.nonzero((excl < remaining) & (remaining <= incl))[0][0])
        padded = np.full(-(-n // 64) * 64, 256, dtype=np.int64)
        padded[:n] = np.where(act, dig, 256)
        w = np.sort(padded.reshape(-1, 64), axis=1)
        wave_digits[p] = int((((w[:, 1:] != w[:, :-1]) & (w[:, 1:] < 256)).sum(1) + (w[:, 0] < 256)).max())
        whole = int(hist[d]) == remaining - int(excl[d])
        remaining -= int(excl[d])
        prefix |= np.uint64(d) << shift
        mask |= np.uint64(0xff) << shift
        if whole:
            break
    return int(prefix), p, wave_digits


def tie_stats(row, k):
    """(number of adjacent equal pairs among the k + 1 largest scores, whether the k-th and the (k+1)-th score are equal)"""
    v = torch.sort(row, descending=True, stable=True)[0][:k + 1]
    return int((v[1:] == v[:-1]).sum()), bool(len(v) > k and v[k] == v[k - 1])


# ---------------------------------------------------------------- section 2: head outputs for scoring.pre_nms
NUM_ANCHORS = 9
MEANS = (0.1, -0.1, 0.05, 0.0)
STDS = (0.1, 0.1, 0.2, 0.2)
WH_RATIO_CLIP = 16 / 1000
FG_THR = 0.3
LAYOUTS = {
    # feature-map sizes (odd A, level bases at B * sum(A) unaligned), strides, nms_pre, per-image (H, W, 3) -- one smaller than the
    # anchor extent, all different -- and per-image scale factors (anisotropic)
    'five': dict(sizes=[(15, 17), (8, 9), (4, 5), (2, 3), (1, 2)], strides=(8, 16, 32, 64, 128), nms_pre=100,
                 img_shapes=[(120, 136, 3), (75, 90, 3), (131, 101, 3)],
                 scale_factors=[(1.25, 0.8, 1.25, 0.8), (0.8, 1.25, 0.8, 1.25), (1.5, 1.1, 1.5, 1.1)]),
    'big': dict(sizes=[(66, 63)], strides=(8,), nms_pre=1000, img_shapes=[(528, 504, 3), (300, 420, 3)],
                scale_factors=[(1.25, 0.8, 1.25, 0.8), (0.8, 1.25, 0.8, 1.25)]),
    'seven': dict(sizes=[(9, 11), (7, 5), (5, 5), (3, 5), (3, 3), (1, 3), (1, 1)], strides=(8, 16, 32, 64, 100, 200, 300), nms_pre=100,
                  img_shapes=[(72, 88, 3), (50, 61, 3), (90, 70, 3)],
                  scale_factors=[(1.25, 0.8, 1.25, 0.8), (0.8, 1.25, 0.8, 1.25), (1.5, 1.1, 1.5, 1.1)]),
}
# (layout, B, C, has_bg, normalize, recipe).  Recipes: 'a' 0.5 N(0,1) with +8 plants; 'b' = 'a' with level 0 all zeros; 'c' logits rounded to
# multiples of 0.5; 'd' the gate case (every row far below 0.3 but row A-1 of level 1 in image 1).
CASES = [
    ('five', 3, 20, False, True, 'a'), ('five', 3, 20, False, True, 'b'), ('five', 3, 20, False, True, 'c'), ('five', 3, 20, False, True, 'd'),
    ('five', 3, 21, True, True, 'a'), ('five', 3, 21, True, True, 'b'), ('five', 3, 21, True, True, 'c'), ('five', 3, 21, True, True, 'd'),
    ('five', 3, 1, False, True, 'a'),
    ('five', 3, 20, False, False, 'a'),
    ('five', 2, 80, False, True, 'a'), ('five', 2, 80, False, True, 'c'), ('five', 2, 81, True, True, 'a'), ('five', 2, 81, True, True, 'c'),
    ('five', 2, 80, False, False, 'a'),
    ('big', 2, 20, False, True, 'a'), ('big', 2, 20, False, True, 'c'), ('big', 2, 21, True, True, 'a'), ('big', 2, 81, True, True, 'a'),
    ('seven', 3, 20, False, True, 'a'), ('seven', 3, 20, False, True, 'b'), ('seven', 3, 21, True, True, 'a'),
]


def case_id(case):
    layout, B, C, has_bg, normalize, recipe = case
    return f"{layout}-B{B}-C{C}{'bg' if has_bg else ''}{'' if normalize else '-raw'}-{recipe}"


def case_seed(case):
    layout, B, C, has_bg, normalize, recipe = case
    return 9000 + 1000 * list(LAYOUTS).index(layout) + 10 * C + 3 * 'abcd'.index(recipe) + int(has_bg) + 2 * int(not normalize)


def _to_nchw(flat, h, w):
    """[B, h*w*9, c] (the kernels' row order) -> the head's [B, 9*c, h, w]"""
    B = flat.shape[0]
    return flat.reshape(B, h, w, -1).permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=2)             # the tests walk the cases one after the other
def build_case(case):
    """head outputs (NCHW float32 lists), anchors, metas of one case; the returned tensors are shared and must not be modified"""
    layout, B, C, has_bg, normalize, recipe = case
    lay = LAYOUTS[layout]
    g = synth.gen(case_seed(case))
    nfg = C - 1 if has_bg else C
    cls, reg, lam = [], [], []
    for l, (h, w) in enumerate(lay['sizes']):
        A = h * w * NUM_ANCHORS
        if recipe == 'd':
            x = 0.1 * torch.randn(B, A, C, generator=g)
            if l == 1:
                x[1, A - 1, 0] += 8.0                    # the last row of a partial 256-row block, one image only
        elif recipe == 'c':
            x = (torch.randn(B, A, C, generator=g)).round() * 0.5        # 0.5 N(0,1) rounded to multiples of 0.5
        else:
            x = 0.5 * torch.randn(B, A, C, generator=g)
            for b in range(B):
                for _ in range(3):
                    x[b, int(torch.randint(0, A, (1,), generator=g)), int(torch.randint(0, nfg, (1,), generator=g))] += 8.0
            if recipe == 'b' and l == 0:
                x.zero_()
        cls.append(_to_nchw(x, h, w))
        # N(0,1) scaled per component: dx, dy of about 0.8 anchor sizes (many boxes leave the image), dw, dh of std 5 after the stds (about
        # 40 % beyond +-4.135 in each of the two signs together)
        r = torch.randn(B, A, 4, generator=g) * torch.tensor([8.0, 8.0, 25.0, 25.0])
        reg.append(_to_nchw(r, h, w))
        lam.append(_to_nchw(torch.rand(B, A, 1, generator=g) * 0.3 + 0.01, h, w))
    anchors = ogeo.grid_anchors(ogeo.gen_base_anchors(lay['strides']), lay['sizes'], lay['strides'])
    return dict(case=case, B=B, C=C, has_bg=has_bg, normalize=normalize, recipe=recipe, nms_pre=lay['nms_pre'], cls=cls, reg=reg, lam=lam,
                anchors=anchors, img_shapes=lay['img_shapes'][:B], scale_factors=[np.asarray(s, np.float32) for s in lay['scale_factors'][:B]],
                A=[h * w * NUM_ANCHORS for h, w in lay['sizes']])


def row_reference(cls_flat, has_bg, normalize=True):
    """[B, A, C] logits (any float dtype) -> dict(scores: what the gather writes, rowmax: what the top-k ranks, max_alpha: what the level
    gate reads).  Lambda_L2.py:269-273 (the same statements as oracle.detect.pre_nms); with has_bg (My_L_ssd_head.py:331-345) the scores are
    the plain softmax over all C logits and both maxima run over the C - 1 foreground columns.  normalize=False (Entropy_ALL / Entropy_Avg):
    the gathered scores are the raw softmax, the ranking is unchanged."""
    alphas = cls_flat.softmax(dim=2)
    if has_bg:
        fg = alphas[..., :-1].max(-1)[0]
        return dict(scores=alphas, rowmax=fg, max_alpha=fg)
    S = alphas.sum(dim=2, keepdim=True) + 1e-20
    scores = alphas / (S + 1e-9)
    return dict(scores=scores if normalize else alphas, rowmax=scores.max(-1)[0], max_alpha=alphas.max(-1)[0])


def decode_all(anchors, reg_flat, img_shapes, scale_factors):
    """every anchor of one level decoded by oracle.geometry.delta2bbox in reg_flat's dtype: boxes [B, A, 4] (clipped per image, divided by
    the scale factors) plus, for the edge shares and the error scale, the unclipped boxes, the coder deltas after stds / means and the
    magnitude of the terms that a coordinate is summed from (|centre| + |shift| + half the decoded size)."""
    dt = reg_flat.dtype
    anc = anchors.to(dt)[None].expand(reg_flat.shape[0], -1, 4)
    kw = dict(means=MEANS, stds=STDS, wh_ratio_clip=WH_RATIO_CLIP)
    clipped = ogeo.delta2bbox(anc, reg_flat, max_shape=[s[:2] for s in img_shapes], **kw)
    raw = ogeo.delta2bbox(anc, reg_flat, max_shape=None, **kw)
    sf = torch.as_tensor(np.stack(scale_factors)).to(dt).unsqueeze(1)
    d = reg_flat * reg_flat.new_tensor(STDS) + reg_flat.new_tensor(MEANS)
    pw, ph = anc[..., 2] - anc[..., 0], anc[..., 3] - anc[..., 1]
    mx = ((anc[..., 0] + anc[..., 2]) * 0.5).abs() + (pw * d[..., 0]).abs() + (raw[..., 2] - raw[..., 0]) * 0.5
    my = ((anc[..., 1] + anc[..., 3]) * 0.5).abs() + (ph * d[..., 1]).abs() + (raw[..., 3] - raw[..., 1]) * 0.5
    mag = torch.stack([mx, my, mx, my], -1) / sf
    return dict(boxes=clipped / sf, raw=raw, d=d, mag=mag.clamp(min=1.0))


@functools.lru_cache(maxsize=2)             # the tests walk the cases one after the other
def reference(case):
    """float64 references of one case, the float32 oracle's deviation from them (e_*: the unit of the test bounds) and the edge flags of
    every anchor.  Per level lists unless noted; computed once and shared (read-only)."""
    c = build_case(case)
    B, C = c['B'], c['C']
    max_ratio = abs(np.log(WH_RATIO_CLIP))
    out = dict(rowmax=[], max_alpha=[], scores=[], boxes=[], mag=[], lam=[], clamp_hi=[], clamp_lo=[], clip0=[], clipW=[], clipH=[],
               rowmax32=[], level_any_fg=[])
    e_rowmax = e_alpha = e_scores = e_boxes = 0.0
    for l in range(len(c['cls'])):
        x32 = nhwc_flat(c['cls'][l], C)
        r32, r64 = row_reference(x32, c['has_bg'], c['normalize']), row_reference(x32.double(), c['has_bg'], c['normalize'])
        e_rowmax = max(e_rowmax, float((r32['rowmax'].double() - r64['rowmax']).abs().max()))
        e_alpha = max(e_alpha, float((r32['max_alpha'].double() - r64['max_alpha']).abs().max()))
        e_scores = max(e_scores, float((r32['scores'].double() - r64['scores']).abs().max()))
        g32 = nhwc_flat(c['reg'][l], 4)
        d32 = decode_all(c['anchors'][l], g32, c['img_shapes'], c['scale_factors'])
        d64 = decode_all(c['anchors'][l], g32.double(), c['img_shapes'], c['scale_factors'])
        e_boxes = max(e_boxes, float(((d32['boxes'].double() - d64['boxes']).abs() / d64['mag']).max()))
        hw = torch.tensor([[s[1], s[0], s[1], s[0]] for s in c['img_shapes']], dtype=torch.float64).unsqueeze(1)       # (W, H, W, H)
        out['rowmax'].append(r64['rowmax']); out['max_alpha'].append(r64['max_alpha']); out['scores'].append(r64['scores'])
        out['rowmax32'].append(r32['rowmax'])
        out['level_any_fg'].append((r64['max_alpha'] > FG_THR).any(dim=1))
        out['boxes'].append(d64['boxes']); out['mag'].append(d64['mag'])
        out['lam'].append(nhwc_flat(c['lam'][l], 1)[..., 0])
        out['clamp_hi'].append((d64['d'][..., 2:] > max_ratio).any(-1)); out['clamp_lo'].append((d64['d'][..., 2:] < -max_ratio).any(-1))
        out['clip0'].append((d64['raw'] < 0).any(-1))
        out['clipW'].append((d64['raw'][..., 0::2] > hw[..., 0::2]).any(-1)); out['clipH'].append((d64['raw'][..., 1::2] > hw[..., 1::2]).any(-1))
    out.update(e_rowmax=e_rowmax, e_alpha=e_alpha, e_scores=e_scores, e_boxes=e_boxes)
    # the level gate compares max_alpha with 0.3: distance of the closest row, to be held against the rounding bound
    out['gate_margin'] = min(float((m - FG_THR).abs().min()) for m in out['max_alpha'])
    return out


def ks_of(c):
    return [c['nms_pre'] if 0 < c['nms_pre'] < a else a for a in c['A']]


def edge_shares(ref, sel):
    """sel: per level [B, k] int64 anchor indices -> share of the selected rows on each decode edge (from the float64 reference)"""
    out = {}
    for name in ('clamp_hi', 'clamp_lo', 'clip0', 'clipW', 'clipH'):
        flags = torch.cat([torch.gather(ref[name][l], 1, s) for l, s in enumerate(sel)], dim=1)
        out[name] = float(flags.double().mean())
    return out


def oracle_selection(case):
    """the float32 oracle's own selection: per level [B, k] indices (stable top-k of the float32 row max, or every anchor)"""
    c, ref = build_case(case), reference(case)
    sel = []
    for l, (A, k) in enumerate(zip(c['A'], ks_of(c))):
        sel.append(stable_topk(ref['rowmax32'][l], k)[1] if k < A else torch.arange(A)[None].expand(c['B'], A))
    return sel
