"""CPU-only case builders and float64 references of the SSD edge tests (tests/test_gpu_ssd_edges.py on the device,
tests/test_ssd_edges_host.py for the preconditions of the committed seeds).  Nothing here touches the GPU.

Section 1 (aod_ssd_loss_fwd / aod_ssd_loss_bwd): head outputs whose negatives tie on purpose, the float64 cross-entropy / SmoothL1 /
gradient references, the kernel's documented selection rule (the k negatives largest by (ce descending, anchor index ascending)) and a
torch-float32 restatement of the kernel's operation order.  Section 2 (generic max-pool, both layouts): bf16-representable images with
real ties, integer upstream gradients, F.max_pool2d in float64 as the exact reference.  Section 3 (L2Norm): rows, weights and the closed
forms in float64, including the kernels' zero-norm contract (k = 0: gx = w * g / eps, nothing into gw)."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from tests import synth

# ---------------------------------------------------------------- section 1: SSD loss with ties
# dist: how the negatives' logit rows are drawn (loss_case).  npos: positives per image, one int for all or one per image.
# kind: where k falls among the negatives' float64 ce values, for EVERY image of the case --
#   'inside' #above < k < #above + #at  |  'end' k == #above + #at, k < #neg  |  'kneg' k == #neg  |  'k0' k == 0
#   'free' the tie-free control  |  'sat' saturated, k reaches into the exact float32 zeros  |  'sat_above' saturated, k stays above them
# grads: which upstream gradients the backward receives: 'cls' (g_cls, g_box), 'noR' (g_noR alone), 'both' (all three)
LossCase = namedtuple('LossCase', 'dist B A C1 npos seed ratio beta kind grads')
N_IGN = 5                        # background anchors per image with label_weight = 0
TIE_DISTS = ('palette', 'all_equal')
TIE_KINDS = ('inside', 'end', 'kneg', 'k0')
MIN_GAP = 1e-3                   # float64 distance from the threshold value to the nearest other negative value (tie cases); smallest here 9.6e-3
LOSS_CASES = [
    LossCase('random', 3, 2500, 21, 40, 11, 3, 1.0, 'free', 'both'),
    LossCase('palette', 3, 8732, 21, 23, 12, 3, 1.0, 'inside', 'cls'),
    LossCase('palette', 3, 2500, 21, 40, 13, 1, 1.0, 'inside', 'both'),
    LossCase('palette', 3, 1025, 81, 30, 14, 3, 0.5, 'inside', 'cls'),
    LossCase('palette', 3, 1024, 2, 60, 15, 3, 1.0, 'inside', 'noR'),
    LossCase('palette', 3, 2500, 21, (0, 0, 0), 27, 3, 1.0, 'end', 'cls'),          # (npos filled in below: END_NPOS)
    LossCase('palette', 3, 1025, 21, 300, 17, 3, 0.5, 'kneg', 'cls'),
    LossCase('palette', 3, 63, 2, 0, 18, 3, 1.0, 'k0', 'both'),
    LossCase('all_equal', 3, 1025, 21, 255, 19, 3, 1.0, 'end', 'both'),             # 4 * 255 = 1025 - N_IGN
    LossCase('all_equal', 3, 2500, 21, 400, 20, 3, 1.0, 'inside', 'cls'),           # k = 1200: the tickets run out in the second chunk
    LossCase('all_equal', 3, 63, 21, 20, 21, 3, 0.5, 'kneg', 'both'),
    LossCase('all_equal', 3, 2500, 81, 0, 22, 3, 1.0, 'k0', 'noR'),
    LossCase('saturated', 3, 2500, 21, 300, 23, 3, 1.0, 'sat', 'both'),
    LossCase('saturated', 3, 1024, 81, 40, 24, 3, 0.5, 'sat_above', 'noR'),
]
# positives per image at which 3 * npos lands exactly on the end of a palette group (found by `python -m tests.ssd_edges_util end 20`;
# tests/test_ssd_edges_host.py holds the case to it)
END_NPOS = (121, 133, 241)
LOSS_CASES[5] = LOSS_CASES[5]._replace(npos=END_NPOS)
AUTOGRAD_CASES = [LOSS_CASES[i] for i in (0, 2, 8, 12)]      # also run through functional_ssd.SSDLossFn


def loss_id(c):
    n = c.npos if isinstance(c.npos, int) else 'x'.join(map(str, c.npos))
    return f'{c.dist}-A{c.A}-C{c.C1}-p{n}-r{c.ratio}-b{c.beta}-{c.kind}-{c.grads}'


def npos_of(c, b):
    return c.npos if isinstance(c.npos, int) else c.npos[b]


@functools.lru_cache(maxsize=None)
def loss_case(c):
    """float32 CPU inputs of one case.  Every draw has a size that does not depend on npos, so one image's anchors, palette assignment and
    rows stay put when npos changes.  Positives keep their `randn * 2` rows in every distribution."""
    B, A, C1 = c.B, c.A, c.C1
    ncls = C1 - 1
    gc = synth.gen(1000 * c.seed)
    P = 3 + c.seed % 4
    pal = torch.randn(P, C1, generator=gc) * 2
    cls = torch.empty(B, A, C1)
    box, bt = torch.empty(B, A, 4), torch.empty(B, A, 4)
    labels = torch.full((B, A), ncls, dtype=torch.int64)
    lw, bw = torch.ones(B, A), torch.zeros(B, A, 4)
    n_rand = min(20, A // 8)
    for b in range(B):
        g = synth.gen(1000 * c.seed + 1 + b)
        perm = torch.randperm(A, generator=g)
        base = torch.randn(A, C1, generator=g) * 2
        pal_idx = torch.randint(0, P, (A,), generator=g)
        margin = torch.rand(A, generator=g) * 18 + 12
        plab = torch.randint(0, ncls, (A,), generator=g)
        box[b] = torch.randn(A, 4, generator=g)
        bt[b] = torch.randn(A, 4, generator=g) * 1.5
        npos = npos_of(c, b)
        pos, ign = perm[:npos], perm[npos:npos + N_IGN]
        if c.dist == 'random':
            rows = base.clone()
        elif c.dist == 'palette':
            rows = pal[pal_idx].clone()
            fresh = perm[A - n_rand:]
            rows[fresh] = base[fresh]
        elif c.dist == 'saturated':
            rows = base.clone()
            rows[:, ncls] += margin
        elif c.dist == 'all_equal':
            rows = pal[0].expand(A, C1).clone()
        else:
            raise ValueError(c.dist)
        rows[pos] = base[pos]
        cls[b] = rows
        labels[b, pos] = plab[pos]
        lw[b, ign] = 0.0
        bw[b, pos] = 1.0
        # planted box differences on the first positives: d == +beta, d == -beta, d == 0 (sixteenths: exact in float32 and float64)
        for j, a in enumerate(pos[:3].tolist()):
            box[b, a] = (box[b, a] * 16).round() / 16
            bt[b, a] = box[b, a] - torch.tensor([c.beta, -c.beta, 0.0, c.beta])
    return dict(cls=cls, box=box, labels=labels, lw=lw, bt=bt, bw=bw, num_classes=ncls)


def upstream(c):
    """upstream gradients, float32.  |g_cls| + |g_noR| <= 1: the gradient tolerances have an absolute part, which belongs to a coefficient
    of training's size (1 / num_total_pos and 1 / A there), not to an arbitrary one"""
    g = synth.gen(1000 * c.seed + 500)
    g_cls = torch.rand(c.B, generator=g) * 0.4 + 0.1
    g_box = torch.rand(c.B, generator=g) * 0.4 + 0.1
    g_noR = torch.rand(c.B, c.A, generator=g) - 0.5
    return {'cls': (g_cls, g_box, None), 'noR': (None, None, g_noR), 'both': (g_cls, g_box, g_noR)}[c.grads]


def ce_atol(c):
    """one float32 ulp at the case's largest |logit|: the kernel forms (logf(s) + m) - x[label], two roundings at that magnitude"""
    return float(np.spacing(np.float32(loss_case(c)['cls'].abs().max())))


def _ce(x, labels, lw):
    m = x.max(-1, keepdim=True).values
    lse = (x - m).exp().sum(-1).log() + m[..., 0]
    return (lse - x.gather(-1, labels[..., None])[..., 0]) * lw


def ce_fp32(c):
    """torch-float32 restatement of the kernel's operation order: running max, one running sum over the classes, (log(s) + m - x[l]) * w"""
    d = loss_case(c)
    x = d['cls']
    m = x[..., 0].clone()
    for j in range(1, c.C1):
        m = torch.maximum(m, x[..., j])
    s = torch.zeros_like(m)
    for j in range(c.C1):
        s = s + (x[..., j] - m).exp()
    return (s.log() + m - x.gather(-1, d['labels'][..., None])[..., 0]) * d['lw']


def select_stable(ce, labels, num_classes, ratio):
    """The kernel's contract on one image: the k = min(ratio * #pos, #neg) negatives largest by (max(ce, 0) descending, index ascending).
    ce: 1-D numpy array (float32 or float64).  Returns the selected negatives as a bool mask and the counts around the threshold."""
    ce = np.maximum(np.asarray(ce), 0)
    labels = np.asarray(labels)
    neg = np.flatnonzero(labels == num_classes)
    npos = int(((labels >= 0) & (labels < num_classes)).sum())
    k = min(ratio * npos, len(neg))
    mask = np.zeros(len(ce), bool)
    out = dict(mask=mask, k=k, npos=npos, nneg=len(neg), thr=None, above=0, at=0, gap=np.inf)
    if k == 0:
        return out
    v = ce[neg]
    order = np.argsort(-v, kind='stable')
    mask[neg[order[:k]]] = True
    thr = v[order[k - 1]]
    other = v[v != thr]
    out.update(thr=thr, above=int((v > thr).sum()), at=int((v == thr).sum()), gap=float(np.abs(other - thr).min()) if len(other) else np.inf)
    return out


def kind_of(s):
    """which of the four places k takes in the selection `s` of one image"""
    if s['k'] == 0:
        return 'k0'
    if s['k'] == s['nneg']:
        return 'kneg'
    return 'end' if s['k'] == s['above'] + s['at'] else 'inside'


def smooth_l1(d, beta):
    ad = d.abs()
    return torch.where(ad < beta, 0.5 * d * d / beta, ad - 0.5 * beta)


@functools.lru_cache(maxsize=None)
def loss_reference(c):
    """float64 on the float32 inputs: ce [B, A], the per-image selections, (cls_sum, box_sum, mean ce) [B, 3]"""
    d = loss_case(c)
    ce = _ce(d['cls'].double(), d['labels'], d['lw'].double())
    sel = [select_stable(ce[b].numpy(), d['labels'][b].numpy(), d['num_classes'], c.ratio) for b in range(c.B)]
    box = (smooth_l1(d['box'].double() - d['bt'].double(), c.beta) * d['bw'].double()).sum((1, 2))
    pos = d['labels'] < d['num_classes']
    cls_sum = torch.stack([ce[b][pos[b]].sum() + ce[b][torch.from_numpy(sel[b]['mask'])].sum() for b in range(c.B)])
    return dict(ce=ce, sel=sel, sums=torch.stack([cls_sum, box, ce.mean(1)], 1))


def loss_grads(c, selected, g_cls, g_box, g_noR):
    """float64 gradients as the kernel header states them: d/dlogits of g_cls[b] * (ce of positives and of the `selected` negatives)
    + g_noR[b][a] * ce[a], d/dpred of g_box[b] * smooth_l1 * w.  selected: bool [B, A]"""
    d = loss_case(c)
    x = d['cls'].double()
    pos = d['labels'] < d['num_classes']
    coef = torch.zeros(c.B, c.A, dtype=torch.float64)
    if g_cls is not None:
        coef += (pos | selected).double() * g_cls.double()[:, None]
    if g_noR is not None:
        coef += g_noR.double()
    coef *= d['lw'].double()
    gl = coef[..., None] * (F.softmax(x, -1) - F.one_hot(d['labels'], c.C1).double())
    diff = d['box'].double() - d['bt'].double()
    gsl = torch.where(diff.abs() < c.beta, diff / c.beta, diff.sign())
    gb = gsl * d['bw'].double() * (g_box.double()[:, None, None] if g_box is not None else 0.0)
    return gl, gb


# ---------------------------------------------------------------- section 2: generic max-pool with real ties
POOL_DISTS = ('relu', 'const', 'half', 'randn')
POOL_TIE_DISTS = ('relu', 'const', 'half')
# (k, s, p, ceil, B, C, H, W)
POOL_GEOMS = [
    (2, 2, 0, True, 1, 64, 75, 75),         # SSD's ceil-mode pools on odd sizes: the last window is clipped
    (2, 2, 0, True, 3, 128, 5, 5),
    (2, 2, 0, True, 1, 64, 1, 1),
    (2, 2, 0, True, 3, 64, 7, 11),
    (3, 1, 1, False, 3, 64, 19, 19),        # pool5
    (3, 1, 1, False, 1, 128, 1, 7),         # the kernel is larger than the image
    (3, 1, 1, False, 3, 64, 2, 5),
    (3, 2, 1, False, 1, 64, 11, 14),
    (3, 2, 1, False, 3, 128, 6, 9),
    (2, 2, 0, False, 3, 64, 7, 5),          # the last row and column never enter a window
    (2, 2, 0, False, 1, 128, 9, 9),
]
# 1 081 600 vectors forward and backward: above the 4096 x 256 and the 2048 x 256 thread caps of both layouts' launches
POOL_BIG = (3, 1, 1, False, 2, 64, 260, 260)
POOL_CAPS = (4096 * 256, 2048 * 256)


def pool_id(geom):
    k, s, p, ceil, B, C, H, W = geom
    return f'k{k}s{s}p{p}{"c" if ceil else "f"}-B{B}-C{C}-{H}x{W}'


@functools.lru_cache(maxsize=4)
def pool_reference(dist, geom):
    """x (bf16-representable), integer upstream gradient in [-8, 8], and F.max_pool2d / its gradient in float64 on the CPU, which routes
    to the first maximum in scan order.  All four are float64 NCHW."""
    k, s, p, ceil, B, C, H, W = geom
    g = synth.gen(3000 + 7 * POOL_DISTS.index(dist) + 31 * H + W + C + k + s)
    x = torch.randn(B, C, H, W, generator=g)
    if dist == 'relu':
        x = x.bfloat16().float().relu()
    elif dist == 'const':
        x = torch.full_like(x, 0.75)
    elif dist == 'half':
        x = (x * 2).round() / 2
    else:
        x = x.bfloat16().float()
    x = x.double().requires_grad_(True)
    y = F.max_pool2d(x, k, s, p, ceil_mode=ceil)
    go = torch.randint(-8, 9, y.shape, generator=g).double()
    y.backward(go)
    return x.detach(), go, y.detach(), x.grad


def pool_tie_windows(x, y, geom):
    """number of windows per (b, c, oy, ox) positions whose maximum occurs more than once"""
    k, s, p, ceil, B, C, H, W = geom
    OH, OW = y.shape[2:]
    xp = F.pad(x, (p, max(0, (OW - 1) * s + k - W - p), p, max(0, (OH - 1) * s + k - H - p)), value=-np.inf)
    cnt = torch.zeros_like(y)
    for dy in range(k):
        for dx in range(k):
            cnt += xp[:, :, dy:dy + (OH - 1) * s + 1:s, dx:dx + (OW - 1) * s + 1:s] == y
    assert bool((cnt >= 1).all())
    return int((cnt > 1).sum())


# ---------------------------------------------------------------- section 3: L2Norm
L2_ROWS = 3 * 19 * 23            # not a multiple of the four rows of a block
L2_C = (64, 512, 1024)           # 1024: the second lane trip of the X-layout kernel (128 octets over 64 lanes)
L2_EPS = 1e-10
L2_ZERO_ROWS = (0, 5, 6, 7, 1000, L2_ROWS - 1)       # a whole block's worth of neighbours, the first and the last row
L2_FWD_BOUND = {'bf16': 8e-3, 'x3': 2e-5}            # of the output's scale: tests/test_gpu_ssd.py, test_x3_ssd_row_kernels_against_fp32
L2_GX_BOUND = {'bf16': 1e-2, 'x3': 5e-5}             # (same two tests, backward)
L2_GW_BOUND = {'bf16': 2e-3, 'x3': 5e-5}
# a value "rounded to the layout": the unit roundoff of bf16's 8 significant bits (half an ulp, 2^-8); the tail is rounded the same way
# relative to a remainder of at most 2^-8 of the value, so head + tail leave 2^-16
L2_ROUND = {'bf16': 2.0 ** -8, 'x3': 2.0 ** -16}


def x_representable(t):
    """float32 values that an X-layout row holds exactly: head = bf16(v), tail = bf16(v - head)"""
    h = t.bfloat16().float()
    return h + (t - h).bfloat16().float()


@functools.lru_cache(maxsize=None)
def l2_case(C, layout, zeros=False):
    """float32 rows [L2_ROWS, C] exact in the layout, weight [C], upstream gradient rows (exact in the layout as well)"""
    g = synth.gen(4000 + C)
    fit = (lambda t: t.bfloat16().float()) if layout == 'bf16' else x_representable
    x = fit(torch.randn(L2_ROWS, C, generator=g) * 3)
    w = torch.rand(C, generator=g) * 10 + 15
    go = fit(torch.randn(L2_ROWS, C, generator=g))
    if zeros:
        x = x.clone()
        x[list(L2_ZERO_ROWS)] = 0.0
    return x, w, go


def l2_reference(x, w, go, eps=L2_EPS):
    """float64 closed forms with the kernels' zero-norm contract: y = w x / (|x| + eps); gx = w g / n - k x with k = <w g, x> / (n^2 |x|),
    k = 0 where |x| = 0; gw = sum over rows of g x / n"""
    x, w, go = x.double(), w.double(), go.double()
    eps = float(np.float32(eps))
    nrm = x.pow(2).sum(1, keepdim=True).sqrt()
    n = nrm + eps
    y = w * x / n
    dot = (w * go * x).sum(1, keepdim=True)
    k = torch.where(nrm > 0, dot / (n * n * nrm.clamp_min(1e-300)), torch.zeros_like(nrm))
    return y, w * go / n - k * x, (go * x / n).sum(0)


def _find_end_npos(tries):
    """search, per image, the positives count at which ratio * npos lands on the end of a palette group of LOSS_CASES[5]"""
    c0, found = LOSS_CASES[5], []
    for b in range(c0.B):
        for n in range(20, 20 + tries * 40):
            c = c0._replace(npos=tuple(n if i == b else 30 for i in range(c0.B)))
            s = loss_reference(c)['sel'][b]
            if kind_of(s) == 'end' and s['gap'] >= 4 * MIN_GAP:
                found.append(n)
                break
        else:
            found.append(None)
    return tuple(found)


if __name__ == '__main__':
    import sys
    if sys.argv[1:2] == ['end']:
        print('END_NPOS =', _find_end_npos(int(sys.argv[2])))
