"""IoU / GIoU box forms of the fused focal + box loss kernels on the GPU: the kernels against the float64 oracle of
tests/iou_loss_util.py in the anchor-normalised frame on the same fp32 operands, the bit identities between the launch forms, the heads
against the reference's own numbers (tests/golden/iou_box_loss.npz), and whole training iterations with GIoU.

Kernel tolerance, per case: max_row |kernel - float64| <= 4 * max_row |float32 oracle - float64| + 2^-22, for the row loss and for each
gradient component.  The float32 oracle is the same torch code evaluated in fp32 on the CPU; the factor covers a different operation order
and transcendentals that differ from libm's in the last place.  Both maxima are printed (measured on an MI355X: the kernel's maxima are
between 1 and 2.4 times the float32 oracle's, at most 9.2e-7 on a gradient of 5.0)."""
import math
import os

import numpy as np
import pytest
import torch

from tests import iou_loss_util as IU
from tests import plain_retina_util as PU
from tests import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 9
LEVEL_ROWS = (300, 70)          # partial last blocks under 256-row (C <= 24) and 64-row (C > 24) blocks
ROWS = sum(LEVEL_ROWS)
# every product and sum of the decode is exact in fp32 AND in float64 for the hand-built rows (powers of two, short mantissas): a tie the
# kernel sees is a tie the float64 oracle sees
MEANS, STDS, CLIP = (0.25, -0.125, 0.5, -0.25), (0.125, 0.5, 0.25, 0.25), 0.25
R = IU.max_ratio_f32(CLIP)      # ln 4 as fp32: sizes stay in [1/4, 4] anchor units
CODER = (MEANS, STDS, CLIP)
EPS = 1e-6


@pytest.fixture(scope='module')
def ho():
    from aod_meh_hua_amd import hipops
    return hipops


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.int16)


def _deltas(t):
    """t-space (centre x, centre y, log w, log h) float64 [n, 4] -> fp32 deltas"""
    return ((t - torch.tensor(MEANS, dtype=torch.float64)) / torch.tensor(STDS, dtype=torch.float64)).float()


def _hand_rows():
    """(pred t, target t, name) in t-space; every value a short binary fraction, R and its neighbour included (t - mean is exact for them)"""
    r_in = float(np.nextafter(np.float32(R), np.float32(0)))
    rows = [
        ((-3.0, 0.0, 0.0, 0.0), (3.0, 0.0, 0.0, 0.0), 'disjoint in x'),
        ((0.0, 2.5, 0.5, -0.5), (0.25, -2.5, 0.0, 0.5), 'disjoint in y'),
        ((-0.5, 0.0, 0.0, 0.0), (0.5, 0.0, 0.0, 0.0), 'touching on a vertical edge: intersection width exactly 0'),
        ((0.0, 1.0, 0.0, 0.0), (0.25, 0.0, 0.0, 0.0), 'touching on a horizontal edge'),
        ((0.125, -0.125, -0.75, -0.5), (0.0, 0.0, 0.5, 0.75), 'prediction inside target'),
        ((0.0, 0.0, 0.75, 0.5), (0.125, 0.0625, -0.5, -0.75), 'target inside prediction'),
        ((0.25, -0.5, 0.5, -0.25), (0.25, -0.5, 0.5, -0.25), 'prediction equal to target: every max / min tied'),
        ((0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), 'equal unit boxes'),
        ((0.0, 0.0, 0.0, 0.5), (0.0, 0.0, 0.0, -0.5), 'same x extent (x ties), nested in y'),
        ((0.25, 0.0, r_in, 0.0), (0.0, 0.0, 1.0, 0.0), 'log w just inside +R'),
        ((0.25, 0.0, R, 0.0), (0.0, 0.0, 1.0, 0.0), 'log w exactly +R'),
        ((0.25, 0.0, 2.25, 0.0), (0.0, 0.0, 1.0, 0.0), 'log w beyond +R'),
        ((0.0, 0.125, 0.0, -r_in), (0.0, 0.0, 0.0, -1.0), 'log h just inside -R'),
        ((0.0, 0.125, 0.0, -R), (0.0, 0.0, 0.0, -1.0), 'log h exactly -R'),
        ((0.0, 0.125, 0.0, -2.25), (0.0, 0.0, 0.0, -1.0), 'log h beyond -R'),
        ((0.125, 0.0, R, R), (0.0, 0.0, R, R), 'both sizes at +R, target too'),
        ((0.0, 0.0, -R, -R), (0.0625, 0.0, -R, -R), 'both sizes at -R, target too'),
        # a 1/4 box on the corner of a 4 box, 2^-9 into it on both axes: IoU = 2^-18 / (16 + 1/16 - 2^-18) < 1e-6
        ((2.125 - 2.0 ** -9, 2.125 - 2.0 ** -9, -R, -R), (0.0, 0.0, R, R), 'IoU below eps'),
    ]
    p = torch.tensor([r[0] for r in rows], dtype=torch.float64)
    t = torch.tensor([r[1] for r in rows], dtype=torch.float64)
    return p, t, [r[2] for r in rows]


_CASES = {}


def _case(C):
    """labels / logits / weights / deltas of the two levels (fp32, CPU): the hand-built rows, ~10 % random positives (a few with weight 1/2),
    every other row weight 0 with finite random deltas"""
    if C in _CASES:
        return _CASES[C]
    g = torch.Generator().manual_seed(700 + C)
    cls = (torch.rand(ROWS, C, generator=g) * 8 - 4).float()
    labels = torch.randint(0, C + 1, (ROWS,), generator=g)
    lw = (torch.rand(ROWS, generator=g) > 0.1).float()
    hp, ht, names = _hand_rows()
    n_hand = hp.shape[0]
    tp = torch.cat([torch.randn(ROWS, 2, generator=g, dtype=torch.float64) * 0.3, (torch.rand(ROWS, 2, generator=g, dtype=torch.float64) * 2 - 1) * 0.98 * R], 1)
    tt = torch.cat([torch.randn(ROWS, 2, generator=g, dtype=torch.float64) * 0.3, (torch.rand(ROWS, 2, generator=g, dtype=torch.float64) * 2 - 1) * 0.98 * R], 1)
    w = (torch.rand(ROWS, generator=g) < 0.10).float()
    w[torch.rand(ROWS, generator=g) < 0.02] = 0.5
    # the hand-built rows: half behind the start of level 0, half around the boundary of the ragged last blocks of level 1
    where = list(range(3, 3 + n_hand // 2)) + list(range(ROWS - (n_hand - n_hand // 2), ROWS))
    tp[where], tt[where], w[where] = hp, ht, 1.0
    w[[0, 255, 256, 299, 300]] = 1.0                     # block and level boundaries carry a live row
    bp, bt = _deltas(tp), _deltas(tt)
    hand_exact = torch.equal(bp[where].double() * torch.tensor(STDS, dtype=torch.float64) + torch.tensor(MEANS, dtype=torch.float64), hp)
    assert hand_exact, 'the hand-built rows must decode exactly'
    bw = w[:, None].expand(-1, 4).contiguous()
    _CASES[C] = dict(cls=cls, labels=labels, lw=lw, bp=bp, bt=bt, bw=bw, w=w, where=where, names=names)
    return _CASES[C]


def _dev(c, **over):
    d = {k: v.cuda() for k, v in c.items() if torch.is_tensor(v)}
    d.update({k: v.cuda() for k, v in over.items()})
    return d


def _kw(form, focal):
    box, linear = IU.split_form(form)
    return dict(form=focal, box_form=box, box_eps=EPS, box_linear=linear, coder=CODER)


def _oracle(c, form, dtype):
    box, linear = IU.split_form(form)
    loss, grad, iou = IU.rows(c['bp'], c['bt'], box, EPS, linear, MEANS, STDS, R, dtype=dtype)
    live = c['w'] != 0
    w = c['w'].to(dtype)
    return (loss * w).double()[live], (grad * w[:, None]).double()[live], iou.double()[live]


def _row_losses(ho, d, rows, kw):
    """w * l of single rows: one-row launches, whose second sum is that row's term exactly"""
    out = []
    for r in rows:
        s = slice(r, r + 1)
        _, sums = ho.edl_focal_l1_fwd(d['cls'][s], d['labels'][s], d['lw'][s], d['bp'][s], d['bt'][s], d['bw'][s], **kw)
        out.append(sums[1:2])
    return torch.cat(out).double().cpu()


def _grad_bufs(rows, C, dtype=torch.float32, pitch_c=None, pitch_b=None):
    """[ceil(rows / A), pitch] buffers: 300 and 70 rows are no multiples of A = 9, the last pixel is partly used"""
    px = -(-rows // A)
    return (torch.zeros(px, pitch_c or A * C, dtype=dtype, device='cuda'), torch.zeros(px, pitch_b or A * 4, dtype=dtype, device='cuda'))


def _unpitch(buf, rows, width, pitch):
    """[pixels, pitch] -> [rows, width]: element (r, c) lives at (r // A) * pitch + (r % A) * width + c"""
    return buf[:, :A * width].reshape(-1, width)[:rows]


@pytest.mark.parametrize('form', IU.FORMS)
@pytest.mark.parametrize('focal', ['edl', 'sigmoid'])
@pytest.mark.parametrize('C', [20, 80])
def test_kernels_against_the_float64_oracle_and_launch_forms_agree(ho, C, focal, form):
    c = _case(C)
    d = _dev(c)
    kw = _kw(form, focal)
    live = (c['w'] != 0).nonzero().squeeze(1).tolist()
    assert 0.08 * ROWS < len(live) < 0.25 * ROWS and set(c['where']) <= set(live)
    # ---- forward: per-level launches, the level-fused launch, single rows
    lv, r0 = [], 0
    for n in LEVEL_ROWS:
        s = slice(r0, r0 + n)
        lv.append(ho.edl_focal_l1_fwd(d['cls'][s], d['labels'][s], d['lw'][s], d['bp'][s], d['bt'][s], d['bw'][s], **kw))
        r0 += n
    noR, sums = ho.edl_focal_l1_levels_fwd(d['cls'], d['labels'], d['lw'], d['bp'], d['bt'], d['bw'], list(LEVEL_ROWS), **kw)
    assert torch.equal(_bits(noR), _bits(torch.cat([p[0] for p in lv]))) and torch.equal(_bits(sums), _bits(torch.stack([p[1] for p in lv], 1)))
    # (the focal rows do not depend on the box form: those of the L1 launch)
    noR_l1, sums_l1 = ho.edl_focal_l1_levels_fwd(d['cls'], d['labels'], d['lw'], d['bp'], d['bt'], d['bw'], list(LEVEL_ROWS), form=focal)
    assert torch.equal(_bits(noR), _bits(noR_l1)) and torch.equal(_bits(sums[[0, 2]]), _bits(sums_l1[[0, 2]]))
    l64, g64, iou64 = _oracle(c, form, torch.float64)
    l32, g32, _ = _oracle(c, form, torch.float32)
    got_l = _row_losses(ho, d, live, kw)
    e_k, e_o = float((got_l - l64).abs().max()), float((l32 - l64).abs().max())
    print(f'C={C} {focal} {form}: {len(live)} live rows, IoU in [{float(iou64.min()):.3g}, {float(iou64.max()):.6g}]')
    print(f'    row loss: kernel max err {e_k:.3e}, float32 oracle max err {e_o:.3e}, max |l| {float(l64.abs().max()):.3f}')
    assert e_k <= 4 * e_o + 2.0 ** -22
    # the level sums are the sums of those rows
    r0 = 0
    for l, n in enumerate(LEVEL_ROWS):
        m = torch.tensor([r0 <= r < r0 + n for r in live])
        want = float(l64[m].sum())
        assert abs(float(sums[1, l]) - want) <= 2e-5 * abs(want), (l, float(sums[1, l]), want)
        r0 += n
    # ---- backward: per-level launches (A = 1, flat rows), the level-fused launch (A = 9), the divided form
    gsum = torch.tensor([[0.5, 0.25], [1.0, 1.0], [0.0, 0.0]], device='cuda')
    one = torch.ones(1, device='cuda')
    per_c, per_b, r0 = [], [], 0
    for l, n in enumerate(LEVEL_ROWS):
        s = slice(r0, r0 + n)
        gc, gb = ho.edl_focal_l1_bwd(d['cls'][s], d['labels'][s], d['lw'][s], d['bp'][s], d['bt'][s], d['bw'][s], gsum[0, l:l + 1].contiguous(), one, None, 0.0, **kw)
        per_c.append(gc), per_b.append(gb)
        r0 += n
    gc, gb = _grad_bufs(ROWS, C)
    ho.edl_focal_l1_levels_bwd(d['cls'], d['labels'], d['lw'], d['bp'], d['bt'], d['bw'], list(LEVEL_ROWS), gsum, None, gc, gb, A, **kw)
    gc_rows, gb_rows = gc.view(-1)[:ROWS * C].view(ROWS, C), gb.view(-1)[:ROWS * 4].view(ROWS, 4)
    assert torch.equal(_bits(gc_rows), _bits(torch.cat(per_c))) and torch.equal(_bits(gb_rows), _bits(torch.cat(per_b)))
    got_g = gb_rows.double().cpu()
    dead = c['w'] == 0
    assert not _bits(gb_rows.cpu()[dead]).any()                                # +0 in every component of every zero-weight row
    for j in range(4):
        e_k, e_o = float((got_g[~dead][:, j] - g64[:, j]).abs().max()), float((g32[:, j] - g64[:, j]).abs().max())
        print(f'    grad[{j}]: kernel max err {e_k:.3e}, float32 oracle max err {e_o:.3e}, max |g| {float(g64[:, j].abs().max()):.3f}')
        assert e_k <= 4 * e_o + 2.0 ** -22
    # g_div: the backward divides the upstream gradients by the forward's divisors itself == dividing upstream
    num_pos = torch.tensor([5, 0, 2], dtype=torch.int32, device='cuda')
    noR2, q, div, nt = ho.edl_focal_l1_levels_fwd(d['cls'], d['labels'], d['lw'], d['bp'], d['bt'], d['bw'], list(LEVEL_ROWS), num_pos=num_pos, **kw)
    assert float(nt) == 8.0 and torch.equal(_bits(q), _bits(sums / div)) and torch.equal(_bits(noR2), _bits(noR))
    gup = torch.tensor([[0.7, 0.3], [1.3, 0.9], [0.0, 0.0]], device='cuda')
    gc2, gb2 = _grad_bufs(ROWS, C)
    ho.edl_focal_l1_levels_bwd(d['cls'], d['labels'], d['lw'], d['bp'], d['bt'], d['bw'], list(LEVEL_ROWS), gup, None, gc2, gb2, A, divisors=div, **kw)
    gc3, gb3 = _grad_bufs(ROWS, C)
    ho.edl_focal_l1_levels_bwd(d['cls'], d['labels'], d['lw'], d['bp'], d['bt'], d['bw'], list(LEVEL_ROWS), (gup / div).contiguous(), None, gc3, gb3, A, **kw)
    assert torch.equal(_bits(gc2), _bits(gc3)) and torch.equal(_bits(gb2), _bits(gb3)) and bool(gb2.any())
    # ---- bf16 store in the prediction conv's padded dZ layout == the fp32 store rounded
    n0 = LEVEL_ROWS[0]
    s = slice(0, n0)
    pc, pb = (A * C + 7) // 8 * 8 + 8, 40
    args = (d['cls'][s], d['labels'][s], d['lw'][s], d['bp'][s], d['bt'][s], d['bw'][s], gsum[0, :1].contiguous(), one, None, 0.0)
    c32, b32 = _grad_bufs(n0, C, torch.float32, pc, pb)
    c16, b16 = _grad_bufs(n0, C, torch.bfloat16, pc, pb)
    ho.edl_focal_l1_bwd(*args, A=A, pitch_cls=pc, pitch_box=pb, grad_cls=c32, grad_bbox=b32, **kw)
    ho.edl_focal_l1_bwd(*args, out_bf16=True, A=A, pitch_cls=pc, pitch_box=pb, grad_cls=c16, grad_bbox=b16, **kw)
    assert torch.equal(_bits(_unpitch(b32, n0, 4, pb)), _bits(per_b[0])) and torch.equal(_bits(_unpitch(c32, n0, C, pc)), _bits(per_c[0]))
    assert torch.equal(_bits(b16), _bits(b32.bfloat16())) and torch.equal(_bits(c16), _bits(c32.bfloat16()))
    assert not b32[:, A * 4:].any() and not c32[:, A * C:].any()
    torch.cuda.synchronize()


@pytest.mark.parametrize('form', IU.FORMS)
@pytest.mark.parametrize('C', [20, 80])
def test_zero_weight_rows_are_skipped_whatever_they_hold(ho, C, form):
    """1e30, inf and NaN in the deltas of the zero-weight rows (prediction and target): the sums are the bits of the same case with those rows
    zeroed, the live gradient rows too, and the rows themselves get +0"""
    c = _case(C)
    dead = (c['w'] == 0).nonzero().squeeze(1)
    fill = torch.tensor([1e30, float('inf'), float('nan'), -float('inf'), -1e30])[torch.arange(dead.numel() * 4) % 5].view(-1, 4)
    kw = _kw(form, 'sigmoid')
    outs = []
    for bad in (False, True):
        bp, bt = c['bp'].clone(), c['bt'].clone()
        bp[dead], bt[dead] = (fill, fill.flip(0)) if bad else (torch.zeros_like(fill), torch.zeros_like(fill))
        d = _dev(c, bp=bp, bt=bt)
        noR, sums = ho.edl_focal_l1_levels_fwd(d['cls'], d['labels'], d['lw'], d['bp'], d['bt'], d['bw'], list(LEVEL_ROWS), **kw)
        gc, gb = _grad_bufs(ROWS, C)
        gs = torch.tensor([[1.0, 1.0], [0.75, 1.5], [0.0, 0.0]], device='cuda')
        ho.edl_focal_l1_levels_bwd(d['cls'], d['labels'], d['lw'], d['bp'], d['bt'], d['bw'], list(LEVEL_ROWS), gs, None, gc, gb, A, **kw)
        outs.append((sums.cpu(), gb.view(-1)[:ROWS * 4].view(ROWS, 4).cpu(), gc.cpu()))
    (s0, b0, c0), (s1, b1, c1) = outs
    assert bool(torch.isfinite(s1).all()) and float(s1[1].abs().min()) > 0
    assert torch.equal(_bits(s0), _bits(s1)) and torch.equal(_bits(b0), _bits(b1)) and torch.equal(_bits(c0), _bits(c1))
    assert not _bits(b1[dead]).any() and bool(b1.any())


@pytest.mark.parametrize('focal', ['edl', 'sigmoid'])
@pytest.mark.parametrize('C', [20, 80])
def test_new_entries_with_box_form_l1_return_the_bits_of_the_old_entries(ho, C, focal):
    """aod_focal_box_*_ex(box form 0) against aod_{edl,sigmoid}_focal_l1_*: sums, rows and both gradients (the coder is not read: NULL)"""
    import ctypes as ct
    from aod_meh_hua_amd import _C
    c = _case(C)
    d = _dev(c)
    ptr, st = _C.ptr, _C.stream
    ff = ho.FOCAL_FORM_IDS[focal]
    lr = ho._level_rows(LEVEL_ROWS)
    L = len(LEVEL_ROWS)
    noR0, sums0 = ho.edl_focal_l1_levels_fwd(d['cls'], d['labels'], d['lw'], d['bp'], d['bt'], d['bw'], list(LEVEL_ROWS), form=focal)
    noR1, sums1 = torch.empty_like(noR0), torch.empty_like(sums0)
    part = torch.empty(int(_C.lib.aod_loss_levels_partials_len(L, lr)), device='cuda')
    _C.call('aod_focal_box_levels_fwd_ex', ff, 0, 0.0, 0, None, None, 0.0, ptr(d['cls']), ptr(d['labels']), ptr(d['lw']), ptr(d['bp']), ptr(d['bt']),
            ptr(d['bw']), L, lr, C, 2.0, 0.25, ptr(noR1), ptr(sums1), ptr(part), None, 0, None, None, st())
    assert torch.equal(_bits(noR0), _bits(noR1)) and torch.equal(_bits(sums0), _bits(sums1))
    gs = torch.tensor([[0.5, 0.25], [1.0, 2.0], [0.125, 0.0]], device='cuda')
    (c0, b0), (c1, b1) = _grad_bufs(ROWS, C), _grad_bufs(ROWS, C)
    ho.edl_focal_l1_levels_bwd(d['cls'], d['labels'], d['lw'], d['bp'], d['bt'], d['bw'], list(LEVEL_ROWS), gs, None, c0, b0, A, form=focal)
    _C.call('aod_focal_box_levels_bwd_ex', ff, 0, 0.0, 0, None, None, 0.0, ptr(d['cls']), ptr(d['labels']), ptr(d['lw']), ptr(d['bp']), ptr(d['bt']),
            ptr(d['bw']), L, lr, C, 2.0, 0.25, ptr(gs), None, None, ptr(c1), ptr(b1), 0, A, A * C, A * 4, st())
    assert torch.equal(_bits(c0), _bits(c1)) and torch.equal(_bits(b0), _bits(b1)) and bool(b0.any())
    # the single-level entries, on level 1 (70 rows)
    s = slice(LEVEL_ROWS[0], ROWS)
    n = LEVEL_ROWS[1]
    x = {k: d[k][s] for k in ('cls', 'labels', 'lw', 'bp', 'bt', 'bw')}
    noR0, sums0 = ho.edl_focal_l1_fwd(x['cls'], x['labels'], x['lw'], x['bp'], x['bt'], x['bw'], form=focal)
    noR1, sums1 = torch.empty_like(noR0), torch.zeros(3, device='cuda')
    part = torch.empty(int(_C.lib.aod_loss_partials_len(n)), device='cuda')
    _C.call('aod_focal_box_fwd_ex', ff, 0, 0.0, 0, None, None, 0.0, ptr(x['cls']), ptr(x['labels']), ptr(x['lw']), ptr(x['bp']), ptr(x['bt']), ptr(x['bw']),
            n, C, 2.0, 0.25, ptr(noR1), ptr(sums1), ptr(part), st())
    assert torch.equal(_bits(noR0), _bits(noR1)) and torch.equal(_bits(sums0), _bits(sums1))
    g1, g2 = torch.full((1,), 0.5, device='cuda'), torch.full((1,), 2.0, device='cuda')
    c0, b0 = ho.edl_focal_l1_bwd(x['cls'], x['labels'], x['lw'], x['bp'], x['bt'], x['bw'], g1, g2, None, 0.25, form=focal)
    c1, b1 = torch.empty_like(c0), torch.empty_like(b0)
    _C.call('aod_focal_box_bwd_ex', ff, 0, 0.0, 0, None, None, 0.0, ptr(x['cls']), ptr(x['labels']), ptr(x['lw']), ptr(x['bp']), ptr(x['bt']), ptr(x['bw']),
            n, C, 2.0, 0.25, ptr(g1), ptr(g2), None, ct.c_float(0.25), 0, ptr(c1), ptr(b1), 0, 1, C, 4, st())
    assert torch.equal(_bits(c0), _bits(c1)) and torch.equal(_bits(b0), _bits(b1))


# ---------------------------------------------------------------------------------------------------------------- the heads
LOSS_CFG = dict(giou=dict(type='GIoULoss', loss_weight=1.0), iou=dict(type='IoULoss'), iou_linear=dict(type='IoULoss', linear=True))


def _head(kind, loss_bbox):
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_head
    name = 'Config_RetinaNet_plain.py' if kind == 'MyRetinaHead' else 'Config_RetinaNet.py'
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_', name))
    hc = dict(cfg.model.bbox_head)
    hc.update(loss_bbox=dict(loss_bbox), reg_decoded_bbox=True, train_cfg=cfg.model.train_cfg, test_cfg=cfg.model.test_cfg)
    return build_head(hc).cuda().train()


def _golden_loss(kind, form, g):
    head = _head(kind, LOSS_CFG[form])
    gen = torch.Generator().manual_seed(9)      # (the box term does not read the logits: seeded ones of the head's own width)
    cls = [torch.randn(PU.B, A * head.cls_out_channels, h, w, generator=gen).cuda() for h, w in PU.LEVELS]
    reg = [torch.from_numpy(g[f'reg{l}']).cuda().requires_grad_(True) for l in range(len(PU.LEVELS))]
    gtb = [torch.from_numpy(g[f'gt_boxes{b}']).cuda() for b in range(PU.B)]
    gtl = [torch.from_numpy(g[f'gt_labels{b}']).cuda() for b in range(PU.B)]
    losses, head_out = head.loss(cls, reg, None, gtb, gtl, synth.metas(PU.B, PU.H, PU.W), Labeled=True, Pseudo=False)
    lb = torch.stack([t.reshape(()) for t in losses['loss_bbox']])
    lb.sum().backward()
    torch.cuda.synchronize()
    assert int(head_out[8]) == int(g['num_total_samples'])
    return lb.detach().cpu(), [r.grad.detach().cpu() for r in reg]


@pytest.mark.parametrize('form', IU.FORMS)
def test_heads_on_the_golden_inputs_against_the_reference_numbers(form):
    """MyRetinaHead: per-level loss_bbox and d sum(loss_bbox) / d bbox_pred against the reference's MyRetinaHead (reg_decoded_bbox=True).
    Tolerance: the project's per-row loss tolerance (rtol 2e-5, losses.hip) on the level sums, 2e-5 * max |grad| on the gradients.
    Lambda_L2Net on the same box maps: the same loss_bbox bits -- the heads share the box code."""
    g = np.load(IU.GOLDEN)
    lb, grads = _golden_loss('MyRetinaHead', form, g)
    want = g[f'loss_bbox_{form}']
    print(form, 'loss_bbox', lb.tolist(), 'reference', want.tolist())
    np.testing.assert_allclose(lb.numpy(), want, rtol=2e-5, atol=0)
    for l in range(len(PU.LEVELS)):
        w = g[f'grad_reg{l}_{form}']
        err = float(np.abs(grads[l].numpy() - w).max())
        print(f'    level {l}: max |grad| {np.abs(w).max():.4g}, max err {err:.3e}')
        assert err <= 2e-5 * float(np.abs(w).max())
    lb2, grads2 = _golden_loss('Lambda_L2Net', form, g)
    assert torch.equal(_bits(lb), _bits(lb2)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, grads2))


KINDS = ('SSL_L_RetinaNet', 'MyRetinaNet')
CD = dict(xi=0.6, momentum=0.99, alpha=0.3, beta=0.2)


def _build_train(kind, tracked=False, lr=2e-4, loss_weight=1.0, seeded=True):
    from aod_meh_hua_amd.apis.train_Lambda import build_optimizers
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    from oracle import model as om
    config, sd = {'SSL_L_RetinaNet': ('configs/_base_/Config_RetinaNet.py', lambda: om.seeded_state_dict(cls_bias=-2.0)),
                  'MyRetinaNet': ('configs/_base_/Config_RetinaNet_plain.py', lambda: PU.plain_state_dict(cls_bias=-2.0))}[kind]
    cfg = Config.fromfile(os.path.join(ROOT, config))
    cfg.model.backbone.pop('init_cfg', None)
    cfg.model.bbox_head.loss_bbox = dict(type='GIoULoss', loss_weight=loss_weight)
    cfg.model.bbox_head.reg_decoded_bbox = True
    if tracked:
        cfg.model.bbox_head.class_difficulty = dict(CD)
    model = build_detector(cfg.model)
    assert type(model).__name__ == kind and type(model.bbox_head.loss_bbox).__name__ == 'GIoULoss'
    if seeded:
        model.load_state_dict(sd(), strict=not tracked)
    else:          # the config's own initialisation (Normal std 0.01 heads: deltas near 0, the positives start at their anchors' IoU)
        torch.manual_seed(0)
        model.init_weights()
    model = model.cuda().train()
    cfg.optimizer.lr = lr
    opt, opt_L = build_optimizers(model, cfg)
    return model, cfg, opt, opt_L


def _batch(seed, B=2, H=128):
    gtb, gtl = synth.random_gts(B, H, H, seed=seed, gmin=1, gmax=3)
    return dict(img=synth.images(B, H, H, seed=seed).cuda(), img_metas=synth.metas(B, H, H), gt_bboxes=[b.cuda() for b in gtb],
                gt_labels=[l.cuda() for l in gtl])


def _eager_iteration(model, opt, opt_L, d):
    out, head_out, feat_out, prev = model.train_step(d, Labeled=True, Pseudo=False)
    opt.zero_grad()
    out['loss'].backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    opt.step()
    if opt_L is not None:
        lossL = model.train_step_L(prev, head_out, feat_out)
        opt_L.zero_grad()
        lossL['loss'].backward()
        opt_L.step()
    return {k: float(v) for k, v in out['log_vars'].items()}, grads, head_out


def _iterations(kind, graphed, tracked=False, seeds=(41, 42)):
    model, cfg, opt, opt_L = _build_train(kind, tracked)
    logs = []
    gs = None
    if graphed:
        from aod_meh_hua_amd.graphs import GraphedTrainStep
        gs = GraphedTrainStep(model, opt, opt_L, warmup=1, Labeled=True, Pseudo=False)
    for seed in seeds:
        d = _batch(seed)
        if graphed:
            logs.append({k: float(v) for k, v in gs(d)['log_vars'].items()})
        else:
            logs.append(_eager_iteration(model, opt, opt_L, d)[0])
    torch.cuda.synchronize()
    cd = model.bbox_head.class_difficulty.detach().cpu().clone() if tracked else None
    return logs, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, cd


@pytest.mark.parametrize('kind', KINDS)
def test_giou_iterations_eager_and_replayed_are_the_same_bits(kind):
    """deterministic mode (ordered column sums): two iterations eager == the same two replayed from the captured graph -- losses and every
    parameter; with class_difficulty on, the EMA still follows its positives and the losses do not move"""
    from aod_meh_hua_amd import functional as AF
    AF.set_deterministic(True)
    try:
        l_e, sd_e, _ = _iterations(kind, False)
        l_g, sd_g, _ = _iterations(kind, True)
        l_t, sd_t, cd = _iterations(kind, False, tracked=True)
    finally:
        AF.set_deterministic(False)
    print(kind, l_e)
    l_g = [{k: v for k, v in d.items() if k != 'loss_L'} for d in l_g]      # (a replayed iteration logs its MEH half as well)
    assert l_e == l_g and all(math.isfinite(v) for d in l_e for v in d.values()) and l_e[0]['loss_bbox'] > 0
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), ('replayed vs eager', k)
        assert torch.equal(sd_e[k], sd_t[k]), ('tracked vs untracked', k)
    assert l_t == l_e and bool((cd < 1).any()) and bool((cd > 0).all())


@pytest.mark.parametrize('kind', KINDS)
def test_giou_iteration_sparse_and_dense_forward_agree(kind, monkeypatch):
    """AOD_SPARSE_FWD=0 and the default: the rows the sparse forward leaves arbitrary have weight 0 and are skipped by the GIoU form -- same
    loss bits, same prediction-conv weight gradients"""
    from aod_meh_hua_amd import functional as AF
    AF.set_deterministic(True)
    try:
        res = []
        for sparse in ('1', '0'):
            monkeypatch.setenv('AOD_SPARSE_FWD', sparse)
            model, cfg, opt, opt_L = _build_train(kind)
            res.append(_eager_iteration(model, opt, opt_L, _batch(41)))
            torch.cuda.synchronize()
    finally:
        AF.set_deterministic(False)
    (l1, g1, _), (l0, g0, _) = res
    assert l1 == l0, (l1, l0)
    keys = [k for k in g1 if '.retina_reg.' in k or '.retina_cls.' in k]
    assert len(keys) == 4
    for k in keys:
        assert torch.equal(g1[k], g0[k]), k
    assert float(g1['bbox_head.retina_reg.weight'].abs().max()) > 0


def _mean_pos_iou(head, head_out):
    """mean IoU of the positives under the predictions of one iteration: the float64 oracle on that iteration's loss operands (head_out)"""
    bp = torch.cat([b.detach().permute(0, 2, 3, 1).reshape(-1, 4) for b in head_out[2]]).cpu()
    bt = torch.cat([t.reshape(-1, 4) for t in head_out[6]]).cpu()
    bw = torch.cat([t.reshape(-1, 4) for t in head_out[7]]).cpu()
    pos = bw[:, 0] > 0
    assert int(pos.sum()) > 0
    _, _, iou = IU.rows(bp[pos], bt[pos], 'giou', 1e-6, False, tuple(head.bbox_coder.means), tuple(head.bbox_coder.stds))
    return float(iou.mean())


@pytest.mark.parametrize('kind', KINDS)
def test_forty_giou_steps_lower_the_box_loss_and_raise_the_iou(kind):
    """2 images of 128^2, fixed seed, the config's initialisation and learning rate (the oracle's seeded checkpoint has O(1) box deltas and
    class losses in the hundreds: its first steps are ruled by the class term), deterministic mode, GIoULoss(loss_weight=2.0) (the
    per-level launches): loss_bbox after 40 steps is
    below its value at step 0, and so is 1 - mean IoU of the positives (the 41st forward shows the predictions the 40 steps left)"""
    from aod_meh_hua_amd import functional as AF
    torch.manual_seed(0)
    AF.set_deterministic(True)
    try:
        model, cfg, opt, opt_L = _build_train(kind, lr=1e-3, loss_weight=2.0, seeded=False)
        d = _batch(43)
        lb, ious = [], []
        for it in range(41):
            log, _, head_out = _eager_iteration(model, opt, opt_L, d)
            lb.append(log['loss_bbox'])
            if it in (0, 40):
                ious.append(_mean_pos_iou(model.bbox_head, head_out))
        torch.cuda.synchronize()
    finally:
        AF.set_deterministic(False)
    print(f'{kind}: loss_bbox {lb[0]:.4f} -> {lb[40]:.4f}, mean IoU of the positives {ious[0]:.4f} -> {ious[1]:.4f}')
    print('    every step:', [round(v, 4) for v in lb])
    assert all(math.isfinite(v) for v in lb) and lb[40] < lb[0] and ious[1] > ious[0]
