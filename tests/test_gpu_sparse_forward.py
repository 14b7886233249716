"""GPU: the sparse forward of the box-regression and MEH towers (reference-precision mode, training).  loss_bbox = sum |d| * bbox_weights and
the MEH loss ((|lam + 1e-9 - loss|) * bbox_weights[..., 0])^2 read the two towers at positive anchors only, and the assigner knows the positives
before the head runs: a chain of row-activity maps (include/aod_hip.h aod_fwd_row_maps; one byte per 64 pyramid rows) says where the output
of each tower layer is needed, and the paired tower launches skip the 256-row tiles outside it (aod_conv2d_grouped_fwd_map).

Checked here: the chain against a numpy restatement of the block rule and against the exact pixel dilation; the grouped launch with two and with
three members (live tiles: the dense launch's bits; dead tiles: zero rows over a NaN prefill); one whole training iteration and three optimizer
steps with the switch on and off, eagerly and replayed as a graph; a batch without any positive.

"Equal" is torch.equal.  The bias gradients of the default mode are fp32-ATOMIC column sums whose last bit depends on the arrival order of the
workgroups (tests/test_gpu_sparse_backward.py: no two runs share it, dense or not), so the comparison of EVERY gradient and of the updated
parameters runs in the deterministic mode, whose column sums are ordered; the default mode's run holds the bias vectors to the 2e-6 that
suite holds such sums to and everything else to equality."""
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_sparse_backward as sb

pytestmark = pytest.mark.gpu

RAGGED = sb.RAGGED                                   # 2 282 rows: a ragged last block inside a partial last tile, a tile across the segment boundary
PYR3 = (2, ((64, 64), (32, 32), (16, 16)))           # 10 752 rows = 42 tiles of 256
CIN = sb.CIN
A = 9


@pytest.fixture(autouse=True)
def x3_mode(monkeypatch):
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    AF.set_precision('bf16x3')
    monkeypatch.setenv('AOD_SPARSE_FWD', '1')
    monkeypatch.setenv('AOD_SPARSE_BWD', '1')
    monkeypatch.setattr(ho, 'SPLITK', False)
    yield
    AF.set_precision(os.environ.get('AOD_CONV_PREC', 'bf16x3'))


# ------------------------------------------------------------------------------------------------ numpy model of the chain
def _dilate_np(m, B, sizes):
    """the documented block rule of a 3 x 3 / pad 1 conv: block b is 1 when an input block overlaps, segment by segment, the linear range
    [first - W - 1, last + W + 1] of its rows cut to the image rows [y_first - 1, y_last + 1] and to the images the block touches"""
    M = sum(B * h * w for h, w in sizes)
    out = np.zeros_like(m)
    for b in range(len(m)):
        r0, r1 = 64 * b, min(64 * b + 63, M - 1)
        s0 = 0
        for h, w in sizes:
            n = B * h * w
            lo, hi = max(r0, s0) - s0, min(r1, s0 + n - 1) - s0
            if lo <= hi:
                a = max(lo - w - 1, (lo // w - 1) * w, (lo // (h * w)) * h * w)
                z = min(hi + w + 1, (hi // w + 2) * w - 1, (hi // (h * w) + 1) * h * w - 1)
                if m[(s0 + a) // 64:(s0 + z) // 64 + 1].any():
                    out[b] = 1
            s0 += n
    return out


def _chain_np(rows, B, sizes, n):
    M = sum(B * h * w for h, w in sizes)
    maps = [sb._block_map(rows, M)]
    for _ in range(n - 1):
        maps.append(_dilate_np(maps[-1], B, sizes))
    return maps


def _weights(rows, M, dev='cuda'):
    """bbox_weights [M * A, 4] with one weighted anchor per listed pixel row (another anchor and column each time)"""
    bw = torch.zeros(M * A, 4, device=dev)
    for i, r in enumerate(rows):
        bw[A * r + i % A, :] = 1.0
    return bw


def _mid(B, sizes):
    h, w = sizes[0]
    return (h // 2) * w + w // 2                     # the middle pixel of the first image of the largest level


def _edge_rows(B, sizes):
    h0, w0 = sizes[0]
    n0 = B * h0 * w0
    M = sum(B * h * w for h, w in sizes)
    mid = (n0 // 2 // 64) * 64 + 64 * 3
    return sorted({0, h0 * w0 - 1, n0 - 1, n0, M - 1, mid - 1, mid})       # image corners, both sides of the segment and of a block boundary


def _chain_gpu(bw, B, sizes, n):
    from aod_meh_hua_amd import hipops as ho
    segs, M = sb._segs(B, sizes)
    maps = ho.fwd_row_maps(bw, segs, A, ho.xw(CIN), CIN, 3, 3, 1, 1, n)
    torch.cuda.synchronize()
    return maps


@pytest.mark.parametrize('pyramid', [RAGGED, PYR3], ids=['ragged', 'three-levels'])
def test_map_chain_is_the_block_rule_and_covers_the_exact_dilation(pyramid):
    B, sizes = pyramid
    M = sum(B * h * w for h, w in sizes)
    for rows in ([_mid(B, sizes)], _edge_rows(B, sizes), []):
        want = _chain_np(rows, B, sizes, 5)
        if rows == [_mid(B, sizes)]:
            # one positive in the middle of the largest level leaves most of F_1 dead: an all-ones chain cannot pass
            assert want[4].sum() >= 1 and want[4].mean() <= 0.5, want[4].mean()
        got = [m.cpu().numpy() for m in _chain_gpu(_weights(rows, M), B, sizes, 5)]
        exact = set(rows)
        for k in range(5):
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, np.nonzero(got[k] != want[k]))
            assert (got[k] >= sb._block_map(exact, M)).all(), k                 # a superset of the pixel-wise +-k dilation
            exact = sb._exact_dilation(exact, B, sizes)
    # a weight in the LAST column of the LAST anchor of a block's last row, and a negative one, count; -0.0 does not
    bw = torch.zeros(M * A, 4, device='cuda')
    bw[A * 63 + A - 1, 3] = 1e-30
    bw[A * (64 * 5), 0] = -2.0
    bw[A * (64 * 9): A * (64 * 10)] = -0.0
    m0 = _chain_gpu(bw, B, sizes, 1)[0].cpu().numpy()
    assert sorted(np.nonzero(m0)[0].tolist()) == [0, 5]


# ------------------------------------------------------------------------------------------------ the grouped launch
def _tiles_live(m, M):
    nt = (M + 255) // 256
    pad = np.zeros(nt * 4, np.uint8)
    pad[:len(m)] = m
    return pad.reshape(nt, 4).any(1)


@pytest.mark.parametrize('pyramid', [RAGGED, PYR3], ids=['ragged', 'three-levels'])
@pytest.mark.parametrize('G', [2, 3])
def test_grouped_forward_skips_dead_tiles_and_keeps_the_live_bits(G, pyramid, monkeypatch):
    from aod_meh_hua_amd import hipops as ho
    B, sizes = pyramid
    segs, M = sb._segs(B, sizes)
    gen = torch.Generator(device='cuda').manual_seed(41)
    rnd = lambda *sh: torch.randn(*sh, device='cuda', generator=gen)
    xs = [rnd(M, ho.xw(CIN)).bfloat16() for _ in range(G)]
    ws = [(rnd(CIN, 9 * ho.xw(CIN)) / (9 * CIN) ** 0.5).bfloat16() for _ in range(G)]
    bias = [rnd(CIN).abs() + 0.5 for _ in range(G)]                          # relu(bias) > 0 everywhere: a skipped row must still be ZERO
    nblk = (M + 63) // 64

    def run(omaps):
        outs = [torch.full((M, ho.xw(CIN)), float('nan'), device='cuda', dtype=torch.bfloat16) for _ in range(G)]
        ho.conv2d_rows_grouped(xs, segs, ws, CIN, 3, 3, 1, 1, 1, pre_shifts=bias, relu=True, outs=outs, omaps=omaps)
        torch.cuda.synchronize()
        return outs
    dense = run(None)
    assert all(bool(torch.isfinite(o.float()).all()) for o in dense)
    fmap = _chain_gpu(_weights([_mid(B, sizes)], M), B, sizes, 3)[2]        # F of a layer two convs below the prediction conv
    live = _tiles_live(fmap.cpu().numpy(), M)
    assert live.any() and not live.all()
    row_live = torch.from_numpy(np.repeat(live, 256)[:M]).cuda()
    got = run([None] + [fmap] * (G - 1))
    assert torch.equal(got[0], dense[0])                                     # the first member is dense
    for g in range(1, G):
        assert torch.equal(got[g][row_live], dense[g][row_live]), g          # live tiles: the dense launch's bits
        assert int(got[g][~row_live].view(torch.int16).count_nonzero()) == 0, g      # dead tiles: +0 heads and tails over the NaN prefill
    # members with DIFFERENT maps (the last one all dead)
    if G == 3:
        zero = torch.zeros(nblk, dtype=torch.uint8, device='cuda')
        got = run([None, fmap, zero])
        assert torch.equal(got[0], dense[0]) and torch.equal(got[1][row_live], dense[1][row_live])
        assert int(got[2].view(torch.int16).count_nonzero()) == 0
    # an all-ones map is the dense launch
    ones = torch.ones(nblk, dtype=torch.uint8, device='cuda')
    got = run([None] + [ones] * (G - 1))
    assert all(torch.equal(a, b) for a, b in zip(got, dense))
    # AOD_SPARSE_FWD=0: the map is passed, nothing is skipped
    monkeypatch.setenv('AOD_SPARSE_FWD', '0')
    got = run([None] + [fmap] * (G - 1))
    assert all(torch.equal(a, b) for a, b in zip(got, dense))


# ------------------------------------------------------------------------------------------------ whole step
def _counting_assign(monkeypatch):
    from aod_meh_hua_amd import hipops as ho
    n = [0]
    real = ho.max_iou_assign

    def counted(*a, **k):
        n[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(ho, 'max_iou_assign', counted)
    return n


def _eager_steps(data, steps, monkeypatch, sparse):
    """`steps` iterations from the seeded weights -> (losses, loss_noR rows and gradients of the FIRST iteration, final parameters, forward-map
    log of the first iteration, bbox weights of the first iteration, assign calls)"""
    from aod_meh_hua_amd import functional as AF
    monkeypatch.setenv('AOD_SPARSE_FWD', '1' if sparse else '0')
    model, opt, opt_L = sb._model()
    pd = dict(model.named_parameters())
    calls = _counting_assign(monkeypatch)
    first = None
    for step in range(steps):
        AF.FWD_MAP_LOG = [] if step == 0 else None
        try:
            out, head_out, feat_out, prev = model.train_step(data, Labeled=True, Pseudo=False)
        finally:
            log, AF.FWD_MAP_LOG = AF.FWD_MAP_LOG, None
        opt.zero_grad()
        out['loss'].backward()
        grads = {k: p.grad.detach().clone() for k, p in pd.items() if p.grad is not None}
        lossL = model.train_step_L(prev, head_out, feat_out)
        opt_L.zero_grad()
        lossL['loss'].backward()
        grads.update({k + '@L': p.grad.detach().clone() for k, p in pd.items() if p.grad is not None and k + '@L' not in grads and
                      ('.retina_L.' in k or '.L_convs.' in k)})
        if step == 0:
            losses = {k: float(v) for k, v in {**out['log_vars'], **lossL['log_vars']}.items()}
            noR = [t.detach().clone() for t in prev]
            bw = torch.cat([t.reshape(-1, 4) for t in head_out[7]]).detach().clone()
            first = (losses, noR, grads, log, bw)
        opt.step()
        opt_L.step()
    torch.cuda.synchronize()
    params = {k: p.detach().clone() for k, p in pd.items()}
    return first, params, calls[0]


def _check_log(log, bw, B, sizes, sparse_rows_expected=True):
    """which launch received which map: four paired launches of three members, the cls member dense, the reg member and the rider with
    F_(i + 1) = D^(4 - i)(m0), m0 from the bbox weights the loss used"""
    assert len(log) == 4, len(log)
    M = sum(B * h * w for h, w in sizes)
    pos_rows = sorted(set((bw.abs().sum(1).nonzero().squeeze(1) // A).tolist()))
    want = _chain_np(pos_rows, B, sizes, 5)
    for i, (members, shape, omaps) in enumerate(log):
        assert members == 3 and shape[0] == M and omaps is not None and omaps[0] is None and omaps[1] is omaps[2], i
        assert np.array_equal(omaps[1].cpu().numpy(), want[4 - i]), i
    return want


def test_whole_step_equals_the_dense_step_in_the_deterministic_mode(monkeypatch):
    """every loss, the loss_noR rows, every parameter gradient of both optimizers and the parameters after three steps"""
    from aod_meh_hua_amd import functional as AF
    data = sb._data()
    AF.set_deterministic(True)
    try:
        on, p_on, calls_on = _eager_steps(data, 3, monkeypatch, True)
        off, p_off, calls_off = _eager_steps(data, 3, monkeypatch, False)
    finally:
        AF.set_deterministic(False)
    assert calls_on == 3 and calls_off == 3                                 # the assign kernels run once per step, on either path
    want = _check_log(on[3], on[4], 2, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1)))
    assert want[0].any() and not want[0].all()                              # (the large boxes of _data: positives on P4 and above, none on P3)
    assert on[0] == off[0], (on[0], off[0])
    assert len(on[1]) == len(off[1]) and all(torch.equal(a, b) for a, b in zip(on[1], off[1]))
    assert set(on[2]) == set(off[2]) and any(k.endswith('@L') for k in on[2])
    for k in on[2]:
        assert torch.equal(on[2][k], off[2][k]), k
    for k in p_on:
        assert torch.equal(p_on[k], p_off[k]), k
    assert bool(all(torch.isfinite(v).all() for v in p_on.values()))


def test_whole_step_equals_the_dense_step_in_the_default_mode(monkeypatch):
    """the default mode (sparse backward on, atomic column sums): losses, loss_noR rows and every filter gradient are equal; the bias
    vectors to the arrival-order bound (see the module text)"""
    data = sb._data()
    on, _, calls = _eager_steps(data, 1, monkeypatch, True)
    off, _, _ = _eager_steps(data, 1, monkeypatch, False)
    assert calls == 1
    _check_log(on[3], on[4], 2, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1)))
    assert on[0] == off[0], (on[0], off[0])
    assert all(torch.equal(a, b) for a, b in zip(on[1], off[1]))
    assert set(on[2]) == set(off[2])
    for k in on[2]:
        if on[2][k].dim() == 4:
            assert torch.equal(on[2][k], off[2][k]), k
        else:
            assert sb._close(on[2][k], off[2][k]), k


def _graph_steps(batches, monkeypatch, sparse):
    from aod_meh_hua_amd.graphs import GraphedTrainStep
    monkeypatch.setenv('AOD_SPARSE_FWD', '1' if sparse else '0')
    model, opt, opt_L = sb._model()
    gs = GraphedTrainStep(model, opt, opt_L, warmup=1, Labeled=True, Pseudo=False)
    losses = []
    for d in batches:                                                        # eager warm-up + capture on the first, replays after it
        out = gs(d)
        losses.append({k: float(v) for k, v in out['log_vars'].items()})
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return losses, grads, {k: p.detach().clone() for k, p in model.named_parameters()}


def test_whole_step_replayed_as_a_graph_equals_the_dense_graph(monkeypatch):
    """the maps are device data at fixed addresses of the graph's pool: a replay follows ITS batch's positives.  Capture on one batch, replay on
    another and on the first again (deterministic mode): losses of every step, the gradients the last replay left, the parameters after 3 steps"""
    from aod_meh_hua_amd import functional as AF
    from tests import synth
    d0 = sb._data()
    gtb, gtl = synth.random_gts(2, 128, 128, seed=24, gmin=1, gmax=3)
    d1 = dict(img=synth.images(2, 128, 128, seed=5).cuda(), img_metas=synth.metas(2, 128, 128), gt_bboxes=[b.cuda() for b in gtb],
              gt_labels=[l.cuda() for l in gtl])
    AF.set_deterministic(True)
    try:
        on = _graph_steps([d0, d1, d0], monkeypatch, True)
        off = _graph_steps([d0, d1, d0], monkeypatch, False)
    finally:
        AF.set_deterministic(False)
    assert on[0] == off[0], (on[0], off[0])
    assert set(on[1]) == set(off[1])
    for k in on[1]:
        assert torch.equal(on[1][k], off[1][k]), k
    for k in on[2]:
        assert torch.equal(on[2][k], off[2][k]), k


def test_a_batch_without_any_positive_trains_and_equals_the_dense_step(monkeypatch):
    """G = 0 in every image: every map is zero, the reg tower and the rider store zero rows only, and nothing is NaN"""
    from tests import synth
    data = dict(img=synth.images(2, 128, 128).cuda(), img_metas=synth.metas(2, 128, 128),
                gt_bboxes=[torch.zeros(0, 4).cuda() for _ in range(2)], gt_labels=[torch.zeros(0, dtype=torch.long).cuda() for _ in range(2)])
    on, p_on, _ = _eager_steps(data, 1, monkeypatch, True)
    off, p_off, _ = _eager_steps(data, 1, monkeypatch, False)
    assert int(on[4].count_nonzero()) == 0
    for members, shape, omaps in on[3]:
        assert omaps is not None and int(omaps[1].count_nonzero()) == 0
    assert all(np.isfinite(v) for v in on[0].values()) and on[0] == off[0], (on[0], off[0])
    assert all(torch.equal(a, b) for a, b in zip(on[1], off[1]))
    for k in on[2]:
        assert bool(torch.isfinite(on[2][k]).all()), k
        if on[2][k].dim() == 4:
            assert torch.equal(on[2][k], off[2][k]), k
        else:
            assert sb._close(on[2][k], off[2][k]), k
    for k in p_on:
        assert bool(torch.isfinite(p_on[k]).all()), k
