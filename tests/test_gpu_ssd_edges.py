"""The kernels that only the SSD configurations run (csrc/ssd_ops.hip and their X-layout twins at the end of csrc/x3_ops.hip) at ties and
edges, against the float64 references of tests/ssd_edges_util.py.

Section 1 calls aod_ssd_loss_fwd / aod_ssd_loss_bwd through the C ABI, so that the `sel4` record is readable, on negatives that tie in
groups of hundreds across every 1024-anchor chunk and every wave.  The selected set is read off a backward with g_cls = 1 and must be the
k negatives largest by (ce descending, anchor index ascending), exactly.  Section 2 pools bf16-representable images with real ties under
integer upstream gradients: every value is exact in both layouts and the comparison with F.max_pool2d in float64 is torch.equal.  Section 3
holds the L2Norm forward of both layouts at 64 / 512 / 1024 channels and pins the zero-norm contract.  The preconditions of the committed
seeds (where k falls, the gaps around the thresholds, the tied windows, the bf16 round trips) are pinned by tests/test_ssd_edges_host.py."""
import os

import numpy as np
import pytest
import torch

from tests import ssd_edges_util as U

pytestmark = pytest.mark.gpu
LOSS_IDS = [U.loss_id(c) for c in U.LOSS_CASES]


@pytest.fixture
def x3_mode():
    """the reference-precision mode, whatever AOD_CONV_PREC names as the suite's default"""
    from aod_meh_hua_amd import functional as AF
    AF.set_precision('bf16x3')
    yield
    AF.set_precision(os.environ.get('AOD_CONV_PREC', 'bf16x3'))


# ---------------------------------------------------------------- section 1: SSD loss
def _dev(c):
    d = U.loss_case(c)
    return {k: d[k].cuda() for k in ('cls', 'labels', 'lw', 'box', 'bt', 'bw')}


def _fwd(c, t):
    from aod_meh_hua_amd._C import call, ptr, stream
    ce = torch.full((c.B, c.A), -7.0, device='cuda')
    sums = torch.full((c.B, 3), -7.0, device='cuda')
    sel = torch.full((c.B, 4), -7, device='cuda', dtype=torch.int32)
    call('aod_ssd_loss_fwd', ptr(t['cls']), ptr(t['labels']), ptr(t['lw']), ptr(t['box']), ptr(t['bt']), ptr(t['bw']), c.B, c.A, c.C1, c.C1 - 1,
         c.ratio, c.beta, ptr(ce), ptr(sums), ptr(sel), stream())
    torch.cuda.synchronize()
    return ce, sums, sel


def _bwd(c, t, ce, sel, g_cls, g_box, g_noR):
    from aod_meh_hua_amd._C import call, ptr, stream
    gl = torch.full((c.B, c.A, c.C1), float('nan'), device='cuda')
    gb = torch.full((c.B, c.A, 4), float('nan'), device='cuda')
    call('aod_ssd_loss_bwd', ptr(t['cls']), ptr(t['labels']), ptr(t['lw']), ptr(t['box']), ptr(t['bt']), ptr(t['bw']), ptr(ce), ptr(sel), c.B, c.A,
         c.C1, c.C1 - 1, c.beta, ptr(g_cls), ptr(g_box), ptr(g_noR), ptr(gl), ptr(gb), stream())
    torch.cuda.synchronize()
    return gl.cpu(), gb.cpu()


def _bits(x):
    return np.maximum(np.asarray(x, np.float32), np.float32(0)).view(np.uint32)


def _own_selection(c, ce):
    """the stable rule on the kernel's own ce (the tensor its backward reads), per image"""
    d = U.loss_case(c)
    return [U.select_stable(ce[b].numpy(), d['labels'][b].numpy(), d['num_classes'], c.ratio) for b in range(c.B)]


@pytest.mark.parametrize('c', U.LOSS_CASES, ids=LOSS_IDS)
def test_ssd_loss_forward_ce_sel4_and_sums(c):
    d, ref, t = U.loss_case(c), U.loss_reference(c), _dev(c)
    ce_d, sums_d, sel_d = _fwd(c, t)
    ce, sums, sel = ce_d.cpu(), sums_d.cpu(), sel_d.cpu().numpy().view(np.uint32)
    atol = U.ce_atol(c)
    err = (ce.double() - ref['ce']).abs()
    print(f'{U.loss_id(c)}: |ce - f64| max {float(err.max()):.3g} (atol {atol:.3g}), worst excess over rtol 1e-5 '
          f'{float((err - 1e-5 * ref["ce"].abs()).max()):.3g}')
    assert bool((err <= atol + 1e-5 * ref['ce'].abs()).all())
    assert bool((ce[d['lw'] == 0] == 0).all())
    # sel4 = (threshold bits, ties selected, #pos, k): counts from the labels, the threshold from a sort of the kernel's own ce
    own = _own_selection(c, ce)
    for b, s in enumerate(own):
        thr = int(_bits(s['thr'])) if s['k'] else 0
        want = (thr, s['k'] - s['above'] if s['k'] else 0, ref['sel'][b]['npos'], ref['sel'][b]['k'])
        assert tuple(int(v) for v in sel[b]) == want, (b, sel[b], want)
        if c.dist in U.TIE_DISTS:                      # groups that tie in any arithmetic: the float64 counts hold on the device
            assert (s['above'], s['at']) == (ref['sel'][b]['above'], ref['sel'][b]['at']), (b, s, ref['sel'][b])
    print(f'{U.loss_id(c)}: sums {sums.tolist()} f64 {ref["sums"].tolist()}')
    assert np.allclose(sums.double().numpy(), ref['sums'].numpy(), rtol=1e-5, atol=1e-6)
    # no floating-point atomics: a second launch gives the same bits
    ce2, sums2, sel2 = _fwd(c, t)
    assert torch.equal(ce2, ce_d) and torch.equal(sums2.view(torch.int32), sums_d.view(torch.int32)) and torch.equal(sel2, sel_d)


@pytest.mark.parametrize('c', U.LOSS_CASES, ids=LOSS_IDS)
def test_ssd_loss_backward_selects_the_stable_set_exactly(c):
    """backward with g_cls = 1 and nothing else: among anchors with label_weight != 0 a background row is non-zero if and only if the
    stable rule on the kernel's ce selects it"""
    d, ref, t = U.loss_case(c), U.loss_reference(c), _dev(c)
    ce_d, _, sel_d = _fwd(c, t)
    gl, gb = _bwd(c, t, ce_d, sel_d, torch.ones(c.B, device='cuda'), None, None)
    assert bool(torch.isfinite(gl).all()) and bool((gb == 0).all())
    own = _own_selection(c, ce_d.cpu())
    bg = (d['labels'] == d['num_classes']).numpy()
    seen = d['lw'].numpy() != 0
    nz = (gl != 0).any(-1).numpy()
    for b, s in enumerate(own):
        got = nz[b] & bg[b]
        assert not (got & ~seen[b]).any()                                              # a zero weight hides its row
        wrong = np.flatnonzero((got != s['mask']) & seen[b] & bg[b])
        assert len(wrong) == 0, (b, wrong[:8], 'selected by the kernel:', got[wrong[:8]])
        hidden = int((s['mask'] & ~seen[b]).sum())                                     # zero-weight anchors that took a ticket
        assert int(got.sum()) + hidden == s['k'] == ref['sel'][b]['k'], (b, int(got.sum()), hidden, s['k'])
        if c.dist in U.TIE_DISTS:
            assert np.array_equal(s['mask'], ref['sel'][b]['mask'])                    # the same set follows from the float64 ce alone
        pos = ~bg[b]
        assert nz[b][pos & seen[b]].all()                                              # every positive receives g_cls


@pytest.mark.parametrize('c', U.LOSS_CASES, ids=LOSS_IDS)
def test_ssd_loss_backward_gradients(c):
    d, t = U.loss_case(c), _dev(c)
    ce_d, _, sel_d = _fwd(c, t)
    ups = U.upstream(c)
    dev = [None if u is None else u.cuda() for u in ups]
    gl, gb = _bwd(c, t, ce_d, sel_d, *dev)
    selected = torch.from_numpy(np.stack([s['mask'] for s in _own_selection(c, ce_d.cpu())]))
    rl, rb = U.loss_grads(c, selected, *ups)
    el, eb = (gl.double() - rl).abs(), (gb.double() - rb).abs()
    print(f'{U.loss_id(c)}: logits grad worst excess over rtol 1e-4 {float((el - 1e-4 * rl.abs()).max()):.3g} (atol 1e-7), '
          f'box grad worst excess over rtol 1e-5 {float((eb - 1e-5 * rb.abs()).max()):.3g} (atol 1e-8)')
    assert np.allclose(gl.numpy(), rl.numpy(), rtol=1e-4, atol=1e-7)
    assert np.allclose(gb.numpy(), rb.numpy(), rtol=1e-5, atol=1e-8)
    if ups[2] is None:                                   # no g_noR: an unselected negative's row is exactly zero
        idle = (d['labels'] == d['num_classes']) & ~selected
        assert bool((gl[idle] == 0).all())
    if ups[1] is None:
        assert bool((gb == 0).all())
    assert bool((gb[d['bw'] == 0] == 0).all()) and bool((gl[d['lw'] == 0] == 0).all())
    gl2, gb2 = _bwd(c, t, ce_d, sel_d, *dev)
    assert torch.equal(gl2.view(torch.int32), gl.view(torch.int32)) and torch.equal(gb2.view(torch.int32), gb.view(torch.int32))


@pytest.mark.parametrize('c', U.AUTOGRAD_CASES, ids=[U.loss_id(c) for c in U.AUTOGRAD_CASES])
def test_ssd_loss_through_autograd(c):
    from aod_meh_hua_amd.functional_ssd import SSDLossFn
    d, ref, t = U.loss_case(c), U.loss_reference(c), _dev(c)
    g_cls, g_box, g_noR = U.upstream(c._replace(grads='both'))
    cd, bd = t['cls'].clone().requires_grad_(True), t['box'].clone().requires_grad_(True)
    cs, bs, ce = SSDLossFn.apply(cd, bd, t['labels'], t['lw'], t['bt'], t['bw'], c.C1 - 1, c.ratio, c.beta)
    ((cs * g_cls.cuda()).sum() + (bs * g_box.cuda()).sum() + (ce * g_noR.cuda()).sum()).backward()
    torch.cuda.synchronize()
    assert np.allclose(cs.detach().cpu().double().numpy(), ref['sums'][:, 0].numpy(), rtol=1e-5, atol=1e-6)
    assert np.allclose(bs.detach().cpu().double().numpy(), ref['sums'][:, 1].numpy(), rtol=1e-5, atol=1e-6)
    assert bool(((ce.detach().cpu().double() - ref['ce']).abs() <= U.ce_atol(c) + 1e-5 * ref['ce'].abs()).all())
    selected = torch.from_numpy(np.stack([s['mask'] for s in _own_selection(c, ce.detach().cpu())]))
    rl, rb = U.loss_grads(c, selected, g_cls, g_box, g_noR)
    assert np.allclose(cd.grad.cpu().numpy(), rl.numpy(), rtol=1e-4, atol=1e-7)
    assert np.allclose(bd.grad.cpu().numpy(), rb.numpy(), rtol=1e-5, atol=1e-8)


# ---------------------------------------------------------------- section 2: generic max-pool, both layouts
def _pool_bf16(x, go, geom):
    from aod_meh_hua_amd.functional_ssd import max_pool
    k, s, p, ceil = geom[:4]
    xd = x.bfloat16().cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = max_pool(xd, k, s, p, ceil)
    y.backward(go.bfloat16().cuda().contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    return y.detach().double().cpu(), xd.grad.double().cpu()


def _rows(t):
    from aod_meh_hua_amd import hipops as ho
    B, C, H, W = t.shape
    return ho.x3_split(t.float().cuda().permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous())


def _nchw(rows, B, H, W, C):
    from aod_meh_hua_amd import hipops as ho
    return ho.x3_merge(rows, C).view(B, H, W, C).permute(0, 3, 1, 2).double().cpu()


def _pool_x3(x, go, geom):
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd.functional_ssd import max_pool
    k, s, p, ceil, B, C, H, W = geom
    xx = AF.as_nchw(_rows(x), B, H, W).requires_grad_(True)
    y = max_pool(xx, k, s, p, ceil)
    OH, OW = y.shape[2:]
    y.backward(AF.as_nchw(_rows(go), B, OH, OW))
    torch.cuda.synchronize()
    return _nchw(AF.as_rows(y.detach()), B, OH, OW, C), _nchw(AF.as_rows(xx.grad), B, H, W, C)


def _check_pool(run, dist, geom):
    x, go, y_ref, gx_ref = U.pool_reference(dist, geom)
    y, gx = run(x, go, geom)
    assert y.shape == y_ref.shape, (dist, y.shape, y_ref.shape)
    assert torch.equal(y, y_ref), (dist, 'forward', int((y != y_ref).sum()))
    assert torch.equal(gx, gx_ref), (dist, 'backward', int((gx != gx_ref).sum()), torch.nonzero(gx != gx_ref)[:4].tolist())


@pytest.mark.parametrize('geom', U.POOL_GEOMS, ids=U.pool_id)
def test_maxpool_bf16_exact_with_ties(geom, bf16_mode):
    for dist in U.POOL_DISTS:
        _check_pool(_pool_bf16, dist, geom)


@pytest.mark.parametrize('geom', U.POOL_GEOMS, ids=U.pool_id)
def test_maxpool_x3_exact_with_ties(geom, x3_mode):
    for dist in U.POOL_DISTS:
        _check_pool(_pool_x3, dist, geom)


def test_maxpool_bf16_second_grid_stride_trip(bf16_mode):
    _check_pool(_pool_bf16, 'relu', U.POOL_BIG)


def test_maxpool_x3_second_grid_stride_trip(x3_mode):
    _check_pool(_pool_x3, 'relu', U.POOL_BIG)


# ---------------------------------------------------------------- section 3: L2Norm
def _l2_run(layout, x, w, go=None):
    """rows in, rows out (float64 on the CPU): y, and gx / gw when an upstream gradient is given"""
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd.functional_ssd import l2norm
    R, C = x.shape
    put = (lambda t: t.bfloat16().cuda()) if layout == 'bf16' else (lambda t: ho.x3_split(t.cuda()))
    get = (lambda r: r.double().cpu()) if layout == 'bf16' else (lambda r: ho.x3_merge(r.contiguous(), C).double().cpu())
    xx = AF.as_nchw(put(x), 1, 1, R).requires_grad_(True)
    wd = w.cuda().requires_grad_(True)
    y = l2norm(xx, wd, U.L2_EPS)
    if go is None:
        torch.cuda.synchronize()
        return get(AF.as_rows(y.detach()))
    y.backward(AF.as_nchw(put(go), 1, 1, R))
    torch.cuda.synchronize()
    return get(AF.as_rows(y.detach())), get(AF.as_rows(xx.grad)), wd.grad.double().cpu()


def _check_l2_forward(layout, C):
    x, w, go = U.l2_case(C, layout)
    y_ref = U.l2_reference(x, w, go)[0]
    y = _l2_run(layout, x, w)
    err = float((y - y_ref).abs().max() / y_ref.abs().max())
    print(f'l2norm {layout} C={C}: forward error {err:.3g} of the scale, bound {U.L2_FWD_BOUND[layout]:.3g}')
    assert y.shape == y_ref.shape and err < U.L2_FWD_BOUND[layout]


@pytest.mark.parametrize('C', U.L2_C)
def test_l2norm_bf16_forward_widths(C, bf16_mode):
    _check_l2_forward('bf16', C)


@pytest.mark.parametrize('C', U.L2_C)
def test_l2norm_x3_forward_widths(C, x3_mode):
    _check_l2_forward('x3', C)


def _check_l2_zero_norm(layout):
    """all-zero pixels: finite everywhere, y == 0 and gx == w * g / eps there, nothing into gw, the other pixels untouched"""
    C = 512
    x, w, go = U.l2_case(C, layout, zeros=True)
    x0 = U.l2_case(C, layout)[0]
    z = list(U.L2_ZERO_ROWS)
    keep = np.setdiff1d(np.arange(U.L2_ROWS), z)
    y, gx, gw = _l2_run(layout, x, w, go)
    y_ref, gx_ref, gw_ref = U.l2_reference(x, w, go)
    assert all(bool(torch.isfinite(t).all()) for t in (y, gx, gw))
    assert bool((y[z] == 0).all())
    rel = float(((gx[z] - gx_ref[z]).abs() / gx_ref[z].abs()).max())
    print(f'l2norm {layout}: gx of the zero rows, relative error {rel:.3g}, bound {1.01 * U.L2_ROUND[layout]:.3g}')
    assert rel <= 1.01 * U.L2_ROUND[layout]                                           # w * g / eps rounded to the layout
    # the other pixels: the same bits as in the batch where those pixels are not zero, and the existing bounds against float64
    y0, gx0, _ = _l2_run(layout, x0, w, go)
    assert torch.equal(y[keep], y0[keep]) and torch.equal(gx[keep], gx0[keep])
    assert float((y[keep] - y_ref[keep]).abs().max() / y_ref.abs().max()) < U.L2_FWD_BOUND[layout]
    assert float((gx[keep] - gx_ref[keep]).abs().max() / gx_ref[keep].abs().max()) < U.L2_GX_BOUND[layout]
    # gw: a gradient that arrives at the zero pixels alone adds exactly nothing to any column (exact under the fp32 atomics too)
    go2 = torch.zeros_like(go)
    go2[z] = go[z]
    gw2 = _l2_run(layout, x, w, go2)[2]
    assert bool((gw2 == 0).all())
    if layout == 'bf16':
        assert np.allclose(gw.numpy(), gw_ref.numpy(), rtol=U.L2_GW_BOUND[layout], atol=U.L2_GW_BOUND[layout])
    else:
        assert float((gw - gw_ref).abs().max() / gw_ref.abs().max()) < U.L2_GW_BOUND[layout]


def test_l2norm_bf16_zero_norm_contract(bf16_mode):
    _check_l2_zero_norm('bf16')


def test_l2norm_x3_zero_norm_contract(x3_mode):
    _check_l2_zero_norm('x3')
