"""Host-side guard of the SSD edge cases (no GPU): the case builders and float64 references of tests/ssd_edges_util.py alone.  It asserts
the preconditions that tests/test_gpu_ssd_edges.py relies on for the committed seeds, so that a seed change cannot silently turn an edge
test into a plain one: k where each tie case says it is, a float64 gap around every threshold that no float32 error can bridge, background
rows whose gradient cannot vanish, saturated rows that really are exact float32 zeros, pooling windows that really tie, expected pooling
values that survive a bf16 round trip, the grid-stride caps really exceeded.  These are conditions, not tolerances."""
import numpy as np
import pytest
import torch

from tests import ssd_edges_util as U

LOSS_IDS = [U.loss_id(c) for c in U.LOSS_CASES]


# ---------------------------------------------------------------- section 1: SSD loss
def test_loss_cases_cover_the_shapes_and_every_place_of_k():
    cs = U.LOSS_CASES
    assert len(set(LOSS_IDS)) == len(cs)
    assert {c.A for c in cs} == {63, 1024, 1025, 2500, 8732} and all(c.B == 3 for c in cs)
    assert {c.C1 for c in cs} == {2, 21, 81}
    assert {c.ratio for c in cs} == {1, 3} and sum(c.ratio == 1 for c in cs) == 1
    assert {c.beta for c in cs} == {1.0, 0.5}
    assert {c.dist for c in cs} == {'random', 'palette', 'saturated', 'all_equal'}
    assert {c.grads for c in cs} == {'cls', 'noR', 'both'}
    assert {c.kind for c in cs if c.dist in U.TIE_DISTS} == set(U.TIE_KINDS)          # all four occur
    assert all(c.kind in U.TIE_KINDS for c in cs if c.dist in U.TIE_DISTS)
    assert all(c in cs for c in U.AUTOGRAD_CASES)


@pytest.mark.parametrize('c', U.LOSS_CASES, ids=LOSS_IDS)
def test_loss_case_meets_its_preconditions(c):
    d, ref = U.loss_case(c), U.loss_reference(c)
    ncls = d['num_classes']
    assert d['cls'].dtype == torch.float32 and d['cls'].shape == (c.B, c.A, c.C1) and bool(torch.isfinite(d['cls']).all())
    assert bool(((d['labels'] >= 0) & (d['labels'] <= ncls)).all())
    bg = d['labels'] == ncls
    # every background row keeps a non-background float64 probability above 1e-30: a selected row cannot have an all-zero float32 gradient
    p = torch.softmax(d['cls'].double(), -1)[..., :ncls].max(-1).values
    assert float(p[bg].min()) > 1e-30
    ce32 = U.ce_fp32(c)
    assert bool((ce32 >= 0).all()) and bool((ref['ce'] >= 0).all())
    for b in range(c.B):
        s = ref['sel'][b]
        ign = (d['lw'][b] == 0)
        assert s['npos'] == U.npos_of(c, b) == int((d['bw'][b, :, 0] == 1).sum()) and s['nneg'] == c.A - s['npos']
        assert int(ign.sum()) == min(U.N_IGN, s['nneg']) and bool(bg[b][ign].all())
        assert int(s['mask'].sum()) == s['k'] == min(c.ratio * s['npos'], s['nneg'])
        print(f'{U.loss_id(c)} b={b}: k {s["k"]} of {s["nneg"]} negatives, above {s["above"]}, at {s["at"]}, gap {s["gap"]:.3g}, '
              f'distinct f64 {len(np.unique(ref["ce"][b][bg[b]].numpy()))}, distinct f32 {len(np.unique(ce32[b][bg[b]].numpy()))}')
        if s['npos'] >= 3:                 # the planted box differences: |d| == beta twice and d == 0, exactly, in float32
            diff = (d['box'][b] - d['bt'][b])[d['bw'][b, :, 0] == 1]
            assert int((diff.abs() == c.beta).sum()) >= 6 and int((diff == 0).sum()) >= 3
        if c.dist in U.TIE_DISTS:
            assert U.kind_of(s) == c.kind, (b, U.kind_of(s), s)
            assert s['gap'] >= U.MIN_GAP, (b, s['gap'])
            if c.kind in ('inside', 'end'):
                assert s['at'] >= 50, s                                       # a group of hundreds, not a chance pair
            # the float32 restatement sees the same groups, hence the same selection
            s32 = U.select_stable(ce32[b].numpy(), d['labels'][b].numpy(), ncls, c.ratio)
            assert np.array_equal(s32['mask'], s['mask']) and (s32['above'], s32['at']) == (s['above'], s['at'])
            if s['k'] and c.kind != 'kneg':
                idx = np.flatnonzero(bg[b].numpy() & (ref['ce'][b].numpy() == s['thr']))
                assert len({i // 1024 for i in idx}) >= max(1, (c.A - 64) // 1024 + 1)   # the group reaches into every chunk of a wave or more
        elif c.dist == 'random':
            assert len(np.unique(ce32[b][bg[b] & ~ign].numpy())) == int((bg[b] & ~ign).sum())         # tie-free in float32 too
        else:
            zeros = int(((ce32[b] == 0) & bg[b] & ~ign).sum())
            assert zeros >= 100, zeros
            nonzero = int(((ce32[b] > 0) & bg[b]).sum())
            assert (s['k'] > nonzero) == (c.kind == 'sat'), (s['k'], nonzero)
    # the bounds of the GPU test are reachable: the float32 restatement meets them against float64
    err = (ce32.double() - ref['ce']).abs()
    print(f'{U.loss_id(c)}: float32 restatement |ce - f64| max {float(err.max()):.3g}, atol {U.ce_atol(c):.3g}')
    assert bool((err <= U.ce_atol(c) + 1e-5 * ref['ce'].abs()).all())


def test_a_saturated_case_mines_into_the_exact_zeros():
    assert any(c.kind == 'sat' for c in U.LOSS_CASES)


def test_stable_rule_tells_an_off_by_one_ticket():
    """the selection rule itself: one ticket too many or too few changes the set"""
    ce = np.array([0.5, 2.0, 0.5, 0.5, 0.0, 0.5, 3.0], np.float32)
    labels = np.array([1, 1, 1, 0, 1, 1, 1])
    s = U.select_stable(ce, labels, 1, 4)
    assert s['k'] == 4 and s['above'] == 2 and s['at'] == 3 and U.kind_of(s) == 'inside'
    assert np.flatnonzero(s['mask']).tolist() == [0, 1, 2, 6]


# ---------------------------------------------------------------- section 2: max-pool
@pytest.mark.parametrize('geom', U.POOL_GEOMS + [U.POOL_BIG], ids=U.pool_id)
def test_pool_cases_tie_and_are_exact_in_bf16(geom):
    k, s, p, ceil, B, C, H, W = geom
    for dist in (U.POOL_DISTS if geom != U.POOL_BIG else ('relu',)):
        x, go, y, gx = U.pool_reference(dist, geom)
        for t in (x, go, y, gx):                                   # every input and every expected value survives a bf16 round trip
            assert torch.equal(t.float().bfloat16().double(), t), dist
        assert float(go.abs().max()) <= 8 and float(gx.abs().max()) <= 72 and torch.equal(gx, gx.round())
        ties = U.pool_tie_windows(x, y, geom)
        print(f'{U.pool_id(geom)} {dist}: {ties} of {y.numel()} windows tie')
        if dist in U.POOL_TIE_DISTS and H * W > 1:
            assert ties > 0, dist
        if (k, s, p, ceil) == (2, 2, 0, False):
            assert H % 2 == 1 and W % 2 == 1 and float(gx[:, :, -1].abs().max()) == 0 and float(gx[:, :, :, -1].abs().max()) == 0
        if ceil:
            assert y.shape[2] == (H + 1) // 2 and (H % 2 == 1 or W % 2 == 1)          # a clipped last window


def test_pool_geometries_cover_the_issue():
    gs = {g[:4] for g in U.POOL_GEOMS}
    assert gs == {(2, 2, 0, True), (3, 1, 1, False), (3, 2, 1, False), (2, 2, 0, False)}
    assert {g[4] for g in U.POOL_GEOMS} == {1, 3} and {g[5] for g in U.POOL_GEOMS} == {64, 128}
    assert any(g[:4] == (3, 1, 1, False) and g[6] == 1 for g in U.POOL_GEOMS) and any(g[:4] == (3, 1, 1, False) and g[6] == 2 for g in U.POOL_GEOMS)
    assert any(g[:4] == (2, 2, 0, True) and g[6] != g[7] for g in U.POOL_GEOMS)
    k, s, p, ceil, B, C, H, W = U.POOL_BIG
    # octets of the bf16 layout and of the X layout, forward (3x3 s1 p1 keeps the size) and backward: a second trip in all four launches
    assert B * H * W * (C // 8) > max(U.POOL_CAPS)


# ---------------------------------------------------------------- section 3: L2Norm
@pytest.mark.parametrize('layout', ['bf16', 'x3'])
def test_l2_cases_are_exact_in_their_layout_and_keep_the_zero_norm_contract(layout):
    assert U.L2_ROWS % 4 != 0
    for C in U.L2_C:
        x, w, go = U.l2_case(C, layout)
        fit = (lambda t: t.bfloat16().float()) if layout == 'bf16' else U.x_representable
        assert torch.equal(fit(x), x) and torch.equal(fit(go), go)
        if layout == 'x3':
            assert not torch.equal(x.bfloat16().float(), x)                           # the tails carry something
    x, w, go = U.l2_case(512, layout, zeros=True)
    x0 = U.l2_case(512, layout)[0]
    z = list(U.L2_ZERO_ROWS)
    keep = np.setdiff1d(np.arange(U.L2_ROWS), z)
    assert float(x[z].abs().max()) == 0 and torch.equal(x[keep], x0[keep]) and float(x0[z].abs().min(1).values.max()) > 0
    y, gx, gw = U.l2_reference(x, w, go)
    y0, gx0, gw0 = U.l2_reference(x0, w, go)
    assert all(bool(torch.isfinite(t).all()) for t in (y, gx, gw))
    assert float(y[z].abs().max()) == 0 and torch.equal(y[keep], y0[keep]) and torch.equal(gx[keep], gx0[keep])
    eps = float(np.float32(U.L2_EPS))
    assert torch.allclose(gx[z], w.double() * go[z].double() / eps, rtol=1e-15, atol=0)
    assert float(gx[z].abs().max()) < 3e38                                            # finite in float32 and bf16
    # the zero rows add nothing to gw: the sum over the other rows alone is the same
    xk, gk = x[keep].double(), go[keep].double()
    others = (gk * xk / (xk.pow(2).sum(1, keepdim=True).sqrt() + eps)).sum(0)
    assert float((gw - others).abs().max()) <= 1e-12 * float(gw.abs().max())         # (float64 sums in another order)
