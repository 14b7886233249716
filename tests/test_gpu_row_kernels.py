"""GPU: the row kernels under and around the FPN neck, both precisions where a kernel has both forms, at 1x1 and one-column maps, H = 2h - 1,
channel pads, and one case each past the grid cap so that the grid-stride loops take a second trip (cases: tests/row_kernels_util.py).
A max selects a stored value and an add of two values is one fp32 operation followed by the kernel's own store, so the pool, the upsample
add, the layout kernels and the element-wise kernels are held to their expectation BIT FOR BIT (x3: the expectation goes through x3_split,
which test_x3_split_is_the_written_out_rounding pins to torch first); the upsample's adjoint is bounded element by element.  Every x3
result must also be canonical (row_kernels_util.canonical)."""
import pytest
import torch
import torch.nn.functional as F

from tests import row_kernels_util as R

pytestmark = pytest.mark.gpu

PRECS = ['bf16x3', 'bf16']


@pytest.fixture
def prec(request):
    """-> whether the x3 forms run: the reference-precision mode (`x3_mode` below), or the fast mode through the suite's `bf16_mode` fixture"""
    from aod_meh_hua_amd import functional as AF
    request.getfixturevalue('bf16_mode' if request.param == 'bf16' else 'x3_mode')
    assert AF.get_precision() == request.param
    return request.param == 'bf16x3'


both = pytest.mark.parametrize('prec', PRECS, indirect=True)


@pytest.fixture
def x3_mode(_default_precision):
    """the reference-precision mode, whatever AOD_CONV_PREC the suite runs under (the autouse fixture restores that mode afterwards)"""
    from aod_meh_hua_amd import functional as AF
    AF.set_precision('bf16x3')


def _canonical(rows, what):
    ok, ties = R.canonical(rows)
    print(f'{what}: {ties} of {rows.numel() // 2} values are half-spacing ties')
    assert ok, f'{what}: an X-layout result that is not the split of its value'
    assert ties <= max(8, rows.numel() // 2 // 100), (what, ties)          # (expected: 2^-10 of the values)


# ---------------------------------------------------------------------------------------------------------- x3_split / x3_merge
@pytest.mark.parametrize('C', R.SPLIT_CHANNELS)
def test_x3_split_is_the_written_out_rounding(C, x3_mode):
    from aod_meh_hua_amd import hipops as ho
    M = R.SPLIT_ROWS
    t = R.randn(C, M, C) * 3
    x = ho.x3_split(t)
    assert x.shape == (M, ho.xw(C)) and x.dtype == torch.bfloat16
    assert R.same_bits(x, R.split_in_torch(t))
    h, l = R.heads_tails(x)
    assert not R.bits(h[:, C:]).any() and not R.bits(l[:, C:]).any(), 'pad channels must be +0'
    back = ho.x3_merge(x, C)
    assert back.shape == (M, C) and torch.equal(back, h[:, :C].float() + l[:, :C].float())
    rel = float(((back.double() - t.double()).abs() / t.double().abs()).max())
    print(f'C={C}: round trip relative error {rel:.3e} (2^-17 = {2.0 ** -17:.3e})')
    assert rel <= 2.0 ** -17
    full = ho.x3_merge(x)
    assert full.shape == (M, ho.xw(C) // 2) and torch.equal(full[:, :C], back) and not full[:, C:].any()
    _canonical(x, f'split C={C}')


# ---------------------------------------------------------------------------------------------------------- max-pool
@both
@pytest.mark.parametrize('sign', ['mixed', 'negative'])
@pytest.mark.parametrize('shape', R.POOL_SHAPES, ids=str)
def test_maxpool(shape, sign, prec):
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd.hipops import Seg
    B, C, H, W = shape
    t = R.randn(H * 1000 + W, B, H, W, C)
    if sign == 'negative':          # padding must act as -inf, not 0
        t = -t.abs() - 0.25
    rows, x = R.rows_of(t, prec)
    out, s = ho.maxpool3x3s2(rows, Seg(B, H, W))
    torch.cuda.synchronize()
    assert (s.B, s.H, s.W) == (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1) and out.shape == (s.rows, rows.shape[1])
    want = F.max_pool2d(x.permute(0, 3, 1, 2).cpu(), 3, 2, 1).permute(0, 2, 3, 1)
    got = R.values_of(out, (B, s.H, s.W, C), prec).cpu()
    assert torch.equal(got, want)
    if sign == 'negative':
        assert float(got.max()) < 0
    if prec:
        _canonical(out, 'pool')


# ---------------------------------------------------------------------------------------------------------- upsample + add
def _expected_sum(lat, top, H, W, x3):
    from aod_meh_hua_amd import hipops as ho
    v = lat + R.up_nearest(top, H, W)          # one fp32 add of two stored values
    flat = v.reshape(-1, v.shape[-1]).contiguous()
    return ho.x3_split(flat) if x3 else flat.bfloat16()


@both
@pytest.mark.parametrize('case', R.UPSAMPLE_CASES, ids=str)
def test_upsample_add(case, prec):
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd.hipops import Seg
    B, C, (h, w), (H, W) = case
    lat_rows, lat = R.rows_of(R.randn(H * 100 + W, B, H, W, C), prec)
    top_rows, top = R.rows_of(R.randn(h * 100 + w + 7, B, h, w, C), prec)
    lat_before, top_before = lat_rows.clone(), top_rows.clone()
    out = ho.upsample_add(lat_rows, Seg(B, H, W), top_rows, Seg(B, h, w))
    torch.cuda.synchronize()
    assert R.same_bits(out, _expected_sum(lat, top, H, W, prec))
    assert R.same_bits(lat_rows, lat_before) and R.same_bits(top_rows, top_before), 'the out-of-place form wrote an operand'
    assert out.data_ptr() != lat_rows.data_ptr()
    if prec:
        _canonical(out, 'upsample_add')


@pytest.mark.parametrize('case', R.UPSAMPLE_CASES, ids=str)
def test_upsample_add_in_place_bf16(case, bf16_mode):
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd.hipops import Seg
    B, C, (h, w), (H, W) = case
    lat_rows, lat = R.rows_of(R.randn(H * 100 + W, B, H, W, C), False)
    top_rows, top = R.rows_of(R.randn(h * 100 + w + 7, B, h, w, C), False)
    top_before = top_rows.clone()
    ret = ho.upsample_add_(lat_rows, Seg(B, H, W), top_rows, Seg(B, h, w))
    torch.cuda.synchronize()
    assert ret.data_ptr() == lat_rows.data_ptr()
    assert R.same_bits(lat_rows, _expected_sum(lat, top, H, W, False)) and R.same_bits(top_rows, top_before)


@both
@pytest.mark.parametrize('case', R.ADJOINT_CASES, ids=str)
def test_upsample_adjoint(case, prec):
    """set form (both precisions; every source element written: the destination starts as NaN) and the bf16 accumulate form on a non-zero
    destination, against autograd of F.interpolate in fp64"""
    fig, acc, got_rows, wrapped = R.adjoint_figures(case, prec)
    bound = R.X3_ADJ_BOUND if prec else R.FAST_ADJ_BOUND
    print(f'{case}: set {fig / bound:.3f} of the bound' + (f', accumulate {acc / bound:.3f}' if acc is not None else ''))
    assert fig <= bound, (fig, bound)
    assert R.same_bits(wrapped, got_rows), 'hipops.upsample_add_bwd is another launch than the one checked'
    if prec:
        _canonical(got_rows, 'adjoint')
    else:
        assert acc <= bound, (acc, bound)


# ---------------------------------------------------------------------------------------------------------- layout
def _image(B, C, H, W):
    return R.randn(C * 7 + H, B, C, H, W) * 2


@pytest.mark.parametrize('size', R.ROWS_SIZES, ids=str)
@pytest.mark.parametrize('C,cpad', R.ROWS_CHANNELS)
def test_nchw_to_rows(C, cpad, size, bf16_mode):
    from aod_meh_hua_amd import hipops as ho
    B, H, W = size
    img = _image(B, C, H, W)
    out, segs = ho.nchw_to_rows(img, cpad)
    torch.cuda.synchronize()
    want = F.pad(img.permute(0, 2, 3, 1).reshape(-1, C), (0, cpad - C)).bfloat16()          # (F.pad writes +0)
    assert (segs[0].B, segs[0].H, segs[0].W, segs[0].row0) == (B, H, W, 0)
    assert R.same_bits(out, want) and not R.bits(out[:, C:]).any()


def _s2d(img):
    """slot (dy * 2 + dx) * C + c of space-to-depth pixel (Y, X) = pixel (2Y + dy, 2X + dx) of channel c; the slots from 4C on are +0"""
    B, C, H, W = img.shape
    v = img.view(B, C, H // 2, 2, W // 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(-1, 4 * C)
    return F.pad(v, (0, 16 - 4 * C))


@both
@pytest.mark.parametrize('size', R.S2D_SIZES, ids=str)
@pytest.mark.parametrize('C', [1, 3, 4])
def test_nchw_to_s2d_rows(C, size, prec):
    from aod_meh_hua_amd import hipops as ho
    B, H, W = size
    img = _image(B, C, H, W)
    out, segs = ho.nchw_to_s2d_rows(img)
    torch.cuda.synchronize()
    assert (segs[0].B, segs[0].H, segs[0].W) == (B, H // 2, W // 2) and out.shape == (B * H * W // 4, 64 if prec else 16)
    v = _s2d(img)
    assert R.same_bits(out, ho.x3_split(v) if prec else v.bfloat16())
    if prec:
        h, l = R.heads_tails(out)
        assert not R.bits(h[:, 4 * C:]).any() and not R.bits(l[:, 4 * C:]).any()
        _canonical(out, 's2d')
    else:
        assert not R.bits(out[:, 4 * C:]).any()


@both
@pytest.mark.parametrize('hw', [(3, 4), (4, 3), (5, 5)])
def test_nchw_to_s2d_rows_refuses_odd_sizes(hw, prec):
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd._C import AodHipError
    with pytest.raises(AodHipError):
        ho.nchw_to_s2d_rows(_image(1, 3, *hw))
    with pytest.raises(AodHipError):
        ho.nchw_to_s2d_rows(_image(1, 5, 4, 4))


@pytest.mark.parametrize('size', R.ROWS_SIZES, ids=str)
@pytest.mark.parametrize('C', [1, 3, 32])
def test_image_to_nhwc_x3(C, size, x3_mode):
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    assert AF.get_precision() == 'bf16x3'
    B, H, W = size
    img = _image(B, C, H, W)
    out = AF.image_to_nhwc(img)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (B, 64, H, W) and out.dtype == torch.bfloat16
    rows = AF.as_rows(out)
    assert rows.data_ptr() == out.data_ptr()
    assert R.same_bits(rows, ho.x3_split(img.permute(0, 2, 3, 1).reshape(-1, C).contiguous()))
    h, l = R.heads_tails(rows)
    assert not R.bits(h[:, C:]).any() and not R.bits(l[:, C:]).any()
    _canonical(rows, 'image_to_nhwc')


# ---------------------------------------------------------------------------------------------------------- element-wise
@pytest.mark.parametrize('n', R.X3_ADD_SIZES)
def test_x3_add(n, x3_mode):
    from aod_meh_hua_amd import hipops as ho
    a, va = R.rows_of(R.randn(1, 1, 1, n // 64, 32), True)
    b, vb = R.rows_of(R.randn(2, 1, 1, n // 64, 32), True)
    assert a.numel() == n
    a0, b0 = a.clone(), b.clone()
    out = ho.x3_add(a, b)
    torch.cuda.synchronize()
    assert R.same_bits(out, ho.x3_split((va + vb).view(-1, 32)))
    assert R.same_bits(a, a0) and R.same_bits(b, b0)
    _canonical(out, 'x3_add')


@pytest.mark.parametrize('n', R.ADD_RELU_SIZES)
def test_add_relu(n, bf16_mode):
    from aod_meh_hua_amd import hipops as ho
    a, b = R.randn(3, n // 8, 8).bfloat16(), R.randn(4, n // 8, 8).bfloat16()
    out = ho.add_relu(a, b)
    torch.cuda.synchronize()
    want = torch.relu(a.float() + b.float()).bfloat16()
    assert R.same_bits(out, want) and float(out.float().min()) >= 0.0 and float(out.float().max()) > 0.0
