"""No device: the fp64 restatement of FPN.forward that tests/test_gpu_fpn.py holds the neck to (tests/fpn_util.py) against the oracle's, and
the nearest-neighbour source index the upsample kernels compute against torch's."""
import pytest
import torch
import torch.nn.functional as F

from tests import fpn_util as U


def _case_operands(case, extra):
    c = U.CASES[case]
    xs, sd, gys = U.raw_operands(case, extra)
    return c, [x.double() for x in xs], {k: v.double() for k, v in sd.items()}, [g.double() for g in gys]


def test_reference_equals_the_oracle_bit_for_bit():
    """the shipped configuration (start_level 1, 'on_input', 5 outputs): oracle.model.fpn on the same fp64 tensors, outputs and gradients"""
    from oracle import model as om
    c, xs, sd, gys = _case_operands('odd', 'on_input')
    assert (c.in_channels, c.out_channels, c.start_level) == U.PROD
    got = U.run_reference(c, 'on_input', xs, sd, gys)
    xo = [x.clone().requires_grad_() for x in xs]
    so = {k: v.clone().requires_grad_() for k, v in sd.items()}
    outs = om.fpn({'neck.' + k: v for k, v in so.items()}, [None] + xo)
    assert len(outs) == U.NUM_OUTS
    want = U.grads_of(xo, so, outs, gys)
    assert set(got) == set(want) and len(got) == 5 + 3 + 16
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert [tuple(o.shape[2:]) for o in outs] == U.out_shapes(c)


@pytest.mark.parametrize('extra', ['on_input', 'on_lateral', 'on_output'])
def test_reference_shapes_and_sources_of_the_extra_levels(extra):
    """start_level 0 and the three extra-conv modes: P6 reads C5, the top lateral or the top output (the other two get no gradient from it)"""
    c, xs, sd, gys = _case_operands('tiny', extra)
    assert c.start_level == 0
    xs = [x.requires_grad_() for x in xs]
    outs = U.reference(xs, sd, 0, extra)
    assert [tuple(o.shape) for o in outs] == [(c.B, c.out_channels, h, w) for h, w in U.out_shapes(c)]
    n = len(xs)
    src = {'on_input': xs[-1], 'on_lateral': F.conv2d(xs[-1], sd[f'lateral_convs.{n - 1}.conv.weight'], sd[f'lateral_convs.{n - 1}.conv.bias']),
           'on_output': outs[n - 1]}[extra]
    assert torch.equal(outs[n], F.conv2d(src, sd[f'fpn_convs.{n}.conv.weight'], sd[f'fpn_convs.{n}.conv.bias'], 2, 1))
    assert set(U.param_shapes(c, extra)) == {k[:-len('.weight')] for k in sd if k.endswith('.weight')}
    assert sd[f'fpn_convs.{n}.conv.weight'].shape[1] == (c.in_channels[-1] if extra == 'on_input' else c.out_channels)


def test_emulation_stores_bf16_in_both_directions():
    x = (torch.randn(64, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 3).requires_grad_()
    g = torch.randn(64, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    y = U.RoundBoth.apply(x)
    y.backward(g)
    assert torch.equal(y.detach(), x.detach().bfloat16().double()) and torch.equal(x.grad, g.bfloat16().double())
    assert not torch.equal(y.detach(), x.detach()) and not torch.equal(x.grad, g)
    # the emulation differs from the fp64 chain in every tensor, and by no more than a few bf16 roundings
    c, xs, sd, gys = _case_operands('tiny', 'on_input')
    q = lambda ts: [t.bfloat16().double() for t in ts]
    xs, gys, sd = q(xs), q(gys), {k: (v.bfloat16().double() if k.endswith('.weight') else v) for k, v in sd.items()}
    ref = U.run_reference(c, 'on_input', xs, sd, gys)
    for junction in (True, False):
        emu = U.run_reference(c, 'on_input', xs, sd, gys, store=U.RoundBoth.apply, junction=junction)
        exact = {k for k in ref if U.err(emu[k], ref[k]) == 0}
        # (an output conv whose output feeds nothing else: its bias gradient is the column sum of the given gradient, which no store touches)
        assert exact == {f'd:fpn_convs.{i}.conv.bias' for i in (0, 1, 2, 4)}, (exact, junction)
        for k in ref:
            assert U.err(emu[k], ref[k]) < 8 * 2.0 ** -8, (k, junction)


def _pairs():
    """every (h, H) of a top-down step or a row-kernel case: all levels of the cases, widths included, and H in {2h - 1, 2h} for h <= 69"""
    from tests import row_kernels_util as R
    pairs = set()
    for c in U.CASES.values():
        for (H, W), (h, w) in zip(c.levels, c.levels[1:]):
            pairs |= {(h, H), (w, W)}
    for (h, w), (H, W) in R.UPSAMPLE_PAIRS:
        pairs |= {(h, H), (w, W)}
    for h in range(1, 70):
        pairs |= {(h, 2 * h - 1), (h, 2 * h)}
    return sorted(pairs)


def test_nearest_index_formula_is_torchs():
    """csrc/elementwise.hip, csrc/x3_ops.hip: source index min(y * h // H, h - 1); the adjoint's range [ceil(s * H / h), ceil((s + 1) * H / h))
    is its preimage"""
    pairs = _pairs()
    assert (7, 13) in pairs and (10, 19) in pairs and (1, 1) in pairs and (33, 66) in pairs and (40, 79) in pairs
    for h, H in pairs:
        want = F.interpolate(torch.arange(h, dtype=torch.float64).view(1, 1, h, 1), size=(H, 1), mode='nearest').view(H).long().tolist()
        got = [min(y * h // H, h - 1) for y in range(H)]
        assert got == want, (h, H)
        for s in range(h):
            y0, y1 = (s * H + h - 1) // h, min(H, ((s + 1) * H + h - 1) // h)
            assert list(range(y0, y1)) == [y for y in range(H) if got[y] == s], (h, H, s)
