"""GPU: the FPN neck as a module -- lateral convs, fork, fused upsample + add, output convs into one pyramid buffer, the extra stride-2 levels
in their three modes, the shared-input gradient junction -- forward and backward against the fp64 restatement of tests/fpn_util.py at
pyramids that are not an exact 2x, in both precisions.  Per run: every output, every input gradient, every weight and bias gradient within
the bound of tests/fpn_util.py (x3: 1e-4 of the tensor's maximum; fast mode: at most twice the error of the bf16-storage emulation, the x3
figure where the emulation is exact); the five
outputs are views of ONE buffer in level order (functional.pyramid_buffer: the head's level-batched convs read them in place); with the
inputs marked as the backbone marks them (functional.share_input_grad) every junction has delivered its sum."""
import pytest
import torch

from tests import fpn_util as U

pytestmark = pytest.mark.gpu

X_RUNS = [r for r in U.RUNS if r[2] == U.X]
B_RUNS = [r for r in U.RUNS if r[2] == U.B16]


@pytest.fixture
def x3_mode(_default_precision):
    """the reference-precision mode, whatever AOD_CONV_PREC the suite runs under (the autouse fixture restores that mode afterwards)"""
    from aod_meh_hua_amd import functional as AF
    AF.set_precision('bf16x3')


def _check(run, junction):
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    c = U.CASES[run[0]]
    assert AF.get_precision() == run[2]
    got, outs = U.run_module(run, junction)
    # one buffer, level order, every level a dense block of rows
    assert len(outs) == U.NUM_OUTS
    wd, r0 = ho.width(c.out_channels), 0
    for i, (o, (h, w)) in enumerate(zip(outs, U.out_shapes(c))):
        assert tuple(o.shape) == (c.B, wd, h, w) and o.dtype == torch.bfloat16, i
        assert o.permute(0, 2, 3, 1).is_contiguous(), i
        assert o.untyped_storage().data_ptr() == outs[0].untyped_storage().data_ptr(), i
        assert o.data_ptr() == outs[0].data_ptr() + r0 * wd * 2, f'level {i} does not start where level {i - 1} ends'
        r0 += c.B * h * w
    figs = U.figures(run, got, junction)
    assert len(figs) == 5 + len(c.levels) + 2 * (len(c.levels) * 2 + 2)
    worst = max(figs, key=lambda k: figs[k][0])
    print(f'{U.run_id(run)} junction={junction}: worst {worst} {figs[worst]}')
    for k, (fig, e, emu) in figs.items():
        if run[2] == U.X:
            assert fig < U.X3_BOUND, (k, fig)
        else:
            assert (emu > 0 or k.endswith('.bias')) and fig <= U.FAST_RATIO, (k, fig, e, emu)


@pytest.mark.parametrize('run', X_RUNS, ids=U.run_id)
def test_fpn_x3(run, x3_mode):
    _check(run, True)


@pytest.mark.parametrize('run', B_RUNS, ids=U.run_id)
def test_fpn_bf16(run, bf16_mode):
    _check(run, True)


@pytest.mark.parametrize('run', B_RUNS, ids=U.run_id)
def test_fpn_bf16_without_junction(run, bf16_mode):
    """(x3 has no such variant: an unmarked leaf with two consumers is summed by torch's bf16 add, which is not the product's path)"""
    _check(run, False)


def test_fpn_junction_counts_its_consumers(x3_mode):
    """'on_input': C5 feeds its lateral conv and the first extra conv, the other levels one conv each"""
    from aod_meh_hua_amd import functional as AF
    run = ('tiny', 'on_input', U.X)
    c, o = U.CASES[run[0]], U.operands(run)
    m = U.build_module(c, run[1], o['sd32'])
    xs = [AF.share_input_grad(x.detach().clone(memory_format=torch.preserve_format).requires_grad_()) for x in o['x_dev']]
    outs = m(tuple(xs))
    assert [x._aod_acc.n for x in xs] == [1, 1, 2]
    torch.autograd.backward(outs, o['g_dev'])
    torch.cuda.synchronize()
    assert all(x._aod_acc.partial is None and x._aod_acc.arrived == 0 for x in xs)
    AF.check_junctions()
