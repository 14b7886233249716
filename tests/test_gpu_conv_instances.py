"""Every kernel instance of the forward / dgrad convolution once, reached through hipops by a default plan (tests/conv_instances_util.py: the
cases, their operands and the fp64 reference).  Per case: (a) routing -- the plan of the launched descriptor is the case's, and the persistent
kernel's launch counter rises by exactly 1 for an X3P case and by 0 otherwise; (b) values, every element, after the ReLU: bf16 mode
allclose(rtol 1e-2, atol 1e-2) for a bf16 and (1e-4, 1e-4) for an fp32 destination, x3 max|got - ref| / max|ref| < 1e-4, column sums 5e-3 / 1e-4
of their largest -- the bounds tests/test_gpu_kernels.py and tests/test_gpu_x3_kernels.py hold these kernels to; (c) nothing else is
written: 64 guard rows behind the destination keep their sentinel bits, an X-layout destination has no non-zero pad column, and an
in-place lattice launch leaves every pixel that is not (even, even) bit-identical.  Members of a grouped launch carry their own operands
and filters and are checked one by one; column sums start non-zero and come back as start + sum."""
import pytest
import torch

from tests import conv_instances_util as U

pytestmark = pytest.mark.gpu


def where(c, plan, idx, N):
    """the worst element in the tile's terms, so that a tail bug names itself"""
    p = dict(zip(U.PLAN_FIELDS, plan))
    bm, bn = (128, 256 if p['wide'] else 128) if p['kind'] == U.X3P else (c.pw_tile if p['kind'] == U.PW else (p['bm'], p['bn']))
    row, col = divmod(idx, N)
    seg, r = 0, row
    rows = [b * h * w for b, h, w in c.segs] if c.dgrad else [s.rows for s in U.geometry(c)[1]]
    while seg + 1 < len(rows) and r >= rows[seg]:
        r -= rows[seg]
        seg += 1
    return f'row {row} (% {bm} = {row % bm}, row {r} of segment {seg}), column {col} (% {bn} = {col % bn})'


@pytest.mark.parametrize('name', list(U.CASES))
def test_instance(name):
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd._C import lib
    names = U.dispatch_variables_set()
    if names:
        pytest.fail(f'{names} set in the environment: the default plans are not what this test launches')
    c = U.CASES[name]
    plan = U.planned(name)
    assert plan == c.plan, (name, dict(zip(U.PLAN_FIELDS, plan)))
    count = lib.aod_conv_x3p_count()
    members = U.run(name)
    assert lib.aod_conv_x3p_count() - count == (1 if c.plan[0] == U.X3P else 0), f'{name}: launches of the persistent kernel'
    assert len(members) == max(c.members, 1)
    N = c.cin if c.dgrad else c.cout
    tol, cs_tol = U.bounds(c)
    for g, m in enumerate(members):
        M = m.ref.shape[0]
        assert m.got.shape == m.ref.shape == (M, N) and float(m.ref.abs().max()) > 0.5
        fig, mabs, worst, cs = U.errors(c, m)
        print(f'{name}[{g}]: ' + (f'relative max error {fig:.3e}' if tol is None else f'max abs error {mabs:.3e}, {fig:.3f} of the bound')
              + (f', column sums {cs:.3e}' if cs is not None else ''))
        at = where(c, plan, worst, N)
        if tol is None:
            assert fig < 1e-4, (name, g, fig, at)
        else:
            assert torch.allclose(m.got, m.ref, rtol=tol[0], atol=tol[1]), (name, g, mabs, fig, at)
        if cs is not None:
            assert cs < cs_tol, (name, g, 'column sums', cs)
        # nothing else is written
        words = m.full[M:].view(torch.int16)
        assert words.shape[0] == U.GUARD and bool((words == U.SENTINEL).all()), f'{name}[{g}]: rows behind the destination were written'
        if c.mode == U.X and not c.out_f32:
            assert m.full.shape[1] == ho.xw(N)
            if ho.xw(N) != 2 * N:                   # (an X-layout destination needs N % 32 == 0 today: no case has pad columns)
                assert float(ho.x3_merge(m.full[:M])[:, N:].abs().max()) == 0.0, f'{name}[{g}]: non-zero pad columns'
        if c.inplace:
            (b, h, w), = c.segs
            lat = torch.zeros(b, h, w, dtype=torch.bool, device='cuda')
            lat[:, ::2, ::2] = True
            off = ~lat.reshape(-1)
            assert torch.equal(m.full[:M][off].view(torch.int16), m.before[off].view(torch.int16)), f'{name}: a pixel off the lattice changed'
            assert not torch.equal(m.full[:M][~off], m.before[~off])


def test_members_of_a_grouped_case_differ():
    """(the operands of member g come from the generator seeded crc32(name) + g)"""
    name = 'bg128_1'
    a, b = U.run(name)
    assert not torch.equal(a.ref, b.ref) and not torch.equal(a.got, b.got)
