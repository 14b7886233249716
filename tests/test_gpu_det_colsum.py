"""GPU: the VALUES of the deterministic mode's column sums (functional.set_deterministic, csrc/determinism.hip) against fp64 -- every producer
of partial rows once, at the shapes where its row index, its pitch or the finalize's loops can go wrong: the epilogue of conv_igemm_kernel
(plain, grouped, the two-pass 256 x 256 tile), conv_splitk_finalize_kernel, x3_act_bwd_kernel, act_bwd_kernel (dbeta | dgamma, the dst2 form
and the dgamma-only form of the finalize), the three pad_cast_colsum kernels and the two L2Norm backward kernels; and the dispatch the mode
changes (no persistent kernel, no streaming 1x1 kernel, no halo kernel for a launch with column sums; sparse and fused backward off).

Every deterministic launch runs twice, behind a poison launch that leaves +1.25e31 and then -1.25e31 in the front of the shared scratch
(tests/det_colsum_util.py): a partial row the launch did not write, or a row the finalize reads beyond those written, ends 26 orders of
magnitude off; the two results must be bit-equal, and each within the bound the kernel's default-mode test holds it to.  The row kernels also
run in the default mode at these shapes.  Every test prints the used fraction of its bounds (docs/LAB_NOTES.md records the largest)."""
import pytest
import torch

from tests import conv_instances_util as U
from tests import det_colsum_util as D

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def relerr(got, ref):
    """max|got - ref| / max|ref| in fp64 (inf when anything is not finite)"""
    d = (got.double() - ref.double()).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    return float(d.max() / (ref.double().abs().max() + 1e-30))


def frac(got, ref, rtol, atol):
    """the used fraction of allclose(rtol, atol): max |got - ref| / (atol + rtol |ref|) (inf when anything is not finite)"""
    ref = ref.double()
    d = (got.double() - ref).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    return float((d / (atol + rtol * ref.abs())).max())


def det_twice(fn):
    """fn() in the deterministic mode behind the + poison and again behind the - poison -> the two results (tuples of tensors, cloned)"""
    out = []
    with D.deterministic():
        for sign in (1, -1):
            D.poison(sign)
            out.append(tuple(t.clone() if t is not None else None for t in fn()))
    torch.cuda.synchronize()
    return out


def default_once(fn):
    from aod_meh_hua_amd._C import lib
    assert lib.aod_get_deterministic() == 0
    out = tuple(t.clone() if t is not None else None for t in fn())
    torch.cuda.synchronize()
    return out


def rnd_gen(seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return lambda *sh: torch.randn(*sh, device='cuda', generator=g)


# --------------------------------------------------------------------------------------------------------------------------- the scratch
def test_every_launch_fits_the_poisoned_extent():
    floats = D.all_floats()
    worst = max(floats, key=floats.get)
    print(f'largest launch: {worst}, {floats[worst]} floats of {D.POISON_FLOATS} poisoned')
    assert len(floats) == 11 + 4 + 4 + 12 + 11 + 2
    assert 0 < floats[worst] < D.POISON_FLOATS, (worst, floats[worst])
    # (the rules above reproduce the launchers': 65 and 1094 strips of the activation backward, 10 row blocks of the split-K finalize)
    assert D.strips(4099, 8) == 65 and D.strips(70001, 1) == 1094 and D.conv_floats('bsplit_d') == 10 * 320
    assert D.x3_pad_cast_form(256) == 'v8' and D.x3_pad_cast_form(260) == 'scalar' and D.x3_pad_cast_form(9) == 'scalar'


# ------------------------------------------------------------------------------------------------------------------------ conv launches
def _clean_dispatch():
    names = U.dispatch_variables_set()
    if names:
        pytest.fail(f'{names} set in the environment: the default plans are not what this test launches')


def test_cases_with_column_sums():
    assert D.COLSUM_CASES == ['b256_1', 'b128w8_1', 'bg256_1', 'bsplit_d', 'bpw_d', 'pw_128x128', 'x256_1', 'xg256_1', 'xsplit_d', 'p1402', 'p9800_d']
    assert set(D.DET_PLANS) == set(D.COLSUM_CASES)
    for name in ('bsplit_d', 'xsplit_d'):
        c = U.CASES[name]
        M = sum(b * h * w for b, h, w in c.segs)
        assert c.plan[0] == U.SPLIT_K and len(c.segs) >= 2 and M % 8 != 0 and c.cin > 256 and c.cin % 256 != 0


@pytest.mark.parametrize('name', list(U.CASES))
def test_plan_in_the_deterministic_mode(name):
    """the mode moves launches WITH column sums off the persistent and the streaming kernel, and nothing else (plan calls only)"""
    _clean_dispatch()
    c = U.CASES[name]
    plan = D.planned_det(name)
    if c.ops & U.COLSUM:
        assert plan == D.DET_PLANS[name], (name, dict(zip(U.PLAN_FIELDS, plan)))
        assert plan[0] not in (U.X3P, U.PW), name
        assert (plan != c.plan) == (c.plan[0] in (U.X3P, U.PW)), name
    else:
        assert plan == c.plan, (name, dict(zip(U.PLAN_FIELDS, plan)))
    assert U.planned(name) == c.plan          # (and the switch is back)


@pytest.mark.parametrize('name', D.COLSUM_CASES)
def test_conv_column_sums(name):
    from aod_meh_hua_amd._C import lib
    _clean_dispatch()
    c = U.CASES[name]
    tol, cs_tol = U.bounds(c)
    ops = U.operands(name)
    same_plan = D.DET_PLANS[name] == c.plan
    free = U.launch(name, ops) if same_plan else None
    runs = []
    with D.deterministic():
        assert U.planned(name) == D.DET_PLANS[name]
        count = lib.aod_conv_x3p_count()
        for sign in (1, -1):
            D.poison(sign)
            runs.append(U.launch(name, ops))
        assert lib.aod_conv_x3p_count() == count, f'{name}: the persistent kernel ran in the deterministic mode'
    assert all(len(r) == max(c.members, 1) for r in runs)
    for g, (a, b) in enumerate(zip(*runs)):
        M = a.ref.shape[0]
        for tag, m in (('+', a), ('-', b)):
            fig, mabs, worst, cs = U.errors(c, m)
            print(f'{name}[{g}] {tag}poison: column sums {cs:.3e} of {cs_tol:g}, rows ' + (f'{fig:.3e}' if tol is None else f'{mabs:.3e} ({fig:.3f} of the bound)'))
            assert cs < cs_tol, (name, g, tag, 'column sums', cs)
            if same_plan:
                assert same(m.full, free[g].full), f'{name}[{g}] {tag}: the rows differ from the default mode\'s'
            elif tol is None:
                assert fig < 1e-4, (name, g, tag, fig)
            else:
                assert torch.allclose(m.got, m.ref, rtol=tol[0], atol=tol[1]), (name, g, tag, mabs, fig)
            words = m.full[M:].view(torch.int16)
            assert words.shape[0] == U.GUARD and bool((words == U.SENTINEL).all()), f'{name}[{g}] {tag}: rows behind the destination were written'
        assert same(a.cs_got, b.cs_got), f'{name}[{g}]: the column sums depend on what the scratch held'
        assert same(a.full, b.full)
    if same_plan:
        for g, m in enumerate(free):          # (the default mode's own sums, on these operands)
            assert U.errors(c, m)[3] < cs_tol, (name, g, 'default mode')


def test_python_gates():
    """with the mode on: no sparse backward, no fused bottleneck backward (both sum their columns with atomics)"""
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd.models.backbones.resnet import Bottleneck
    blk = Bottleneck(512, 128).cuda().eval()
    for prec in ('bf16x3', 'bf16'):
        AF.set_precision(prec)
        x = torch.randn(2, 512, 8, 8, device='cuda')
        rows = x.permute(0, 2, 3, 1).reshape(-1, 512).contiguous()
        xx = AF.as_nchw(ho.x3_split(rows) if prec == 'bf16x3' else rows.bfloat16(), 2, 8, 8).requires_grad_()
        assert ho.sparse_bwd() == (prec == 'bf16x3')
        assert isinstance(AF.bwd_chain_for(blk, xx), AF.BwdChain)
        with D.deterministic():
            assert ho.DETERMINISTIC and AF.mode_key() == (prec, True)
            assert ho.sparse_bwd() is False
            assert AF.bwd_chain_for(blk, xx) is None
        assert not ho.DETERMINISTIC and ho.sparse_bwd() == (prec == 'bf16x3')


def test_halo_dgrad_with_column_sums_stays_on_the_general_kernel(bf16_mode, monkeypatch):
    """AOD_HALO_CONV=all routes qualifying 3x3 dgrads to aod_halo_conv3x3, whose column sums are atomics: not in the deterministic mode"""
    from aod_meh_hua_amd import hipops as ho
    rnd = rnd_gen(3)
    B, H, W, Cin, O = 2, 9, 11, 64, 40
    segs = [ho.Seg(B, H, W, 0)]
    dz = rnd(B * H * W, O).bfloat16()
    wq = (rnd(O, Cin, 3, 3) / 19.0).bfloat16().float()
    wd = ho.pack_weight_dgrad(wq, O)
    mask = rnd(B * H * W, Cin).bfloat16()
    calls = []
    orig = ho.call
    monkeypatch.setattr(ho, 'call', lambda name, *a: (calls.append(name), orig(name, *a))[1])
    monkeypatch.setattr(ho, 'HALO_ALL', True)
    monkeypatch.setattr(ho, 'HALO_CONV', True)

    def go(colsum):
        calls.clear()
        cs = torch.zeros(Cin, device='cuda') if colsum else None
        out = ho.conv2d_dgrad_rows(dz, segs, segs, wd, Cin, 3, 3, 1, 1, 1, mask=mask, colsum=cs)
        torch.cuda.synchronize()
        return [n for n in calls if n.startswith('aod_halo') or n.startswith('aod_conv2d')], out, cs
    assert go(True)[0] == ['aod_halo_conv3x3'] and go(False)[0] == ['aod_halo_conv3x3']
    with D.deterministic():
        D.poison(1)
        names, out_a, cs_a = go(True)
        assert names == ['aod_conv2d_ws'], names
        D.poison(-1)
        _, out_b, cs_b = go(True)
        assert go(False)[0] == ['aod_halo_conv3x3']          # (without column sums nothing is order-dependent: the route stays)
    assert same(cs_a, cs_b) and same(out_a, out_b)
    dzn = dz.double().cpu().view(B, H, W, O).permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv_transpose2d(dzn, wq.double().cpu(), stride=1, padding=1).permute(0, 2, 3, 1).reshape(-1, Cin)
    ref = torch.where(mask.double().cpu() > 0, ref, torch.zeros_like(ref))
    e = relerr(cs_a.cpu(), ref.sum(0))
    print(f'halo-shaped dgrad on the general kernel: column sums {e:.3e} of 5e-3')
    assert e < 5e-3 and torch.allclose(out_a.double().cpu(), ref, rtol=1e-2, atol=1e-2)


# -------------------------------------------------------------------------------------------------------------------------- row kernels
@pytest.fixture
def x3_mode(_default_precision):
    from aod_meh_hua_amd import functional as AF
    AF.set_precision('bf16x3')
    yield


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('M,C', D.ACT_SHAPES)
def test_x3_act_bwd(M, C, relu, x3_mode):
    from aod_meh_hua_amd import hipops as ho
    rnd = rnd_gen(11 + M)
    gx, ax = ho.x3_split(rnd(M, C)), ho.x3_split(rnd(M, C))
    g64 = ho.x3_merge(gx, C).double()
    ref = torch.where(ho.x3_merge(ax, C) > 0, g64, torch.zeros_like(g64)) if relu else g64
    want_dz = not (M == 63 and not relu)
    fn = lambda: [t for i, t in enumerate(ho.act_bwd(gx, ax if relu else None, relu=relu, want_dz=want_dz)) if i in (0, 2)]
    free, (a, b) = default_once(fn), det_twice(fn)
    assert (free[0] is None) == (not want_dz)
    for tag, (dz, cs) in (('default', free), ('+poison', a), ('-poison', b)):
        e = relerr(cs[:C], ref.sum(0))
        print(f'x3_act_bwd {M} x {C} relu {relu} {tag}: column sums {e / 1e-5:.3f} of the bound')
        assert cs.shape == (C,) and e < 1e-5, (tag, e)
        if want_dz:
            assert relerr(ho.x3_merge(dz, C), ref) < 2e-5
    assert same(a[1], b[1]), 'the column sums depend on what the scratch held'
    if want_dz:
        assert same(a[0], free[0]) and same(b[0], free[0])


def _act_operands(M, N, seed):
    rnd = rnd_gen(seed)
    u = torch.Generator(device='cuda').manual_seed(seed + 1)
    uni = lambda n: torch.rand(n, device='cuda', generator=u)
    o = dict(g=rnd(M, N).bfloat16(), a=torch.relu(rnd(M, N)).bfloat16(), z=rnd(M, N).bfloat16(), mean=rnd(N) * 0.1, invstd=1.0 / torch.sqrt(uni(N) + 0.5),
             g32=rnd(M, N))
    o['scale'] = (uni(N) + 0.5) * o['invstd']
    gm = torch.where(o['a'] > 0, o['g'].double(), torch.zeros(M, N, dtype=torch.float64, device='cuda'))
    o['ref_dbeta'], o['ref_dgamma'] = gm.sum(0), (gm * (o['z'].double() - o['mean'].double()) * o['invstd'].double()).sum(0)
    o['ref_dz'], o['ref_gm'] = gm * o['scale'].double(), gm
    return o


@pytest.mark.parametrize('M,N', D.ACT_BF16_SHAPES)
def test_act_bwd(M, N, bf16_mode):
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd._C import call, ptr, stream
    o = _act_operands(M, N, 100 + M)
    figs = {}

    def note(key, tag, f):
        figs[key] = max(figs.get(key, 0.0), f)
        assert f < 1, (key, tag, f)
    # (1) bf16 g, relu, BN: dbeta and dgamma in one finalize (dst2)
    fn = lambda: ho.act_bwd(o['g'], o['a'], o['z'], o['scale'], o['mean'], o['invstd'], relu=True, want_gm=True)
    free, (a, b) = default_once(fn), det_twice(fn)
    for tag, (dz, gm, dbeta, dgamma) in (('default', free), ('+poison', a), ('-poison', b)):
        note('dbeta', tag, frac(dbeta, o['ref_dbeta'], 1e-3, 1e-2))
        note('dgamma', tag, frac(dgamma, o['ref_dgamma'], 1e-3, 2e-2))
        assert frac(dz, o['ref_dz'], 1e-2, 1e-2) < 1 and frac(gm, o['ref_gm'], 1e-2, 1e-3) < 1
    assert same(a[2], b[2]) and same(a[3], b[3]), 'the column sums depend on what the scratch held'
    assert all(same(r[0], free[0]) and same(r[1], free[1]) for r in (a, b))
    # (2) fp32 g, no relu, no z: dbeta alone
    fn = lambda: [t for i, t in enumerate(ho.act_bwd(o['g32'], relu=False)) if i in (0, 2)]
    free, (a, b) = default_once(fn), det_twice(fn)
    for tag, (dz, dbeta) in (('default', free), ('+poison', a), ('-poison', b)):
        note('dbeta fp32', tag, frac(dbeta, o['g32'].double().sum(0), 1e-3, 1e-2))
        assert torch.equal(dz, o['g32'].bfloat16())
    assert same(a[1], b[1]) and same(a[0], free[0])
    # (3) dgamma alone (dbeta null): the finalize reads the SECOND partial image; destinations start non-zero, the finalize adds
    start = rnd_gen(7)(N)

    def dgamma_only():
        dg = start.clone()
        call('aod_act_bwd', ptr(o['g']), ptr(o['a']), ptr(o['z']), ptr(o['scale']), ptr(o['mean']), ptr(o['invstd']), None, None, None, ptr(dg),
             M, N, 1, 0, stream())
        return (dg,)
    free, (a, b) = default_once(dgamma_only), det_twice(dgamma_only)
    for tag, (dg,) in (('default', free), ('+poison', a), ('-poison', b)):
        note('dgamma alone', tag, frac(dg, start.double() + o['ref_dgamma'], 1e-3, 2e-2))
    assert same(a[0], b[0])
    # ... and both through the raw entry with non-zero starts
    def both():
        db, dg = start.clone(), (2 * start).clone()
        call('aod_act_bwd', ptr(o['g']), ptr(o['a']), ptr(o['z']), ptr(o['scale']), ptr(o['mean']), ptr(o['invstd']), None, None, ptr(db), ptr(dg),
             M, N, 1, 0, stream())
        return db, dg
    (a, b) = det_twice(both)
    note('dbeta', 'start', frac(a[0], start.double() + o['ref_dbeta'], 1e-3, 1e-2))
    note('dgamma', 'start', frac(a[1], 2 * start.double() + o['ref_dgamma'], 1e-3, 2e-2))
    assert same(a[0], b[0]) and same(a[1], b[1])
    print(f'act_bwd {M} x {N}: used fractions ' + ', '.join(f'{k} {v:.3f}' for k, v in figs.items()))


def _x3_pad_cast_check(M, N, gg, ro, ref, runs, nan_col=None):
    """runs: (tag, (dz, cs[, map])) of one shape; ref fp64 [M, N]"""
    from aod_meh_hua_amd import hipops as ho
    Np = ho.xw(N) // 2
    cols = [c for c in range(N) if c != nan_col]
    cs_ref = ref[:, cols].sum(0)
    worst = 0.0
    for tag, r in runs:
        dz, cs = r[0], r[1]
        e = relerr(cs[:N][cols], cs_ref)
        worst = max(worst, e)
        assert cs.shape == (Np,) and e < 1e-5, (M, N, tag, e)
        assert float(cs[N:].abs().max()) == 0.0 if Np > N else True
        if nan_col is not None:
            assert bool(torch.isnan(cs[nan_col]))
        if nan_col is None:
            if D.x3_pad_cast_form(N) == 'v8':          # heads / tails are the roundings of x3_split, bit for bit
                assert torch.equal(dz, ho.x3_split(torch.nn.functional.pad(ref.float(), (0, Np - N))))
            else:
                assert relerr(ho.x3_merge(dz, N), ref) < 2e-5
                if Np > N:
                    assert float(ho.x3_merge(dz)[:, N:].abs().max()) == 0.0
    return worst


@pytest.mark.parametrize('M,N', D.X3_PAD_CAST)
def test_x3_pad_cast_colsum(M, N, x3_mode):
    from aod_meh_hua_amd import hipops as ho
    rnd = rnd_gen(1000 + N + M)
    gg = rnd(M, N)
    ro = rnd(M, N) if M > 63 else None
    ref = (torch.where(ro > 0, gg, torch.zeros_like(gg)) if ro is not None else gg).double()
    fn = lambda: ho.pad_cast_colsum(gg, ho.xw(N), ro)
    free, (a, b) = default_once(fn), det_twice(fn)
    worst = _x3_pad_cast_check(M, N, gg, ro, ref, (('default', free), ('+poison', a), ('-poison', b)))
    print(f'x3_pad_cast_colsum {M} x {N} ({D.x3_pad_cast_form(N)}): column sums {worst / 1e-5:.3f} of the bound')
    assert same(a[1], b[1]), 'the column sums depend on what the scratch held'
    assert same(a[0], free[0]) and same(b[0], free[0])


@pytest.mark.parametrize('M,N', D.X3_PAD_CAST_MAP)
def test_x3_pad_cast_colsum_row_map(M, N, x3_mode):
    """the row-activity map: byte b = any value of rows 64 b .. 64 b + 63 fails v == 0 (a NaN counts, -0 does not)"""
    from aod_meh_hua_amd import hipops as ho
    rnd = rnd_gen(2000 + N)
    gg, ro = rnd(M, N), rnd(M, N)
    nb = (M + 63) // 64
    blocks = torch.arange(M, device='cuda') // 64
    gg[(blocks % 3 == 0) | (blocks == nb - 1)] = 0.0          # whole blocks of zeros, the ragged last one among them
    gg[64 * 6 + 5:64 * 6 + 9] = -0.0
    nan_row, nan_col = 64 * 9 + 17, N - 2                    # (block 9 is all zero but for this)
    gg[nan_row, nan_col] = float('nan')
    ro[nan_row, nan_col] = 1.0
    ref = torch.where(ro > 0, gg, torch.zeros_like(gg)).double()
    want = torch.zeros(nb * 64, dtype=torch.bool, device='cuda')
    want[:M] = (ref != 0).any(1)
    want = want.view(nb, 64).any(1).to(torch.uint8)
    assert int(want[9]) == 1 and int(want[6]) == 0 and int(want[nb - 1]) == 0 and 0 < int(want.sum()) < nb
    fn = lambda: ho.pad_cast_colsum(gg, ho.xw(N), ro, want_map=True)
    free, (a, b) = default_once(fn), det_twice(fn)
    plain = default_once(lambda: ho.pad_cast_colsum(gg, ho.xw(N), ro))
    for tag, (dz, cs, rmap) in (('default', free), ('+poison', a), ('-poison', b)):
        assert rmap.dtype == torch.uint8 and torch.equal(rmap, want), (tag, int((rmap != want).sum()))
        assert same(dz, plain[0])
    _x3_pad_cast_check(M, N, gg, ro, ref, (('default', free), ('+poison', a), ('-poison', b)), nan_col=nan_col)
    assert same(a[1], b[1])


@pytest.mark.parametrize('N', D.PAD_CAST_N)
def test_pad_cast_colsum(N, bf16_mode):
    from aod_meh_hua_amd import hipops as ho
    npad = (N + 7) // 8 * 8
    worst = 0.0
    for M in D.PAD_CAST_M(N):
        rnd = rnd_gen(3000 + N + M)
        g32, ro = rnd(M, N), rnd(M, N)
        for g in (g32, g32.bfloat16()):
            for relu_out in (None, ro):
                ref = g.double() if relu_out is None else torch.where(ro > 0, g.double(), torch.zeros(M, N, dtype=torch.float64, device='cuda'))
                fn = lambda: ho.pad_cast_colsum(g, npad, relu_out)
                free, (a, b) = default_once(fn), det_twice(fn)
                for tag, (dz, cs) in (('default', free), ('+poison', a), ('-poison', b)):
                    f = frac(cs[:N], ref.sum(0), 1e-4, 1e-3)
                    worst = max(worst, f)
                    assert cs.shape == (npad,) and f < 1, (M, N, g.dtype, relu_out is not None, tag, f)
                    assert dz.shape == (M, npad) and torch.equal(dz[:, :N], ref.bfloat16())
                    if npad > N:
                        assert float(dz[:, N:].float().abs().max()) == 0.0 and float(cs[N:].abs().max()) == 0.0
                assert same(a[1], b[1]), 'the column sums depend on what the scratch held'
                assert same(a[0], free[0]) and same(b[0], free[0])
    print(f'pad_cast_colsum N = {N}: column sums {worst:.3f} of allclose(1e-4, 1e-3)')


@pytest.mark.parametrize('prec', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('B,H,W,C', D.L2NORM)
def test_l2norm_bwd(B, H, W, C, prec):
    import numpy as np
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    from aod_meh_hua_amd.functional_ssd import l2norm
    AF.set_precision(prec)
    rnd = rnd_gen(6 + C)
    x3 = prec == 'bf16x3'
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    give = lambda r: ho.x3_split(r) if x3 else r.bfloat16()
    seen = lambda r: (ho.x3_merge(give(r), C) if x3 else give(r)).double()
    x, go = rows(rnd(B, C, H, W) * 3), rows(rnd(B, C, H, W))
    w = torch.rand(C, device='cuda', generator=torch.Generator(device='cuda').manual_seed(C)) * 10 + 15
    xr, wr = seen(x).requires_grad_(), w.double().requires_grad_()
    (wr * xr / (xr.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)).backward(seen(go))

    def fn():
        xd = AF.as_nchw(give(x), B, H, W).requires_grad_(True)
        wd = w.clone().requires_grad_(True)
        l2norm(xd, wd, 1e-10).backward(AF.as_nchw(give(go), B, H, W))
        gx = AF.as_rows(xd.grad)
        return (ho.x3_merge(gx, C) if x3 else gx), wd.grad
    free, (a, b) = default_once(fn), det_twice(fn)
    for tag, (gx, gw) in (('default', free), ('+poison', a), ('-poison', b)):
        if x3:          # tests/test_gpu_x3_kernels.py test_x3_ssd_row_kernels_against_fp32
            ex, ew = relerr(gx, xr.grad), relerr(gw, wr.grad)
            print(f'l2norm_bwd x3 C = {C} {tag}: gx {ex / 5e-5:.3f}, gw {ew / 5e-5:.3f} of the bound')
            assert ex < 5e-5 and ew < 5e-5, (tag, ex, ew)
        else:           # tests/test_gpu_ssd.py test_l2norm_fwd_bwd
            ex, fw = relerr(gx, xr.grad), frac(gw, wr.grad, 2e-3, 2e-3)
            print(f'l2norm_bwd bf16 C = {C} {tag}: gx {ex / 1e-2:.3f}, gw {fw:.3f} of the bound')
            assert ex < 1e-2 and fw < 1, (tag, ex, fw)
            assert np.isfinite(gw.cpu().numpy()).all()
    assert same(a[1], b[1]), 'the scale gradient depends on what the scratch held'
    assert same(a[0], free[0]) and same(b[0], free[0])
