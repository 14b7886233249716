"""The FPN neck (aod_meh_hua_amd/models/necks/fpn.py) on its own against an fp64 restatement of FPN.forward: the cases of
tests/test_fpn_host.py (the restatement against oracle.model.fpn, the nearest-index formula of the row kernels; no device) and
tests/test_gpu_fpn.py (the module, forward and backward, in both precisions).

A case is (B, [(H, W) of the levels the neck reads]): pyramids whose levels are NOT an exact 2x of the next (13 = 2 * 7 - 1), a one-row top,
1x1 onto 1x1, and an exact-2x control.  A run is (case, add_extra_convs, precision).  Operands come from a CPU generator seeded by the case
name: unit-scale inputs, weights randn / sqrt(fan_in), biases 0.1 * randn, one random gradient per output level; they are the values the
module is given -- bf16-representable in the fast mode, x3_merge(x3_split(t)) in the reference-precision mode (x3).

reference() restates FPN.forward with F.conv2d, + and F.interpolate(size=..., mode='nearest') on fp64 CPU tensors; gradients are autograd's.
With `store` it is the EMULATION of the fast mode: the same fp64 chain with a bf16 rounding wherever the module stores a bf16 tensor, in
both directions (RoundBoth).  Forward those are the lateral outputs, the merged laterals and the outputs.  Backward the module stores
more often than it does forward, and the emulation rounds at each of those stores: the gradient an output conv's dgrad writes for its
merged lateral, the gradient the upsample's adjoint writes for the level above, their sum (torch's bf16 add), the input gradients, and --
where C5 feeds two convs -- the first consumer's part of its gradient (the junction's partial sum; without the junction both parts and
their sum).  What the emulation does not have is the fp32 accumulation order of the kernels, which can flip any of these roundings.

Bounds.  err(a, b) = max|a - b| / max|b| per tensor (every output, every input gradient, every weight and bias gradient):
    x3         err(module, fp64) < 1e-4, the figure tests/test_gpu_x3_kernels.py and tests/conv_instances_util.py hold the x3 kernels to;
    fast mode  err(module, fp64) <= 2 * err(emulation, fp64).  Where the emulation makes no rounding at all (the bias gradient of an output conv
               whose output feeds nothing else is the column sum of the given gradient) the module's only error is its fp32 accumulation,
               and the bound is the x3 figure.
The trailing comment of a run is its largest figure over all tensors measured on an MI355X (`python -m tests.fpn_util record`): x3 the error,
fast mode the module's error over the emulation's, with the shared-input junction / without it."""
import sys
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests import synth

B16, X = 'bf16', 'bf16x3'
Case = namedtuple('Case', 'B levels in_channels out_channels start_level')
PROD = ([256, 512, 1024, 2048], 256, 1)          # configs/_base_/Config_RetinaNet.py: reaches the production plans (split-K for P6)
SMALL = ([64, 128, 256], 64, 0)
NUM_OUTS = 5
CASES = {
    'odd': Case(2, [(13, 19), (7, 10), (4, 5)], *PROD),          # 13 = 2*7 - 1, 19 = 2*10 - 1, 7 = 2*4 - 1; P6 2x3, P7 1x2
    'tiny': Case(1, [(3, 5), (2, 3), (1, 2)], *SMALL),           # a one-row top
    'degenerate': Case(1, [(2, 2), (1, 1), (1, 1)], *SMALL),     # 1x1 onto 1x1
    'even': Case(3, [(16, 24), (8, 12), (4, 6)], *SMALL),        # the exact-2x control
}
RUNS = []


def _run(case, extra, prec):
    RUNS.append((case, extra, prec))


_run('odd', 'on_input', X)              # 9.1e-06
_run('odd', 'on_lateral', X)            # 8.0e-06 (5.0e-04 before FPN.forward forked the top lateral three ways)
_run('odd', 'on_output', X)             # 9.0e-06 (2.3e-03 before FPN.forward forked the last backbone level's output)
_run('tiny', 'on_input', X)             # 1.1e-05
_run('tiny', 'on_lateral', X)           # 1.1e-05 (5.8e-04 before)
_run('tiny', 'on_output', X)            # 9.2e-06 (2.5e-03 before)
_run('degenerate', 'on_input', X)       # 1.1e-05
_run('even', 'on_input', X)             # 1.0e-05
_run('odd', 'on_input', B16)            # 1.00 / 1.00
_run('odd', 'on_lateral', B16)          # 1.05 / 1.05
_run('odd', 'on_output', B16)           # 1.00 / 1.00
_run('tiny', 'on_input', B16)           # 1.00 / 1.00
_run('tiny', 'on_lateral', B16)         # 1.00 / 1.00
_run('tiny', 'on_output', B16)          # 1.00 / 1.00
_run('degenerate', 'on_input', B16)     # 1.00 / 1.00
_run('even', 'on_input', B16)           # 1.00 / 1.00
X3_BOUND, FAST_RATIO = 1e-4, 2.0


def run_id(run):
    return '-'.join(run)


# ---------------------------------------------------------------------------------------------------------- the fp64 restatement
class RoundBoth(torch.autograd.Function):
    """a stored bf16 tensor: the value is rounded on the way forward, its gradient on the way back"""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().to(g.dtype)


def reference(feats, sd, start_level=1, extra='on_input', num_outs=NUM_OUTS, store=None, junction=True):
    """FPN.forward (necks/fpn.py:151-202) on the tensors `feats` (one per backbone level; those below start_level are not read) with the
    parameters `sd` ('lateral_convs.{i}.conv.weight', ...).  store: None, or RoundBoth.apply for the fast mode's emulation (module docstring);
    junction: whether the inputs carry the shared-input gradient junction (it decides where C5's two gradient parts are rounded)."""
    st = store if store is not None else (lambda t: t)
    two = store is not None and extra == 'on_input' and num_outs > len(feats) - start_level          # C5 feeds two convs
    w = lambda k: (sd[k + '.conv.weight'], sd[k + '.conv.bias'])
    n = len(feats) - start_level
    xs = [st(feats[i + start_level]) for i in range(n)]
    top_in = st(xs[-1]) if two and not junction else xs[-1]
    lat = [st(F.conv2d(top_in if i == n - 1 else xs[i], *w(f'lateral_convs.{i}'))) for i in range(n)]
    for i in range(n - 1, 0, -1):
        lat[i - 1] = st(lat[i - 1] + F.interpolate(st(lat[i]), size=lat[i - 1].shape[2:], mode='nearest'))
    outs = [st(F.conv2d(st(lat[i]), *w(f'fpn_convs.{i}'), 1, 1)) for i in range(n)]
    if num_outs > n:
        src = {'on_input': st(xs[-1]) if two else xs[-1], 'on_lateral': st(lat[-1]), 'on_output': st(outs[-1])}[extra]
        outs.append(st(F.conv2d(src, *w(f'fpn_convs.{n}'), 2, 1)))
        for i in range(n + 1, num_outs):
            outs.append(st(F.conv2d(st(outs[-1]), *w(f'fpn_convs.{i}'), 2, 1)))
    return outs


def extra_hw(hw, k):
    """sizes of k successive 3x3 / stride-2 / pad-1 levels below (h, w)"""
    out = []
    for _ in range(k):
        hw = ((hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1)
        out.append(hw)
    return out


def out_shapes(c):
    """(H, W) of the NUM_OUTS output levels (the same for the three extra-conv modes: P6 follows C5's size, which is the top lateral's)"""
    return list(c.levels) + extra_hw(c.levels[-1], NUM_OUTS - len(c.levels))


def param_shapes(c, extra):
    """name -> shape of every parameter of FPN(c.in_channels, c.out_channels, NUM_OUTS, c.start_level, add_extra_convs=extra)"""
    O, n, sh = c.out_channels, len(c.in_channels) - c.start_level, {}
    for i in range(n):
        sh[f'lateral_convs.{i}.conv'] = (O, c.in_channels[i + c.start_level], 1, 1)
        sh[f'fpn_convs.{i}.conv'] = (O, O, 3, 3)
    for i in range(n, NUM_OUTS):
        sh[f'fpn_convs.{i}.conv'] = (O, c.in_channels[-1] if (i == n and extra == 'on_input') else O, 3, 3)
    return sh


def raw_operands(case, extra):
    """CPU fp32, before they are made representable: (inputs [B, C, H, W] of the levels read, parameters, output gradients)"""
    c = CASES[case]
    gen = synth.gen(zlib.crc32(case.encode()) % 100000)          # (the same inputs under the three extra-conv modes)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    xs = [rnd(c.B, c.in_channels[i + c.start_level], h, w) for i, (h, w) in enumerate(c.levels)]
    gys = [rnd(c.B, c.out_channels, h, w) for h, w in out_shapes(c)]
    gen = synth.gen(zlib.crc32(f'{case}/{extra}'.encode()) % 100000)
    sd = {}
    for k, s in param_shapes(c, extra).items():
        sd[k + '.weight'] = rnd(*s) / (s[1] * s[2] * s[3]) ** 0.5
        sd[k + '.bias'] = 0.1 * rnd(s[0])
    return xs, sd, gys


def grads_of(xs, sd, outs, gys):
    """-> name -> tensor: the outputs, the input gradients and every parameter gradient of one backward pass driven by `gys`"""
    torch.autograd.backward(outs, gys)
    res = {f'out{i}': o.detach() for i, o in enumerate(outs)}
    res.update({f'dx{i}': x.grad for i, x in enumerate(xs)})
    res.update({'d:' + k: p.grad for k, p in sd.items()})
    return res


def run_reference(c, extra, xs64, sd64, gys64, store=None, junction=True):
    xs = [x.clone().requires_grad_() for x in xs64]
    sd = {k: v.clone().requires_grad_() for k, v in sd64.items()}
    feats = [None] * c.start_level + xs
    return grads_of(xs, sd, reference(feats, sd, c.start_level, extra, store=store, junction=junction), gys64)


def err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    d = (a - b).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    return float(d.max() / b.abs().max())


# ---------------------------------------------------------------------------------------------------------- the module on the device
def _to_device(t, prec):
    """CPU fp32 [B, C, H, W] -> (the tensor the module is given: bf16 NHWC, or X rows, viewed [B, width, H, W]; its values as fp64 on the CPU)"""
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    Bn, C, H, W = t.shape
    rows = t.permute(0, 2, 3, 1).reshape(Bn * H * W, C).contiguous().cuda()
    if prec == X:
        xr = ho.x3_split(rows)
        val = ho.x3_merge(xr, C)
    else:
        xr = rows.bfloat16()
        val = xr.float()
    return AF.as_nchw(xr, Bn, H, W), val.view(Bn, H, W, C).permute(0, 3, 1, 2).double().cpu().contiguous()


def _values(t, C):
    """fp64 CPU [B, C, H, W] values of a tensor the module returned (outputs, input gradients)"""
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd import hipops as ho
    Bn, _, H, W = t.shape
    rows = AF.as_rows(t)
    v = ho.x3_merge(rows, C) if ho.X3 else rows.float()
    return v.view(Bn, H, W, C).permute(0, 3, 1, 2).double().cpu()


def _param_values(sd32, prec):
    """the parameter values the module computes with: weights as its packing keeps them (bf16 / head + tail); biases stay fp32"""
    from aod_meh_hua_amd import hipops as ho
    out = {}
    for k, v in sd32.items():
        if k.endswith('.weight'):
            if prec == X:
                flat = v.reshape(v.shape[0], -1).contiguous().cuda()
                v = ho.x3_merge(ho.x3_split(flat), flat.shape[1]).cpu().view(v.shape)
            else:
                v = v.bfloat16().float()
        out[k] = v
    return out


def build_module(c, extra, sd32):
    from aod_meh_hua_amd.models.necks.fpn import FPN
    m = FPN(list(c.in_channels), c.out_channels, NUM_OUTS, start_level=c.start_level, add_extra_convs=extra)
    missing = m.load_state_dict(sd32, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.cuda().train()


_OPERANDS, _REFS = {}, {}


def operands(run):
    """(device inputs' source tensors, fp64 values of inputs / parameters / output gradients) of a run, built once"""
    if run not in _OPERANDS:
        from aod_meh_hua_amd import functional as AF
        case, extra, prec = run
        assert AF.get_precision() == prec
        xs, sd, gys = raw_operands(case, extra)
        sd = _param_values(sd, prec)
        dx = [_to_device(x, prec) for x in xs]
        dg = [_to_device(g, prec) for g in gys]
        _OPERANDS[run] = dict(x_dev=[d[0] for d in dx], x64=[d[1] for d in dx], g_dev=[d[0] for d in dg], g64=[d[1] for d in dg],
                              sd32=sd, sd64={k: v.double() for k, v in sd.items()})
    return _OPERANDS[run]


def references(run, junction=True):
    """the fp64 tensors of the run under 'ref' (built once, never modified); fast mode: also the emulation's, under 'emu'"""
    c, o = CASES[run[0]], operands(run)
    r = _REFS.setdefault(run, {})
    if 'ref' not in r:
        r['ref'] = run_reference(c, run[1], o['x64'], o['sd64'], o['g64'])
    if run[2] == X:
        return r
    key = 'emu_junction' if junction else 'emu_plain'
    if key not in r:
        r[key] = run_reference(c, run[1], o['x64'], o['sd64'], o['g64'], store=RoundBoth.apply, junction=junction)
    return dict(ref=r['ref'], emu=r[key])


def run_module(run, junction=True):
    """one forward and one backward pass of the module on the run's operands -> (name -> fp64 CPU tensor like grads_of, the output tensors)"""
    from aod_meh_hua_amd import functional as AF
    c, o = CASES[run[0]], operands(run)
    m = build_module(c, run[1], o['sd32'])
    xs = [x.detach().clone(memory_format=torch.preserve_format).requires_grad_() for x in o['x_dev']]
    if junction:
        for x in xs:
            AF.share_input_grad(x)          # as the backbone marks its stage outputs (resnet.py)
    outs = m(tuple([None] * c.start_level + xs))
    torch.autograd.backward(outs, o['g_dev'])
    torch.cuda.synchronize()
    if junction:
        AF.check_junctions()                # every junction delivered its sum
    O = c.out_channels
    res = {f'out{i}': _values(y.detach(), O) for i, y in enumerate(outs)}
    for i, x in enumerate(xs):
        assert x.grad is not None and x.grad.shape == x.shape, f'dx{i}'
        res[f'dx{i}'] = _values(x.grad, c.in_channels[i + c.start_level])
    for k, p in m.state_dict(keep_vars=True).items():
        assert p.grad is not None, k
        res['d:' + k] = p.grad.double().cpu()
    return res, outs


def figures(run, got, junction=True):
    """name -> the figure the bound is on (x3: the error; fast mode: the error over the emulation's) and the two errors"""
    r = references(run, junction)
    out = {}
    for k, ref in r['ref'].items():
        e = err(got[k], ref)
        if run[2] == X:
            out[k] = (e, e, None)
        else:
            ee = err(r['emu'][k], ref)
            out[k] = (e / ee if ee > 0 else FAST_RATIO * e / X3_BOUND, e, ee)          # (no store on its way: FAST_RATIO <=> the x3 figure)
    return out


def record(ids):
    from aod_meh_hua_amd import functional as AF
    for run in RUNS:
        if ids and run_id(run) not in ids:
            continue
        AF.set_precision(run[2])
        figs = []
        for junction in ((True, False) if run[2] == B16 else (True,)):
            f = figures(run, run_module(run, junction)[0], junction)
            worst = max(f, key=lambda k: f[k][0])
            figs.append((f[worst][0], worst))
        print(run_id(run) + ': ' + ' / '.join((f'{v:.1e}' if run[2] == X else f'{v:.2f}') + f' ({k})' for v, k in figs), flush=True)


if __name__ == '__main__':
    if sys.argv[1] == 'record':
        record(sys.argv[2:])
