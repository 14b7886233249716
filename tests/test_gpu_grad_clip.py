"""GPU: gradient-norm clipping inside FusedSGD (optimizer_config.grad_clip; csrc/elementwise.hip grad_sqsum_multi_kernel,
grad_clip_finalize_kernel, sgd_multi_kernel's device-resident coefficient).  Ground truth is torch.nn.utils.clip_grad_norm_ +
torch.optim.SGD in fp64 on the CPU with the fp32 CPU run as the yardstick; the fused path is never its own reference, except where the
statement IS bit-equality of two fused runs (repeatability, the unclipped twin, graph replay against eager)."""
import copy
import os

import pytest
import torch

from tests.test_gpu_parity_geometry_sgd import _param_set

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_NORM = 35.0
KW = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4)
EPS32 = float(torch.finfo(torch.float32).eps)
BIG = 96 * 256 * 16 + 4099            # past one sweep of the 96-block grid (4 x 16 B per thread): the grid-stride loop runs again
MISALIGNED, NO_GRAD = 20, 33          # positions of the two special parameters in the extended set


def _shapes():
    """_param_set() (sizes 1, 35, 180, 1 000 003, ...) extended to 60 tensors = two 48-pointer chunks; odd sizes, sizes below / at / above
    one block's 1024-element vector share, one tensor beyond a whole sweep of the grid.  The added tensors have at least 67 elements: the
    per-tensor bound compares the MAXIMUM rounding error of the fused run with that of torch's fp32 run, and over a handful of elements
    torch's maximum is near zero by chance as often as not (four steps of fp32 torch arithmetic against themselves, re-associated, already
    miss the bound on a 2-element tensor) -- the sizes below 4 and below one vector that matter to the kernels are in the base set."""
    extra = [(BIG,)] + [(n,) for n in (67, 129, 257, 515, 1023, 1024, 1025, 4095, 4096, 4097, 5003)]
    extra += [(8 + 2 * k, 9 + k) for k in range(39)]
    return extra


@pytest.fixture(scope='module')
def p0():
    """the shared initial values (CPU fp32, never modified): index MISALIGNED becomes a view 4 bytes into its storage, NO_GRAD never gets
    a gradient"""
    gen = torch.Generator().manual_seed(7)
    ps = _param_set() + [torch.randn(*s, generator=gen) * 0.05 for s in _shapes()]
    assert len(ps) == 60 and ps[MISALIGNED].numel() == 5003
    return ps


def _grads(p0, seed, scale):
    gen = torch.Generator().manual_seed(seed)
    return [None if i == NO_GRAD else torch.randn(p.shape, generator=gen) * scale for i, p in enumerate(p0)]


def _fused_params(p0):
    out = []
    for i, p in enumerate(p0):
        if i == MISALIGNED:
            base = torch.zeros(p.numel() + 1, device='cuda')
            base[1:].copy_(p.cuda())
            q = torch.nn.Parameter(base[1:])
            assert q.data_ptr() % 16 == 4
        else:
            q = torch.nn.Parameter(p.clone().cuda())
        out.append(q)
    return out


def _set_fused_grads(fused, grads):
    for i, (q, g) in enumerate(zip(fused, grads)):
        if g is None:
            q.grad = None
        elif i == MISALIGNED:                       # the norm kernel's vector test is on the GRADIENT pointer
            base = torch.zeros(g.numel() + 1, device='cuda')
            base[1:].copy_(g.cuda())
            q.grad = base[1:]
            assert q.grad.data_ptr() % 16 == 4
        else:
            q.grad = g.clone().cuda()


def _momenta(opt, params):
    return [opt.state[q]['momentum_buffer'] if 'momentum_buffer' in opt.state.get(q, {}) else None for q in params]


def _bits_equal(a, b):
    return all((x is None and y is None) or torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32)) for x, y in zip(a, b))


def test_four_steps_against_fp64_clip_grad_norm_and_sgd(p0):
    """Steps 0, 1 clip (norm ~1400 and ~700 against max_norm 35; step 1 with grad_scale 0.5, which is inside the norm), step 2 does not
    (norm ~14: coef exactly 1.0 and the step equals an unclipped FusedSGD's bit for bit), step 3 has all-zero gradients (norm 0, coef 1,
    nothing NaN).  LR x0.1 before step 2, device-resident LR from step 1 on."""
    from aod_meh_hua_amd.optim import FusedSGD
    fused = _fused_params(p0)
    ref = [torch.nn.Parameter(p.clone().double()) for p in p0]
    ref32 = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = FusedSGD(fused, grad_clip=dict(max_norm=MAX_NORM, norm_type=2), **KW)
    r64, r32 = torch.optim.SGD(ref, **KW), torch.optim.SGD(ref32, **KW)
    assert float(opt.param_groups[0]['lr']) == 1e-3
    for step, (mag, gscale) in enumerate([(1.0, 1.0), (1.0, 0.5), (0.01, 1.0), (0.0, 1.0)]):
        grads = _grads(p0, 100 + step, mag)
        if step == 1:
            opt.device_lr()
        if step == 2:
            for o in (opt, r64, r32):
                o.param_groups[0]['lr'] = 1e-4
        _set_fused_grads(fused, grads)
        opt.grad_scale = gscale
        for i, g in enumerate(grads):              # the references see the scaled gradient (a power of two: exact)
            ref[i].grad = None if g is None else (g * gscale).double()
            ref32[i].grad = None if g is None else g * gscale
        plain = None
        if step == 2:                               # the unclipped twin: same parameters, momentum, LR, gradients
            twin = [torch.nn.Parameter(q.detach().clone()) for q in fused]
            plain = FusedSGD(twin, **dict(KW, lr=1e-4))
            for q, t in zip(fused, twin):
                t.grad = None if q.grad is None else q.grad.clone()
                if 'momentum_buffer' in opt.state.get(q, {}):
                    plain.state[t]['momentum_buffer'] = opt.state[q]['momentum_buffer'].clone()
            plain.device_lr()
            plain.step()
        kept = [None if q.grad is None else q.grad.clone() for q in fused]
        opt.step()
        n64 = float(torch.nn.utils.clip_grad_norm_(ref, MAX_NORM))
        n32 = float(torch.nn.utils.clip_grad_norm_(ref32, MAX_NORM))
        r64.step(), r32.step()
        torch.cuda.synchronize()
        norm, coef, skipped, _ = opt.clip_state().cpu().tolist()
        print(f'\nstep {step}: total_norm fused {norm!r} fp64 {n64!r} torch-fp32 {n32!r} coef {coef!r}')
        # .grad is left unclipped
        assert _bits_equal([q.grad for q in fused], kept), step
        assert skipped == 0
        if n64 == 0.0:
            assert norm == 0.0 and coef == 1.0
        else:
            e_f, e_t = abs(norm - n64) / n64, abs(n32 - n64) / n64
            print(f'         rel. error of the norm: fused {e_f:.3e} torch-fp32 {e_t:.3e} bound {max(2 * e_t, 16 * EPS32):.3e}')
            assert e_f <= max(2.0 * e_t, 16 * EPS32), (step, e_f, e_t)
        if step < 2:
            assert 0 < coef < 0.1 and abs(coef - MAX_NORM / (n64 + 1e-6)) <= 1e-5 * coef, (step, coef)
        else:
            assert coef == 1.0, (step, coef)
        worst = (0.0, 0.0, -1)
        for i in range(len(p0)):
            got, ideal = fused[i].detach().cpu(), ref[i].detach()
            assert bool(torch.isfinite(got).all()), (step, i)
            e_fused = float((got.double() - ideal).abs().max())
            e_torch = float((ref32[i].detach().double() - ideal).abs().max())
            scale = float(ideal.abs().max())
            worst = max(worst, (e_fused / max(2.0 * e_torch, 1e-7 * scale), e_fused, i))
            assert e_fused <= max(2.0 * e_torch, 1e-7 * scale), (step, i, e_fused, e_torch, scale)
        print(f'         worst parameter error / bound {worst[0]:.3f} (tensor {worst[2]}, error {worst[1]:.3e})')
        assert NO_GRAD is not None and torch.equal(fused[NO_GRAD].detach().cpu(), p0[NO_GRAD])      # no gradient: never touched
        if plain is not None:
            assert _bits_equal(fused, twin) and _bits_equal(_momenta(opt, fused), _momenta(plain, twin))
            assert plain.clip_state() is None


def test_same_step_twice_from_the_same_state_gives_the_same_bits(p0):
    from aod_meh_hua_amd.optim import FusedSGD
    fused = _fused_params(p0)
    opt = FusedSGD(fused, grad_clip=dict(max_norm=MAX_NORM), **KW)
    _set_fused_grads(fused, _grads(p0, 201, 1.0))
    opt.step()                                                          # (momentum buffers exist from here on)
    _set_fused_grads(fused, _grads(p0, 202, 0.7))
    snap_p, snap_m = [q.detach().clone() for q in fused], [None if m is None else m.clone() for m in _momenta(opt, fused)]
    runs = []
    for _ in range(2):
        with torch.no_grad():
            for q, v, m, mv in zip(fused, snap_p, _momenta(opt, fused), snap_m):
                q.copy_(v)
                if m is not None:
                    m.copy_(mv)
        opt.step()
        torch.cuda.synchronize()
        runs.append((opt.clip_state().clone(), [q.detach().clone() for q in fused], [None if m is None else m.clone() for m in _momenta(opt, fused)]))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert float(runs[0][0][0]) > MAX_NORM
    assert _bits_equal(runs[0][1], runs[1][1]) and _bits_equal(runs[0][2], runs[1][2])
    assert not _bits_equal(runs[0][1], snap_p)


def test_non_finite_gradient_default_and_skip(p0):
    """one inf in one gradient: the norm is inf.  Default: the update is non-finite (torch: clip_grad_norm_(error_if_nonfinite=False)
    leaves NaN at that element too).  skip_nonfinite: parameters and momentum untouched, the step counted, the next finite step normal."""
    from aod_meh_hua_amd.optim import FusedSGD
    clip = dict(max_norm=MAX_NORM, norm_type=2)
    good, good2 = _grads(p0, 301, 1.0), _grads(p0, 302, 1.0)
    bad = [None if g is None else g.clone() for g in good]
    bad[5][17] = float('inf')
    # torch, fp32 CPU: the element that held the inf ends up NaN
    tp = [torch.nn.Parameter(p.clone()) for p in p0]
    topt = torch.optim.SGD(tp, **KW)
    for q, g in zip(tp, bad):
        q.grad = None if g is None else g.clone()
    assert not torch.isfinite(torch.nn.utils.clip_grad_norm_(tp, MAX_NORM))
    topt.step()
    assert not bool(torch.isfinite(tp[5]).all())
    # default policy
    fused = _fused_params(p0)
    opt = FusedSGD(fused, grad_clip=clip, **KW)
    _set_fused_grads(fused, bad)
    opt.step()
    torch.cuda.synchronize()
    st = opt.clip_state().cpu()
    assert torch.isinf(st[0]) and torch.isnan(st[1]) and float(st[2]) == 0
    assert not bool(torch.isfinite(fused[5]).all())
    assert torch.equal(fused[NO_GRAD].detach().cpu(), p0[NO_GRAD])
    # skip policy, beside a twin that never sees the bad step
    fa, fb = _fused_params(p0), _fused_params(p0)
    oa, ob = FusedSGD(fa, grad_clip=clip, skip_nonfinite=True, **KW), FusedSGD(fb, grad_clip=clip, skip_nonfinite=True, **KW)
    for f, o in ((fa, oa), (fb, ob)):
        _set_fused_grads(f, good)
        o.step()
    before_p, before_m = [q.detach().clone() for q in fa], [None if m is None else m.clone() for m in _momenta(oa, fa)]
    _set_fused_grads(fa, bad)
    oa.step()
    torch.cuda.synchronize()
    st = oa.clip_state().cpu()
    assert torch.isinf(st[0]) and float(st[1]) == -1.0 and float(st[2]) == 1.0
    assert _bits_equal(fa, before_p) and _bits_equal(_momenta(oa, fa), before_m)
    for f, o in ((fa, oa), (fb, ob)):
        _set_fused_grads(f, good2)
        o.step()
    torch.cuda.synchronize()
    assert _bits_equal(fa, fb) and _bits_equal(_momenta(oa, fa), _momenta(ob, fb))
    assert all(bool(torch.isfinite(q).all()) for q in fa)
    assert float(oa.clip_state()[2]) == 1.0 and float(ob.clip_state()[2]) == 0.0 and 0 < float(oa.clip_state()[1]) < 1


def test_captured_step_reads_the_coefficient_on_the_device(p0):
    """step() captured ONCE; replays on gradients rewritten in place -- a clipping magnitude, then a non-clipping one -- equal the eager
    step on the same inputs bit for bit: the coefficient is produced and consumed on the device, not frozen at capture."""
    from aod_meh_hua_amd.optim import FusedSGD
    clip = dict(max_norm=MAX_NORM, norm_type=2)
    fa, fb = _fused_params(p0), _fused_params(p0)
    oa, ob = FusedSGD(fa, grad_clip=clip, **KW), FusedSGD(fb, grad_clip=clip, **KW)
    first = _grads(p0, 401, 1.0)
    for f, o in ((fa, oa), (fb, ob)):
        _set_fused_grads(f, first)
        o.device_lr()                                # device LR + clip state / workspace: allocated before the capture
        o.step()                                     # momentum buffers exist: the captured launches are the steady-state ones
    torch.cuda.synchronize()
    state_ptr = oa.clip_state().data_ptr()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        oa.step()
    assert oa.clip_state().data_ptr() == state_ptr
    torch.cuda.synchronize()
    assert _bits_equal(fa, fb), 'a capture must not execute the step'
    coefs = []
    for seed, mag in ((402, 0.8), (403, 0.01), (404, 2.0)):
        new = _grads(p0, seed, mag)
        with torch.no_grad():
            for f in (fa, fb):
                for q, v in zip(f, new):
                    if v is not None:
                        q.grad.copy_(v.cuda())           # in place: the graph holds these addresses
        g.replay()
        ob.step()
        torch.cuda.synchronize()
        sa, sb = oa.clip_state().cpu(), ob.clip_state().cpu()
        assert torch.equal(sa.view(torch.int32), sb.view(torch.int32)), (seed, sa, sb)
        assert _bits_equal(fa, fb) and _bits_equal(_momenta(oa, fa), _momenta(ob, fb)), seed
        coefs.append(float(sa[1]))
    assert coefs[0] < 0.1 and coefs[1] == 1.0 and coefs[2] < coefs[0], coefs


# ------------------------------------------------------------------ end to end: the runner, eager and replayed
def _seed_model():
    from oracle import model as omodel
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet.py'))
    cfg.model.backbone.pop('init_cfg')
    model = build_detector(cfg.model)
    model.load_state_dict(omodel.seeded_state_dict(cls_bias=-2.0), strict=True)
    cfg.optimizer.lr = 2e-4
    return cfg, model


def _run(cfg, model0, batches, grad_clip, iters, work_dir):
    from aod_meh_hua_amd.apis.train_Lambda import build_optimizers
    from aod_meh_hua_amd.mmcv_lite import MMDataParallel
    from aod_meh_hua_amd.utils.Epoch_Based_Runner_Lambda import MyEpochBasedRunnerLambda
    cfg = copy.deepcopy(cfg)
    cfg.optimizer_config = dict(grad_clip=grad_clip)
    model = MMDataParallel(copy.deepcopy(model0).cuda().train())
    opt, opt_L = build_optimizers(model, cfg)
    runner = MyEpochBasedRunnerLambda(model, optimizer=opt, work_dir=str(work_dir))
    runner.optimizer_L = opt_L
    losses, logs, after_first = [], [], None
    for it in range(iters):
        runner.run_iter(batches[it], train_mode=True, Labeled=True, Pseudo=False)
        out = runner.outputs
        losses.append((out['loss'].detach().clone(), torch.as_tensor(out['log_vars']['loss_L']).detach().clone()))
        logs.append(dict(out['log_vars']))
        if it == 0:
            after_first = {k: v.detach().clone() for k, v in model.module.state_dict().items()}
    torch.cuda.synchronize()
    return dict(losses=losses, logs=logs, after_first=after_first, runner=runner, opt=opt, opt_L=opt_L,
                sd={k: v.detach().clone() for k, v in model.module.state_dict().items()})


def test_runner_clips_eager_and_replayed_alike(tmp_path, monkeypatch):
    """optimizer_config.grad_clip through build_optimizers + MyEpochBasedRunnerLambda.run_iter on the synthetic dataset (2 x 128^2), in the
    deterministic mode (ordered column sums: eager and replayed iterations are the same bits, tests/test_gpu_graphs.py).  max_norm = half the
    norm a probe iteration measures, so the first iteration certainly clips."""
    from aod_meh_hua_amd import functional as AF
    from aod_meh_hua_amd.datasets import build_dataloader, build_dataset
    ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=6, size=(128, 128)))
    batches = list(build_dataloader(ds, 2, 0, dist=False, shuffle=False))
    assert len(batches) == 3
    cfg, model0 = _seed_model()
    AF.set_deterministic(True)
    try:
        monkeypatch.setenv('AOD_HIP_GRAPH', '0')
        probe = _run(cfg, model0, batches, dict(max_norm=1e30, norm_type=2), 1, tmp_path / 'probe')      # never clips, but measures
        norm0, coef0 = probe['opt'].clip_state()[:2].tolist()
        assert coef0 == 1.0 and norm0 > 0 and norm0 == float(probe['logs'][0]['grad_norm'])
        M = 0.5 * norm0
        clip = dict(max_norm=M, norm_type=2)
        plain = _run(cfg, model0, batches, None, 1, tmp_path / 'plain')
        assert 'grad_norm' not in plain['logs'][0] and 'grad_norm_L' not in plain['logs'][0]
        assert plain['opt'].clip_state() is None and plain['opt_L'].clip_state() is None
        eager = _run(cfg, model0, batches, clip, 3, tmp_path / 'eager')
        monkeypatch.setenv('AOD_HIP_GRAPH', '1')
        graph = _run(cfg, model0, batches, clip, 3, tmp_path / 'graph')
    finally:
        AF.set_deterministic(False)
    assert graph['runner']._graph_step[1].cache, 'the second and third iteration must have been replayed'
    assert getattr(eager['runner'], '_graph_step', None) is None
    for run in (eager, graph):
        for lv in run['logs']:
            for k in ('grad_norm', 'grad_norm_L'):
                assert torch.is_tensor(lv[k]) and lv[k].dim() == 0 and bool(torch.isfinite(lv[k])) and float(lv[k]) > 0, (k, lv[k])
        assert run['opt'].grad_clip == clip and run['opt_L'].grad_clip == clip
    # iteration 1 of the clipped run: the probe's norm, clipped to M -> coef ~0.5, and other parameters than without clipping
    assert float(eager['logs'][0]['grad_norm']) == norm0
    changed = [k for k, v in eager['after_first'].items() if v.is_floating_point() and not torch.equal(v, plain['after_first'][k])]
    assert 'bbox_head.retina_cls.weight' in changed and 'backbone.layer4.2.conv3.weight' in changed, changed[:8]
    # the probe never clipped: it IS the unclipped run, bit for bit
    assert all(torch.equal(v, plain['after_first'][k]) for k, v in probe['after_first'].items())
    # eager == replay: losses, logged norms, parameters, bit for bit
    for it, ((la, lLa), (lb, lLb)) in enumerate(zip(eager['losses'], graph['losses'])):
        assert float(la) == float(lb) and float(lLa) == float(lLb), (it, float(la), float(lb), float(lLa), float(lLb))
    for a, b in zip(eager['logs'], graph['logs']):
        assert float(a['grad_norm']) == float(b['grad_norm']) and float(a['grad_norm_L']) == float(b['grad_norm_L'])
    diff = [k for k, v in eager['sd'].items() if not torch.equal(v, graph['sd'][k])]
    assert not diff, diff[:8]
