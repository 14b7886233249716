"""Optimizer plumbing: FusedSGD (torch.optim.SGD semantics on the multi-tensor HIP kernel) and the mmcv-style
`build_optimizer` used by apis/train_Lambda.py:54."""
import ctypes as C

import torch

from ._C import call, stream


class FusedSGD(torch.optim.Optimizer):
    """SGD with momentum / weight decay; one kernel launch per <= 48 tensors instead of ~5 small launches per
    parameter.  The parameter list is re-read from param_groups every step (the reference edits it in place:
    RemoveParamFromOptim, apis/train_Lambda.py:97-109).

    grad_clip=dict(max_norm=M, norm_type=2) (mmcv's optimizer_config.grad_clip) clips by the total gradient norm over ALL groups as
    torch.nn.utils.clip_grad_norm_ does -- coef = min(1, M / (norm + 1e-6)), norm taken of g * grad_scale, i.e. after a data-parallel
    all-reduce -- but entirely on the device: aod_grad_norm_multi leaves the coefficient in device memory and the SGD launches read it
    there, so a step() captured in a HIP graph clips by the norm of the gradients it is replayed on.  Unlike clip_grad_norm_ the `.grad`
    tensors are NOT rewritten (the coefficient is folded into the update; the parameter update is the same).  A non-finite norm makes the
    update non-finite (clip_grad_norm_(error_if_nonfinite=False)); with skip_nonfinite=True such a step leaves parameters and momentum
    buffers untouched and is counted in clip_state()[2].  Without grad_clip, step() launches exactly what it launched before."""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0, weight_decay=0.0, nesterov=False, grad_clip=None, skip_nonfinite=False):
        assert dampening == 0 and not nesterov, 'the AL configs use plain momentum SGD'
        if grad_clip is not None:
            grad_clip = dict(grad_clip)
            if 'max_norm' not in grad_clip:
                raise ValueError(f'grad_clip needs max_norm: {grad_clip}')
            if float(grad_clip.get('norm_type', 2)) != 2.0:
                raise ValueError(f'grad_clip norm_type={grad_clip["norm_type"]!r}: only the 2-norm is implemented')
            if not float(grad_clip['max_norm']) > 0:
                raise ValueError(f'grad_clip max_norm must be positive: {grad_clip["max_norm"]!r}')
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        self.grad_scale = 1.0
        self._lr_dev = {}          # group index -> [device fp32 scalar, value]: used once device_lr() has been called (HIP-graph replay)
        self.grad_clip, self.skip_nonfinite = grad_clip, bool(skip_nonfinite)
        # device state {total_norm, coef, skipped_steps, reserved} and the partial-sum workspace: allocated once and kept for the optimizer's
        # lifetime (a captured graph holds their addresses; a workspace that had to grow keeps its predecessors alive)
        self._clip_state, self._clip_ws, self._clip_keep = None, None, []

    def _clip_buffers(self, ntensors, dev):
        need = 96 * max(int(ntensors), 1)          # aod_grad_norm_multi: at most 96 partials per tensor
        if self._clip_state is None or self._clip_ws.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('FusedSGD(grad_clip=...): call device_lr() (or run one eager step) before capturing step() in a graph')
            if self._clip_state is None:
                self._clip_state = torch.zeros(4, dtype=torch.float32, device=dev)
            if self._clip_ws is not None:
                self._clip_keep.append(self._clip_ws)
            self._clip_ws = torch.empty(need, dtype=torch.float32, device=dev)

    def clip_state(self):
        """Device tensor {total_norm, coef, skipped_steps, reserved} of the last step() (no sync; zeros before the first step), or None
        when clipping is off.  The same tensor every call: clone what must survive the next step."""
        return self._clip_state if self.grad_clip is not None else None

    def device_lr(self):
        """Keep each group's learning rate in device memory and make step() read it from there, so that a step() captured in a HIP
        graph follows the schedule.  Call before every replay (outside capture): uploads only when a value changed."""
        for gi, group in enumerate(self.param_groups):
            ent = self._lr_dev.get(gi)
            if ent is None:
                dev = group['params'][0].device
                self._lr_dev[gi] = [torch.full((1,), float(group['lr']), dtype=torch.float32, device=dev), float(group['lr'])]
            elif ent[1] != float(group['lr']):
                ent[0].fill_(float(group['lr']))
                ent[1] = float(group['lr'])
        if self.grad_clip is not None:
            params = [p for g in self.param_groups for p in g['params']]
            if params:
                self._clip_buffers(len(params), params[0].device)

    @torch.no_grad()
    def step(self, closure=None):
        if self._lr_dev and not torch.cuda.is_current_stream_capturing():
            self.device_lr()          # eager step between graph replays: the schedule may have changed group['lr'] since the last upload
        from . import functional as _AF
        _AF._WgradQueue.flush()       # (weight gradients still queued by a backward pass: launched before anything reads them; normally empty)
        touched, keep = [], []        # keep: contiguous gradient copies must outlive the launch that reads their raw pointers
        batches = []                  # (group index, group, first, ps, gs, ms, ns): the gradient list is complete before anything is launched
        for gi, group in enumerate(self.param_groups):
            ps, gs, ms, ns, first = [], [], [], [], None
            for p in group['params']:
                if p.grad is None:
                    continue
                assert p.dtype == torch.float32 and p.is_contiguous()
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                keep.append(g)
                st = self.state[p]
                is_first = 'momentum_buffer' not in st
                if is_first:
                    st['momentum_buffer'] = torch.empty_like(p)
                if first is None:
                    first = is_first
                if is_first != first:      # mixed fresh/old buffers: flush what we have, start a new batch
                    batches.append((gi, group, first, ps, gs, ms, ns))
                    ps, gs, ms, ns, first = [], [], [], [], is_first
                ps.append(p.data_ptr()), gs.append(g.data_ptr()), ms.append(st['momentum_buffer'].data_ptr()), ns.append(p.numel())
                touched.append(p)
            batches.append((gi, group, first, ps, gs, ms, ns))
        coef = None
        if self.grad_clip is not None and touched:
            coef = self._grad_norm([g for b in batches for g in b[4]], [n for b in batches for n in b[6]], touched[0].device)
        for gi, group, first, ps, gs, ms, ns in batches:
            self._gi = gi
            self._launch(ps, gs, ms, ns, group, first, coef)
        # the kernel writes through raw pointers: tell autograd / the parameter-preparation registry (functional.ParamPrep keys on
        # tensor._version) that these parameters changed, without one no-op kernel per tensor
        if touched:
            torch._C._autograd._unsafe_set_version_counter(touched, [p._version + 1 for p in touched])

    def _grad_norm(self, gs, ns, dev):
        """one aod_grad_norm_multi over the gradients of all groups -> the device address of the clip coefficient"""
        n = len(gs)
        self._clip_buffers(n, dev)
        from .hipops import prof_bytes
        prof_bytes('grad_norm_multi', sum(ns) * 4,          # algorithmic bytes: every gradient read once
                   lambda: call('aod_grad_norm_multi', (C.c_void_p * n)(*gs), (C.c_int64 * n)(*ns), n, float(self.grad_scale),
                                float(self.grad_clip['max_norm']), int(self.skip_nonfinite), C.c_void_p(self._clip_ws.data_ptr()),
                                self._clip_ws.numel(), C.c_void_p(self._clip_state.data_ptr()), stream()))
        return C.c_void_p(self._clip_state.data_ptr() + 4)

    def _launch(self, ps, gs, ms, ns, group, first, coef=None):
        n = len(ps)
        if n == 0:
            return
        arr = C.c_void_p * n
        ent = self._lr_dev.get(self._gi)
        from .hipops import prof_bytes
        args = (arr(*ps), arr(*gs), arr(*ms), (C.c_int64 * n)(*ns), n, float(group['lr']),
                C.c_void_p(ent[0].data_ptr()) if ent is not None else None, float(group['momentum']),
                float(group['weight_decay']), int(bool(first)), float(self.grad_scale))
        # algorithmic bytes: p, g, m read + p, m written = 20 B per parameter (16 on the first step: no momentum read)
        if coef is None:
            prof_bytes('sgd_multi', sum(ns) * (16 if first else 20), lambda: call('aod_sgd_multi', *args, stream()))
        else:
            prof_bytes('sgd_multi', sum(ns) * (16 if first else 20), lambda: call('aod_sgd_multi_clipped', *args, coef, stream()))


def build_optimizer(model, cfg, grad_clip=None, skip_nonfinite=False):
    """mmcv.runner.build_optimizer subset: dict(type='SGD', lr, momentum, weight_decay) over all trainable params.  grad_clip /
    skip_nonfinite: mmcv's optimizer_config.grad_clip, applied inside FusedSGD.step()."""
    cfg = dict(cfg)
    t = cfg.pop('type')
    assert t == 'SGD', 'the AL configs use SGD'
    cfg.pop('paramwise_cfg', None)
    module = model.module if hasattr(model, 'module') else model
    return FusedSGD([p for p in module.parameters() if p.requires_grad], grad_clip=grad_clip, skip_nonfinite=skip_nonfinite, **cfg)
