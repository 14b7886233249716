"""Autograd wrappers around the HIP kernels (C ABI via hipops).  No torch compute ops on the hot
path: every forward/backward below enqueues hand-written gfx950 kernels; torch supplies device
memory, the autograd tape and streams.

Tensor convention between modules: logical shape [B, C, H, W] (what the reference's host code
indexes), memory = NHWC bf16 (torch.channels_last), i.e. a [B*H*W, C] row tensor for the kernels.
"""
import torch
from torch.autograd import Function

from . import hipops as ho
from .hipops import Seg


# --------------------------------------------------------------------------- layout helpers
def as_rows(x):
    """[B,C,H,W] channels_last -> [B*H*W, C] view (copies only if the caller handed NCHW-contiguous data)."""
    B, C, H, W = x.shape
    xr = x.permute(0, 2, 3, 1)
    if not xr.is_contiguous():
        xr = xr.contiguous()
    return xr.view(B * H * W, C)


def as_nchw(rows, B, H, W):
    return rows.view(B, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def multi_rows(tensors):
    """Several [B,C,H,W] tensors (pyramid levels) -> (base row tensor, segs) without copying when
    every level starts a whole number of rows after the lowest-addressed one; else one torch.cat."""
    rows = [as_rows(t) for t in tensors]
    if len(rows) == 1:
        t = tensors[0]
        return rows[0], [Seg(t.shape[0], t.shape[2], t.shape[3], 0)]
    rb = rows[0].shape[1] * rows[0].element_size()
    base = min(rows, key=lambda r: r.data_ptr())
    offs = [r.data_ptr() - base.data_ptr() for r in rows]
    span = max(o + r.numel() * r.element_size() for o, r in zip(offs, rows))
    if all(o % rb == 0 for o in offs) and span < (1 << 31):       # kernels address operands with 32-bit buffer offsets
        return base, [Seg(t.shape[0], t.shape[2], t.shape[3], o // rb) for t, o in zip(tensors, offs)]
    cat = torch.cat(rows)
    segs, r0 = [], 0
    for t in tensors:
        segs.append(Seg(t.shape[0], t.shape[2], t.shape[3], r0))
        r0 += t.shape[0] * t.shape[2] * t.shape[3]
    return cat, segs


def dense_segs(segs):
    out, r = [], 0
    for s in segs:
        out.append(Seg(s.B, s.H, s.W, r))
        r += s.rows
    return out


# --------------------------------------------------------------------------- batched parameter preparation
import ctypes as _C
import weakref as _weakref


class _PrepRec(_C.Structure):
    _fields_ = [('w', _C.c_void_p), ('gamma', _C.c_void_p), ('beta', _C.c_void_p), ('mean', _C.c_void_p), ('var', _C.c_void_p),
                ('wf', _C.c_void_p), ('wd', _C.c_void_p), ('scale', _C.c_void_p), ('shift', _C.c_void_p), ('invstd', _C.c_void_p),
                ('O', _C.c_int32), ('I', _C.c_int32), ('RS', _C.c_int32), ('Ipad', _C.c_int32), ('Opad', _C.c_int32), ('blk0', _C.c_int32),
                ('eps', _C.c_float), ('pad_', _C.c_int32), ('pad2_', _C.c_int64 * 2)]


class _PrepItem:
    __slots__ = ('srcs', 'ver', 'wf', 'wd', 'scale', 'shift', 'invstd', 'eps', 'dims', 'nblk', 'x3')


class ParamPrep:
    """Everything a conv launch derives from its parameters -- packed bf16 weight images (forward and dgrad) and the folded eval-mode BN
    vectors -- kept in per-layer STATIC buffers and refreshed for ALL registered layers by ONE kernel (aod_param_prep) the first time a
    stale layer is used: after an optimizer step that is one launch per iteration instead of ~270 small ones.  Staleness is detected
    through tensor._version of (weight, gamma, beta, running_mean, running_var)."""

    def __init__(self):
        self.items, self.order, self.table, self.dirty, self.tables = {}, [], None, True, {}
        self.stems = []                   # weak references to stem convs whose derived space-to-depth filter is a registered weight

    def watch_stem(self, conv):
        self.stems = [r for r in self.stems if r() is not None and r() is not conv] + [_weakref.ref(conv)]

    def _versions(self, it):
        return tuple(-1 if t is None else t._version for t in (r() if r is not None else None for r in it.srcs))

    def get(self, w, bn, cin_pad, eps):
        """cin_pad: width of the conv's input rows (bf16 mode: channels padded to 8; reference-precision mode: the X-layout width)"""
        it = self.items.get((id(w), ho.X3))
        if it is not None and it.srcs[0]() is not w:
            it = None
        if it is None:
            it = self._register(w, bn, cin_pad, eps)
        if it.ver != self._versions(it):
            self.refresh()
        return it

    def _register(self, w, bn, cin_pad, eps):
        O, I, R, S = w.shape
        dev = w.device
        it = _PrepItem()
        it.srcs = [_weakref.ref(w)] + [(_weakref.ref(t) if t is not None else None) for t in (bn if bn is not None else (None,) * 4)]
        it.x3 = ho.X3
        if it.x3:
            assert cin_pad == ho.xw(I), f'x3: input rows of {cin_pad} columns for a filter with {I} input channels'
            opad = ho.xw(O)
            it.wf = torch.empty(O, R, S, cin_pad, dtype=torch.bfloat16, device=dev)
            it.wd = torch.empty(I, R, S, opad, dtype=torch.bfloat16, device=dev) if I % 32 == 0 else None    # (dX would need an X-layout width)
        else:
            opad = (O + 7) // 8 * 8
            it.wf = torch.empty(O, R, S, cin_pad, dtype=torch.bfloat16, device=dev)
            it.wd = torch.empty(I, R, S, opad, dtype=torch.bfloat16, device=dev) if cin_pad == I else None      # no dgrad through a padded stem
        if bn is not None:
            it.scale, it.shift, it.invstd = (torch.empty(O, dtype=torch.float32, device=dev) for _ in range(3))
        else:
            it.scale = it.shift = it.invstd = None
        it.eps, it.dims, it.ver = float(eps), (O, I, R * S, cin_pad, opad), None
        if R * S <= 9 and it.x3:
            it.nblk = (opad // 64) * (cin_pad // 64)                         # 32 x 32 LOGICAL channel tiles, each a head and a tail band
        elif R * S <= 9:
            it.nblk = ((opad + 31) // 32) * ((cin_pad + 31) // 32)           # 32 x 32 channel tiles (aod_param_prep)
        else:
            it.nblk = (max(O * R * S * cin_pad, I * R * S * opad if it.wd is not None else 0, O) + 2047) // 2048
        self.items[(id(w), it.x3)] = it
        self.dirty = True
        return it

    def refresh_if_stale(self):
        for r in self.stems:              # derived weights first: an in-place rewrite bumps the version the items below watch
            conv = r()
            if conv is not None and not torch.cuda.is_current_stream_capturing():
                _stem_w4(conv)
        # (only the ACTIVE arithmetic mode's images: after a mode switch in one process the other mode's items stay stale until get() meets
        # them again in their own mode -- ADVICE r4: every optimizer step re-packed both sets)
        if any(it.x3 == ho.X3 and it.ver != self._versions(it) for it in self.items.values()):
            self.refresh()

    def refresh(self):
        assert not torch.cuda.is_current_stream_capturing(), \
            'parameter preparation inside a HIP-graph capture: call PREP.refresh_if_stale() before capturing / replaying'
        # drop layers whose weight died (a model is rebuilt every active-learning cycle)
        dead = [k for k, it in self.items.items() if it.srcs[0]() is None or any(r is not None and r() is None for r in it.srcs[1:])]
        for k in dead:
            del self.items[k]
            self.dirty = True
        if self.dirty:
            self.order = list(self.items.values())
            self.tables = {}
            self.dirty = False
        # only the STALE layers are re-derived.  Which layers are stale together repeats (all trainable layers of one model after its
        # optimizer step; never the frozen stem / layer1; never a second, frozen model): one device table per staleness pattern.
        stale = tuple(i for i, it in enumerate(self.order) if it.x3 == ho.X3 and it.ver != self._versions(it))
        if not stale:
            return
        ent = self.tables.get(stale)
        if ent is None:
            if len(self.tables) > 16:
                self.tables.clear()
            recs = (_PrepRec * len(stale))()
            blk = 0
            for r, i in zip(recs, stale):
                it = self.order[i]
                src = [x() if x is not None else None for x in it.srcs]
                for t in src:
                    assert t is None or (t.dtype == torch.float32 and t.is_contiguous()), 'parameters must be contiguous fp32'
                r.w, r.gamma, r.beta, r.mean, r.var = (None if t is None else t.data_ptr() for t in src)
                r.wf, r.wd = it.wf.data_ptr(), (it.wd.data_ptr() if it.wd is not None else None)
                r.scale, r.shift, r.invstd = ((t.data_ptr() if t is not None else None) for t in (it.scale, it.shift, it.invstd))
                r.O, r.I, r.RS, r.Ipad, r.Opad = it.dims
                r.blk0, r.eps, r.pad_ = blk, it.eps, int(it.x3)          # (pad_ = flags: bit 0 = X3 images)
                blk += it.nblk
            host = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8)
            dev = self.order[stale[0]].wf.device
            ent = self.tables[stale] = (host.to(dev), blk)
        self.table = ent[0]           # (kept alive for captured graphs by graphs._pin_caches)
        ho.call('aod_param_prep', ho.ptr(ent[0]), len(stale), ent[1], ho.stream())
        for i in stale:
            self.order[i].ver = self._versions(self.order[i])


PREP = ParamPrep()


# --------------------------------------------------------------------------- conv (+BN/bias, +res, +ReLU)
import os as _os
_FUSE_ACT = _os.environ.get('AOD_FUSE_ACT', '1') != '0'      # debug switch for A/B timing


# precision of the conv stack: 'bf16' (bf16 operands, fp32 accumulation) or 'bf16x3' -- the REFERENCE-PRECISION mode: every activation,
# gradient and packed filter travels as a bf16 head + tail pair (X-layout rows, hipops.xw) and every product is three MFMAs, in the same
# kernels with the same fused epilogues (csrc/conv.hip "X3", csrc/x3_ops.hip): fp32-grade results at ~3x the matrix work.  In that mode a
# tensor handed between modules has the logical shape [B, xw(C), H, W]; x3_to_f32() gives its fp32 [B, C, H, W] values.
_PREC = _os.environ.get('AOD_CONV_PREC', 'bf16x3')        # default: the reference's precision (the reference computes in fp32)
assert _PREC in ('bf16', 'bf16x3'), f'AOD_CONV_PREC={_PREC!r}: bf16x3 (reference precision) or bf16 (fast mode)'
ho.X3 = _PREC == 'bf16x3'


def set_precision(p):
    global _PREC
    assert p in ('bf16', 'bf16x3')
    _PREC = p
    ho.X3 = p == 'bf16x3'


def x3_to_f32(x, channels=None):
    """fp32 [B, C, H, W] values of an X-layout activation (identity cast in the bf16 mode and for fp32 tensors)"""
    if not ho.X3 or x.dtype != torch.bfloat16:
        return x.float()
    B, Wd, H, W = x.shape
    rows = ho.x3_merge(as_rows(x), channels)
    return as_nchw(rows, B, H, W)


class ForkFn(Function):
    """Reference-precision mode: a tensor that feeds n consumers.  Autograd would add the n gradients with torch's bf16 add, which rounds
    the heads and the tails of an X-layout tensor separately (8 significant bits); here the sum is formed on the values (aod_x3_add)."""

    @staticmethod
    def forward(ctx, x, n):
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        tot = None
        for g in gs:
            if g is None:
                continue
            g = g.contiguous(memory_format=torch.channels_last)
            tot = g if tot is None else as_nchw(ho.x3_add(as_rows(tot), as_rows(g)), g.shape[0], g.shape[2], g.shape[3])
        return tot, None


def fork(x, n):
    """n handles of `x` for n consumers (fpn.py:163-202: a lateral feeds its output conv and the level below; Lambda_L2.py:85-94: a pyramid
    level feeds the cls and the reg tower).  bf16 mode: x itself n times (autograd's own accumulation)."""
    if not ho.X3 or n == 1 or not (torch.is_grad_enabled() and x.requires_grad):
        return [x] * n
    return list(ForkFn.apply(x, n))


def get_precision():
    return _PREC


def mode_key():
    """what a captured HIP graph's kernels depend on besides shapes: the arithmetic mode and the deterministic switch (graphs.py keys its
    caches with it -- a graph captured in one mode must not be replayed for a call made in the other)"""
    return (_PREC, bool(ho.DETERMINISTIC))


class ActSlot:
    """Side channel between a conv and the ONE conv that consumes its ReLU output.  The consumer's dgrad epilogue applies the producer's
    ReLU mask and sums the columns (aod_conv2d res / mask / colsum), so the producer's backward receives the finished masked gradient and
    its bias / BN-shift gradient instead of running an elementwise pass over the activation."""
    __slots__ = ('masked', 's1', 'res_ok', 'res_grad')

    def __init__(self):
        self.masked, self.s1 = False, None
        # residual form (ResNet identity blocks): the activation also feeds the `res` input of a later conv; that conv leaves its
        # residual gradient here instead of returning it, and the consuming conv's dgrad epilogue adds it before masking
        self.res_ok, self.res_grad = False, None


class BwdChain:
    """The three convs of ONE identity bottleneck (128 / 256 planes) whose dgrads run as one launch (aod_bottleneck_bwd).  conv3's backward
    comes first: when every ActSlot hand-over of the block is in place (conv3 -> t2, conv2 -> t1, conv1 -> x with the skip gradient) it
    launches the whole chain, keeps its own result and leaves the other two here; conv2's and conv1's backward pick them up instead of
    launching their dgrads.  Weight gradients stay per conv (they read the same bits)."""
    __slots__ = ('meta', 'x_rows', 'prep', 'out')

    def __init__(self):
        self.meta, self.x_rows, self.prep, self.out = {}, {}, {}, {}


def bwd_chain_for(blk, x):
    """a BwdChain for a block whose training forward qualifies for the fused kernels (same conditions; AOD_FUSE_BOTTLENECK_BWD=0 switches
    the fused backward off), else None"""
    on = _os.environ.get('AOD_FUSE_BOTTLENECK_BWD', '1') != '0' and not ho.DETERMINISTIC     # (the fused chain sums its columns with atomics of its own)
    # (reference-precision mode: aod_bottleneck128x3_bwd, the 128-plane stage only like the forward; AOD_FUSE_BOTTLENECK128_X3_BWD=0 switches it off)
    if ho.X3 and _os.environ.get('AOD_FUSE_BOTTLENECK128_X3_BWD', '1') == '0':
        return None
    return BwdChain() if on and _FUSE_ACT and bottleneck128_train_applies(blk, x) else None


def set_deterministic(on=True):
    """the reference's `--deterministic` (tools/train_RetinaNet.py:56-68 -> cudnn.deterministic): bias / BN-shift column sums as ordered sums
    of per-workgroup partials instead of fp32 atomics (aod_set_deterministic; everything else on the training path is ordered by
    construction).  Call on the training device, outside a graph capture; graphs captured before the switch keep their old kernels."""
    ho.set_deterministic(on)


class GradAcc:
    """Gradient junction of a tensor that feeds SEVERAL convs (a ResNet stage output: the next stage's conv1 and downsample conv, and the
    neck's lateral conv).  Autograd would run the three dgrads into three tensors and add them with two elementwise passes (62 us for C3 at
    16 x 64 x 64 x 512).  Instead every consumer's dgrad takes the running sum as its epilogue's residual operand (dX = conv_T(dZ, W) + partial)
    and hands back None until the last registered consumer has run, which returns the total.  Consumers register in forward
    (conv_bn_act(shared_input=True)), so the count is exactly the convs that were applied to the tensor; `check_junctions()` (called when the
    next iteration starts) fails loudly if a registered consumer never ran its backward and a partial sum was left behind."""
    __slots__ = ('n', 'arrived', 'partial', 'slot', '__weakref__')

    def __init__(self, slot=None):
        self.n, self.arrived, self.partial = 0, 0, None
        # ActSlot of the conv that PRODUCED the tensor (a stage output is the ReLU output of the last block's conv3): the last consumer's
        # dgrad epilogue then also applies that ReLU's mask to the finished sum and column-sums it -- the producer's backward starts from the
        # masked gradient instead of an elementwise pass over the stage output (aod_act_bwd: 54 us for C3)
        self.slot = slot


_JUNCTIONS = []


def share_input_grad(x):
    """mark `x` (a tensor that requires grad, about to feed several convs) as a gradient junction"""
    if torch.is_grad_enabled() and x.requires_grad and _os.environ.get('AOD_GRAD_JUNCTIONS', '1') != '0':
        x._aod_acc = GradAcc(getattr(x, '_aod_slot', None) if _FUSE_ACT and _os.environ.get('AOD_JUNCTION_MASK', '1') != '0' else None)
        _JUNCTIONS.append(_weakref.ref(x._aod_acc))
    return x


def check_junctions():
    """every junction of the previous backward pass delivered its sum (or never started one)"""
    global _JUNCTIONS
    for r in _JUNCTIONS:
        a = r()
        if a is not None and a.partial is not None:
            a.partial = None
            _JUNCTIONS = []
            raise RuntimeError('a shared-input gradient junction was left with a partial sum: one of the convs registered on a tensor never '
                               'ran its backward (its output did not reach the loss); gradients behind that tensor were lost')
    _JUNCTIONS = []


# --------------------------------------------------------------------------- gradient cuts (segmented backward, data parallelism)
_CUTS = None


class grad_cuts:
    """`with grad_cuts() as cuts: out = model.train_step(...)`: the backbone marks its stage outputs with cut() and the autograd graph of the
    iteration falls apart into SEGMENTS that backward_segments() runs one after the other -- head + neck first, then the backbone stages
    from the deepest to the shallowest.  Between two segments the gradients of the finished one are complete, so their bucket all-reduce
    (parallel.GradSync.start(..., segment=k)) is launched while the next segment still computes: SURVEY 8(e) 'all-reduce overlapped with
    the main backward'.  Each segment is one Python call, hence one HIP-graph segment in graphs.GraphedTrainStep."""

    def __enter__(self):
        global _CUTS
        self.prev, _CUTS = _CUTS, []
        return _CUTS

    def __exit__(self, *exc):
        global _CUTS
        _CUTS = self.prev
        return False


def cut(x):
    """inside grad_cuts(): a detached copy of `x` (same memory) that requires grad; (x, copy) is recorded so that backward_segments() can
    resume the backward pass at `x` with the gradient that arrived at the copy.  Outside: x itself."""
    if _CUTS is None or not torch.is_grad_enabled() or not x.requires_grad:
        return x
    xc = x.detach().requires_grad_()
    if getattr(x, '_aod_slot', None) is not None:
        xc._aod_slot = x._aod_slot          # the junction on the copy finishes the producer's activation backward across the cut (GradAcc.slot)
    _CUTS.append((x, xc))
    return xc


def backward_segments(loss, cuts, after=None):
    """loss.backward() in len(cuts) + 1 pieces: segment 0 ends at the cut copies, segment k continues from the k-th deepest cut.  `after(k)`
    is called when segment k's gradients are final (the caller starts their all-reduce there).  Same gradients as one backward() call: a
    cut copy is a leaf whose .grad receives exactly what would have flowed on (the junction protocol, GradAcc, spans the cut)."""
    loss.backward()
    if after is not None:
        after(0)
    for k, (x, xc) in enumerate(reversed(cuts)):
        g, xc.grad = xc.grad, None
        if g is not None:
            x.backward(g)
        if after is not None:
            after(k + 1)


def _grad_rows(gouts, y_segs, O, device):
    """the upstream gradient of a (level-batched) conv as one dense row tensor [M, O] (O = the row width of the conv's output)"""
    if len(gouts) == 1 and gouts[0] is not None:
        return as_rows(gouts[0])
    parts = []
    for g, s in zip(gouts, y_segs):
        parts.append(as_rows(g) if g is not None else torch.zeros(s.rows, O, device=device, dtype=torch.bfloat16))
    dt = torch.float32 if any(p.dtype == torch.float32 for p in parts) else torch.bfloat16
    # the level gradients usually ARE adjacent slices of one buffer (the dX of the next tower conv): view, don't copy
    rb = O * parts[0].element_size()
    adjacent = all(p.dtype == dt and p.is_contiguous() for p in parts) and all(
        parts[i + 1].data_ptr() == parts[i].data_ptr() + parts[i].shape[0] * rb for i in range(len(parts) - 1))
    if adjacent:
        return torch.as_strided(parts[0], (sum(p.shape[0] for p in parts), O), (O, 1))
    return torch.cat([p.to(dt) for p in parts])


def _grad_slice(w, device):
    """data parallelism (parallel.GradSync.attach): the weight gradient is unpacked straight into this parameter's slice of the flat
    all-reduce buffer; autograd installs the returned slice as .grad, so the all-reduce runs in place.  A second use of the same weight
    inside one backward pass gets a fresh tensor (autograd then adds it into the slice)."""
    dst = getattr(w, '_aod_grad_view', None)
    if dst is not None and (w.__dict__.get('_aod_view_busy') or dst.device != device
                            or (w.grad is not None and w.grad.data_ptr() == dst.data_ptr())):
        dst = None          # (.grad already IS the slice and was not reset to None: autograd will add into it)
    if dst is not None:
        w._aod_view_busy = True
        dst = dst.detach()  # a tensor object of its own on the same memory: autograd installs it as .grad without a copy
    return dst


_S1_OF = {}      # data_ptr of a masked gradient handed to a residual branch -> (its column sums, the tensor); emptied after every pass
# Sparse backward (hipops.sparse_bwd): data_ptr of a gradient row tensor -> (its row-activity map, the tensor); emptied after every pass.  The
# box-regression and MEH gradients are zero at every non-positive anchor: retina_reg / retina_L's backward builds the map of its dZ
# (pad_cast_colsum), every tower dgrad hands the map of its dX on to the layer below, whose dgrad skips the tiles that only zero rows reach.
_ROW_MAPS = {}
MAP_LOG = None       # tests: a list that receives every (gradient rows shape, map) pair in the order the backward pass produced them
FWD_MAP_LOG = None   # tests: a list that receives (members, output rows shape, per-member forward maps or None) of every paired tower launch


def _map_of(dz):
    e = _ROW_MAPS.get(dz.data_ptr())
    return e[0] if e is not None and e[1].shape == dz.shape and e[1].dtype == dz.dtype and ho.sparse_bwd() else None


def _keep_map(dx, rmap):
    if rmap is not None:
        if MAP_LOG is not None:
            MAP_LOG.append((tuple(dx.shape), rmap))
        _WgradQueue.begin_pass()        # (registers the callback that empties the table at the end of the pass)
        _ROW_MAPS[dx.data_ptr()] = (rmap, dx)


class _WgradQueue:
    """Weight gradients of consecutive convs are LAUNCHED TOGETHER (hipops.wgrad_unpack_group: one grouped wgrad + one grouped unpack for up
    to four layers).  Alone a backbone layer needs 100+ pixel splits of its few tiles to fill the chip and leaves as many partial slabs (a
    256-KB filter: 30 MB); in a group every member needs a fraction of them.  A conv's backward therefore only QUEUES its weight gradient
    and returns the (not yet written) gradient tensors; the queue is flushed when it holds four jobs, when a job cannot share the grid of
    the waiting ones, and at the end of the backward pass (autograd callback) -- i.e. before anything can read a gradient:
      * autograd installs a returned tensor as .grad without reading it only if .grad is None and nothing else refers to the tensor (the job
        keeps aliases); a parameter whose .grad exists, or that is used twice in one pass (the engine adds the two gradients when the second
        arrives), is not deferred -- and the second use flushes the queue first;
      * segmented backward passes (data parallelism) are separate engine runs: every segment's gradients are complete when its run returns.
    Sparse backward: jobs whose dZ carries a row-activity map (retina_reg / retina_L and the reg / MEH tower convs) wait in a queue of their
    OWN.  A grouped launch is one round of co-resident workgroups and lasts as long as its slowest one, so a mapped member beside a dense one
    would save nothing; mapped members together finish after their share of the few active pixel blocks.  The four cls tower filters left in
    the dense queue are the same four geometries as before (cls, reg, cls, reg), so their group plan -- slab count, summation order -- is
    unchanged; retina_cls loses its launch partner retina_reg and runs on its stand-alone plan (other slab boundaries: another fp32
    summation order of the same products)."""
    jobs, seen, task, deferred = [], set(), -1, []
    sparse_jobs = []
    enabled = _os.environ.get('AOD_WGRAD_GROUP', '1') != '0'

    @classmethod
    def flush(cls):
        for name in ('jobs', 'sparse_jobs'):
            jobs = getattr(cls, name)
            setattr(cls, name, [])
            if jobs:
                ho.wgrad_unpack_group(jobs)

    @classmethod
    def _verify(cls):
        """Every deferred gradient was handed to autograd UNWRITTEN on the assumption that AccumulateGrad installs the very tensor as .grad
        (no read, no copy).  That is an implementation detail of the engine (use count, layout contract, grad mode): check it instead of
        trusting it -- where .grad turned out to be another tensor (a clone taken before the launch filled ours), copy the finished values in."""
        deferred, cls.deferred = cls.deferred, []
        for _, pref, t in deferred:
            p = pref()
            if p is None or p.grad is None:
                continue
            g = p.grad
            if g.data_ptr() != t.data_ptr() and g.shape == t.shape:
                g.copy_(t)

    @classmethod
    def _end_of_pass(cls):
        cls.task = -1
        cls.seen.clear()
        _S1_OF.clear()
        _ROW_MAPS.clear()
        cls.flush()
        cls._verify()

    @classmethod
    def begin_pass(cls):
        """one end-of-pass callback per autograd run, recognised by the engine's graph-task id: a pass that died with an exception never ran
        its callback -- its leftovers must not leak into the next pass (they are launched now: their tensors are still alive and nobody
        reads them), and the next pass must get a callback of its own.  Called by everything that leaves per-pass state behind (queued
        jobs, _S1_OF entries), so that a pass without a trainable conv weight cleans up too."""
        tid = torch._C._current_graph_task_id()
        if tid != cls.task:
            cls.flush()
            cls.deferred = []
            cls.task = tid
            cls.seen.clear()
            _S1_OF.clear()
            _ROW_MAPS.clear()
            if tid >= 0:
                torch.autograd.Variable._execution_engine.queue_callback(cls._end_of_pass)

    @classmethod
    def submit(cls, job, wid, defer):
        cls.begin_pass()
        # deterministic mode: every weight gradient is launched ALONE -- a job's slab count (= its fp32 summation order) must not depend on
        # which neighbours happened to share its grouped launch, and those differ between one backward pass and the same pass cut into
        # segments (data parallelism): the 3-iteration data-parallel run then equals its one-process emulation again
        if wid in cls.seen or not (defer and cls.enabled) or ho.DETERMINISTIC:
            cls.flush()
            job.run_alone()
            # a second use of a weight inside one pass: the engine ADDS the two gradients -- .grad is then no longer "our tensor or a clone
            # of it", so the first use's entry must not be checked against it
            cls.deferred = [e for e in cls.deferred if e[0] != wid]
            cls.seen.add(wid)
            return False
        cls.seen.add(wid)
        name = 'sparse_jobs' if job.zmap is not None else 'jobs'
        q = getattr(cls, name)
        if q and ho.wgrad_group_splits(q + [job]) is None:
            setattr(cls, name, [])
            ho.wgrad_unpack_group(q)
            q = getattr(cls, name)
        q.append(job)
        if len(q) == 4:
            setattr(cls, name, [])
            ho.wgrad_unpack_group(q)
        return True


def _wgrad(x_rows, x_segs, dz, dsegs, R, S, stride, pad, dil, alg, w, O, I, dst, scale=None, bn=None, gamma=None, zmap=None):
    """weight gradient (+ BN weight gradient when bn = (s1, mean, invstd)) of one conv through the queue -> (gw, ggamma)"""
    dev = dz.device
    gw = dst if dst is not None else torch.empty(O, I, R, S, dtype=torch.float32, device=dev)
    wdot = torch.empty(O, dtype=torch.float32, device=dev) if bn is not None else None
    # (aliases, not the tensors themselves: autograd steals a returned gradient -- s1 is also the BN-shift gradient -- only while it holds the
    # one reference to it; otherwise it clones, one tiny copy launch per vector)
    job = ho.WgradJob(x_rows, x_segs, dz, dsegs, R, S, stride, pad, dil, alg, O, I, gw.detach(), scale=scale,
                      w=w.detach() if bn is not None else None, wdot=wdot.detach() if wdot is not None else None,
                      bn=tuple(t.detach() for t in bn) if bn is not None else None, zmap=zmap)
    # deferral hands autograd tensors that are written LATER (see _WgradQueue): only when nothing can read a gradient before the end-of-pass
    # flush -- no hooks on the parameters, no anomaly mode (it checks every returned gradient for NaNs), no graph being built on the backward
    hooked = lambda p: p is not None and bool(p._backward_hooks or getattr(p, '_post_accumulate_grad_hooks', None))
    defer = (R * S <= 9 and w.grad is None and (gamma is None or gamma.grad is None) and not torch.is_grad_enabled()
             and not torch.is_anomaly_enabled() and not hooked(w) and not hooked(gamma))
    if _WgradQueue.submit(job, id(w), defer):
        # (the job's ALIASES: a second reference to the returned tensors themselves would make the engine clone them -- see above)
        _WgradQueue.deferred.append((id(w), _weakref.ref(w), job.gw))
        if job.wdot is not None and gamma is not None:
            _WgradQueue.deferred.append((id(w), _weakref.ref(gamma), job.wdot))
    return gw, wdot


class ConvFn(Function):
    """y = act(conv(x, w) * scale + shift + res) over one or several pyramid levels sharing `w`.

    forward(ctx, meta, w, gamma, beta, mean, var, bias, res, *xs) -> tuple(len(xs)) of [B,N,OH,OW]
    meta: dict(stride, pad, dil, relu, out_f32, eps)."""

    @staticmethod
    def forward(ctx, meta, w, gamma, beta, mean, var, bias, res, *xs):
        O, I, R, S = w.shape
        cin = xs[0].shape[1]
        x_rows, x_segs = multi_rows(xs)
        pi = PREP.get(w, (gamma, beta, mean, var) if gamma is not None else None, cin, meta['eps'])
        wp, scale, shift, invstd = pi.wf, pi.scale, pi.shift, pi.invstd
        if gamma is None and bias is not None:
            shift = bias.detach()
        res_rows = as_rows(res) if res is not None else None
        out_rows = as_rows(meta['out']) if meta.get('out') is not None else None      # caller-provided destination (pyramid slice)
        # the pre-BN activations z are NOT kept: the BN weight gradient comes from <w, dW> (see backward)
        if meta.get('pre') is not None:
            # the output was already computed by a fused multi-conv launch (bottleneck128_train_fwd): this call only records the autograd
            # node -- saved tensors, slots and backward are exactly those of the stand-alone launch
            y_rows, y_segs = meta['pre'], ho.out_segs(x_segs, R, S, meta['stride'], meta['pad'], meta['dil'])
        else:
            r = ho.conv2d_rows(x_rows, x_segs, wp, O, R, S, meta['stride'], meta['pad'], meta['dil'], pre_scale=scale,
                               pre_shift=shift, res=res_rows, relu=meta['relu'], out_f32=meta['out_f32'], out=out_rows, alg=(I, O))
            y_rows, y_segs = r[0], r[1]
        ctx.meta, ctx.x_segs, ctx.y_segs = meta, x_segs, y_segs
        ctx.has_bn, ctx.has_bias, ctx.has_res = gamma is not None, bias is not None, res is not None
        ctx.nx = len(xs)
        ctx.scope = ho.SCOPE
        ctx.save_for_backward(w, gamma, mean, scale, invstd, x_rows, y_rows if meta['relu'] else None)
        if meta.get('chain') is not None:
            ch, role = meta['chain']
            ch.meta[role], ch.x_rows[role], ch.prep[role] = meta, x_rows, (w, gamma, mean, cin, x_segs)
        outs = tuple(as_nchw(y_rows[s.row0:s.row0 + s.rows], s.B, s.H, s.W) for s in y_segs)
        return outs

    @staticmethod
    def backward(ctx, *gouts):
        with ho.scope(ctx.scope):          # (bench.py's per-part listing: the backward launches count for the part their forward ran in)
            return ConvFn._backward(ctx, *gouts)

    @staticmethod
    def _backward(ctx, *gouts):
        w, gamma, mean, scale, invstd, x_rows, a_rows = ctx.saved_tensors
        meta = ctx.meta
        O, I, R, S = w.shape
        cin = x_rows.shape[1]
        y_segs = ctx.y_segs
        X = ho.X3
        Opad = ho.xw(O) if X else (O + 7) // 8 * 8                   # row width of dZ
        g_rows = _grad_rows(gouts, y_segs, O if (meta['out_f32'] or not X) else Opad, w.device)
        dsegs = dense_segs(y_segs)
        need_w = ctx.needs_input_grad[1]
        need_x = any(ctx.needs_input_grad[8:])
        need_res = ctx.has_res and ctx.needs_input_grad[7]
        gw = ggamma = gbeta = gbias = gres = None
        if (meta['out_f32'] and X) or (Opad != O and not X):
            # prediction convs (N = 180 / 36 / 9, fp32 outputs): pad + cast + column sums in one pass
            if meta.get('sparse_grad') and X and ho.sparse_bwd():
                dz, gbias_v, rmap = ho.pad_cast_colsum(g_rows, Opad, a_rows if meta['relu'] else None, want_map=True)
                _keep_map(dz, rmap)
            else:
                dz, gbias_v = ho.pad_cast_colsum(g_rows, Opad, a_rows if meta['relu'] else None)
            gm = None
        else:
            # gm = g * [y > 0] (bf16) and its column sums S1.  With y = z*scale + shift the gradient w.r.t. z is gm*scale[n]; it is never
            # materialised: the scale is folded into the dgrad weights and into the unpack of dW.  BN gradients (eval-mode statistics):
            #   dbeta = S1,   dgamma = invstd * (sum_m gm*z - mean*S1),   sum_m gm[m,n]*z[m,n] = <w[n], dW_gm[n]>   (z = <w[n], patch(m)>)
            relu = meta['relu']
            slot = meta.get('slot')
            if slot is not None and slot.masked and g_rows.dtype == torch.bfloat16:
                dz, s1 = g_rows, slot.s1                      # the consumer's dgrad epilogue already did the activation backward
                slot.masked, slot.s1 = False, None
            else:
                plain = (not relu) and g_rows.dtype == torch.bfloat16
                known = _S1_OF.pop(g_rows.data_ptr(), None) if plain and _os.environ.get('AOD_S1_REUSE', '1') != '0' else None
                if known is not None and known[1].shape == g_rows.shape:
                    dz, s1 = g_rows, known[0]       # the gradient of a residual branch IS the block's masked gradient: its column sums exist
                else:
                    dz, _, s1, _ = ho.act_bwd(g_rows, a_rows, None, None, None, None, relu=relu, want_gm=False, want_dz=not plain)
                    if plain:
                        dz = g_rows
            gbias_v = s1
        need_bn = ctx.has_bn and ctx.needs_input_grad[2]
        if ctx.has_bias and ctx.needs_input_grad[6]:
            gbias = gbias_v[:O]
        if need_res:
            res_slot = meta.get('res_slot')
            if res_slot is not None:
                res_slot.res_grad = dz                  # picked up by the dgrad epilogue of the conv that consumes the same activation
            else:
                s = y_segs[0]
                gres = as_nchw(dz, s.B, s.H, s.W)       # the residual branch sees gm itself
                if (Opad == O or X) and len(y_segs) == 1:
                    # ... so a conv without ReLU at the end of that branch (the downsample conv + BN of a block's first bottleneck) needs no
                    # pass of its own for the column sums; the entry keeps dz alive, so its address cannot be handed out again meanwhile
                    _WgradQueue.begin_pass()        # (registers the callback that empties _S1_OF even if no weight gradient is queued in this pass)
                    _S1_OF[dz.data_ptr()] = (s1, dz)
        x_segs = ctx.x_segs
        if need_w or need_bn:
            dst = _grad_slice(w, dz.device) if need_w else None
            gw, ggamma = _wgrad(x_rows, x_segs, dz, dsegs, R, S, meta['stride'], meta['pad'], meta['dil'], (I, O), w, O, I, dst,
                                scale=scale if ctx.has_bn else None, bn=(s1, mean, invstd) if need_bn else None, gamma=gamma if need_bn else None,
                                zmap=_map_of(dz))
            if need_bn:
                gbeta = s1
            if not need_w:
                gw = None
        gxs = [None] * ctx.nx
        if need_x:
            wd = PREP.get(w, (gamma, None, mean, None) if ctx.has_bn else None, cin, meta['eps']).wd    # registered in forward
            if ho.width(I) != cin or wd is None:   # stem: channel-padded input; dX only for the real channels is never needed (image)
                raise RuntimeError('dgrad through a channel-padded input is not supported')
            xd = dense_segs(x_segs)
            in_slot = meta.get('in_slot')
            fuse = in_slot is not None and all(a.row0 == b.row0 for a, b in zip(x_segs, xd)) and all(ctx.needs_input_grad[8:])
            s1_in = ho.zeros_f32(I, dz.device) if fuse else None
            res_g = in_slot.res_grad if in_slot is not None else None
            if res_g is not None and not fuse:
                raise RuntimeError('a deferred residual gradient was left for a conv that cannot fuse it')
            acc = meta.get('in_acc')
            jslot = None
            if acc is not None:                 # gradient junction: the running sum of the other consumers' dX rides on this dgrad's epilogue
                assert not fuse and len(xd) == 1
                res_g = acc.partial
                if acc.arrived == acc.n - 1 and acc.slot is not None and dz.dtype == torch.bfloat16 and xd[0].row0 == x_segs[0].row0:
                    jslot = acc.slot            # last consumer: its epilogue finishes the producer's activation backward as well
                    s1_in = ho.zeros_f32(I, dz.device)
            ch, role = meta.get('chain') or (None, 0)
            dx = None
            if ch is not None and fuse and acc is None and dz.dtype == torch.bfloat16:
                if role == 3 and res_g is None and _chain_ready(ch, meta):
                    # the whole block's dgrad chain in one launch; G = dz is also the skip gradient conv1's epilogue adds
                    s0 = x_segs[0]
                    pis = {3: PREP.get(w, (gamma, None, mean, None) if ctx.has_bn else None, cin, meta['eps'])}
                    for r in (2, 1):
                        w_, g_, m_, cin_, _ = ch.prep[r]
                        pis[r] = PREP.get(w_, (g_, None, m_, None) if g_ is not None else None, cin_, ch.meta[r]['eps'])
                    gx, dx, gt1, cx, s1_in, c1 = ho.bottleneck_bwd(dz, s0.B, s0.H, s0.W, pis[3].wd, pis[2].wd, pis[1].wd, x_rows, ch.x_rows[2], ch.x_rows[1])
                    ch.out[2], ch.out[1] = (gt1, c1), (gx, cx)
                elif role in ch.out:
                    dx, s1_in = ch.out.pop(role)
                    if role == 1:
                        ch.meta.clear(), ch.x_rows.clear(), ch.prep.clear()
            if dx is None:
                # a 1x1 / stride-2 conv (a stage's downsample conv) that is not the junction's last consumer adds into the running sum IN
                # PLACE: only the (even, even) pixels change, and the library then runs a plain GEMM over the dZ pixels (conv.hip, lattice launch)
                inplace = (acc is not None and res_g is not None and jslot is None and not fuse and R == 1 and S == 1 and meta['stride'] == 2
                           and meta['pad'] == 0 and res_g.dtype == torch.bfloat16 and _os.environ.get('AOD_DGRAD_INPLACE', '1') != '0')
                rmap = _map_of(dz) if (res_g is None and not inplace) else None
                dx = ho.conv2d_dgrad_rows(dz, dsegs, xd, wd, I, R, S, meta['stride'], meta['pad'], meta['dil'],
                                          res=res_g, mask=x_rows if (fuse or jslot is not None) else None, colsum=s1_in, alg=(I, O),
                                          out=res_g if inplace else None, in_map=rmap)
                if rmap is not None:
                    dx, omap = dx
                    _keep_map(dx, omap)
            if fuse:
                in_slot.masked, in_slot.s1, in_slot.res_grad = True, s1_in, None
            if jslot is not None:
                jslot.masked, jslot.s1 = True, s1_in
            gxs = [as_nchw(dx[s.row0:s.row0 + s.rows], s.B, s.H, s.W) if ctx.needs_input_grad[8 + i] else None
                   for i, s in enumerate(xd)]
            if acc is not None:
                acc.arrived += 1
                if acc.arrived < acc.n:
                    acc.partial, gxs = dx, [None]           # not the last consumer: autograd gets nothing yet
                else:
                    acc.partial, acc.arrived = None, 0
        return (None, gw, ggamma, gbeta, None, None, gbias, gres) + tuple(gxs)


def _chain_ready(ch, meta3):
    """every hand-over of the block is in place: conv2 and conv1 fuse their producers' activation backward, the skip gradient of conv3 is
    routed to conv1's epilogue, one dense level each"""
    if set(ch.meta) != {1, 2, 3} or ch.out:
        return False
    m1, m2 = ch.meta[1], ch.meta[2]
    sl1, sl2 = m1.get('in_slot'), m2.get('in_slot')
    if sl1 is None or sl2 is None or meta3.get('res_slot') is not sl1 or sl1.res_grad is None:
        return False
    if m1.get('in_acc') is not None or m2.get('in_acc') is not None:
        return False
    for r in (1, 2, 3):
        segs = ch.prep[r][4]
        if len(segs) != 1 or segs[0].row0 != 0:
            return False
    return True


def conv_bn_act(xs, w, bn=None, bias=None, res=None, stride=1, pad=0, dil=1, relu=False, out_f32=False, out=None, sole_consumer=False,
                shared_input=False, pre=None, chain=None, sparse_grad=False):
    """xs: tensor or list of tensors (levels).  bn: object with weight/bias/running_mean/running_var/eps.
    sole_consumer: the caller guarantees that every x is the ReLU output of a conv_bn_act call and feeds NOTHING but this conv, which
    lets this conv's dgrad epilogue perform that producer's activation backward (ActSlot).  sole_consumer='res': x additionally feeds
    the `res` input of ONE later conv_bn_act call (ResNet identity block), whose residual gradient is then routed through this conv.
    sparse_grad (fp32 prediction convs): the caller knows the output's gradient to be zero in most rows (box regression, MEH: zero at every
    anchor that is not positive) -- the backward then carries a row-activity map down the tower (hipops.sparse_bwd)."""
    single = torch.is_tensor(xs)
    xl = [xs] if single else list(xs)
    meta = dict(stride=stride, pad=pad, dil=dil, relu=relu, out_f32=out_f32, eps=bn.eps if bn is not None else 0.0, out=out, pre=pre,
                sparse_grad=bool(sparse_grad and out_f32))
    if chain is not None and torch.is_grad_enabled():
        meta['chain'] = chain
    if torch.is_grad_enabled():
        if relu and not out_f32:
            meta['slot'] = ActSlot()
        if sole_consumer and _FUSE_ACT:
            slots = [getattr(x, '_aod_slot', None) for x in xl]
            if slots[0] is not None and all(sl is slots[0] for sl in slots) and all(x.requires_grad for x in xl):
                if sole_consumer != 'res' or len(xl) == 1:
                    meta['in_slot'] = slots[0]
                    slots[0].res_ok = sole_consumer == 'res'
        if shared_input and len(xl) == 1:
            acc = getattr(xl[0], '_aod_acc', None)
            if acc is not None and 'in_slot' not in meta:
                meta['in_acc'] = acc
                acc.n += 1
        rs = getattr(res, '_aod_slot', None) if res is not None else None
        if rs is not None and rs.res_ok:
            meta['res_slot'] = rs
            rs.res_ok = False                      # exactly one residual consumer
    if bn is not None:
        outs = ConvFn.apply(meta, w, bn.weight, bn.bias, bn.running_mean, bn.running_var, None, res, *xl)
    else:
        outs = ConvFn.apply(meta, w, None, None, None, None, bias, res, *xl)
    if meta.get('slot') is not None:
        for o in outs:
            o._aod_slot = meta['slot']
    return outs[0] if single else list(outs)


class ConvPairFn(Function):
    """Two same-shape tower convs (conv + bias + ReLU, bf16, stride 1; Lambda_L2.py:85-94: cls_convs[i] and reg_convs[i]) as ONE grouped
    launch forward and ONE grouped dgrad launch backward (aod_conv2d_grouped): alone each leaves a third of its last round of workgroups
    idle, together their 2 x 341 tiles of 256 x 256 run at the big tile's rate.  Same results as two ConvFn calls, same ActSlot protocol
    (the consumer's dgrad epilogue performs the producer's ReLU backward + bias column sums).

    forward(ctx, meta, wA, bA, wB, bB, *xsA, *xsB) -> (*ysA, *ysB)"""

    @staticmethod
    def forward(ctx, meta, wA, bA, wB, bB, *xs):
        nl = len(xs) // 2
        O, I, R, S = wA.shape
        rows, segs = zip(multi_rows(xs[:nl]), multi_rows(xs[nl:]))
        assert segs[0] == segs[1] and wB.shape == wA.shape, 'paired tower convs need identical geometry'
        cin = rows[0].shape[1]
        pis = [PREP.get(w, None, cin, 0.0) for w in (wA, wB)]
        rows, wfs, shifts = list(rows), [pi.wf for pi in pis], [bA.detach(), bB.detach()]
        rider = meta.get('rider')
        if rider is not None:
            # a third conv of the same geometry that belongs to ANOTHER autograd pass (the MEH tower on the detached pyramid, trained by its
            # own loss and optimizer right after this pass): its forward rides in this grid -- 3 x 341 tiles = 3.996 rounds of the CUs instead
            # of 2.66 + 1.33 -- and its output waits in meta['rider_out'] for the conv_bn_act(pre=...) call that records its autograd node
            convL, xL = rider
            rows.append(xL)
            wfs.append(PREP.get(convL.weight, None, cin, 0.0).wf)
            shifts.append(convL.bias.detach())
        # sparse forward (hipops.sparse_fwd): fwd_map = where the outputs of the reg member and of the rider are needed; the cls member is dense
        fmap = meta.get('fwd_map')
        omaps = [None, fmap] + ([fmap] if rider is not None else []) if fmap is not None else None
        if FWD_MAP_LOG is not None:
            FWD_MAP_LOG.append((len(rows), (sum(s.rows for s in segs[0]), ho.width(O)), omaps))
        outs, y_segs = ho.conv2d_rows_grouped(rows, list(segs[0]), wfs, O, R, S, 1, meta['pad'], meta['dil'], pre_shifts=shifts, relu=True,
                                              alg=(I, O), omaps=omaps)
        if rider is not None:
            meta['rider_out'] = outs[2]
        ctx.meta, ctx.x_segs, ctx.y_segs, ctx.nl = meta, list(segs[0]), y_segs, nl
        ctx.save_for_backward(wA, wB, rows[0], rows[1], outs[0], outs[1])
        return tuple(as_nchw(o[s.row0:s.row0 + s.rows], s.B, s.H, s.W) for o in outs[:2] for s in y_segs)

    @staticmethod
    def backward(ctx, *gouts):
        wA, wB, xA, xB, yA, yB = ctx.saved_tensors
        meta, nl, y_segs, x_segs = ctx.meta, ctx.nl, ctx.y_segs, ctx.x_segs
        O, I, R, S = wA.shape
        dsegs, xd = dense_segs(y_segs), dense_segs(x_segs)
        dzs, gws, gbs = [], [], []
        for gi, (w, x_rows, a_rows) in enumerate(((wA, xA, yA), (wB, xB, yB))):
            g_rows = _grad_rows(gouts[gi * nl:(gi + 1) * nl], y_segs, ho.width(O), w.device)
            slot = meta['slot'][gi]
            if slot is not None and slot.masked and g_rows.dtype == torch.bfloat16:
                dz, s1 = g_rows, slot.s1                      # the consumer's dgrad epilogue already did the activation backward
                slot.masked, slot.s1 = False, None
            else:
                dz, _, s1, _ = ho.act_bwd(g_rows, a_rows, None, None, None, None, relu=True, want_gm=False, want_dz=True)
            dzs.append(dz)
            gbs.append(s1[:O] if ctx.needs_input_grad[2 + 2 * gi] else None)
            gw = None
            if ctx.needs_input_grad[1 + 2 * gi]:
                gw, _ = _wgrad(x_rows, x_segs, dz, dsegs, R, S, 1, meta['pad'], meta['dil'], (I, O), w, O, I, _grad_slice(w, dz.device),
                               zmap=_map_of(dz))
            gws.append(gw)
        gxs = [None] * (2 * nl)
        need = [any(ctx.needs_input_grad[5 + gi * nl:5 + (gi + 1) * nl]) for gi in range(2)]
        if any(need):
            assert all(need), 'paired tower convs: both inputs need gradients or neither'
            wds = [PREP.get(w, None, xA.shape[1], 0.0).wd for w in (wA, wB)]
            dense = all(a.row0 == b.row0 for a, b in zip(x_segs, xd))
            in_slots = meta['in_slot']
            fuse = [sl is not None and dense for sl in in_slots]
            assert all(sl is None or sl.res_grad is None for sl in in_slots)
            s1_in = [ho.zeros_f32(I, dzs[0].device) if f else None for f in fuse]
            rmaps = [_map_of(dz) for dz in dzs]
            dxs = ho.conv2d_dgrad_rows_grouped(dzs, dsegs, xd, wds, I, R, S, 1, meta['pad'], meta['dil'],
                                               masks=[xA if fuse[0] else None, xB if fuse[1] else None], colsums=s1_in, alg=(I, O),
                                               in_maps=rmaps if any(m is not None for m in rmaps) else None)
            if any(m is not None for m in rmaps):
                dxs, omaps = dxs
                for dx, om in zip(dxs, omaps):
                    _keep_map(dx, om)
            for gi in range(2):
                if fuse[gi]:
                    in_slots[gi].masked, in_slots[gi].s1 = True, s1_in[gi]
                for i, s in enumerate(xd):
                    gxs[gi * nl + i] = as_nchw(dxs[gi][s.row0:s.row0 + s.rows], s.B, s.H, s.W)
        return (None, gws[0], gbs[0], gws[1], gbs[1]) + tuple(gxs)


def conv_pair_act(xsA, xsB, convA, convB, sole_consumer=False, rider=None, fwd_map=None):
    """cls / reg tower convs of one depth (ConvModule.conv holders: weight, bias, padding, dilation) on their own level lists; falls back to
    two conv_bn_act calls whenever the grouped form does not apply.  rider = (conv holder, input rows [M, C]): a third conv of the same shape
    whose forward (no autograd) is computed in the same launch; then returns (ya, yb, rider output rows or None).
    fwd_map (sparse forward, hipops.fwd_row_maps): row-activity map of where the outputs of convB and of the rider are NEEDED -- their other
    256-row tiles come back as zero rows; convA stays dense.  Ignored (dense) where the grouped form or the rider does not apply."""
    import os
    wA, wB = convA.weight, convB.weight
    # (reference-precision mode: the grouped launch exists for the 256 x 256 tile only -- N % 256 == 0 and a deep filter)
    x3_ok = not ho.X3 or (wA.shape[0] % 256 == 0 and wA.shape[1] % 32 == 0 and wA.shape[1] * wA.shape[2] * wA.shape[3] >= 1024)
    ok = (x3_ok and os.environ.get('AOD_GROUP_TOWERS', '1') != '0' and wA.shape == wB.shape and wA.shape[0] % 8 == 0
          and wA.shape[0] >= 128 and convA.bias is not None and convB.bias is not None and convA.stride[0] == convB.stride[0] == 1
          and convA.padding == convB.padding and convA.dilation == convB.dilation and len(xsA) == len(xsB)
          and all(a.shape == b.shape and a.dtype == torch.bfloat16 for a, b in zip(xsA, xsB)))
    if not ok:
        r = (conv_bn_act(list(xsA), wA, bias=convA.bias, pad=convA.padding[0], dil=convA.dilation[0], relu=True, sole_consumer=sole_consumer),
             conv_bn_act(list(xsB), wB, bias=convB.bias, pad=convB.padding[0], dil=convB.dilation[0], relu=True, sole_consumer=sole_consumer))
        return r if rider is None else r + (None,)
    meta = dict(pad=convA.padding[0], dil=convA.dilation[0], slot=[None, None], in_slot=[None, None])
    if rider is not None:
        cl = rider[0]
        if (cl.weight.shape == wA.shape and cl.bias is not None and cl.padding == convA.padding and cl.dilation == convA.dilation
                and cl.stride[0] == 1 and rider[1].dtype == torch.bfloat16):
            meta['rider'] = rider
    if fwd_map is not None and ho.sparse_fwd() and 'rider' in meta and convA.stride[0] == 1 and torch.is_grad_enabled():
        meta['fwd_map'] = fwd_map
    grad = torch.is_grad_enabled()
    if grad:
        meta['slot'] = [ActSlot(), ActSlot()]
        if sole_consumer and _FUSE_ACT:
            for gi, xl in enumerate((xsA, xsB)):
                slots = [getattr(x, '_aod_slot', None) for x in xl]
                if slots[0] is not None and all(sl is slots[0] for sl in slots) and all(x.requires_grad for x in xl):
                    meta['in_slot'][gi] = slots[0]
                    slots[0].res_ok = False
    outs = ConvPairFn.apply(meta, wA, convA.bias, wB, convB.bias, *xsA, *xsB)
    nl = len(xsA)
    ya, yb = list(outs[:nl]), list(outs[nl:])
    if grad:
        for gi, ys in enumerate((ya, yb)):
            for o in ys:
                o._aod_slot = meta['slot'][gi]
    return (ya, yb) if rider is None else (ya, yb, meta.get('rider_out'))


def conv_towers_nograd(xss, convs, relu=True):
    """Inference-only: the same-depth convs of several head towers (list of parameter holders with .weight / .bias, identical shape)
    applied to their own level lists `xss[g]` in ONE grouped launch (hipops.conv2d_rows_grouped): cls / reg / evidence towers of the
    scoring pass.  Returns one level list per tower."""
    assert not torch.is_grad_enabled()
    G = len(convs)
    rows, segs = zip(*[multi_rows(list(xs)) for xs in xss])
    assert all(sg == segs[0] for sg in segs), 'towers must see the same pyramid geometry'
    w0 = convs[0].weight
    O, I, R, S = w0.shape
    pis = [PREP.get(c.weight, None, rows[0].shape[1], 0.0) for c in convs]
    outs, dsegs = ho.conv2d_rows_grouped(list(rows), list(segs[0]), [pi.wf for pi in pis], O, R, S, convs[0].stride[0], convs[0].padding[0],
                                         convs[0].dilation[0], pre_shifts=[c.bias.detach() if c.bias is not None else None for c in convs], relu=relu,
                                         alg=(I, O))
    return [[as_nchw(o[s.row0:s.row0 + s.rows], s.B, s.H, s.W) for s in dsegs] for o in outs]


# --------------------------------------------------------------------------- MC-dropout forwards (csrc/dropout.hip)
class DropoutSites(dict):
    """site name -> (site index, table offset, channels), in the order of the oracle's keyed ReLU sites (oracle/model.py `_relu`):
    'backbone.bn1'; '<block>.bn1' / '.bn2' / '.out'; 'bbox_head.cls_convs.<i>@<level>' (level-major).  T = table width (sum of the channel
    counts); prefix[id(module)] = the name a Bottleneck / the backbone / the head builds its site names from."""
    T = 0
    prefix = None

    def offsets(self, device):
        """the sites' first table columns as the device int32 array aod_dropout2d_masks reads (one per device, cached)"""
        cache = self.__dict__.setdefault('_dev', {})
        t = cache.get(device)
        if t is None:
            t = cache[device] = torch.tensor([v[1] for v in self.values()], dtype=torch.int32).to(device)
        return t


def dropout_sites(model):
    """The Dropout2d sites of an MC-dropout forward of a ResNet + FPN + Lambda_L2Net detector: one per ReLU application that feeds the
    classification maps -- the backbone's and the cls tower's (a tower conv is applied once per pyramid level: one site per (conv, level));
    FPN has no ReLU, and the reg / MEH towers are not run by that forward."""
    m = getattr(model, 'module', model)
    bb, head = m.backbone, m.bbox_head
    if not (hasattr(bb, 'res_layers') and hasattr(head, 'cls_convs')):
        raise NotImplementedError(f'dropout_sites: MC-dropout sites are defined for the ResNet + Lambda_L2Net detectors, not for '
                                  f'{type(bb).__name__} / {type(head).__name__} (SSD / VGG sites are not built)')
    sites = DropoutSites()
    sites.prefix = {id(bb): 'backbone', id(head): 'bbox_head'}

    def add(name, ch):
        sites[name] = (len(sites), sites.T, int(ch))
        sites.T += int(ch)
    add('backbone.bn1', bb.conv1.out_channels)
    for li, lname in enumerate(bb.res_layers):
        for bi, blk in enumerate(getattr(bb, lname)):
            p = f'backbone.layer{li + 1}.{bi}'
            sites.prefix[id(blk)] = p
            add(p + '.bn1', blk.conv1.out_channels)
            add(p + '.bn2', blk.conv2.out_channels)
            add(p + '.out', blk.conv3.out_channels)
    levels = int(m.neck.num_outs) if getattr(m, 'with_neck', False) else len(bb.out_indices)
    for l in range(levels):
        for i, cm in enumerate(head.cls_convs):
            add(f'bbox_head.cls_convs.{i}@{l}', cm.conv.out_channels)
    return sites


_MCD = None        # (table [Bmax, T] fp32, DropoutSites) while a dropout forward runs; None: nothing below launches or branches


class mc_dropout:
    """Context of ONE stochastic forward (isEval=True, justOut=True, no autograd): the whole-block inference fusions stand down
    (bottleneck64_applies / bottleneck128_applies), so every ReLU output on the path exists in memory, and each is multiplied in place by its
    site's slice of `table` (dropout_apply).  The table is read at run time: a captured forward replays with whatever it holds then."""

    def __init__(self, table, sites):
        self.state = (table, sites)

    def __enter__(self):
        global _MCD
        assert not torch.is_grad_enabled(), 'MC-dropout forwards run under torch.no_grad() (dropout in training is not built)'
        self.prev, _MCD = _MCD, self.state
        return self

    def __exit__(self, *exc):
        global _MCD
        _MCD = self.prev


class MCDropoutState:
    """(factor table, DropoutSites) as ONE opaque object: what travels to simple_test as the `mc_dropout` keyword.  MMDataParallel's scatter
    rebuilds tuples and dicts on the way (a DropoutSites would arrive as a plain dict); an object of another type passes as it is."""
    __slots__ = ('table', 'sites')

    def __init__(self, table, sites):
        self.table, self.sites = table, sites


def mc_dropout_active():
    return _MCD is not None


def dropout_apply(ys, names, owner=None):
    """Dropout2d behind a ReLU: y *= factors of site `name`, in place, for a tensor or a level list `ys` ([B, width(C), H, W] conv
    outputs) and their site names (`owner`: the module whose DropoutSites.prefix the names are relative to).  A level list whose members
    are row ranges of one buffer (a level-batched conv's outputs) takes ONE launch (aod_dropout2d_apply_multi), else one per level."""
    table, sites = _MCD
    single = torch.is_tensor(ys)
    yl, nl = ([ys], [names]) if single else (list(ys), list(names))
    if owner is not None:
        nl = [sites.prefix[id(owner)] + n for n in nl]
    ents = [sites[n] for n in nl]
    rows = []
    for y, (_, off, ch) in zip(yl, ents):
        r = as_rows(y)
        assert r.data_ptr() == y.data_ptr() and r.shape[1] == ho.width(ch), (tuple(y.shape), ch)      # a view of y: the product is y's
        rows.append(r)
    B = yl[0].shape[0]
    ch = ents[0][2]
    rb = rows[0].shape[1] * rows[0].element_size()
    base = min(rows, key=lambda r: r.data_ptr())
    offs = [r.data_ptr() - base.data_ptr() for r in rows]
    if 1 < len(rows) <= 8 and all(o % rb == 0 for o in offs) and all(e[2] == ch for e in ents) and all(y.shape[0] == B for y in yl):
        ho.dropout2d_apply_multi(base, table, B, [(o // rb, y.shape[2] * y.shape[3], e[1]) for o, y, e in zip(offs, yl, ents)], ch)
    else:
        for y, r, e in zip(yl, rows, ents):
            ho.dropout2d_apply(r, table, e[1], y.shape[0], y.shape[2] * y.shape[3], e[2])
    return ys


# --------------------------------------------------------------------------- stem helpers
def image_to_nhwc(img, cpad=8):
    """fp32 NCHW image batch -> bf16 NHWC rows viewed as [B, cpad, H, W] (no grad: images are leaves)."""
    B, C, H, W = img.shape
    if ho.X3:          # one 32-channel band of X rows (SSD's VGG reads the image with a 3x3 conv; the ResNet stem takes the space-to-depth form)
        rows = torch.empty(B * H * W, 64, dtype=torch.bfloat16, device=img.device)
        ho.call('aod_x3_nchw_f32_to_nhwc', ho.ptr(img.detach().float().contiguous()), ho.ptr(rows), B, C, H, W, ho.stream())
        return as_nchw(rows, B, H, W)
    rows, _ = ho.nchw_to_rows(img.detach().float(), cpad)
    return as_nchw(rows, B, H, W)


def bottleneck64_applies(blk, x):
    """a 64-channel, stride-1 bottleneck (resnet.py:262-301) whose forward keeps nothing for a backward pass: inference, or a frozen
    block (layer1 under frozen_stages = 1) on an input that needs no gradient"""
    if _MCD is not None:          # MC-dropout forward: the three-launch form, a Dropout2d behind each ReLU
        return False
    if _os.environ.get('AOD_FUSE_BOTTLENECK', '1') == '0' or blk.planes != 64 or x.dtype != torch.bfloat16:
        return False
    if ho.X3 and _os.environ.get('AOD_FUSE_BOTTLENECK_X3', '1') == '0':
        return False
    c1, c2, c3 = blk.conv1, blk.conv2, blk.conv3
    if (tuple(c2.stride) != (1, 1) or tuple(c2.dilation) != (1, 1) or tuple(c1.stride) != (1, 1) or c1.in_channels % 64 != 0
            or c3.out_channels != 256 or blk.norm1.training or blk.norm2.training or blk.norm3.training):
        return False
    if not torch.is_grad_enabled():
        return True
    return not x.requires_grad and not any(q.requires_grad for q in blk.parameters())


def bottleneck64_ds_fused(blk, x):
    """the downsample branch of the stage's first 64-plane block (1x1, stride 1, 64 -> 256 channels + eval BN) rides in the block's launch
    (aod_bottleneck64x3_ds_fwd / aod_bottleneck64_ds_fwd; AOD_FUSE_BOTTLENECK_DS=0: a launch of its own)"""
    ds = blk.downsample
    if ds is None or _os.environ.get('AOD_FUSE_BOTTLENECK_DS', '1') == '0' or x.shape[1] != ho.width(64):
        return False
    c, n = ds[0], ds[1]
    return (tuple(c.weight.shape) == (256, 64, 1, 1) and tuple(c.stride) == (1, 1) and tuple(c.padding) == (0, 0) and c.bias is None
            and not n.training and (not torch.is_grad_enabled() or not any(q.requires_grad for q in list(c.parameters()) + list(n.parameters()))))


def bottleneck64_fwd(x, blk, identity):
    """the whole block in one launch (aod_bottleneck64_fwd); `identity` = x or the downsample branch's output (None: bottleneck64_ds_fused)"""
    B, Cin, H, W = x.shape
    bn = lambda n: (n.weight, n.bias, n.running_mean, n.running_var)
    p1 = PREP.get(blk.conv1.weight, bn(blk.norm1), Cin, blk.norm1.eps)                 # (Cin = the row width of x: the X-layout width in the x3 mode)
    p2 = PREP.get(blk.conv2.weight, bn(blk.norm2), ho.width(64), blk.norm2.eps)
    p3 = PREP.get(blk.conv3.weight, bn(blk.norm3), ho.width(64), blk.norm3.eps)
    ds = None
    if identity is None:
        pd = PREP.get(blk.downsample[0].weight, bn(blk.downsample[1]), Cin, blk.downsample[1].eps)
        ds = (pd.wf, pd.scale, pd.shift)
    out = ho.bottleneck64_fwd(as_rows(x.detach()), B, H, W, p1.wf, p1.scale, p1.shift, p2.wf, p2.scale, p2.shift, p3.wf, p3.scale, p3.shift,
                              as_rows(identity.detach()) if identity is not None else None, ds=ds)
    return as_nchw(out, B, H, W)


def _wide_stage(blk):
    """128 planes (layer2, aod_bottleneck128_fwd) or 256 planes (layer3, aod_bottleneck256_fwd; AOD_FUSE_BOTTLENECK256=0 switches it off).
    Reference-precision mode: the 128-plane stage only (aod_bottleneck128x3_fwd, csrc/bottleneck128_x3.hip; AOD_FUSE_BOTTLENECK128_X3=0 switches it
    off) -- on X rows a 256-plane tile's intermediates and filter stream do not fit the CU's LDS / L2 path."""
    if ho.X3:
        return blk.planes == 128 and _os.environ.get('AOD_FUSE_BOTTLENECK128_X3', '1') != '0'
    return blk.planes == 128 or (blk.planes == 256 and _os.environ.get('AOD_FUSE_BOTTLENECK256', '1') != '0')


def bottleneck128_applies(blk, x):
    """an identity bottleneck of the 128-plane stage (resnet.py:262-301: 512 -> 128 -> 128 -> 512, stride 1, no downsample branch) whose
    forward keeps nothing for a backward pass (inference / frozen): one launch (aod_bottleneck128_fwd)"""
    if _MCD is not None:
        return False
    if _os.environ.get('AOD_FUSE_BOTTLENECK128', '1') == '0' or not _wide_stage(blk) or blk.downsample is not None:
        return False
    c1, c2, c3 = blk.conv1, blk.conv2, blk.conv3
    if (x.dtype != torch.bfloat16 or c1.in_channels != 4 * blk.planes or c3.out_channels != 4 * blk.planes or tuple(c1.stride) != (1, 1) or tuple(c2.stride) != (1, 1)
            or tuple(c2.dilation) != (1, 1) or tuple(c2.padding) != (1, 1) or blk.norm1.training or blk.norm2.training or blk.norm3.training):
        return False
    if not torch.is_grad_enabled():
        return True
    return not x.requires_grad and not any(q.requires_grad for q in blk.parameters())


def bottleneck128_train_applies(blk, x):
    """the same block under autograd (trainable layer2 in the training step): the fused launch also writes the two intermediates, and the
    three convs are recorded as autograd nodes around its outputs (conv_bn_act(pre=...)): forward = one launch, backward unchanged"""
    if not torch.is_grad_enabled() or _os.environ.get('AOD_FUSE_BOTTLENECK128_TRAIN', '1') == '0':
        return False
    if (_os.environ.get('AOD_FUSE_BOTTLENECK128', '1') == '0' or not _wide_stage(blk) or blk.downsample is not None
            or x.dtype != torch.bfloat16):
        return False
    c1, c2, c3 = blk.conv1, blk.conv2, blk.conv3
    return (c1.in_channels == 4 * blk.planes and c3.out_channels == 4 * blk.planes and tuple(c1.stride) == (1, 1) and tuple(c2.stride) == (1, 1)
            and tuple(c2.dilation) == (1, 1) and tuple(c2.padding) == (1, 1) and not (blk.norm1.training or blk.norm2.training or blk.norm3.training))


def bottleneck128_train_fwd(x, blk):
    """(t1, t2, y) row tensors of the fused launch for a block under autograd"""
    B, Cin, H, W = x.shape
    bn = lambda n: (n.weight, n.bias, n.running_mean, n.running_var)
    p1 = PREP.get(blk.conv1.weight, bn(blk.norm1), Cin, blk.norm1.eps)                  # (Cin = the row width of x: the X-layout width in the x3 mode)
    p2 = PREP.get(blk.conv2.weight, bn(blk.norm2), ho.width(blk.planes), blk.norm2.eps)
    p3 = PREP.get(blk.conv3.weight, bn(blk.norm3), ho.width(blk.planes), blk.norm3.eps)
    with torch.no_grad():
        y, t1, t2 = ho.bottleneck128_fwd(as_rows(x.detach()), B, H, W, p1.wf, p1.scale, p1.shift, p2.wf, p2.scale, p2.shift, p3.wf, p3.scale,
                                         p3.shift, keep=True)
    return t1, t2, y


def bottleneck128_fwd(x, blk):
    B, Cin, H, W = x.shape
    bn = lambda n: (n.weight, n.bias, n.running_mean, n.running_var)
    p1 = PREP.get(blk.conv1.weight, bn(blk.norm1), Cin, blk.norm1.eps)
    p2 = PREP.get(blk.conv2.weight, bn(blk.norm2), ho.width(blk.planes), blk.norm2.eps)
    p3 = PREP.get(blk.conv3.weight, bn(blk.norm3), ho.width(blk.planes), blk.norm3.eps)
    out = ho.bottleneck128_fwd(as_rows(x.detach()), B, H, W, p1.wf, p1.scale, p1.shift, p2.wf, p2.scale, p2.shift, p3.wf, p3.scale, p3.shift)
    return as_nchw(out, B, H, W)


def _stem_w4(conv):
    """[O, C, 7, 7] stem filter regrouped for the space-to-depth input: [O, 4C, 4, 4] with w4[o, (dy*2+dx)*C + c, R, S] =
    w7[o, c, 2R + dy - 1, 2S + dx - 1] (zero where that tap index is -1).  ONE persistent tensor per conv module, rewritten IN PLACE when
    the 7x7 weight's version changes: captured HIP graphs and the parameter-preparation table keep pointing at valid memory, and
    PREP.refresh_if_stale() (which runs before every graph replay) re-checks the watched convs, so a load_state_dict / resume / broadcast
    into the frozen stem after a capture reaches the replays."""
    w7 = conv.weight
    ent = conv.__dict__.get('_aod_w4')
    if ent is None or ent[1].device != w7.device or ent[2]() is not conv:        # (a deep-copied module carries its source's entry)
        O, Cc = w7.shape[:2]
        ent = conv.__dict__['_aod_w4'] = [None, torch.empty(O, 4 * Cc, 4, 4, dtype=torch.float32, device=w7.device), _weakref.ref(conv)]
        PREP.watch_stem(conv)
    if ent[0] != w7._version:
        O, Cc = w7.shape[:2]
        wp = torch.zeros(O, Cc, 8, 8, dtype=torch.float32, device=w7.device)
        wp[:, :, 1:, 1:] = w7.detach().float()                                   # index r + 1 = 2R + dy
        ent[1].copy_(wp.view(O, Cc, 4, 2, 4, 2).permute(0, 3, 5, 1, 2, 4).reshape(O, 4 * Cc, 4, 4))     # [o, dy, dx, c, R, S]
        ent[0] = w7._version
    return ent[1]


def stem_s2d_applies(img, conv, bn):
    """the frozen 7x7 / stride-2 / pad-3 stem on an fp32 image with even sides (resnet.py:575-600 with frozen_stages >= 0)"""
    return ((ho.X3 or _os.environ.get('AOD_STEM_S2D', '1') != '0') and img.dtype == torch.float32 and img.dim() == 4
            and img.shape[1] <= 4 and img.shape[2] % 2 == 0 and img.shape[3] % 2 == 0 and tuple(conv.weight.shape[2:]) == (7, 7)
            and tuple(conv.stride) == (2, 2) and tuple(conv.padding) == (3, 3) and tuple(conv.dilation) == (1, 1) and conv.bias is None
            and not conv.weight.requires_grad and not any(p.requires_grad for p in bn.parameters()) and not bn.training)


def stem_conv_s2d(img, conv, bn):
    """relu(bn(conv7x7_s2(img))) of the frozen stem as a 4x4 / stride-1 conv over the space-to-depth image (aod_nchw_f32_to_s2d_bf16):
    contiguous 128-B filter rows instead of 49 scattered 16-B taps, K = 256 instead of 392.  No autograd graph (nothing here trains)."""
    B, Cc, H, W = img.shape
    O = conv.weight.shape[0]
    rows, segs = ho.nchw_to_s2d_rows(img.detach())
    w4 = _stem_w4(conv)
    pi = PREP.get(w4, (bn.weight, bn.bias, bn.running_mean, bn.running_var), rows.shape[1], bn.eps)
    dst = [Seg(B, H // 2, W // 2, 0)]                 # (the natural output of a 4x4 / pad-2 filter has one more row and column)
    y, _ = ho.conv2d_rows(rows, segs, pi.wf, O, 4, 4, 1, 2, 1, pre_scale=pi.scale, pre_shift=pi.shift, relu=True, dst_segs=dst,
                          alg=(49.0 * Cc / 16.0, O))      # algorithmic FLOPs: the 7 x 7 x C filter
    return as_nchw(y, B, H // 2, W // 2)


def stem_pool_s2d(img, conv, bn):
    """max_pool_3x3_s2(relu(bn(conv7x7_s2(img)))) of the frozen stem in one launch after the layout kernel (aod_stem_pool_fwd): the
    64-channel conv output stays in LDS.  AOD_STEM_POOL_FUSE=0: conv and pool as separate launches."""
    B, Cc, H, W = img.shape
    O = conv.weight.shape[0]
    if _os.environ.get('AOD_STEM_POOL_FUSE', '1') == '0' or (ho.X3 and (Cc != 3 or O != 64)):
        return max_pool_3x3_s2(stem_conv_s2d(img, conv, bn))
    if ho.X3:
        # reference-precision mode: image -> pooled X rows in one launch (csrc/stem_x3.hip); the X filter image is the one the s2d conv uses
        pi = PREP.get(_stem_w4(conv), (bn.weight, bn.bias, bn.running_mean, bn.running_var), ho.xw(16), bn.eps)
        H2, W2 = H // 2, W // 2
        H4, W4 = (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1
        out = torch.empty(B * H4 * W4, ho.xw(O), dtype=torch.bfloat16, device=img.device)
        src = img.detach().contiguous()
        ho.prof_flops('fwd', (B * H2 * W2, O, 2 * 49 * Cc, 49, 2), 2.0 * B * H2 * W2 * O * 49 * Cc,
                      lambda: ho.call('aod_stem_pool_x3_fwd', ho.ptr(src), ho.ptr(pi.wf), ho.ptr(pi.scale), ho.ptr(pi.shift), ho.ptr(out), B, Cc, H, W,
                                      ho.stream()))
        return as_nchw(out, B, H4, W4)
    assert O == 64 and Cc <= 4
    rows, segs = ho.nchw_to_s2d_rows(img.detach())
    pi = PREP.get(_stem_w4(conv), (bn.weight, bn.bias, bn.running_mean, bn.running_var), 16, bn.eps)
    H2, W2 = H // 2, W // 2
    H4, W4 = (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1
    out = torch.empty(B * H4 * W4, O, dtype=torch.bfloat16, device=img.device)
    flops = 2.0 * B * H2 * W2 * O * 49 * Cc                   # algorithmic: the 7 x 7 x C filter on every conv output
    ho.prof_flops('fwd', (B * H2 * W2, O, 49 * Cc, 49, 2), flops,
                  lambda: ho.call('aod_stem_pool_fwd', ho.ptr(rows), ho.ptr(pi.wf), ho.ptr(pi.scale), ho.ptr(pi.shift), ho.ptr(out), B, H2, W2, ho.stream()))
    return as_nchw(out, B, H4, W4)


def max_pool_3x3_s2(x):
    """resnet.py:610 -- only used inside the frozen stem (no backward needed)."""
    assert not x.requires_grad, 'maxpool backward is not implemented (stem is frozen, resnet.py:612-628)'
    B, C, H, W = x.shape
    rows, s = ho.maxpool3x3s2(as_rows(x), Seg(B, H, W))
    return as_nchw(rows, s.B, s.H, s.W)


class UpsampleAddFn(Function):
    """FPN top-down step: out = lateral + nearest_upsample(top)  (fpn.py:163-172)."""

    @staticmethod
    def forward(ctx, lateral, top):
        B, C, H, W = lateral.shape
        h, w = top.shape[2:]
        out = ho.upsample_add(as_rows(lateral), Seg(B, H, W), as_rows(top), Seg(B, h, w))
        ctx.dims = (B, C, H, W, h, w)
        return as_nchw(out, B, H, W)

    @staticmethod
    def backward(ctx, g):
        B, C, H, W, h, w = ctx.dims
        g_rows = as_rows(g)
        gt = None
        if ctx.needs_input_grad[1]:
            gt = as_nchw(ho.upsample_add_bwd(g_rows, Seg(B, H, W), Seg(B, h, w)), B, h, w)
        return (g if ctx.needs_input_grad[0] else None), gt


def pyramid_buffer(shapes, channels, device, dtype=torch.bfloat16):
    """One flat [sum(B*H*W), C] allocation + per-level [B,C,H,W] channels_last views (adjacent levels: a
    level-batched conv reads them as segments of ONE buffer, no copy, 32-bit offsets)."""
    rows = sum(b * h * w for b, h, w in shapes)
    flat = torch.empty(rows, ho.width(channels) if dtype == torch.bfloat16 else channels, device=device, dtype=dtype)
    views, r = [], 0
    for b, h, w in shapes:
        views.append(as_nchw(flat[r:r + b * h * w], b, h, w))
        r += b * h * w
    return flat, views


def upsample_add(lateral, top):
    return UpsampleAddFn.apply(lateral, top)


# --------------------------------------------------------------------------- losses
class PackedLosses(list):
    """The per-level loss terms of one name (loss_cls / loss_bbox / loss_noR / loss_L) as the reference hands them to `_parse_losses`
    (SSL_Lambda.py:126-154) -- a list -- plus `.packed`: ONE device vector whose sum is the sum of the per-level means the reference
    forms with a `.mean()` and an add per level.  `_parse_losses` sums the vector (one launch, and one in backward) instead."""

    def __init__(self, items, packed, group=None):
        super().__init__(items)
        self.packed = packed
        # (matrix, row): `packed` is row `row` of a matrix whose rows are the packed vectors of several loss names (the level-fused loss launch
        # returns loss_cls / loss_bbox / loss_noR as one [3, L] tensor): `_parse_losses` then sums the matrix once instead of row by row
        self.group = group


class GradArena:
    """The per-level gradients of one prediction conv's output (retina_cls / retina_reg / retina_L: one loss launch per level,
    Lambda_L2.py:112-121,235-241) land in adjacent row ranges of ONE buffer per conv: the conv's level-batched backward then reads them in
    place (`_grad_rows` sees adjacent slices) instead of concatenating five tensors first (63 MB of fp32 class-logit gradients per step)."""

    def __init__(self, rows_per_level):
        self.row0, r = [], 0
        for n in rows_per_level:
            self.row0.append(r)
            r += int(n)
        self.rows, self.bufs = r, {}

    def slice(self, name, level, rows, width, device):
        buf = self.bufs.get(name)
        if buf is None:
            buf = self.bufs[name] = torch.empty(self.rows, width, dtype=torch.float32, device=device)
        assert buf.shape[1] == width and rows == (self.row0[level + 1] if level + 1 < len(self.row0) else self.rows) - self.row0[level]
        return buf[self.row0[level]:self.row0[level] + rows]


class RetinaLossFn(Function):
    """Per level: (loss_cls_sum, loss_bbox_sum, loss_noR[N]) = fused EDL softmax-focal + L1
    (Lambda_L2.py:112-121).  Sums are NOT yet divided by avg_factor (done by the caller with a
    device scalar so that no host sync is needed)."""

    @staticmethod
    def forward(ctx, cls_score, bbox_pred, labels, label_w, bbox_t, bbox_w, gamma, alpha, num_classes, arena=None, level=0, form='edl', box=None):
        """form: 'edl' (softmax -> logit -> focal) or 'sigmoid' (the focal term on the raw logits, MyRetinaHead.py:91-109), hipops.FOCAL_FORMS
        box: None (L1 on the deltas) or box_kwargs(...) -- the IoU / GIoU term on the decoded boxes, hipops.BOX_FORMS"""
        B, AC, H, W = cls_score.shape
        ctx.arena, ctx.level, ctx.form = arena, level, form
        ctx.box = box = dict(box or {})
        # (an output nobody differentiates -- the loss_noR rows, which train_step detaches -- arrives as None in backward instead of a
        # zero-filled tensor of its size that backward would then add the row-sum gradient to: two launches per level)
        ctx.set_materialize_grads(False)
        A = AC // num_classes
        cls_rows = as_rows(cls_score).view(-1, num_classes)
        box_rows = as_rows(bbox_pred).view(-1, 4)
        labels = labels.reshape(-1).contiguous()
        label_w = label_w.reshape(-1).contiguous()
        bbox_t = bbox_t.reshape(-1, 4).contiguous()
        bbox_w = bbox_w.reshape(-1, 4).contiguous()
        noR, sums = ho.edl_focal_l1_fwd(cls_rows, labels, label_w, box_rows, bbox_t, bbox_w, gamma, alpha, form=form, **box)
        ctx.save_for_backward(cls_rows, box_rows, labels, label_w, bbox_t, bbox_w)
        ctx.cfg = (gamma, alpha, cls_score.shape, bbox_pred.shape)
        return sums[0], sums[1], noR, sums[2]      # sums[2] = sum(noR): lets the caller form mean(loss_noR) without a pass over the rows

    @staticmethod
    def backward(ctx, g_cls, g_box, g_noR, g_sum):
        cls_rows, box_rows, labels, label_w, bbox_t, bbox_w = ctx.saved_tensors
        gamma, alpha, cshape, bshape = ctx.cfg
        dev = cls_rows.device
        g_cls = torch.zeros(1, device=dev) if g_cls is None else g_cls.reshape(1).float().contiguous()
        g_box = torch.zeros(1, device=dev) if g_box is None else g_box.reshape(1).float().contiguous()
        g_noR_t = None if g_noR is None else g_noR.float().contiguous()
        scalar = False
        if g_sum is not None:          # gradient of the row SUM: one device scalar for every row
            if g_noR_t is None:
                g_noR_t, scalar = g_sum.reshape(1).float().contiguous(), True
            else:
                g_noR_t = g_noR_t + g_sum.float()
        B, AC, H, W = cshape
        dst_c = dst_b = None
        if ctx.arena is not None:              # this level's rows of the level-batched gradient buffers
            dst_c = ctx.arena.slice('cls', ctx.level, B * H * W, AC, dev).view(-1, cls_rows.shape[1])
            dst_b = ctx.arena.slice('box', ctx.level, B * H * W, bshape[1], dev).view(-1, 4)
        gc, gb = ho.edl_focal_l1_bwd(cls_rows, labels, label_w, box_rows, bbox_t, bbox_w, g_cls, g_box, g_noR_t, 0.0, gamma, alpha,
                                     g_noR_is_scalar=scalar, grad_cls=dst_c, grad_bbox=dst_b, form=ctx.form, **ctx.box)
        return (as_nchw(gc.view(B * H * W, AC), B, H, W), as_nchw(gb.view(B * H * W, bshape[1]), B, H, W),
                None, None, None, None, None, None, None, None, None, None, None)


def box_kwargs(box_form='l1', eps=1e-6, linear=False, coder=None):
    """The box-form arguments of the fused loss launches (hipops.edl_focal_l1_*) as RetinaLossFn / RetinaLossLevelsFn carry them: None for
    the L1 term (the launches then run exactly what they ran before the box forms existed), a dict otherwise."""
    if box_form == 'l1':
        return None
    return dict(box_form=box_form, box_eps=float(eps), box_linear=bool(linear), coder=coder)


def dense_concat(tensors):
    """The tensors as ONE contiguous view when each is contiguous and starts where the previous one ends (pyramid levels of a level-batched
    conv's output, level-major target arrays): tensors[0]'s storage seen as [sum(rows), *shape[1:]].  None otherwise."""
    t0 = tensors[0]
    tail = tuple(t0.shape[1:])
    end = t0.data_ptr()
    rows = 0
    for t in tensors:
        if t.dtype != t0.dtype or tuple(t.shape[1:]) != tail:
            return None
        if t.numel() == 0:               # (an empty level occupies no rows wherever it points)
            continue
        if not t.is_contiguous() or t.data_ptr() != end:
            return None
        end += t.numel() * t.element_size()
        rows += t.shape[0]
    if t0.untyped_storage().data_ptr() + t0.untyped_storage().nbytes() < end:
        return None
    shape = (rows,) + tail
    stride, acc = [], 1
    for d in reversed(shape):
        stride.append(acc)
        acc *= d
    return t0.as_strided(shape, tuple(reversed(stride)))


LOSS_LEVELS = __import__('os').environ.get('AOD_LOSS_LEVELS', '1') != '0'      # 0: one loss launch per pyramid level (the earlier form)


class RetinaLossLevelsFn(Function):
    """RetinaLossFn for ALL pyramid levels in one launch per pass (the reference: loss_single once per level through multi_apply,
    L_anchor_head.py:306-314 -> Lambda_L2.py:105-121).  Inputs are the dense all-level views (dense_concat); returns (sums [3, L], loss_noR
    [all rows]).  Same blocks, same summation orders as the per-level launches: identical bits (tests/test_gpu_kernels.py)."""

    @staticmethod
    def forward(ctx, cls_rows, box_rows, labels, label_w, bbox_t, bbox_w, gamma, alpha, level_rows, shapes, num_pos=None, form='edl', box=None):
        """num_pos (int32 [B], the assigner's per-image positive counts): the sums come back divided -- rows 0, 1 by num_total_samples =
        sum_b max(num_pos[b], 1), row 2 by the level's row count (L_anchor_head.py:266-288,300-303; SSL_Lambda.py:136-141) -- and
        num_total_samples as a third output; the clamp / sum / cast / cat / divide launches of the tensor form are inside the reduction."""
        ctx.set_materialize_grads(False)
        ctx.form = form
        ctx.box = box = dict(box or {})      # (None: the L1 term; functional.box_kwargs)
        div = nt = None
        if num_pos is None:
            noR, sums = ho.edl_focal_l1_levels_fwd(cls_rows, labels, label_w, box_rows, bbox_t, bbox_w, level_rows, gamma, alpha, form=form, **box)
        else:
            noR, sums, div, nt = ho.edl_focal_l1_levels_fwd(cls_rows, labels, label_w, box_rows, bbox_t, bbox_w, level_rows, gamma, alpha, num_pos,
                                                            form=form, **box)
        ctx.save_for_backward(cls_rows, box_rows, labels, label_w, bbox_t, bbox_w, div)
        ctx.cfg = (gamma, alpha, tuple(level_rows), shapes)
        if nt is None:
            return sums, noR
        nt = nt.view(())
        ctx.mark_non_differentiable(nt)
        return sums, noR, nt

    @staticmethod
    def backward(ctx, g_sums, g_noR, g_nt=None):
        cls_rows, box_rows, labels, label_w, bbox_t, bbox_w, div = ctx.saved_tensors
        gamma, alpha, level_rows, (A, AC, A4) = ctx.cfg
        dev = cls_rows.device
        L = len(level_rows)
        g_sums = torch.zeros(3, L, device=dev) if g_sums is None else g_sums.float().contiguous()
        g_rows = None
        if g_noR is not None:              # (nobody on the training path differentiates the rows: train_step detaches them)
            g2 = g_sums[2] if div is None else g_sums[2] / div[2]
            # (the per-level row counts as a cached DEVICE tensor and an explicit output size: no host-to-device copy, no host sync --
            # the expression stays capturable in a HIP graph)
            g_rows = (g_noR.float() + torch.repeat_interleave(g2, _level_rows_dev(level_rows, dev), output_size=sum(level_rows))).contiguous()
        gc = torch.empty(cls_rows.shape[0] // A, AC, dtype=torch.float32, device=dev)
        gb = torch.empty(cls_rows.shape[0] // A, A4, dtype=torch.float32, device=dev)
        ho.edl_focal_l1_levels_bwd(cls_rows, labels, label_w, box_rows, bbox_t, bbox_w, level_rows, g_sums, g_rows, gc, gb, A, gamma, alpha, divisors=div,
                                   form=ctx.form, **ctx.box)
        return gc.view(cls_rows.shape), gb.view(box_rows.shape), None, None, None, None, None, None, None, None, None, None, None


_LEVEL_ROWS_DEV = {}


def _level_rows_dev(level_rows, dev):
    key = (tuple(level_rows), dev)
    t = _LEVEL_ROWS_DEV.get(key)
    if t is None:
        if len(_LEVEL_ROWS_DEV) > 64:
            _LEVEL_ROWS_DEV.clear()
        t = _LEVEL_ROWS_DEV[key] = torch.tensor(list(level_rows), device=dev)
    return t


class MEHLossLevelsFn(Function):
    """MEHLossFn for all pyramid levels in one launch per pass (Lambda_L2.py:235-241 once per level): lam / loss_noR / bbox_w are the dense
    all-level views; returns the per-level sums [L]."""

    @staticmethod
    def forward(ctx, lam, loss_noR, bbox_w, level_rows, A, form='l2'):
        out = ho.meh_loss_levels_fwd(lam, loss_noR, bbox_w, level_rows, form=form)
        ctx.save_for_backward(lam, loss_noR, bbox_w)
        ctx.cfg = (tuple(level_rows), A, form)
        return out

    @staticmethod
    def backward(ctx, g):
        lam, loss_noR, bw = ctx.saved_tensors
        level_rows, A, form = ctx.cfg
        gl = torch.empty(lam.numel() // A, A, dtype=torch.float32, device=lam.device)
        ho.meh_loss_levels_bwd(lam, loss_noR, bw, level_rows, g.float().contiguous(), gl, A, form=form)
        return gl.view(lam.shape), None, None, None, None, None


class _LevelViewsFn(Function):
    """[B, C, H, W] pyramid-level tensors (adjacent row ranges of one buffer) -> their dense [all rows, C] view, for the level-fused loss
    launches; backward hands every level its row range of the ONE gradient buffer as a view -- what GradArena does for the per-level launches:
    the prediction conv's level-batched backward reads the ranges in place (`_grad_rows`), nothing is concatenated or copied."""

    @staticmethod
    def forward(ctx, dense, *levels):
        ctx.shapes = [tuple(t.shape) for t in levels]
        return dense.view_as(dense)

    @staticmethod
    def backward(ctx, g):
        outs, r = [], 0
        for B, C, H, W in ctx.shapes:
            outs.append(as_nchw(g[r:r + B * H * W].view(B * H * W, C), B, H, W))
            r += B * H * W
        return (None,) + tuple(outs)


def dense_levels(levels):
    """Dense [sum(B*H*W), C] fp32 view of adjacent pyramid-level tensors that carries their autograd history (None when not adjacent)."""
    rows = [as_rows(t) for t in levels]
    with torch.no_grad():
        dense = dense_concat([r.detach() for r in rows])
    if dense is None:
        return None
    return _LevelViewsFn.apply(dense, *levels)


class MEHLossFn(Function):
    """sum(((|lambda + 1e-9 - loss_noR|) * w)^2) for one level (Lambda_L2.py:235-241); form = 'l1' / 'msle': the sums of Lambda_L1.py:239-241 /
    Lambda_MSLE.py:239-242 (hipops.MEH_FORMS)."""

    @staticmethod
    def forward(ctx, L_score, loss_noR, bbox_w, arena=None, level=0, form='l2'):
        ctx.arena, ctx.level, ctx.form = arena, level, form
        lam = as_rows(L_score).view(-1)
        bw = bbox_w.reshape(-1, 4).contiguous()
        loss_noR = loss_noR.contiguous()
        out = ho.meh_loss_fwd(lam, loss_noR, bw, form=form)
        ctx.save_for_backward(lam, loss_noR, bw)
        ctx.shape = L_score.shape
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lam, loss_noR, bw = ctx.saved_tensors
        B, A, H, W = ctx.shape
        dst = ctx.arena.slice('lam', ctx.level, B * H * W, A, lam.device).view(-1, 1) if ctx.arena is not None else None
        gl = ho.meh_loss_bwd(lam, loss_noR, bw, g.reshape(1).float().contiguous(), grad=dst, form=ctx.form)
        return as_nchw(gl.view(B * H * W, A), B, H, W), None, None, None, None, None
