"""calculate_uncertainty / single_gpu_uncertainty / single_gpu_test with the reference's names and kwargs
(mmdet/apis/test.py:19-195).

Re-design for 8 x MI355X: the pool is SHARDED -- each rank scores the contiguous block
[r*ceil(N/W), (r+1)*ceil(N/W)) of the loader's dataset and the per-image fp32 scores are all-gathered over RCCL
(the reference's loader is dist=False, so every rank would score the whole pool).  Scores stay on the device
inside the loop; the host syncs once per pool.  The Philox stream is keyed by the global image index, so the
result is bit-identical for any world size."""
import os
import time
import weakref as _weakref

import numpy as np
import torch

from ..datasets import DeviceImageBatch
from ..mmcv_lite import DataContainer, ProgressBar
from ..parallel import gather_rows, gather_scores, gather_scores_indexed, get_dist_info, shard_batches, shard_range


class Uncertainty_fns:
    @staticmethod
    def Random(cfg, *args, **kwargs):
        return torch.randperm(len(args[1].dataset)).numpy()

    @staticmethod
    @torch.no_grad()
    def Entropy_NMS(cfg, *args, **kwargs):
        model, dataloader = args
        model.eval()
        # test_cfg.hua_estimator ('mc' | 'closed'): forwarded only when it selects something else than the default, so that a default run
        # keeps its kwargs -- and with them the key of its captured scoring graph
        tc = getattr(getattr(model, 'module', model), 'test_cfg', None)
        est = tc.get('hua_estimator') if hasattr(tc, 'get') else getattr(tc, 'hua_estimator', None)
        if est and est != 'mc' and 'hua_estimator' not in kwargs:
            kwargs['hua_estimator'] = est
        unc = single_gpu_uncertainty(model, dataloader, isUnc=cfg.uncertainty_type, uPool=cfg.uncertainty_pool,
                                     uPool2=cfg.uncertainty_pool2, **kwargs)
        return unc.cpu() if torch.is_tensor(unc) else [u.cpu() if torch.is_tensor(u) else u for u in unc]

    Entropy_ALL = Entropy_NMS          # test.py:52-63: same loop; the head switches on cfg.uncertainty_pool (ComputeScaleUnc path)
    Entropy_Avg = Entropy_NMS          # CalMCDropoutUnc.py:65-76: same loop again (Lambda_L2Net_NoL: ComputeAvgUnc + AggregateAvgUnc)

    @staticmethod
    @torch.no_grad()
    def _posterior(pool, cfg, *args, **kwargs):
        # posterior uncertainty pools: the Entropy_NMS loop (sharding, prefetch, captured scoring graph, one gather) with the
        # pool's own name; the head reads `unc_aggregate` ('max' | 'mean' | 'sum', default 'max') and `score_thr` (default 0.3).  No lambda
        # and no uPool2 are read: every head offers these pools, MyRetinaHead and the SSD head included
        model, dataloader = args
        model.eval()
        if kwargs.get('class_weighted'):
            sync_class_difficulty(model)
        else:
            kwargs.pop('class_weighted', None)      # (off: the default kwargs, and with them the key of the captured scoring graph)
        unc = single_gpu_uncertainty(model, dataloader, isUnc=getattr(cfg, 'uncertainty_type', None) or 'Epistemic', uPool=pool, **kwargs)
        return unc.cpu() if torch.is_tensor(unc) else [u.cpu() if torch.is_tensor(u) else u for u in unc]

    @staticmethod
    def Entropy(cfg, *args, **kwargs):
        return Uncertainty_fns._posterior('Entropy', cfg, *args, **kwargs)

    @staticmethod
    def Margin(cfg, *args, **kwargs):
        return Uncertainty_fns._posterior('Margin', cfg, *args, **kwargs)

    @staticmethod
    def LeastConf(cfg, *args, **kwargs):
        return Uncertainty_fns._posterior('LeastConf', cfg, *args, **kwargs)

    @staticmethod
    def Coreset(cfg, *args, **kwargs):
        # diversity-based selection (Sener & Savarese, ICLR 2018): needs the labelled set as the initial centers.  The HUA options that
        # calculate_uncertainty's callers pass for the Entropy_* pools (score_thr, clsW, ...) have no meaning for a descriptor pass
        model, dataloader = args
        return Coreset_uncertainty(cfg, model, dataloader, **_labelled_options('Coreset', kwargs, score_thr=False))

    @staticmethod
    def CDAL(cfg, *args, **kwargs):
        # contextual diversity (Agarwal et al., ECCV 2020), core-set form: like Coreset it needs the labelled set as the initial centers and
        # reads none of the HUA options -- but score_thr, which is its own region threshold too (default 0.3, the same foreground threshold)
        model, dataloader = args
        return CDAL_uncertainty(cfg, model, dataloader, **_labelled_options('CDAL', kwargs))

    @staticmethod
    def CCMS(cfg, *args, **kwargs):
        # uncertainty pre-selection + instance-level diversity (PPAL, Yang et al., CVPR 2024): needs the labelled set (it is
        # excluded from the candidates) and selects by rank like Coreset.  Of the HUA options only score_thr is read (the object gate);
        # candidate_factor, max_obj, measure and aggregate are its own
        model, dataloader = args
        own = {k: kwargs[k] for k in ('candidate_factor', 'max_obj', 'measure', 'aggregate') if kwargs.get(k) is not None}
        if kwargs.get('class_weighted'):
            own['class_weighted'] = True
        return CCMS_uncertainty(cfg, model, dataloader, **_labelled_options('CCMS', kwargs), **own)

    @staticmethod
    def PPAL(cfg, *args, **kwargs):
        # PPAL (Yang et al., CVPR 2024) whole: CCMS with stage 1 ranked by the difficulty-calibrated entropy -- every detection's
        # entropy times the weight of its class, from the class-difficulty EMA the head kept while it trained (bbox_head.class_difficulty)
        return Uncertainty_fns.CCMS(cfg, *args, **dict(kwargs, class_weighted=True))

    @staticmethod
    def _enms_options(kwargs):
        # what ENMS / DivProto read of calculate_uncertainty's kwargs: score_thr (the object gate, default 0.3) and their own options; the
        # other HUA options have no meaning for them
        own = {k: kwargs[k] for k in ('max_obj', 'measure', 't_enms') if kwargs.get(k) is not None}
        if kwargs.get('class_weighted'):
            own['class_weighted'] = True
        return own

    @staticmethod
    def ENMS(cfg, *args, **kwargs):
        # entropy-NMS uncertainty (Wu et al., CVPR 2022): ordinary scores, no labelled set is read
        model, dataloader = args
        thr = kwargs.get('score_thr')
        return ENMS_uncertainty(cfg, model, dataloader, score_thr=0.3 if thr is None else thr, **Uncertainty_fns._enms_options(kwargs))

    @staticmethod
    def DivProto(cfg, *args, **kwargs):
        # ENMS + the progressive diversity pick (Wu et al., CVPR 2022): needs the labelled set (it is excluded from the sweep)
        # and selects by rank like Coreset
        model, dataloader = args
        own = Uncertainty_fns._enms_options(kwargs)
        own.update({k: kwargs[k] for k in ('t_intra', 't_inter', 'alpha', 'beta', 'class_balance') if kwargs.get(k) is not None})
        return DivProto_uncertainty(cfg, model, dataloader, **_labelled_options('DivProto', kwargs), **own)

    @staticmethod
    def BADGE(cfg, *args, **kwargs):
        # gradient embeddings + k-means++ seeding (Ash et al., ICLR 2020): needs the labelled set (it is excluded from the
        # seeding) and selects by rank like Coreset.  Of the HUA options only score_thr is read (the object gate); max_obj and seed are its own
        model, dataloader = args
        own = {k: kwargs[k] for k in ('max_obj', 'seed') if kwargs.get(k) is not None}
        return BADGE_uncertainty(cfg, model, dataloader, **_labelled_options('BADGE', kwargs), **own)

    @staticmethod
    def KMeansPP(cfg, *args, **kwargs):
        # k-means++ seeding on the Core-set descriptors: Core-set's randomised, density-following counterpart.  Needs the
        # labelled set; like Coreset it reads none of the HUA options
        model, dataloader = args
        own = {k: kwargs[k] for k in ('seed',) if kwargs.get(k) is not None}
        return KMeansPP_uncertainty(cfg, model, dataloader, **_labelled_options('KMeansPP', kwargs, score_thr=False), **own)

    @staticmethod
    def _loc_stability(combine, cfg, *args, **kwargs):
        # localization stability (Kao et al., ACCV 2018): reads score_thr (the object gate, default 0.3), sigmas, seed and
        # same_class; the HUA options that calculate_uncertainty's callers pass for the Entropy_* pools have no meaning for it
        model, dataloader = args
        own = {k: kwargs[k] for k in ('sigmas', 'seed', 'same_class') if kwargs.get(k) is not None}
        thr = kwargs.get('score_thr')
        return LocStability_uncertainty(cfg, model, dataloader, score_thr=0.3 if thr is None else thr, combine=combine, **own)

    @staticmethod
    def LocStability(cfg, *args, **kwargs):
        return Uncertainty_fns._loc_stability('ls', cfg, *args, **kwargs)

    @staticmethod
    def LocStability_C(cfg, *args, **kwargs):
        return Uncertainty_fns._loc_stability('ls+c', cfg, *args, **kwargs)

    @staticmethod
    def Consistency(cfg, *args, **kwargs):
        # prediction consistency under mirroring (Elezi et al., CVPR 2022; CALD): reads score_thr (the object gate, default 0.3),
        # views, mode, unc_aggregate and same_class; the HUA options that calculate_uncertainty's callers pass for the Entropy_* pools have
        # no meaning for it
        model, dataloader = args
        own = {k: kwargs[k] for k in ('views', 'mode', 'same_class') if kwargs.get(k) is not None}
        if kwargs.get('unc_aggregate') is not None:
            own['aggregate'] = kwargs['unc_aggregate']
        thr = kwargs.get('score_thr')
        return Consistency_uncertainty(cfg, model, dataloader, score_thr=0.3 if thr is None else thr, **own)

    @staticmethod
    def Entropy_NoNMS(cfg, *args, **kwargs):
        # the reference's own Entropy_NoNMS path calls ComputeScaleUnc with L_scores=None (Lambda_L2.py:404-405,364) and raises a
        # TypeError on the first batch: there is no behaviour to reproduce
        raise NotImplementedError('uncertainty_pool=Entropy_NoNMS is not runnable in the reference either (L_scores is None there)')


# captured scoring graphs, per model (weak keys; a GraphedScore holds its model weakly too, so a dead model frees its graph memory pool by
# reference counting -- and nothing unpicklable hangs in the module's __dict__: copy.deepcopy(model) keeps working after a pool was scored)
_GSCORE = _weakref.WeakKeyDictionary()


_SHARD_STATE = dict(interleaved=False, imbalance=None, over=0)       # pool partition across ranks (single_gpu_uncertainty)


def calculate_uncertainty(cfg, *args, **kwargs):
    """test.py:65-70."""
    return getattr(Uncertainty_fns, cfg.uncertainty_pool)(cfg, *args, **kwargs)


def sync_class_difficulty(model, src=0):
    """Before a class-weighted pool pass: with torch.distributed initialised, rank `src`'s class_difficulty goes to every rank --
    each rank's EMA followed its own batches, and the ranks must weight alike to rank one pool -- then the head's class_weight buffer is
    recomputed from it in place (head.refresh_class_weight: device ops, no host sync), so a captured scoring graph reads current values.
    A head without the option raises (ValueError; the SSD heads NotImplementedError) before any batch is scored.  Returns the head."""
    m = getattr(model, 'module', model)
    head = getattr(m, 'bbox_head', m)
    if getattr(head, 'class_difficulty_cfg', None) is None:
        from ..scoring import _class_weight
        _class_weight(head, None, dict(class_weighted=True))
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.broadcast(head.class_difficulty, src=src)
    head.refresh_class_weight()
    return head


def _labelled_options(pool, kwargs, score_thr=True):
    """what a diversity pool's wrapper hands on of calculate_uncertainty's kwargs: X_L (required), budget, and score_thr (default 0.3)
    where the pool reads one"""
    if kwargs.get('X_L') is None:
        raise TypeError(f"Uncertainty_fns.{pool} needs the labelled indices: calculate_uncertainty(cfg, model, data_loader, X_L=X_L)")
    own = dict(X_L=kwargs['X_L'], budget=kwargs.get('budget'))
    if score_thr:
        thr = kwargs.get('score_thr')
        own['score_thr'] = 0.3 if thr is None else thr
    return own


def _unwrap(x):
    if isinstance(x, (list, tuple)):          # test-mode pipelines (MultiScaleFlipAug): one entry per augmentation, the metas in containers
        return [v.data[0] if isinstance(v, DataContainer) else v for v in x]
    return x.data if isinstance(x, DataContainer) else x


def _inputs(batch):
    """the forward's inputs of a collated batch"""
    return {k: _unwrap(v) for k, v in batch.items() if k in ('img', 'img_metas')}


def _shard_batches(dataset, batches, collate, workers):
    """(idxs, collated batch) over this rank's batches (lists of global image indices) of the pool.  workers > 0: worker processes decode / resize / normalise the
    images ahead of the GPU (the reference builds its pool loader with cfg.data.workers_per_gpu workers, tools/train_RetinaNet.py:224-225,
    mmdet/datasets/builder.py:76-139) into PINNED host memory, `prefetch` batches deep, so that the H2D copy of batch i + 1 and the host work
    of batches i + 2.. overlap the scoring graph of batch i; at ~4 000 images/s of GPU rate a single-process PIL decode + resize would bound
    the pool loop by more than 10x.  workers == 0: the synchronous loop (same batches, same order)."""
    if workers <= 0 or not batches:
        for idxs in batches:
            yield idxs, collate([dataset[i] for i in idxs])
        return
    from torch.utils.data import DataLoader
    dl = DataLoader(dataset, batch_sampler=batches, num_workers=workers, collate_fn=collate, pin_memory=False, prefetch_factor=4)
    for idxs, batch in zip(batches, dl):
        yield idxs, batch


def _pin(x):
    """pinned copy of a host tensor (asynchronous H2D source); DataContainers / lists are walked; a DeviceImageBatch (device transforms)
    pins its one byte buffer and is turned into the image batch by the scoring graph's fill or by the model's scatter"""
    if isinstance(x, DeviceImageBatch):
        return x.pin_memory()
    if torch.is_tensor(x):
        return x.pin_memory() if x.device.type == 'cpu' and not x.is_pinned() else x
    if isinstance(x, (list, tuple)):
        return type(x)(_pin(v) for v in x)
    return x


def _single(data):
    """one image tensor (or DeviceImageBatch) for the whole batch: the only form a GraphedScore takes"""
    return isinstance(data['img'], (list, tuple)) and len(data['img']) == 1


class _PoolPass:
    """One pool-sized pass over data_loader.dataset: the plumbing under single_gpu_uncertainty, single_gpu_ensemble, single_gpu_mcdropout
    and single_gpu_map.  It owns this rank's batches (the ONE parallel.shard_batches call), their GLOBAL image ids as one device tensor
    sliced per batch without a host sync (they key the Philox streams of the HUA sampler and of the dropout masks), the loader (prefetch
    workers into pinned memory, or the dataset's own device_batch), the progress bar, and the gather of the per-image scores.  A driver
    adds its graph (_graphed), its forward (_replay_or_eager) and what it does with the outputs.
    device_batch=False: a dataset's device_batch is not used (single_gpu_map takes the host loader always)."""

    def __init__(self, data_loader, dev, interleaved=False, device_batch=True):
        self.dataset, self.dev, self.interleaved = data_loader.dataset, dev, interleaved
        self.N = len(self.dataset)
        self.rank, self.world = get_dist_info()
        self.bs = data_loader.batch_size or 1
        self.my_batches = shard_batches(self.N, self.bs, self.rank, self.world, interleaved)
        self.my_idx = [i for b in self.my_batches for i in b]
        self.all_ids = torch.tensor(self.my_idx, dtype=torch.int64).to(dev)
        # images produced on the device (datasets.DevicePhiloxPool): no host collate / H2D
        self.device_side = device_batch and hasattr(self.dataset, 'device_batch')
        workers = int(os.environ.get('AOD_POOL_WORKERS', getattr(data_loader, 'num_workers', 0) or 0))
        self._stream = (((idxs, None) for idxs in self.my_batches) if self.device_side
                        else _shard_batches(self.dataset, self.my_batches, data_loader.collate_fn, workers))
        self.prog_bar = ProgressBar(len(self.my_idx))

    def batches(self, to_device=False, static_image=None):
        """yields (idxs, image_ids, data): data holds `img` / `img_metas` only, unwrapped, the images pinned when the device is a GPU.
        to_device: a single-image-list batch goes to the device ONCE here (one H2D copy / one transform launch) for drivers that run
        several forwards on it; single_gpu_uncertainty leaves that copy to GraphedScore._fill_img (from pinned memory, on its conv stream).
        static_image (GraphedScore.static_image): the device-generated pool writes its batch straight into the buffer the next replay reads."""
        dataset, dev, pos = self.dataset, self.dev, 0
        for idxs, data in self._stream:
            image_ids = self.all_ids[pos:pos + len(idxs)]
            pos += len(idxs)
            if self.device_side:
                out = static_image((len(idxs), 3) + tuple(dataset.size)) if static_image is not None and hasattr(dataset, 'size') else None
                data = dataset.device_batch(idxs, dev, image_ids=image_ids, out=out)
            else:
                data = _inputs(data)
                if dev.type == 'cuda':
                    data['img'] = _pin(data['img'])
            if to_device and dev.type == 'cuda' and _single(data):
                img = data['img'][0]
                img = img.to_device(dev) if isinstance(img, DeviceImageBatch) else img.to(dev, non_blocking=True)
                data['img'] = [img]
            yield idxs, image_ids, data
            self.prog_bar.update(len(idxs))

    def cat(self, chunks):
        return torch.cat(chunks) if chunks else torch.zeros(0, device=self.dev)

    def gather(self, local):
        """this rank's scores (in my_idx order) -> the full [N] vector on every rank"""
        if not self.interleaved:
            return gather_scores(local, self.N)
        per = -(-(-(-self.N // self.bs)) // self.world) * self.bs       # slots per rank of the interleaved partition: ceil(ceil(N / bs) / world) batches of bs
        return gather_scores_indexed(local, self.my_idx, self.N, per=per)


def _option_key(kwargs):
    """the part of a graph's cache key that names the forward's options, whatever order they were passed in; None when a value is not a
    hashable primitive (no caching, no graph: str() of a tensor / object could collide)"""
    if not all(isinstance(v, (bool, int, float, str, type(None))) for v in kwargs.values()):
        return None
    return tuple(sorted((k, type(v).__name__, v) for k, v in kwargs.items()))


def _graphed(model, dev, prefix, kwargs, cache=None, **ctor):
    """The GraphedScore(model, rescale=True, **ctor, **kwargs) cached under prefix + _option_key(kwargs), built on first use; None (the
    caller runs eagerly) when AOD_HIP_GRAPH=0, off the GPU, or for options that cannot be keyed.  cache: default _GSCORE[model] -- one
    captured graph per (model, options): a pool is scored once per AL cycle with a freshly built model, but callers that score several
    pools with one model (bench, tests) must not pay the capture again."""
    opts = _option_key(kwargs)
    if opts is None or dev.type != 'cuda' or os.environ.get('AOD_HIP_GRAPH', '1') == '0':
        return None
    if cache is None:
        cache = _GSCORE.setdefault(model, {})
    g = cache.get(prefix + opts)
    if g is None:
        from ..graphs import GraphedScore
        g = cache[prefix + opts] = GraphedScore(model, rescale=True, **ctor, **kwargs)
    return g


def _replay_or_eager(gscore, data, image_ids, eager, **maybe_kw):
    """the captured forward's outputs while single-image-list batches keep one shape (GraphedScore.maybe), else eager()'s"""
    if gscore is not None and _single(data):
        out = gscore.maybe(data['img'][0], data['img_metas'][0], image_ids, **maybe_kw)
        if out is not None:
            return out
    return eager()


def single_gpu_uncertainty(model, data_loader, **kwargs):
    """test.py:90-135, sharded.  Returns a [N] fp32 tensor (N = len(dataset)) identical on every rank."""
    model.eval()
    dev = next(model.parameters()).device
    # partition of the pool over the ranks (parallel.shard_batches): AOD_POOL_SHARD = contiguous | interleaved | auto (default: contiguous
    # until a pass measured more than 5 % imbalance between the ranks' loop times -- then every later pass of this process strides the batches)
    shard_mode = os.environ.get('AOD_POOL_SHARD', 'auto')
    interleaved = shard_mode == 'interleaved' or (shard_mode == 'auto' and _SHARD_STATE['interleaved'])
    pool = _PoolPass(data_loader, dev, interleaved)
    bs, world = pool.bs, pool.world
    chunks, conf_chunks = [], []
    kwargs.setdefault('scaleUnc', False)
    # HIP-graph replay of the scoring batch (graphs.GraphedScore) while batches keep one shape; side-effect options stay eager
    plain = not any(kwargs.get(k) for k in ('showNMS', 'saveUnc', 'saveMaxConf', 'scaleUnc', 'draw'))
    gscore = _graphed(model, dev, (), kwargs, isEval=False, batchIdx=0) if plain else None
    timed = world > 1 and dev.type == 'cuda' and torch.distributed.is_available() and torch.distributed.is_initialized()
    if timed:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    for idxs, image_ids, data in pool.batches(static_image=gscore.static_image if gscore is not None else None):
        def eager():
            with torch.no_grad():
                return model(return_loss=False, rescale=True, isEval=False, batchIdx=idxs[0] // bs, image_ids=image_ids, **data, **kwargs)
        # (replayed scores are read after gscore.sync() below)
        result, unc, *others = _replay_or_eager(gscore, data, image_ids, eager, defer=True)
        chunks.append(torch.as_tensor(unc, dtype=torch.float32, device=dev).reshape(-1))
        if kwargs.get('saveMaxConf'):          # test.py:130,134
            conf_chunks.append(torch.as_tensor(others[0], dtype=torch.float32, device=dev).reshape(-1))
    if gscore is not None:
        gscore.sync()                       # deferred selection halves (second stream) -> this stream
    local = pool.cat(chunks)
    if timed:           # load balance of this pass: every rank learns every rank's loop time and takes the same decision for the next pass
        import torch.distributed as dist
        ev1.record()
        ev1.synchronize()
        t = torch.tensor([ev0.elapsed_time(ev1)], device=dev)
        ts = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(ts, t)
        ts = torch.cat(ts)
        _SHARD_STATE['imbalance'] = float((ts.max() - ts.min()) / ts.max().clamp_min(1e-9))
        # (two CONSECUTIVE passes over the threshold: a pass that captured its scoring graph or started its loader workers measures that, not
        # the pool -- ADVICE r4)
        _SHARD_STATE['over'] = _SHARD_STATE['over'] + 1 if _SHARD_STATE['imbalance'] > 0.05 else 0
        if _SHARD_STATE['over'] >= 2:
            _SHARD_STATE['interleaved'] = True
    if kwargs.get('saveMaxConf'):
        return pool.gather(local), pool.gather(pool.cat(conf_chunks))
    return pool.gather(local)


@torch.no_grad()
def single_gpu_ensemble(models, data_loader, n_cls=None, **kwargs):
    """Ensemble_MI (mmdet/apis/CalEnsembleUnc.py:137-162) for 2 <= K <= 32 built models, on _PoolPass's loop: the pool is sharded
    over the ranks, batches come from the prefetch workers through pinned memory, the scores stay on the device and are gathered once.
    Returns a [N] fp32 tensor identical on every rank.

    Per batch: K forwards (isEval=True, justOut=True: classification maps only), then ONE aod_ensemble_mi launch pair on the same stream
    (scoring.ensemble_mi).  While the batch shape repeats (and AOD_HIP_GRAPH != 0) each member replays its own captured forward and hands
    back its graph's static maps; the MI kernel runs eagerly behind the K replays on the caller's stream, so it has read them before the
    next batch's replays overwrite them.  n_cls: classes per anchor row, default the head's cls_out_channels."""
    from ..scoring import ensemble_mi
    models = list(models)
    if not 2 <= len(models) <= 32:
        raise ValueError(f'single_gpu_ensemble: 2..32 ensemble members are supported, got {len(models)}')
    for m in models:
        m.eval()
    dev = next(models[0].parameters()).device
    pool = _PoolPass(data_loader, dev)
    if n_cls is None:
        n_cls = getattr(models[0], 'module', models[0]).bbox_head.cls_out_channels
    # one graph per MEMBER: a model listed twice gets two (each owns the static maps it hands back)
    gscores = [_graphed(m, dev, ('just_out', sum(1 for o in models[:k] if o is m)), kwargs, isEval=True, justOut=True)
               for k, m in enumerate(models)]
    chunks = []
    for idxs, image_ids, data in pool.batches(to_device=True):          # every member reads the one device tensor
        members = [_replay_or_eager(g, data, image_ids,
                                    lambda: m(return_loss=False, rescale=True, isEval=True, justOut=True, **data, **kwargs))
                   for g, m in zip(gscores, models)]
        chunks.append(ensemble_mi(members, n_cls))
    return pool.gather(pool.cat(chunks))


def Ensemble_uncertainty(cfg, *models, data_loader=None, **kwargs):
    """mmdet/apis/CalEnsembleUnc.py:86-88 with the reference's name and argument order (cfg, m1, m2, m3, data_loader), for 2..32 members:
    the loader is the last positional argument or the `data_loader` keyword.  Returns the CPU score tensor update_X_L takes."""
    models = list(models)
    if data_loader is None:
        if not models:
            raise TypeError('Ensemble_uncertainty(cfg, m1, m2, ..., data_loader): no data loader given')
        data_loader = models.pop()
    if not hasattr(data_loader, 'dataset'):
        raise TypeError('Ensemble_uncertainty(cfg, m1, m2, ..., data_loader): the last argument must be the pool loader')
    return single_gpu_ensemble(models, data_loader, **kwargs).cpu()


_MCD_STACKS = _weakref.WeakKeyDictionary()      # model -> {map shapes: the preallocated [n][L] stack of a batch shape}
_MCD_STATE = _weakref.WeakKeyDictionary()       # model -> {(batch size, options): the static factor table and the captured forward that reads it}


def _mcd_adjacent(out):
    """the maps are fp32 and lie back to back in one storage (the row ranges of a level-batched prediction conv's output buffer)"""
    base = out[0].untyped_storage().data_ptr()
    return all(t.dtype == torch.float32 and t.untyped_storage().data_ptr() == base for t in out) and all(
        out[l + 1].data_ptr() == out[l].data_ptr() + 4 * out[l].numel() for l in range(len(out) - 1))


def _mcd_stack(model, out, n):
    """n slots for the L classification maps of one batch shape.  The maps of a level-batched prediction conv are adjacent row ranges of one
    buffer: a slot is then ONE flat allocation with the same per-level views, filled by one device copy per sample; else L copies."""
    key = (n,) + tuple((tuple(t.shape), tuple(t.stride())) for t in out)
    cache = _MCD_STACKS.setdefault(model, {})
    st = cache.get(key)
    if st is None:
        sizes = [t.numel() for t in out]
        flat = _mcd_adjacent(out)
        slots = []
        for _ in range(n):
            if flat:
                buf, o, views = torch.empty(sum(sizes), dtype=torch.float32, device=out[0].device), 0, []
                for t, sz in zip(out, sizes):
                    views.append(buf.as_strided(tuple(t.shape), tuple(t.stride()), o))
                    o += sz
                slots.append((buf, views))
            else:
                slots.append((None, [torch.empty_like(t) for t in out]))
        st = cache[key] = (flat, sum(sizes), slots)
    return st


@torch.no_grad()
def single_gpu_mcdropout(model, data_loader, n=25, rate=0.1, seed=0, n_cls=None, **kwargs):
    """MCDropout_MI (mmdet/apis/CalMCDropoutUnc.py:137-163) on _PoolPass's loop: the pool is sharded over the ranks, batches come from
    the prefetch workers through pinned memory (one H2D copy per batch), the scores stay on the device and are gathered once.  Returns a [N]
    fp32 tensor identical on every rank.

    Per batch and per sample k = 0..n-1: one aod_dropout2d_masks launch writes the Dropout2d factors of every site into the static table
    (keyed by seed, k and the GLOBAL image ids), one forward with a Dropout2d(rate) behind every ReLU that feeds the classification maps
    (functional.mc_dropout: eval mode, isEval=True, justOut=True), one device copy of the maps into slot k of a preallocated stack; then ONE
    scoring.ensemble_mi call over the n slots.  While the batch shape repeats (and AOD_HIP_GRAPH != 0) the n forwards are n replays of ONE
    captured forward, which reads the table the mask kernel has just rewritten.  An image's score is a function of (weights, image, seed,
    image id, n, rate) only: the same bits alone, in any batch, on any rank count, eager or replayed."""
    from .. import functional as AF
    from .. import hipops as ho
    from ..scoring import ensemble_mi
    rate, n = float(rate), int(n)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f'single_gpu_mcdropout: rate must be in [0, 1), got {rate}')
    if not 2 <= n <= 32:
        raise ValueError(f'single_gpu_mcdropout: 2..32 stochastic forwards are supported (scoring.ensemble_mi takes up to 32 members), got n = {n}')
    sites = AF.dropout_sites(model)               # NotImplementedError for the SSD detectors (VGG sites are not built)
    L = len({k.rsplit('@', 1)[1] for k in sites if '@' in k})
    if n * L > 256:
        raise ValueError(f'single_gpu_mcdropout: n * levels = {n} * {L} exceeds the 256 map pointers of one ensemble_mi launch')
    model.eval()
    dev = next(model.parameters()).device
    pool = _PoolPass(data_loader, dev)
    if n_cls is None:
        n_cls = getattr(model, 'module', model).bbox_head.cls_out_channels
    # the static factor table [bs, T] and the captured forward that reads it: one entry per (model, batch size, options)
    opts = _option_key(kwargs)
    ent = {} if opts is None else _MCD_STATE.setdefault(model, {}).setdefault((pool.bs,) + opts, {})      # (options that cannot be keyed: not kept)
    if 'table' not in ent:
        ent['table'] = torch.ones(pool.bs, sites.T, dtype=torch.float32, device=dev)
    table = ent['table']
    offsets = sites.offsets(dev)
    state = AF.MCDropoutState(table, sites)
    gscore = _graphed(model, dev, ('graph',), kwargs, cache=ent, isEval=True, justOut=True, mc_dropout=state)
    chunks = []
    for idxs, image_ids, data in pool.batches(to_device=True):          # the n forwards read the one device tensor
        stack = None
        for k in range(n):
            ho.dropout2d_masks(table, image_ids, offsets, rate, seed, k)
            out = _replay_or_eager(gscore, data, image_ids, lambda: model(return_loss=False, rescale=True, isEval=True, justOut=True,
                                                                           mc_dropout=state, **data, **kwargs))
            if stack is None:
                stack = _mcd_stack(model, out, n)
            flat, total, slots = stack
            buf, views = slots[k]
            if flat and _mcd_adjacent(out):       # (a replay overwrites the graph's static maps: every sample is copied out)
                buf.copy_(out[0].as_strided((total,), (1,)))
            else:
                for d, t in zip(views, out):
                    d.copy_(t)
        chunks.append(ensemble_mi([views for _, views in stack[2]], n_cls))
    return pool.gather(pool.cat(chunks))


def MCDropout_uncertainty(cfg, model, data_loader, **kwargs):
    """mmdet/apis/CalMCDropoutUnc.py:86-88 with the reference's name and argument order.  kwargs: n (default 25 forwards), rate (0.1), seed,
    n_cls.  Returns the CPU score tensor update_X_L takes."""
    return single_gpu_mcdropout(model, data_loader, **kwargs).cpu()


def _fpn_neck(model, what):
    """the model's FPN neck; `what` opens the refusal of a detector without one ('<driver>: <its descriptors>')"""
    module = getattr(model, 'module', model)
    neck = getattr(module, 'neck', None)
    if not (hasattr(neck, 'num_outs') and isinstance(getattr(neck, 'out_channels', None), int)):
        raise NotImplementedError(f'{what} are built for the FPN pyramid of the RetinaNet detectors, not for {type(module).__name__} / '
                                  f'{type(neck).__name__} (SSD: its source maps do not share a channel count)')
    return neck


def _row_store_pass(model, data_loader, prefix, ctor, fkw, store, write):
    """The pool pass under the three descriptor drivers, on _PoolPass's loop: one forward per batch (model(..., **ctor, **fkw); while the
    batch shape repeats it replays the graph cached under `prefix`), then write(out, rows) puts the batch's rows into the preallocated
    [N, ...] pool tensors `store` (a dict) behind it on the same stream, so the graph's static outputs have been read before the next replay
    overwrites them.  Returns the dict of the pool tensors made whole on every rank (parallel.gather_rows)."""
    model.eval()
    dev = next(iter(store.values())).device
    pool = _PoolPass(data_loader, dev)
    gscore = _graphed(model, dev, prefix, fkw, **ctor)
    for idxs, image_ids, data in pool.batches():
        out = _replay_or_eager(gscore, data, image_ids, lambda: model(return_loss=False, rescale=True, **ctor, **data, **fkw))
        write(out, slice(idxs[0], idxs[0] + len(idxs)))          # (a batch is a run of consecutive images)
    owned = torch.zeros(pool.N, dtype=torch.bool, device=dev)
    owned[pool.all_ids] = True
    return {name: gather_rows(t, owned)[0] for name, t in store.items()}


@torch.no_grad()
def single_gpu_descriptors(model, data_loader, **kwargs):
    """Core-set descriptors of the whole pool on _PoolPass's loop: the pool is sharded over the ranks, batches come from the prefetch
    workers through pinned memory, and while the batch shape repeats (and AOD_HIP_GRAPH != 0) the forward (isEval=True, justFeat=True:
    backbone + neck, no head) replays one captured graph; the descriptor launch (scoring.pool_descriptor) runs eagerly behind the replay on
    the same stream, so it has read the graph's static neck outputs before the next replay overwrites them, and writes its rows straight
    into the preallocated [N, D] matrix.  parallel.gather_rows makes the matrix whole on every rank.  Returns the device [N, D] fp32
    tensor, D = levels * channels of the neck (RetinaNet: 1280); a row's bits depend on its image alone -- not on the batch size, the rank
    count, or eager / replayed execution."""
    from ..scoring import pool_descriptor
    neck = _fpn_neck(model, 'single_gpu_descriptors: Core-set descriptors')
    Cc, D = int(neck.out_channels), int(neck.num_outs) * int(neck.out_channels)
    desc = torch.zeros(len(data_loader.dataset), D, dtype=torch.float32, device=next(model.parameters()).device)
    return _row_store_pass(model, data_loader, ('just_feat',), dict(isEval=True, justFeat=True), kwargs, dict(desc=desc),
                           lambda feats, rows: pool_descriptor(feats, out=desc[rows], channels=Cc))['desc']


def _pick_scores(picks, N):
    """the picks of a selection in the form update_X_L takes, a CPU [N] fp32 vector: pick t = 0 .. budget - 1 scores budget - t, every
    other image 0"""
    budget = picks.numel()
    scores = torch.zeros(N, dtype=torch.float32, device=picks.device)
    scores[picks] = torch.arange(budget, 0, -1, dtype=torch.float32, device=picks.device)
    return scores.cpu()


def Coreset_uncertainty(cfg, model, data_loader, X_L=None, budget=None, **kwargs):
    """Core-set acquisition (O. Sener, S. Savarese, "Active Learning for Convolutional Neural Networks: A Core-Set Approach", ICLR 2018;
    the reference has none) in the form update_X_L takes: descriptors of the whole pool (single_gpu_descriptors), then k-center greedy
    with the labelled images X_L as centers (scoring.kcenter_greedy; every rank runs it on the same matrix and gets the same picks).
    budget: default cfg.X_S_size.  Returns a CPU [N] fp32 vector: the image picked at step t = 0 .. budget - 1 scores budget - t, every
    other image 0 -- with a falsy zeroRate update_X_L's arg[-X_S_size:] selects exactly the picks."""
    from ..scoring import kcenter_greedy
    if X_L is None:
        raise TypeError('Coreset_uncertainty(cfg, model, data_loader, X_L=...): the labelled indices X_L are the initial centers')
    budget = int(cfg.X_S_size if budget is None else budget)
    desc = single_gpu_descriptors(model, data_loader, **kwargs)
    return _pick_scores(kcenter_greedy(desc, X_L, budget)[0], desc.shape[0])


@torch.no_grad()
def single_gpu_cdal_descriptors(model, data_loader, score_thr=0.3, **kwargs):
    """CDAL descriptors of the whole pool on _PoolPass's loop: the pool is sharded over the ranks, batches come from the prefetch workers
    through pinned memory, and while the batch shape repeats (and AOD_HIP_GRAPH != 0) the forward (isEval=True, justOut=True: the
    classification maps only) replays one captured graph -- the one single_gpu_ensemble keeps for a single member; the descriptor launch
    (scoring.cdal_descriptor) runs eagerly behind the replay on the same stream, so it has read the graph's static maps before the next
    replay overwrites them, and writes its rows straight into the preallocated [N, D] matrix.  parallel.gather_rows makes the matrix whole
    on every rank.  Returns the device [N, D] fp32 tensor, D = 2 * cls_out_channels^2 (VOC: 800) = [P | ln P]; a row's bits depend on its
    image alone -- not on the batch size, the rank count, or eager / replayed execution."""
    from ..scoring import CDAL_MAX_CLASSES, cdal_descriptor
    module = getattr(model, 'module', model)
    head = getattr(module, 'bbox_head', None)
    n_cls = getattr(head, 'cls_out_channels', None)
    if not isinstance(n_cls, int) or n_cls != getattr(head, 'num_classes', None):
        raise NotImplementedError(f'single_gpu_cdal_descriptors: CDAL descriptors are built for the RetinaNet heads (a softmax over the '
                                  f'foreground classes), not for {type(module).__name__} / {type(head).__name__} (SSD: its rows carry a '
                                  'background column)')
    if n_cls > CDAL_MAX_CLASSES:
        raise ValueError(f'single_gpu_cdal_descriptors: up to {CDAL_MAX_CLASSES} classes are supported (2 * C^2 <= 2048 descriptor columns), '
                         f'the head has {n_cls}')
    desc = torch.zeros(len(data_loader.dataset), 2 * n_cls * n_cls, dtype=torch.float32, device=next(model.parameters()).device)
    return _row_store_pass(model, data_loader, ('just_out', 0), dict(isEval=True, justOut=True), kwargs, dict(desc=desc),
                           lambda maps, rows: cdal_descriptor(maps, n_cls, score_thr, out=desc[rows]))['desc']


def CDAL_uncertainty(cfg, model, data_loader, X_L=None, budget=None, score_thr=0.3, **kwargs):
    """CDAL acquisition (S. Agarwal, H. Arora, S. Anand, C. Arora, "Contextual Diversity for Active Learning", ECCV 2020, core-set form;
    the reference has none) in the form update_X_L takes: class-mixture descriptors of the whole pool (single_gpu_cdal_descriptors), then
    k-center greedy under the symmetrised KL divergence with the labelled images X_L as centers (scoring.kcenter_greedy(metric='symkl');
    every rank runs it on the same matrix and gets the same picks).  budget: default cfg.X_S_size.  Returns a CPU [N] fp32 vector: the
    image picked at step t = 0 .. budget - 1 scores budget - t, every other image 0 -- with a falsy zeroRate update_X_L's
    arg[-X_S_size:] selects exactly the picks."""
    from ..scoring import kcenter_greedy
    if X_L is None:
        raise TypeError('CDAL_uncertainty(cfg, model, data_loader, X_L=...): the labelled indices X_L are the initial centers')
    budget = int(cfg.X_S_size if budget is None else budget)
    desc = single_gpu_cdal_descriptors(model, data_loader, score_thr=score_thr, **kwargs)
    return _pick_scores(kcenter_greedy(desc, X_L, budget, metric='symkl')[0], desc.shape[0])


@torch.no_grad()
def single_gpu_object_descriptors(model, data_loader, max_obj=32, score_thr=0.3, measure='entropy', aggregate='sum', **kwargs):
    """CCMS object descriptors and the stage-1 score of the whole pool on _PoolPass's loop: the pool is sharded over the
    ranks, batches come from the prefetch workers through pinned memory, and while the batch shape repeats (and AOD_HIP_GRAPH != 0) the
    forward (isEval=True, _padded=True, objDesc=max_obj: backbone, neck, the two prediction towers, selection, NMS, the posterior score
    and the gather -- one graph on one stream, the form single_gpu_map uses) replays one captured graph.  The rows of its static outputs
    are copied into preallocated pool tensors behind each replay on the same stream, so they have been read before the next replay
    overwrites them; parallel.gather_rows makes the pool tensors whole on every rank.

    Returns a dict of device tensors: unc [N] fp32 (the posterior `measure` aggregated by `aggregate` over the detections whose score
    exceeds score_thr: Posterior_uncertainty's bits), feat [N, max_obj, C] fp32, cls [N, max_obj] int32 (-1 pad), w [N, max_obj] fp32,
    cnt [N] int32, missing [N] int32 (always 0).  The feature store is N * max_obj * C * 4 bytes: 542 MB for the 16 551 images of
    VOC07+12 trainval at max_obj = 32, C = 256.  A row's bits depend on its image alone -- not on the batch size, the rank count, or
    eager / replayed execution."""
    from ..scoring import CCMS_MAX_OBJ, UNC_AGGREGATES, UNC_MEASURES
    if measure not in UNC_MEASURES:
        raise ValueError(f"single_gpu_object_descriptors: unknown measure {measure!r} (expected 'entropy', 'margin' or 'leastconf')")
    if aggregate not in UNC_AGGREGATES:
        raise ValueError(f"single_gpu_object_descriptors: unknown aggregate {aggregate!r} (expected 'max', 'mean' or 'sum')")
    max_obj, score_thr = int(max_obj), float(score_thr)
    if not 1 <= max_obj <= CCMS_MAX_OBJ:
        raise ValueError(f'single_gpu_object_descriptors: max_obj must be in 1..{CCMS_MAX_OBJ}, got {max_obj}')
    if score_thr != score_thr:
        raise ValueError('single_gpu_object_descriptors: score_thr is NaN')
    neck = _fpn_neck(model, 'single_gpu_object_descriptors: CCMS object descriptors')
    N, Cc, dev = len(data_loader.dataset), int(neck.out_channels), next(model.parameters()).device
    store = dict(unc=torch.zeros(N, dtype=torch.float32, device=dev), feat=torch.zeros(N, max_obj, Cc, dtype=torch.float32, device=dev),
                 cls=torch.full((N, max_obj), -1, dtype=torch.int32, device=dev), w=torch.zeros(N, max_obj, dtype=torch.float32, device=dev),
                 cnt=torch.zeros(N, dtype=torch.int32, device=dev), missing=torch.zeros(N, dtype=torch.int32, device=dev))
    kwargs.setdefault('isUnc', False)
    fkw = dict(kwargs, objDesc=max_obj, score_thr=score_thr, unc_measure=measure, unc_aggregate=aggregate)

    def write(out, rows):
        for dst, t in zip(store.values(), out[3:]):
            dst[rows].copy_(t)
    return _row_store_pass(model, data_loader, ('obj_desc',), dict(isEval=True, _padded=True), fkw, store, write)


def CCMS_uncertainty(cfg, model, data_loader, X_L=None, budget=None, candidate_factor=4, max_obj=32, score_thr=0.3, measure='entropy',
                     aggregate='sum', class_weighted=False, **kwargs):
    """CCMS acquisition (the two-stage pick of PPAL: C. Yang, L. Huang, E. J. Crowley, "Plug and Play Active Learning for Object
    Detection", CVPR 2024; its training-side class-difficulty EMA: class_weighted below; the reference has none) in the form update_X_L takes.
    Stage 1: the posterior score of every image (single_gpu_object_descriptors) ranks the unlabelled images; the top
    M = min(ceil(candidate_factor * budget), #unlabelled) are the candidates (scoring.ccms_candidates).  Stage 2: the [M, M]
    category-conditioned matching distance between them (scoring.ccms_distance), then k-center greedy on it with no initial centers
    (scoring.kcenter_greedy_matrix): the first pick is the most uncertain candidate, every later one the candidate farthest from the picks
    so far.  Every rank runs stage 2 on the same tensors and gets the same picks.  budget: default cfg.X_S_size.  Returns a CPU [N] fp32
    vector: the image picked at step t = 0 .. budget - 1 scores budget - t, every other image 0 -- with a falsy zeroRate update_X_L's
    arg[-X_S_size:] selects exactly the picks.
    class_weighted=True (Uncertainty_fns.PPAL): stage 1 ranks by the difficulty-calibrated measure -- every detection's value times
    the weight of its class, from the class-difficulty EMA of a head built with bbox_head.class_difficulty; the published PPAL rule."""
    from ..scoring import ccms_candidates, ccms_distance, kcenter_greedy_matrix
    if X_L is None:
        raise TypeError('CCMS_uncertainty(cfg, model, data_loader, X_L=...): the labelled indices X_L are excluded from the candidates')
    budget = int(cfg.X_S_size if budget is None else budget)
    if class_weighted:
        sync_class_difficulty(model)
        kwargs['class_weighted'] = True
    pool = single_gpu_object_descriptors(model, data_loader, max_obj=max_obj, score_thr=score_thr, measure=measure, aggregate=aggregate, **kwargs)
    cand = ccms_candidates(pool['unc'], X_L, budget, candidate_factor)
    ci = torch.from_numpy(cand).to(pool['unc'].device)
    dist = ccms_distance(pool['feat'][ci].contiguous(), pool['cls'][ci].contiguous(), pool['w'][ci].contiguous(), pool['cnt'][ci].contiguous())
    return _pick_scores(ci[kcenter_greedy_matrix(dist, [], budget)[0]], pool['unc'].shape[0])


@torch.no_grad()
def single_gpu_enms(model, data_loader, max_obj=32, score_thr=0.3, measure='entropy', t_enms=0.5, keep_objects=False, **kwargs):
    """ENMS scores and class prototypes of the whole pool on _PoolPass's loop: single_gpu_object_descriptors' pass -- sharded,
    prefetched, the forward (isEval=True, _padded=True, objDesc=max_obj, objUnc=True: the descriptors and the per-object measure h in
    their slots) replayed from one captured graph while the batch shape repeats -- with scoring.enms_prototypes run per batch behind the
    replay on the same stream, on the graph's static outputs; its rows are copied into preallocated pool tensors, which
    parallel.gather_rows makes whole on every rank.  The object features are not kept: the prototype store takes their place.

    Returns a dict of device tensors: enms [N] fp32 (the entropy-NMS score: the sum of `measure` over the objects that survive the
    feature-similarity NMS at t_enms), kept [N] int32, proto [N, max_obj, C] fp32, pcls [N, max_obj] int32 (-1 pad), pconf [N, max_obj]
    fp32, pcnt [N] int32, missing [N] int32 (always 0); keep_objects=True adds h, w [N, max_obj] fp32, cls [N, max_obj] int32 and cnt [N]
    int32, the objects the scores were made of.  A row's bits depend on its image alone -- not on the batch size, the rank count, or eager /
    replayed execution."""
    from ..scoring import CCMS_MAX_OBJ, UNC_MEASURES, enms_prototypes
    if measure not in UNC_MEASURES:
        raise ValueError(f"single_gpu_enms: unknown measure {measure!r} (expected 'entropy', 'margin' or 'leastconf')")
    max_obj, score_thr, t_enms = int(max_obj), float(score_thr), float(t_enms)
    if not 1 <= max_obj <= CCMS_MAX_OBJ:
        raise ValueError(f'single_gpu_enms: max_obj must be in 1..{CCMS_MAX_OBJ}, got {max_obj}')
    if score_thr != score_thr or t_enms != t_enms:
        raise ValueError('single_gpu_enms: score_thr or t_enms is NaN')
    neck = _fpn_neck(model, 'single_gpu_enms: ENMS / DivProto object descriptors')
    N, Cc, dev = len(data_loader.dataset), int(neck.out_channels), next(model.parameters()).device
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    store = dict(enms=f32(N), kept=i32(N), proto=f32(N, max_obj, Cc), pcls=torch.full((N, max_obj), -1, dtype=torch.int32, device=dev),
                 pconf=f32(N, max_obj), pcnt=i32(N), missing=i32(N))
    if keep_objects:
        store.update(h=f32(N, max_obj), w=f32(N, max_obj), cls=torch.full((N, max_obj), -1, dtype=torch.int32, device=dev), cnt=i32(N))
    kwargs.setdefault('isUnc', False)
    fkw = dict(kwargs, objDesc=max_obj, objUnc=True, score_thr=score_thr, unc_measure=measure, unc_aggregate='sum')

    def write(out, rows):
        feat, cls, w, cnt, missing, h = out[4:10]
        res = enms_prototypes(feat, cls, w, h, cnt, t_enms)
        for name, t in zip(('enms', 'kept', 'proto', 'pcls', 'pconf', 'pcnt'), res):
            store[name][rows].copy_(t)
        store['missing'][rows].copy_(missing)
        if keep_objects:
            for name, t in (('h', h), ('w', w), ('cls', cls), ('cnt', cnt)):
                store[name][rows].copy_(t)
    return _row_store_pass(model, data_loader, ('enms',), dict(isEval=True, _padded=True), fkw, store, write)


def ENMS_uncertainty(cfg, model, data_loader, max_obj=32, score_thr=0.3, measure='entropy', t_enms=0.5, class_weighted=False, **kwargs):
    """Entropy-NMS uncertainty (the first half of Wu, Chen, Huang, "Entropy-based Active Learning for Object Detection with
    Progressive Diversity Constraint", CVPR 2022; the reference has none) in the form update_X_L takes: per image the sum of the posterior
    `measure` over the objects that survive an NMS by feature similarity (single_gpu_enms), so that near-duplicate instances of one class
    count once.  Returns the CPU [N] fp32 vector; these are ordinary scores, zeroRate stays on.  class_weighted as in CCMS_uncertainty."""
    if class_weighted:
        sync_class_difficulty(model)
        kwargs['class_weighted'] = True
    return single_gpu_enms(model, data_loader, max_obj=max_obj, score_thr=score_thr, measure=measure, t_enms=t_enms, **kwargs)['enms'].cpu()


def DivProto_uncertainty(cfg, model, data_loader, X_L=None, budget=None, max_obj=32, score_thr=0.3, measure='entropy', t_enms=0.5,
                         t_intra=0.7, t_inter=0.3, alpha=0.5, beta=0.75, class_balance=True, class_weighted=False, **kwargs):
    """ENMS + DivProto acquisition (Wu, Chen, Huang, CVPR 2022; the reference has none) in the form update_X_L takes: the ENMS
    score and the class prototypes of every image (single_gpu_enms), the unlabelled images ordered by that score
    (scoring.divproto_order), then the progressive pick on the device (scoring.divproto_select): an image whose every class prototype
    repeats one already picked (cosine above t_intra) is passed over, and with class_balance the share beta of the budget goes to images
    that bring a class the picks hold least.  Every rank runs the pick on the same tensors and gets the same picks.  budget: default
    cfg.X_S_size.  Returns a CPU [N] fp32 vector: the image picked at step t = 0 .. budget - 1 scores budget - t, every other image 0 --
    with a falsy zeroRate update_X_L's arg[-X_S_size:] selects exactly the picks.  class_weighted as in CCMS_uncertainty."""
    from ..scoring import divproto_order, divproto_select
    if X_L is None:
        raise TypeError('DivProto_uncertainty(cfg, model, data_loader, X_L=...): the labelled indices X_L are excluded from the sweep')
    budget = int(cfg.X_S_size if budget is None else budget)
    if class_weighted:
        sync_class_difficulty(model)
        kwargs['class_weighted'] = True
    pool = single_gpu_enms(model, data_loader, max_obj=max_obj, score_thr=score_thr, measure=measure, t_enms=t_enms, **kwargs)
    module = getattr(model, 'module', model)
    n_cls = int(module.bbox_head.num_classes)
    order = divproto_order(pool['enms'], X_L)
    picks, _ = divproto_select(order, pool['proto'], pool['pcls'], pool['pconf'], pool['pcnt'], n_cls, budget, t_intra=t_intra, t_inter=t_inter,
                               alpha=alpha, beta=beta, class_balance=class_balance)
    return _pick_scores(picks, pool['enms'].shape[0])


@torch.no_grad()
def single_gpu_badge_embeddings(model, data_loader, max_obj=32, score_thr=0.3, **kwargs):
    """BADGE gradient embeddings of the whole pool on _PoolPass's loop: single_gpu_object_descriptors' pass -- sharded,
    prefetched, the forward (isEval=True, _padded=True, objDesc=max_obj, objPost=True: the object descriptors and the posterior rows in
    their slots) replayed from one captured graph of its own while the batch shape repeats -- with the embedding launch
    (scoring.badge_embedding) run per batch behind the replay on the same stream, on the graph's static outputs, straight into the
    preallocated [N, D] store, which parallel.gather_rows makes whole on every rank.  Only the RetinaNet detectors are supported (evidence
    heads and the plain baseline); SSD raises NotImplementedError.

    Returns a dict of device tensors: emb [N, D] fp32, D = num_classes * C (class-major; an image without an object has the zero row),
    cnt [N] int32, missing [N] int32 (always 0).  The store is N * num_classes * C * 4 bytes: 339 MB for the 16 551 images of VOC07+12
    trainval (20 x 256 columns), 9.7 GB for the 118 287 of COCO train2017 (80 x 256).  A row's bits depend on its image alone -- not on
    the batch size, the rank count, or eager / replayed execution."""
    from ..scoring import BADGE_MAX_CLASSES, CCMS_MAX_OBJ, badge_embedding
    max_obj, score_thr = int(max_obj), float(score_thr)
    if not 1 <= max_obj <= CCMS_MAX_OBJ:
        raise ValueError(f'single_gpu_badge_embeddings: max_obj must be in 1..{CCMS_MAX_OBJ}, got {max_obj}')
    if score_thr != score_thr:
        raise ValueError('single_gpu_badge_embeddings: score_thr is NaN')
    neck = _fpn_neck(model, 'single_gpu_badge_embeddings: BADGE gradient embeddings')
    module = getattr(model, 'module', model)
    n_cls = int(module.bbox_head.num_classes)
    if not 1 <= n_cls <= BADGE_MAX_CLASSES:
        raise ValueError(f'single_gpu_badge_embeddings: up to {BADGE_MAX_CLASSES} classes are supported, the head has {n_cls}')
    N, Cc, dev = len(data_loader.dataset), int(neck.out_channels), next(model.parameters()).device
    store = dict(emb=torch.zeros(N, n_cls * Cc, dtype=torch.float32, device=dev), cnt=torch.zeros(N, dtype=torch.int32, device=dev),
                 missing=torch.zeros(N, dtype=torch.int32, device=dev))
    kwargs.setdefault('isUnc', False)
    fkw = dict(kwargs, objDesc=max_obj, objPost=True, score_thr=score_thr, unc_measure='entropy', unc_aggregate='sum')

    def write(out, rows):
        feat, cls, _, cnt, missing, post = out[4:10]
        badge_embedding(feat, post, cls, cnt, n_cls, out=store['emb'][rows])
        store['cnt'][rows].copy_(cnt)
        store['missing'][rows].copy_(missing)
    return _row_store_pass(model, data_loader, ('badge',), dict(isEval=True, _padded=True), fkw, store, write)


def _seed_scores(desc, X_L, budget, seed):
    """k-means++ seeding of `budget` rows of desc outside X_L (scoring.kmeanspp_seed; the draws come from np.random.default_rng(seed) on
    the host, so every rank picks alike) in the form update_X_L takes"""
    from ..scoring import kmeanspp_seed
    return _pick_scores(kmeanspp_seed(desc, X_L, budget, seed=seed)[0], desc.shape[0])


def BADGE_uncertainty(cfg, model, data_loader, X_L=None, budget=None, max_obj=32, score_thr=0.3, seed=0, **kwargs):
    """BADGE acquisition (J. T. Ash, C. Zhang, A. Krishnamurthy, J. Langford, A. Agarwal, "Deep Batch Active Learning by
    Diverse, Uncertain Gradient Lower Bounds", ICLR 2020; the reference has none) in the form update_X_L takes: the gradient embedding of
    every image (single_gpu_badge_embeddings: per object the gradient of the cross-entropy under the detection's own label times the
    neck row of its anchor's cell, summed over the image's objects), then k-means++ seeding on the unlabelled rows
    (scoring.kmeanspp_seed): the first pick is the longest embedding, every later one is drawn in proportion to its squared distance
    from the picks so far, so an uncertain image (a long row) far from the picks is likely.  The labelled images X_L are excluded, not
    centres.  seed: of the host draws; every rank runs the seeding on the same matrix with the same draws and gets the same picks.
    budget: default cfg.X_S_size.  Returns a CPU [N] fp32 vector: the image picked at step t = 0 .. budget - 1 scores budget - t, every
    other image 0 -- with a falsy zeroRate update_X_L's arg[-X_S_size:] selects exactly the picks."""
    if X_L is None:
        raise TypeError('BADGE_uncertainty(cfg, model, data_loader, X_L=...): the labelled indices X_L are excluded from the seeding')
    budget = int(cfg.X_S_size if budget is None else budget)
    pool = single_gpu_badge_embeddings(model, data_loader, max_obj=max_obj, score_thr=score_thr, **kwargs)
    return _seed_scores(pool['emb'], X_L, budget, seed)


def KMeansPP_uncertainty(cfg, model, data_loader, X_L=None, budget=None, seed=0, **kwargs):
    """k-means++ acquisition: BADGE's seeding on Core-set's descriptors (single_gpu_descriptors) -- pure diversity, and
    Core-set's randomised counterpart: where k-center greedy takes the farthest row and so chases outliers, D^2 sampling follows the
    density of the pool.  X_L, budget, seed and the returned vector as in BADGE_uncertainty."""
    if X_L is None:
        raise TypeError('KMeansPP_uncertainty(cfg, model, data_loader, X_L=...): the labelled indices X_L are excluded from the seeding')
    budget = int(cfg.X_S_size if budget is None else budget)
    return _seed_scores(single_gpu_descriptors(model, data_loader, **kwargs), X_L, budget, seed)


def Posterior_uncertainty(cfg, model, data_loader, measure='entropy', aggregate='max', score_thr=0.3, class_weighted=False, **kwargs):
    """Uncertainty sampling on the detector's own class posterior ("Entropy" in the paper's tables, margin and least confidence
    after Brust et al., VISAPP 2019, and Roy et al., BMVC 2018; the reference has none) in the form update_X_L takes: per detection whose
    score exceeds score_thr the entropy / 1-vs-2 margin / least confidence of its class posterior, aggregated over the image's detections
    by max / mean / sum; an image without such a detection scores 0.  One forward per image; the pool pass is single_gpu_uncertainty's
    (sharded, prefetched, one captured graph while the batch shape repeats, one gather).  Every detector has it: the evidence heads (their
    EDL-normalised scores), the plain RetinaNet (sigmoid scores) and SSD (softmax with background); the config's uncertainty_pool is not
    read.  Returns the CPU [N] fp32 vector; these are ordinary scores, zeroRate stays on.
    class_weighted=True: every detection's value is multiplied by the weight of its class, from the class-difficulty EMA of a head
    built with bbox_head.class_difficulty (the evidence heads and MyRetinaHead; any other head raises)."""
    from ..scoring import UNC_AGGREGATES, UNC_MEASURES
    if measure not in UNC_MEASURES:
        raise ValueError(f"Posterior_uncertainty: unknown measure {measure!r} (expected 'entropy', 'margin' or 'leastconf')")
    if aggregate not in UNC_AGGREGATES:
        raise ValueError(f"Posterior_uncertainty: unknown aggregate {aggregate!r} (expected 'max', 'mean' or 'sum')")
    score_thr = float(score_thr)
    if score_thr != score_thr:
        raise ValueError('Posterior_uncertainty: score_thr is NaN')
    pool = {'entropy': 'Entropy', 'margin': 'Margin', 'leastconf': 'LeastConf'}[measure]
    if class_weighted:
        kwargs['class_weighted'] = True
    return getattr(Uncertainty_fns, pool)(cfg, model, data_loader, unc_aggregate=aggregate, score_thr=score_thr, **kwargs)


def _batch_sizes(dev):
    """sizes(metas) -> int32 [B, 2] (h, w) of a batch on the device, kept by value (a pool re-uses a handful of them)"""
    cache = {}

    def sizes(metas):
        key = tuple((int(m['img_shape'][0]), int(m['img_shape'][1])) for m in metas)
        hw = cache.get(key)
        if hw is None:
            if len(cache) > 256:
                cache.clear()
            hw = cache[key] = torch.tensor(key, dtype=torch.int32).to(dev)
        return hw
    return sizes


def _view_stacks(who, model, pool, gscore, n_views, prep, view, fkw, kwargs):
    """The batch loop of the pool passes that score an image by several detection forwards on copies of it (single_gpu_loc_stability: noisy
    copies; single_gpu_consistency: mirrored copies).  Per batch: the clean forward model(return_loss=False, rescale=True, **fkw, **kwargs),
    then per view k = 0 .. n_views - 1 one view(k, img, out, prep(img, metas), image_ids) launch into a reused scratch batch and one
    forward; the outputs of every forward are copied into slot k + 1 of a preallocated stack (slot 0: the clean ones; a replay overwrites
    the graph's static outputs).  Yields (stack, preps) per batch: the tuple of stacked outputs [n_views + 1, ...] and prep's value for
    every image tensor of the batch.
    While the batch shape repeats the n_views + 1 forwards are replays of gscore's ONE captured graph: a shape is captured when a batch
    repeats the previous batch's shape, as in single_gpu_map.  A batch whose shape is seen for the first time (a ragged last batch, every
    batch of a variable-shape pool) makes all its forwards eagerly, and so does a batch that is a list of several image tensors, every one
    of which gets its own view launch."""
    from .. import functional as AF
    dev = pool.dev
    stacks, scratch = {}, {}
    for idxs, image_ids, data in pool.batches(to_device=True):          # the n_views + 1 forwards read the one device tensor
        # the batch as the model takes it: a list of image tensors (one entry; test-time augmentation lists have more) and their metas
        listed = isinstance(data['img'], (list, tuple))
        imgs = list(data['img']) if listed else [data['img']]
        metas = list(data['img_metas']) if listed else [data['img_metas']]
        if len(imgs) != len(metas) or not all(torch.is_tensor(t) and t.dim() == 4 for t in imgs):
            raise ValueError(f'{who}: a batch must hold [B, C, H, W] image tensors, one list of metas for each')
        imgs = [t.to(dev, non_blocking=True).float().contiguous() for t in imgs]      # (a one-tensor batch is on the device already)
        preps = [prep(t, m) for t, m in zip(imgs, metas)]
        g = None
        if gscore is not None and _single(data):
            gkey = (tuple(imgs[0].shape), AF.mode_key())
            if gkey in gscore.cache or gkey == gscore.pending:
                g = gscore
            else:
                gscore.pending = gkey
        stack = None
        for k in range(-1, n_views):
            xs = imgs
            if k >= 0:
                xs = []
                for a, (t, p) in enumerate(zip(imgs, preps)):
                    out = scratch.get((a, tuple(t.shape)))
                    if out is None:
                        out = scratch[(a, tuple(t.shape))] = torch.empty_like(t)
                    xs.append(view(k, t, out, p, image_ids))
            d = dict(data, img=xs if listed else xs[0])
            outs = _replay_or_eager(g, d, image_ids, lambda: model(return_loss=False, rescale=True, **fkw, **d, **kwargs))
            if stack is None:
                key = tuple((tuple(t.shape), t.dtype) for t in outs)
                stack = stacks.get(key)
                if stack is None:
                    stack = stacks[key] = tuple(torch.empty((n_views + 1,) + tuple(t.shape), dtype=t.dtype, device=dev) for t in outs)
            for dst, t in zip(stack, outs):
                dst[k + 1].copy_(t)
        yield stack, preps


def _noise_inv_std(img_metas, channels):
    """1 / std_c of a batch's normalisation in the tensor's channel order (img_metas[...]['img_norm_cfg']['std']; a meta without one was
    not normalised by the pipeline: std 1, Collect's own default).  One value for the whole batch, else ValueError."""
    stds = []
    for m in img_metas:
        cfg = m.get('img_norm_cfg') if hasattr(m, 'get') else None
        std = np.ones(channels, np.float64) if cfg is None else np.asarray(cfg['std'], np.float64).reshape(-1)
        if std.size != channels or not np.all(np.isfinite(std)) or not np.all(std > 0):
            raise ValueError(f'single_gpu_loc_stability: img_norm_cfg std {std.tolist()} does not hold {channels} finite positive values')
        stds.append(std)
    if any(not np.array_equal(s, stds[0]) for s in stds[1:]):
        raise ValueError('single_gpu_loc_stability: the images of one batch were normalised with different std '
                         f'({sorted({tuple(s.tolist()) for s in stds})}); the noise is scaled by one std per channel')
    return [float(1.0 / v) for v in stds[0]]


def _check_sigmas(sigmas):
    from ..scoring import LOCSTAB_MAX_LEVELS
    try:
        sigmas = tuple(float(s) for s in sigmas)
    except TypeError:
        raise ValueError(f'single_gpu_loc_stability: sigmas must be a sequence of noise levels, got {sigmas!r}') from None
    if not 1 <= len(sigmas) <= LOCSTAB_MAX_LEVELS:
        raise ValueError(f'single_gpu_loc_stability: 1..{LOCSTAB_MAX_LEVELS} noise levels are supported, got {len(sigmas)}')
    if not all(s >= 0.0 and s != float('inf') for s in sigmas):
        raise ValueError(f'single_gpu_loc_stability: every noise level must be finite and >= 0, got {sigmas}')
    return sigmas


@torch.no_grad()
def single_gpu_loc_stability(model, data_loader, sigmas=(8, 16, 24, 32, 40, 48), seed=0, score_thr=0.3, same_class=False, combine='ls',
                             **kwargs):
    """Localization stability (C.-C. Kao, T.-Y. Lee, P. Sen, M.-Y. Liu, "Localization-Aware Active Learning for Object Detection", ACCV
    2018; the reference has none) on _PoolPass's loop: the pool is sharded over the ranks, batches come from the prefetch workers
    through pinned memory (one H2D copy per batch), the scores stay on the device and are gathered once.  Returns a [N] fp32 tensor
    identical on every rank.

    Per batch: the clean detection forward (isEval=True, padded outputs), then per noise level k one aod_pixel_noise launch into a reused
    scratch batch (keyed by seed, k and the GLOBAL image ids; sigmas in 0..255 pixel units, scaled by the batch's img_norm_cfg std) and one
    forward; (dets, labels, num) are copied into slot k of a preallocated stack after every forward, then ONE scoring.loc_stability launch.
    While the batch shape repeats (and AOD_HIP_GRAPH != 0) the K + 1 forwards are K + 1 replays of the ONE captured detection graph
    single_gpu_map uses (the same key: an evaluation and a stability pass of one model share the capture): a shape is captured when a
    batch repeats the previous batch's shape, as in single_gpu_map.  A batch whose shape is seen for the first time (a ragged last batch,
    every batch of a variable-shape pool) makes all its K + 1 forwards eagerly, and so does a batch that is a list of several image
    tensors, every one of which gets its own noise launch (the detectors here refuse such test-time augmentation lists themselves).  It
    needs nothing but detections, so every detector has it.  An image's score is a function of (weights, image, seed, image id, sigmas) only: the same bits
    alone, in any batch, on any rank count, eager or replayed."""
    from .. import hipops as ho
    from ..scoring import LOCSTAB_COMBINES, loc_stability
    sigmas = _check_sigmas(sigmas)
    if combine not in LOCSTAB_COMBINES:
        raise ValueError(f"single_gpu_loc_stability: unknown combine {combine!r} (expected 'ls' or 'ls+c')")
    score_thr = float(score_thr)
    if score_thr != score_thr:
        raise ValueError('single_gpu_loc_stability: score_thr is NaN')
    seed = int(seed)
    kwargs.setdefault('isUnc', False)              # (single_gpu_map's option set: the two passes share one graph key)
    model.eval()
    dev = next(model.parameters()).device
    pool = _PoolPass(data_loader, dev)
    gscore = _graphed(model, dev, ('eval_padded',), kwargs, isEval=True, _padded=True)
    sizes, chunks = _batch_sizes(dev), []

    def prep(t, metas):
        return _noise_inv_std(metas, int(t.shape[1])), sizes(metas)

    def noisy(k, t, out, p, image_ids):
        return ho.pixel_noise(t, out, p[1], p[0], sigmas[k], k, seed, image_ids)

    for stack, _ in _view_stacks('single_gpu_loc_stability', model, pool, gscore, len(sigmas), prep, noisy, dict(isEval=True, _padded=True),
                                 kwargs):
        chunks.append(loc_stability(*stack, score_thr=score_thr, same_class=same_class, combine=combine))
    return pool.gather(pool.cat(chunks))


def LocStability_uncertainty(cfg, model, data_loader, **kwargs):
    """Localization-stability acquisition in the form update_X_L takes (single_gpu_loc_stability; kwargs: sigmas, seed, score_thr,
    same_class, combine 'ls' | 'ls+c').  Larger scores are selected first; these are ordinary scores, zeroRate stays on.  The config is not
    read.  Returns the CPU [N] fp32 vector."""
    return single_gpu_loc_stability(model, data_loader, **kwargs).cpu()


def _frame_extent(img_metas):
    """(w / scale_x, h / scale_y) of every image of a batch in Python floats: the extent of the frame that rescaled detections lie in
    (img_shape (h, w, ...), scale_factor (sx, sy, sx, sy) or one number; a meta without a scale factor was not resized: 1)"""
    out = []
    for m in img_metas:
        h, w = float(m['img_shape'][0]), float(m['img_shape'][1])
        sf = m.get('scale_factor') if hasattr(m, 'get') else None
        sf = np.ones(2, np.float64) if sf is None else np.asarray(sf, np.float64).reshape(-1)
        sx, sy = (float(sf[0]), float(sf[1])) if sf.size >= 2 else (float(sf[0]), float(sf[0]))
        if not (sx > 0.0 and sy > 0.0 and sx != float('inf') and sy != float('inf')):
            raise ValueError(f'single_gpu_consistency: scale_factor {sf.tolist()} does not hold finite positive values')
        out.append((w / sx, h / sy))
    return tuple(out)


@torch.no_grad()
def single_gpu_consistency(model, data_loader, views=('hflip',), mode='both', aggregate='max', score_thr=0.3, same_class=False, _stats=None,
                           **kwargs):
    """Prediction consistency under mirroring (I. Elezi et al., "Not All Labels Are Equal: Rationalizing the Labeling Costs for Training
    Object Detection", CVPR 2022; CALD: W. Yu et al., "Consistency-based Active Learning for Object Detection", CVPR Workshops 2022; DESIGN
    3q; the reference has none) on _PoolPass's loop: the pool is sharded over the ranks, batches come from the prefetch workers through
    pinned memory (one H2D copy per batch), the scores stay on the device and are gathered once.  Returns a [N] fp32 tensor identical on
    every rank.

    Per batch: the clean detection forward (isEval=True, padded outputs, detPost=True: the detections and the class-posterior row of every
    one), then per view one aod_flip_images launch into a reused scratch batch (the image mirrored inside its img_shape, the pad left where
    the collate put it; the metas are passed unchanged) and one forward; the five outputs are copied into slot v of a preallocated stack
    after every forward, then ONE scoring.det_consistency launch: the views' boxes are mapped back into the rescaled frame of extent
    (w / scale_x, h / scale_y), every clean detection above score_thr is matched to the box of largest IoU of every view, and the image is
    scored by 1 - IoU (mode 'box'), the Jensen-Shannon divergence of the two posterior rows ('cls') or their mean ('both'), averaged over the
    views and aggregated over the detections by max / mean / sum.  While the batch shape repeats (and AOD_HIP_GRAPH != 0) the V + 1 forwards
    are V + 1 replays of ONE captured graph under its own key ('eval_post',): a shape is captured when a batch repeats the previous batch's
    shape, as in single_gpu_map.  A batch whose shape is seen for the first time makes all its V + 1 forwards eagerly, and so does a batch
    that is a list of several image tensors, every one of which gets its own flip launch.  It needs nothing but detections and their score
    rows, so every detector has it.  An image's score is a function of (weights, image, metas, views, options) only: the same bits alone, in
    any batch, on any rank count, eager or replayed.  _stats (a dict): receives 'missing', the [N] count of detections without a posterior
    row (always 0)."""
    from .. import hipops as ho
    from ..scoring import ACTIVATION_LAYOUT, CONSISTENCY_MODES, UNC_AGGREGATES, consistency_views, det_consistency
    views = tuple(views) if isinstance(views, (list, tuple)) else views
    consistency_views(views, 'single_gpu_consistency')
    if mode not in CONSISTENCY_MODES:
        raise ValueError(f"single_gpu_consistency: unknown mode {mode!r} (expected 'box', 'cls' or 'both')")
    if aggregate not in UNC_AGGREGATES:
        raise ValueError(f"single_gpu_consistency: unknown aggregate {aggregate!r} (expected 'max', 'mean' or 'sum')")
    score_thr = float(score_thr)
    if score_thr != score_thr:
        raise ValueError('single_gpu_consistency: score_thr is NaN')
    kwargs.setdefault('isUnc', False)
    model.eval()
    dev = next(model.parameters()).device
    module = getattr(model, 'module', model)
    layout = ACTIVATION_LAYOUT[getattr(getattr(module, 'bbox_head', module), 'last_activation')]
    pool = _PoolPass(data_loader, dev)
    gscore = _graphed(model, dev, ('eval_post',), kwargs, isEval=True, _padded=True, detPost=True)
    sizes, ext_cache, chunks, miss_chunks = _batch_sizes(dev), {}, [], []

    def prep(t, metas):
        """(int32 [B, 2] (h, w), fp32 [B, 2] extent (w, h)) of a batch on the device, the extents kept by value like the sizes"""
        key = _frame_extent(metas)
        ext = ext_cache.get(key)
        if ext is None:
            if len(ext_cache) > 256:
                ext_cache.clear()
            ext = ext_cache[key] = torch.tensor(key, dtype=torch.float32).to(dev)
        return sizes(metas), ext

    def mirrored(v, t, out, p, image_ids):
        return ho.flip_images(t, out, p[0], views[v])

    for stack, preps in _view_stacks('single_gpu_consistency', model, pool, gscore, len(views), prep, mirrored,
                                     dict(isEval=True, _padded=True, detPost=True), kwargs):
        ext = preps[0][1]                 # (rescaled detections of every entry of a list batch lie in the one original frame)
        chunks.append(det_consistency(*stack[:4], views, ext, layout, mode=mode, aggregate=aggregate, score_thr=score_thr,
                                      same_class=same_class))
        if _stats is not None:
            miss_chunks.append(stack[4].sum(0).float())
    if _stats is not None:
        _stats['missing'] = pool.gather(pool.cat(miss_chunks))
    return pool.gather(pool.cat(chunks))


def Consistency_uncertainty(cfg, model, data_loader, **kwargs):
    """Consistency acquisition in the form update_X_L takes (single_gpu_consistency; kwargs: views, mode 'both' | 'box' | 'cls', aggregate
    'max' | 'mean' | 'sum', score_thr, same_class).  Larger scores are selected first; these are ordinary scores, zeroRate stays on.  The
    config is not read.  Returns the CPU [N] fp32 vector."""
    return single_gpu_consistency(model, data_loader, **kwargs).cpu()


@torch.no_grad()
def single_gpu_test(model, data_loader, show=False, out_dir=None, show_score_thr=0.3, **kwargs):
    """test.py:138-195 (detection results for evaluation; isEval=True).  detUnc=True: returns (results, unc_results) where
    unc_results[i][c] is a (k, 2) float32 array (aleatoric, epistemic), row-aligned with results[i][c]; the box arrays keep five columns
    (eval_map reads the score from column -1)."""
    model.eval()
    results, unc_results = [], []
    for data in data_loader:
        data = _inputs(data)
        kw = dict(kwargs)
        kw.setdefault('isUnc', False)              # EvalHook forwards the whole `evaluation` dict (interval popped): isUnc, metric, ...
        out = model(return_loss=False, rescale=True, isEval=True, **data, **kw)
        if kw.get('detUnc'):
            results.extend(out[0]), unc_results.extend(out[1])
        else:
            results.extend(out)
    return (results, unc_results) if kwargs.get('detUnc') else results


def eval_annotations(dataset):
    """[dataset.get_ann_info(i)] read once per dataset object (VOC: one XML parse per image) and kept on it."""
    anns = getattr(dataset, '_eval_annotations', None)
    if anns is None or len(anns) != len(dataset):
        anns = [dataset.get_ann_info(i) for i in range(len(dataset))]
        try:
            dataset._eval_annotations = anns
        except AttributeError:
            pass
    return anns


@torch.no_grad()
def single_gpu_map(model, data_loader, iou_thr=0.5, dataset=None, show=False, out_dir=None, show_score_thr=0.3, logger='silent',
                   scale_ranges=None, tpfp_fn=None, annotations=None, _timing=None, **kwargs):
    """Evaluation on the device: detect (isEval=True, padded outputs) -> aod_eval_match -> core.evaluation_device.DeviceMapAccumulator, one
    D2H copy per evaluation.  Returns (mean_ap, eval_results) for a float `iou_thr`, a list of such pairs for a list of thresholds -- each
    bit-identical to eval_map(single_gpu_test(model, data_loader), annotations, iou_thr=thr, dataset=dataset).

    The loop is _PoolPass's: the test set is sharded over the ranks (shard_batches), batches come from the prefetch workers
    through pinned memory, and while the batch shape repeats (and AOD_HIP_GRAPH != 0) the detection pass replays one captured graph
    (single stream: isEval has no two-phase form); the match kernel runs eagerly behind the replay on the same stream, so it has read the
    graph's static outputs before the next replay overwrites them.  `annotations`: the dataset's, when the caller already holds them.
    `_timing` (a dict; tools/eval_throughput.py): the loop is followed by a device sync and its wall time lands in _timing['pass_s']."""
    t_start = time.perf_counter()
    from ..core.evaluation import print_map_summary
    from ..core.evaluation_device import DeviceMapAccumulator
    if kwargs.get('detUnc'):
        raise ValueError('single_gpu_map: detUnc is not offered on the device metric; use single_gpu_test(detUnc=True)')
    for k in ('device_metric', 'metric', 'proposal_nums', 'interval'):          # EvalHook forwards the whole `evaluation` dict
        kwargs.pop(k, None)
    kwargs.setdefault('isUnc', False)
    single = isinstance(iou_thr, (int, float))
    iou_thrs = [float(iou_thr)] if single else [float(t) for t in iou_thr]
    model.eval()
    ds = data_loader.dataset
    N = len(ds)
    module = getattr(model, 'module', model)
    dev = next(model.parameters()).device
    acc = DeviceMapAccumulator(module.bbox_head.num_classes, iou_thrs, module.bbox_head.test_cfg.max_per_img, N, dev,
                               scale_ranges=scale_ranges, tpfp_fn=tpfp_fn)
    anns = annotations if annotations is not None else eval_annotations(ds)
    assert len(anns) == N
    pool = _PoolPass(data_loader, dev, device_batch=False)
    gscore = _graphed(model, dev, ('eval_padded',), kwargs, isEval=True, _padded=True)
    for idxs, image_ids, data in pool.batches():
        dets, labels, num = _replay_or_eager(gscore, data, image_ids,
                                             lambda: model(return_loss=False, rescale=True, isEval=True, _padded=True, **data, **kwargs))
        acc.update(idxs, dets, labels, num, [anns[i] for i in idxs])
    if _timing is not None:
        torch.cuda.synchronize()
        _timing['pass_s'] = time.perf_counter() - t_start
    acc.gather()
    res = acc.finalize(dataset)
    for mean_ap, eval_results in res:
        print_map_summary(mean_ap, eval_results, dataset, None, logger=logger)
    return res[0] if single else res


def coco_eval_infos(dataset):
    """[dataset.get_eval_info(i)] read once per dataset object (CocoDataset.eval_infos keeps them)"""
    if hasattr(dataset, 'eval_infos'):
        return dataset.eval_infos()
    if not hasattr(dataset, 'get_eval_info'):
        raise TypeError(f'{type(dataset).__name__} has no get_eval_info: the COCO bbox metric needs a CocoDataset, or eval_infos=')
    return [dataset.get_eval_info(i) for i in range(len(dataset))]


@torch.no_grad()
def single_gpu_coco_map(model, data_loader, iou_thrs=None, proposal_nums=(100, 300, 1000), classwise=False, metric_items=None,
                        logger='silent', eval_infos=None, _timing=None, **kwargs):
    """COCO bbox evaluation on the device: detect (isEval=True, padded outputs) -> aod_coco_match -> core.coco_eval_device
    .DeviceCocoAccumulator, one D2H copy per evaluation.  Returns the dict of
    dataset.evaluate(single_gpu_test(model, data_loader), metric='bbox', iou_thrs=..., classwise=..., metric_items=...), value for value.

    The loop is single_gpu_map's: the test set is sharded over the ranks (_PoolPass), batches come from the prefetch workers through
    pinned memory, and while the batch shape repeats (and AOD_HIP_GRAPH != 0) the detection pass replays the captured ('eval_padded',)
    graph; the match kernel runs eagerly behind the replay on the same stream, so it has read the graph's static outputs before the next
    replay overwrites them.  `eval_infos`: the dataset's get_eval_info list, when the caller already holds it.  `_timing` (a dict;
    tools/eval_throughput.py): the loop is followed by a device sync and its wall time lands in _timing['pass_s'], the gathered
    DeviceCocoAccumulator in _timing['accumulator']."""
    t_start = time.perf_counter()
    from ..core.coco_eval import check_metric
    from ..core.coco_eval_device import DeviceCocoAccumulator
    if kwargs.get('detUnc'):
        raise ValueError('single_gpu_coco_map: detUnc is not offered on the device metric; use single_gpu_test(detUnc=True)')
    check_metric(kwargs.pop('metric', 'bbox'))
    for k in ('device_metric', 'interval', 'show', 'out_dir', 'show_score_thr'):          # EvalHook forwards the whole `evaluation` dict
        kwargs.pop(k, None)
    kwargs.setdefault('isUnc', False)
    model.eval()
    ds = data_loader.dataset
    N = len(ds)
    module = getattr(model, 'module', model)
    dev = next(model.parameters()).device
    acc = DeviceCocoAccumulator(module.bbox_head.num_classes, iou_thrs, module.bbox_head.test_cfg.max_per_img, N, dev,
                                proposal_nums=proposal_nums)
    infos = eval_infos if eval_infos is not None else coco_eval_infos(ds)
    assert len(infos) == N
    pool = _PoolPass(data_loader, dev, device_batch=False)
    gscore = _graphed(model, dev, ('eval_padded',), kwargs, isEval=True, _padded=True)
    for idxs, image_ids, data in pool.batches():
        dets, labels, num = _replay_or_eager(gscore, data, image_ids,
                                             lambda: model(return_loss=False, rescale=True, isEval=True, _padded=True, **data, **kwargs))
        acc.update(idxs, dets, labels, num, [infos[i] for i in idxs])
    if _timing is not None:
        torch.cuda.synchronize()
        _timing['pass_s'] = time.perf_counter() - t_start
    acc.gather()
    if _timing is not None:
        _timing['accumulator'] = acc          # (the tests read its unrounded precision array)
    return acc.finalize(getattr(ds, 'CLASSES', None), classwise=classwise, metric_items=metric_items, logger=logger)
