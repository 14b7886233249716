"""calculate_uncertainty / single_gpu_uncertainty / single_gpu_test with the reference's names and kwargs
(mmdet/apis/test.py:19-195).

Re-design for 8 x MI355X: the pool is SHARDED -- each rank scores the contiguous block
[r*ceil(N/W), (r+1)*ceil(N/W)) of the loader's dataset and the per-image fp32 scores are all-gathered over RCCL
(the reference's loader is dist=False, so every rank would score the whole pool).  Scores stay on the device
inside the loop; the host syncs once per pool.  The Philox stream is keyed by the global image index, so the
result is bit-identical for any world size."""
import numpy as np
import torch

from ..datasets import DeviceImageBatch
from ..mmcv_lite import DataContainer, ProgressBar
from ..parallel import gather_scores, gather_scores_indexed, get_dist_info, shard_batches, shard_range


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
    def Entropy_NoNMS(cfg, *args, **kwargs):
        # the reference's own Entropy_NoNMS path calls ComputeScaleUnc with L_scores=None (Lambda_L2.py:404-405,364) and raises a
        # TypeError on the first batch: there is no behaviour to reproduce
        raise NotImplementedError('uncertainty_pool=Entropy_NoNMS is not runnable in the reference either (L_scores is None there)')


# captured scoring graphs, per model (weak keys; a GraphedScore holds its model weakly too, so a dead model frees its graph memory pool by
# reference counting -- and nothing unpicklable hangs in the module's __dict__: copy.deepcopy(model) keeps working after a pool was scored)
import weakref as _weakref
_GSCORE = _weakref.WeakKeyDictionary()


_SHARD_STATE = dict(interleaved=False, imbalance=None, over=0)       # pool partition across ranks (single_gpu_uncertainty)


def calculate_uncertainty(cfg, *args, **kwargs):
    """test.py:65-70."""
    return getattr(Uncertainty_fns, cfg.uncertainty_pool)(cfg, *args, **kwargs)


def _unwrap(x):
    return x.data if isinstance(x, DataContainer) else x


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


def single_gpu_uncertainty(model, data_loader, **kwargs):
    """test.py:90-135, sharded.  Returns a [N] fp32 tensor (N = len(dataset)) identical on every rank."""
    model.eval()
    dataset = data_loader.dataset
    N = len(dataset)
    rank, world = get_dist_info()
    bs = data_loader.batch_size or 1
    # partition of the pool over the ranks (parallel.shard_batches): AOD_POOL_SHARD = contiguous | interleaved | auto (default: contiguous
    # until a pass measured more than 5 % imbalance between the ranks' loop times -- then every later pass of this process strides the batches)
    import os
    shard_mode = os.environ.get('AOD_POOL_SHARD', 'auto')
    interleaved = shard_mode == 'interleaved' or (shard_mode == 'auto' and _SHARD_STATE['interleaved'])
    my_batches = shard_batches(N, bs, rank, world, interleaved)
    collate = data_loader.collate_fn
    prog_bar = ProgressBar(sum(len(b) for b in my_batches))
    chunks, conf_chunks = [], []
    kwargs.setdefault('scaleUnc', False)
    # HIP-graph replay of the scoring batch (graphs.GraphedScore) while batches keep one shape; side-effect options stay eager
    plain = not any(kwargs.get(k) for k in ('showNMS', 'saveUnc', 'saveMaxConf', 'scaleUnc', 'draw'))
    others = []
    gscore = None
    if plain and os.environ.get('AOD_HIP_GRAPH', '1') != '0' and next(model.parameters()).is_cuda:
        from ..graphs import GraphedScore
        # one captured graph per (model, options): a pool is scored once per AL cycle with a freshly built model, but callers that score
        # several pools with one model (bench, tests) must not pay the capture again
        # (the key holds hashable primitives only; any other option value -> no caching, no graph: str() of a tensor / object could collide)
        if all(isinstance(v, (bool, int, float, str, type(None))) for v in kwargs.values()):
            cache = _GSCORE.setdefault(model, {})
            key = tuple(sorted((k, type(v).__name__, v) for k, v in kwargs.items()))
            gscore = cache.get(key)
            if gscore is None:
                gscore = cache[key] = GraphedScore(model, rescale=True, isEval=False, batchIdx=0, **kwargs)
    dev = next(model.parameters()).device
    device_side = hasattr(dataset, 'device_batch')       # images produced on the device (datasets.DevicePhiloxPool): no host collate / H2D
    my_idx = [i for b in my_batches for i in b]
    all_ids = torch.tensor(my_idx, dtype=torch.int64).to(dev)             # GLOBAL image ids: they key the Philox streams of the HUA sampler
    workers = int(os.environ.get('AOD_POOL_WORKERS', getattr(data_loader, 'num_workers', 0) or 0))
    batches = ((idxs, None) for idxs in my_batches) if device_side else _shard_batches(dataset, my_batches, collate, workers)
    timed = world > 1 and dev.type == 'cuda' and torch.distributed.is_available() and torch.distributed.is_initialized()
    if timed:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    pos = 0
    for idxs, data in batches:
        s = idxs[0]
        image_ids = all_ids[pos:pos + len(idxs)]
        pos += len(idxs)
        if device_side:
            out = gscore.static_image((len(idxs), 3) + tuple(dataset.size)) if gscore is not None and hasattr(dataset, 'size') else None
            data = dataset.device_batch(idxs, dev, image_ids=image_ids, out=out)
        else:
            data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
            if dev.type == 'cuda':
                data['img'] = _pin(data['img'])
        out = None
        if gscore is not None and isinstance(data['img'], (list, tuple)) and len(data['img']) == 1:
            out = gscore.maybe(data['img'][0], data['img_metas'][0], image_ids, defer=True)       # (scores are read after gscore.sync() below)
        if out is not None:
            result, unc = out
        else:
            with torch.no_grad():
                result, unc, *others = model(return_loss=False, rescale=True, isEval=False, batchIdx=s // bs, image_ids=image_ids, **data, **kwargs)
        chunks.append(torch.as_tensor(unc, dtype=torch.float32, device=dev).reshape(-1))
        if kwargs.get('saveMaxConf'):          # test.py:130,134
            conf_chunks.append(torch.as_tensor(others[0], dtype=torch.float32, device=dev).reshape(-1))
        prog_bar.update(len(idxs))
    dev = next(model.parameters()).device
    if gscore is not None:
        gscore.sync()                       # deferred selection halves (second stream) -> this stream
    local = torch.cat(chunks) if chunks else torch.zeros(0, device=dev)
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
    per = -(-(-(-N // bs)) // world) * bs       # slots per rank of the interleaved partition: ceil(ceil(N / bs) / world) batches of bs
    gather = (lambda v: gather_scores_indexed(v, my_idx, N, per=per)) if interleaved else (lambda v: gather_scores(v, N))
    if kwargs.get('saveMaxConf'):
        conf = torch.cat(conf_chunks) if conf_chunks else torch.zeros(0, device=dev)
        return gather(local), gather(conf)
    return gather(local)


@torch.no_grad()
def single_gpu_ensemble(models, data_loader, n_cls=None, **kwargs):
    """Ensemble_MI (mmdet/apis/CalEnsembleUnc.py:137-162) for 2 <= K <= 32 built models, on single_gpu_uncertainty's loop: the pool is sharded
    over the ranks, batches come from the prefetch workers through pinned memory, the scores stay on the device and are gathered once.
    Returns a [N] fp32 tensor identical on every rank.

    Per batch: K forwards (isEval=True, justOut=True: classification maps only), then ONE aod_ensemble_mi launch pair on the same stream
    (scoring.ensemble_mi).  While the batch shape repeats (and AOD_HIP_GRAPH != 0) each member replays its own captured forward and hands
    back its graph's static maps; the MI kernel runs eagerly behind the K replays on the caller's stream, so it has read them before the
    next batch's replays overwrite them.  n_cls: classes per anchor row, default the head's cls_out_channels."""
    import os
    from ..scoring import ensemble_mi
    models = list(models)
    if not 2 <= len(models) <= 32:
        raise ValueError(f'single_gpu_ensemble: 2..32 ensemble members are supported, got {len(models)}')
    for m in models:
        m.eval()
    dataset = data_loader.dataset
    N = len(dataset)
    rank, world = get_dist_info()
    bs = data_loader.batch_size or 1
    my_batches = shard_batches(N, bs, rank, world, False)
    dev = next(models[0].parameters()).device
    if n_cls is None:
        n_cls = getattr(models[0], 'module', models[0]).bbox_head.cls_out_channels
    gscores = None
    if (os.environ.get('AOD_HIP_GRAPH', '1') != '0' and dev.type == 'cuda'
            and all(isinstance(v, (bool, int, float, str, type(None))) for v in kwargs.values())):
        from ..graphs import GraphedScore
        gscores = []
        for k, m in enumerate(models):
            # one graph per MEMBER: a model listed twice gets two (each owns the static maps it hands back)
            key = ('just_out', sum(1 for o in models[:k] if o is m)) + tuple(sorted((n, type(v).__name__, v) for n, v in kwargs.items()))
            cache = _GSCORE.setdefault(m, {})
            g = cache.get(key)
            if g is None:
                g = cache[key] = GraphedScore(m, rescale=True, isEval=True, justOut=True, **kwargs)
            gscores.append(g)
    device_side = hasattr(dataset, 'device_batch')
    my_idx = [i for b in my_batches for i in b]
    all_ids = torch.tensor(my_idx, dtype=torch.int64).to(dev)
    workers = int(os.environ.get('AOD_POOL_WORKERS', getattr(data_loader, 'num_workers', 0) or 0))
    batches = ((idxs, None) for idxs in my_batches) if device_side else _shard_batches(dataset, my_batches, data_loader.collate_fn, workers)
    prog_bar = ProgressBar(len(my_idx))
    chunks = []
    pos = 0
    for idxs, data in batches:
        image_ids = all_ids[pos:pos + len(idxs)]
        pos += len(idxs)
        if device_side:
            data = dataset.device_batch(idxs, dev, image_ids=image_ids)
        else:
            data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
            if dev.type == 'cuda':
                data['img'] = _pin(data['img'])
        single = isinstance(data['img'], (list, tuple)) and len(data['img']) == 1
        if single and dev.type == 'cuda':
            # the batch goes to the device ONCE (one H2D copy / one transform launch); every member reads that tensor
            img = data['img'][0]
            img = img.to_device(dev) if isinstance(img, DeviceImageBatch) else img.to(dev, non_blocking=True)
            data['img'] = [img]
        members = []
        for k, m in enumerate(models):
            out = None
            if gscores is not None and single:
                out = gscores[k].maybe(data['img'][0], data['img_metas'][0], image_ids)
            if out is None:
                out = m(return_loss=False, rescale=True, isEval=True, justOut=True, **data, **kwargs)
            members.append(out)
        chunks.append(ensemble_mi(members, n_cls))
        prog_bar.update(len(idxs))
    local = torch.cat(chunks) if chunks else torch.zeros(0, device=dev)
    return gather_scores(local, N)


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
    """MCDropout_MI (mmdet/apis/CalMCDropoutUnc.py:137-163) on single_gpu_ensemble's loop: the pool is sharded over the ranks, batches come from
    the prefetch workers through pinned memory (one H2D copy per batch), the scores stay on the device and are gathered once.  Returns a [N]
    fp32 tensor identical on every rank.

    Per batch and per sample k = 0..n-1: one aod_dropout2d_masks launch writes the Dropout2d factors of every site into the static table
    (keyed by seed, k and the GLOBAL image ids), one forward with a Dropout2d(rate) behind every ReLU that feeds the classification maps
    (functional.mc_dropout: eval mode, isEval=True, justOut=True), one device copy of the maps into slot k of a preallocated stack; then ONE
    scoring.ensemble_mi call over the n slots.  While the batch shape repeats (and AOD_HIP_GRAPH != 0) the n forwards are n replays of ONE
    captured forward, which reads the table the mask kernel has just rewritten.  An image's score is a function of (weights, image, seed,
    image id, n, rate) only: the same bits alone, in any batch, on any rank count, eager or replayed."""
    import os
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
    dataset = data_loader.dataset
    N = len(dataset)
    rank, world = get_dist_info()
    bs = data_loader.batch_size or 1
    my_batches = shard_batches(N, bs, rank, world, False)
    dev = next(model.parameters()).device
    if n_cls is None:
        n_cls = getattr(model, 'module', model).bbox_head.cls_out_channels
    # the static factor table [bs, T] and the captured forward that reads it: one pair per (model, batch size, options)
    primitives = all(isinstance(v, (bool, int, float, str, type(None))) for v in kwargs.values())
    key = (bs,) + (tuple(sorted((k, type(v).__name__, v) for k, v in kwargs.items())) if primitives else ())
    cache = _MCD_STATE.setdefault(model, {})
    ent = cache.get(key) if primitives else None
    if ent is None:
        ent = dict(table=torch.ones(bs, sites.T, dtype=torch.float32, device=dev), g=None)
        if primitives:
            cache[key] = ent
    table = ent['table']
    offsets = sites.offsets(dev)
    gscore = None
    if os.environ.get('AOD_HIP_GRAPH', '1') != '0' and dev.type == 'cuda' and primitives:
        if ent['g'] is None:
            from ..graphs import GraphedScore
            ent['g'] = GraphedScore(model, rescale=True, isEval=True, justOut=True, mc_dropout=AF.MCDropoutState(table, sites), **kwargs)
        gscore = ent['g']
    device_side = hasattr(dataset, 'device_batch')
    my_idx = [i for b in my_batches for i in b]
    all_ids = torch.tensor(my_idx, dtype=torch.int64).to(dev)
    workers = int(os.environ.get('AOD_POOL_WORKERS', getattr(data_loader, 'num_workers', 0) or 0))
    batches = ((idxs, None) for idxs in my_batches) if device_side else _shard_batches(dataset, my_batches, data_loader.collate_fn, workers)
    prog_bar = ProgressBar(len(my_idx))
    chunks = []
    pos = 0
    for idxs, data in batches:
        image_ids = all_ids[pos:pos + len(idxs)]
        pos += len(idxs)
        if device_side:
            data = dataset.device_batch(idxs, dev, image_ids=image_ids)
        else:
            data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
            if dev.type == 'cuda':
                data['img'] = _pin(data['img'])
        single = isinstance(data['img'], (list, tuple)) and len(data['img']) == 1
        if single and dev.type == 'cuda':
            # the batch goes to the device ONCE; the n forwards read that tensor
            img = data['img'][0]
            img = img.to_device(dev) if isinstance(img, DeviceImageBatch) else img.to(dev, non_blocking=True)
            data['img'] = [img]
        stack = None
        for k in range(n):
            ho.dropout2d_masks(table, image_ids, offsets, rate, seed, k)
            out = None
            if gscore is not None and single:
                out = gscore.maybe(data['img'][0], data['img_metas'][0], image_ids)
            if out is None:
                out = model(return_loss=False, rescale=True, isEval=True, justOut=True, mc_dropout=AF.MCDropoutState(table, sites), **data, **kwargs)
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
        prog_bar.update(len(idxs))
    local = torch.cat(chunks) if chunks else torch.zeros(0, device=dev)
    return gather_scores(local, N)


def MCDropout_uncertainty(cfg, model, data_loader, **kwargs):
    """mmdet/apis/CalMCDropoutUnc.py:86-88 with the reference's name and argument order.  kwargs: n (default 25 forwards), rate (0.1), seed,
    n_cls.  Returns the CPU score tensor update_X_L takes."""
    return single_gpu_mcdropout(model, data_loader, **kwargs).cpu()


@torch.no_grad()
def single_gpu_test(model, data_loader, show=False, out_dir=None, show_score_thr=0.3, **kwargs):
    """test.py:138-195 (detection results for evaluation; isEval=True).  detUnc=True: returns (results, unc_results) where
    unc_results[i][c] is a (k, 2) float32 array (aleatoric, epistemic), row-aligned with results[i][c]; the box arrays keep five columns
    (eval_map reads the score from column -1)."""
    model.eval()
    results, unc_results = [], []
    for data in data_loader:
        data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
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

    The loop is single_gpu_uncertainty's: the test set is sharded over the ranks (shard_batches), batches come from the prefetch workers
    through pinned memory, and while the batch shape repeats (and AOD_HIP_GRAPH != 0) the detection pass replays one captured graph
    (single stream: isEval has no two-phase form); the match kernel runs eagerly behind the replay on the same stream, so it has read the
    graph's static outputs before the next replay overwrites them.  `annotations`: the dataset's, when the caller already holds them.
    `_timing` (a dict; tools/eval_throughput.py): the loop is followed by a device sync and its wall time lands in _timing['pass_s']."""
    import os
    import time
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
    rank, world = get_dist_info()
    bs = data_loader.batch_size or 1
    my_batches = shard_batches(N, bs, rank, world, False)
    gscore = None
    if os.environ.get('AOD_HIP_GRAPH', '1') != '0' and dev.type == 'cuda' and all(isinstance(v, (bool, int, float, str, type(None))) for v in kwargs.values()):
        from ..graphs import GraphedScore
        cache = _GSCORE.setdefault(model, {})
        key = ('eval_padded',) + tuple(sorted((k, type(v).__name__, v) for k, v in kwargs.items()))
        gscore = cache.get(key)
        if gscore is None:
            gscore = cache[key] = GraphedScore(model, rescale=True, isEval=True, _padded=True, **kwargs)
    my_idx = [i for b in my_batches for i in b]
    all_ids = torch.tensor(my_idx, dtype=torch.int64).to(dev)
    workers = int(os.environ.get('AOD_POOL_WORKERS', getattr(data_loader, 'num_workers', 0) or 0))
    prog_bar = ProgressBar(len(my_idx))
    pos = 0
    for idxs, data in _shard_batches(ds, my_batches, data_loader.collate_fn, workers):
        image_ids = all_ids[pos:pos + len(idxs)]
        pos += len(idxs)
        data = {k: _unwrap(v) for k, v in data.items() if k in ('img', 'img_metas')}
        if dev.type == 'cuda':
            data['img'] = _pin(data['img'])
        out = None
        if gscore is not None and isinstance(data['img'], (list, tuple)) and len(data['img']) == 1:
            out = gscore.maybe(data['img'][0], data['img_metas'][0], image_ids)
        if out is None:
            out = model(return_loss=False, rescale=True, isEval=True, _padded=True, **data, **kwargs)
        dets, labels, num = out
        acc.update(idxs, dets, labels, num, [anns[i] for i in idxs])
        prog_bar.update(len(idxs))
    if _timing is not None:
        torch.cuda.synchronize()
        _timing['pass_s'] = time.perf_counter() - t_start
    acc.gather()
    res = acc.finalize(dataset)
    for mean_ap, eval_results in res:
        print_map_summary(mean_ap, eval_results, dataset, None, logger=logger)
    return res[0] if single else res
