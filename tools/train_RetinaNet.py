#!/usr/bin/env python
"""Active-learning driver with the reference's CLI and control flow (tools/train_RetinaNet.py:49-255):
seeds = 20, per cycle {build + init model, outer_epoch x train_detector_SSL phases, save, HUA-score the pool, select}.

    python tools/train_RetinaNet.py --work-dir demo --synthetic 64            # synthetic VOC-shaped pool (no dataset needed)
    python -m torch.distributed.run --nproc-per-node 8 tools/train_RetinaNet.py --launcher pytorch ...   # one rank per MI355X
"""
import argparse
import math
import os
import os.path as osp
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from aod_meh_hua_amd.apis import calculate_uncertainty, train_detector_SSL  # noqa: E402
from aod_meh_hua_amd.datasets import apply_device_transforms, build_dataloader, build_dataset  # noqa: E402
from aod_meh_hua_amd.mmcv_lite import Config, MMDataParallel, mkdir_or_exist  # noqa: E402
from aod_meh_hua_amd.models import build_detector  # noqa: E402
from aod_meh_hua_amd.utils import get_root_logger  # noqa: E402
from aod_meh_hua_amd.utils.active_datasets import create_X_L_file, get_X_L_0_prev, update_X_L  # noqa: E402
from aod_meh_hua_amd.utils.functions import DelJunkSave, EditCfg, ResumeCycle  # noqa: E402

# module-level knobs, as in the reference (:28-43)
onlyEval = False
load_cycle = -1
resume_cycle = -1
isSave = True
editCfg = {'uncertainty_pool2': 'objectSum_scaleMax_classSum'}
clsW = False
zeroRate = 0.15
saveMaxConf = False
useMaxConf = 'False'
score_thr = 0.3
iou_thr = 0.9
CLASS_DIFFICULTY = dict(xi=0.6, momentum=0.99, alpha=0.3, beta=0.2)      # PPAL's constants (--class-difficulty, --uncertainty-pool PPAL)


def parse_args(default_config='configs/_base_/Config_RetinaNet.py', default_size=512):
    base_dir = osp.dirname(osp.dirname(osp.abspath(__file__)))
    p = argparse.ArgumentParser(description='Train a detector (active learning, MEH + HUA)')
    p.add_argument('--config', default=osp.join(base_dir, default_config))
    p.add_argument('--work-dir', default='WORK_DIR')
    p.add_argument('--resume-from')
    p.add_argument('--load-from')
    p.add_argument('--bbox-head', help='head type written into cfg.model.bbox_head.type: Lambda_L2Net (default) or one of the ablation heads '
                                       'Lambda_L1Net | Lambda_MSLENet | Lambda_L2Net_ablation | Lambda_L2Net_NoL')
    p.add_argument('--uncertainty-pool', default=None,
                   help="pool scoring rule (default: the config's uncertainty_pool): Random | Entropy_NMS | Entropy_ALL | Entropy_Avg | Coreset "
                        '| CDAL (Entropy_Avg: Lambda_L2Net_NoL only; Coreset: k-center greedy on pooled pyramid descriptors, zeroRate off; '
                        'CDAL: k-center greedy on class-mixture descriptors under the symmetrised KL divergence, zeroRate off) '
                        '| Entropy | Margin | LeastConf (uncertainty sampling on the class posterior of every detection, aggregated per '
                        'image by --unc-aggregate; every head has them, the plain RetinaNet and SSD included) '
                        '| LocStability | LocStability_C (localization stability, Kao et al., ACCV 2018: how far the boxes of the clean '
                        'detections move under Gaussian pixel noise of the strengths --noise-levels; LocStability_C adds 1 - the largest '
                        'detection score; reads detections only, so every detector has them) '
                        '| Consistency (prediction consistency under mirroring, Elezi et al., CVPR 2022, and CALD, Yu et al., CVPRW 2022: '
                        'detect on the image and on the mirrored copies --consistency-views, map the boxes back and score the disagreement '
                        'in box position and class posterior, --consistency-mode, aggregated per image by --unc-aggregate; every detector '
                        'has it) '
                        '| CCMS (two-stage pick after PPAL, Yang et al., CVPR 2024: the --candidate-factor x budget most uncertain images by '
                        'the summed posterior entropy, then k-center greedy under the category-conditioned matching distance between '
                        'their objects; RetinaNet detectors, zeroRate off) '
                        '| PPAL (CCMS with its first stage ranked by the difficulty-calibrated entropy: every detection times the weight of its '
                        "class, from the class-difficulty EMA the head keeps while it trains; switches --class-difficulty on, zeroRate off) "
                        '| ENMS (entropy-NMS uncertainty, Wu et al., CVPR 2022: the posterior entropy summed over the objects that survive an '
                        'NMS by feature similarity, --enms-thr; ordinary scores; RetinaNet detectors) '
                        '| DivProto (ENMS + the progressive diversity pick of the same paper: sweep the images by ENMS score, pass over those '
                        'whose class prototypes repeat a pick, --intra-thr, and give the share --minority-beta of the budget to images that '
                        'bring one of the --minority-alpha least-held classes with a confidence above --inter-thr; RetinaNet detectors, '
                        'zeroRate off) '
                        '| BADGE (Ash et al., ICLR 2020: the gradient embedding of every image -- per object the cross-entropy gradient under '
                        'its own label times its neck feature, summed -- then k-means++ seeding on the unlabelled rows, --selection-seed; '
                        'RetinaNet detectors, zeroRate off) '
                        '| KMeansPP (the same k-means++ seeding on the Coreset descriptors: pure diversity that follows the density of the '
                        'pool; RetinaNet detectors, zeroRate off)')
    p.add_argument('--selection-seed', type=int, default=0,
                   help='BADGE / KMeansPP pools: seed of the k-means++ draws; cycle c draws with seed + c (default: 0)')
    p.add_argument('--enms-thr', type=float, default=0.5,
                   help='ENMS / DivProto pools: an object is dropped when its feature cosine to a picked object of its class exceeds this (default: 0.5)')
    p.add_argument('--intra-thr', type=float, default=0.7,
                   help='DivProto pool: an image is redundant when every one of its class prototypes has a cosine above this to a picked one (default: 0.7)')
    p.add_argument('--inter-thr', type=float, default=0.3,
                   help='DivProto pool: a class counts as present in an image when its largest detection score exceeds this (default: 0.3)')
    p.add_argument('--minority-alpha', type=float, default=0.5,
                   help='DivProto pool: the share of the classes, the least-held first, that count as minority classes, in (0, 1] (default: 0.5)')
    p.add_argument('--minority-beta', type=float, default=0.75,
                   help='DivProto pool: the share of the budget reserved for images that bring a minority class, in (0, 1] (default: 0.75)')
    p.add_argument('--no-class-balance', action='store_true', help='DivProto pool: switch the minority-class stage off (intra-class check only)')
    p.add_argument('--class-difficulty', action='store_true',
                   help="track PPAL's per-class difficulty EMA while training (config key model.bbox_head.class_difficulty = dict(xi=0.6, "
                        'momentum=0.99, alpha=0.3, beta=0.2)); the Entropy / Margin / LeastConf / CCMS pools then weight every detection by its '
                        "class (class_weighted).  RetinaNet heads; each rank's EMA follows its own batches, rank 0's is used for the pool pass")
    p.add_argument('--loss-bbox', choices=['L1', 'IoU', 'GIoU'], default=None,
                   help='box regression loss of the RetinaNet heads: L1 on the encoded deltas, or IoU / GIoU on the decoded boxes (config keys '
                        'model.bbox_head.loss_bbox and model.bbox_head.reg_decoded_bbox, set together); default: what the config says')
    p.add_argument('--loss-bbox-weight', type=float, default=None,
                   help='loss_weight of --loss-bbox (default: 1.0, or what the config says when --loss-bbox is not given)')
    p.add_argument('--candidate-factor', type=float, default=4.0,
                   help='CCMS pool: the candidate set holds ceil(factor x budget) of the most uncertain unlabelled images (default: 4)')
    p.add_argument('--max-objects', type=int, default=32,
                   help='CCMS / ENMS / DivProto / BADGE pools: objects described per image, the first K detections above --hua-score-thr (default: 32, '
                        'at most 64)')
    p.add_argument('--noise-levels', default='8,16,24,32,40,48',
                   help='noise strengths of the LocStability pools: up to 16 comma-separated standard deviations in 0..255 pixel units '
                        '(default: 8,16,24,32,40,48)')
    p.add_argument('--noise-seed', type=int, default=0, help='seed of the pixel noise of the LocStability pools (default: 0)')
    p.add_argument('--consistency-views', default='hflip',
                   help='views of the Consistency pool: 1..3 distinct comma-separated names of hflip, vflip, hvflip (default: hflip)')
    p.add_argument('--consistency-mode', default='both',
                   help='what the Consistency pool scores: box (1 - IoU of the matched boxes), cls (Jensen-Shannon divergence of their class '
                        'posteriors) or both (their mean; default)')
    p.add_argument('--unc-aggregate', choices=['max', 'mean', 'sum'], default='max',
                   help="how the Entropy / Margin / LeastConf / Consistency pools aggregate an image's per-detection values (default: max)")
    p.add_argument('--hua-score-thr', type=float, default=score_thr,
                   help='score_thr handed to calculate_uncertainty; read by Lambda_L2Net_ablation / Lambda_L2Net_NoL, as the region '
                        'threshold by the CDAL pool, and as the object gate by the Entropy / Margin / LeastConf pools')
    p.add_argument('--hua-iou-thr', type=float, default=iou_thr,
                   help='iou_thr handed to calculate_uncertainty; read by Lambda_L2Net_ablation / Lambda_L2Net_NoL only')
    p.add_argument('--uncertainty', help='uncertainty type (accepted like the reference accepts it, tools/train_RetinaNet.py:56: never read there either)')
    p.add_argument('--no-validate', default=False, help='whether not to evaluate during training')
    group_gpus = p.add_mutually_exclusive_group()
    group_gpus.add_argument('--gpus', type=int, default=None, help='number of gpus to use (only applicable to non-distributed training)')
    group_gpus.add_argument('--gpu-ids', type=int, default=None, nargs='+', help='ids of gpus to use (only applicable to non-distributed training)')
    p.add_argument('--deterministic', action='store_true',
                   help='the reference sets cuDNN to deterministic here; the HIP kernels reduce in a fixed order already (slab-ordered weight '
                        'gradients, ordered split-K) except the fp32-atomic column sums of bias / BN-shift gradients -- the flag switches those '
                        'to ordered partial sums as well (aod_set_deterministic: two runs from the same state are then bit-identical; ~1 %% slower)')
    p.add_argument('--launcher', choices=['none', 'pytorch', 'slurm', 'mpi'], default='none', help='job launcher')
    p.add_argument('--local_rank', type=int, default=0)
    p.add_argument('--Unc-type', type=str)
    p.add_argument('--precision', choices=['bf16x3', 'bf16'], default=None,
                   help='arithmetic of the conv stack (default: AOD_CONV_PREC or bf16x3): bf16x3 = reference precision, bf16 = fast mode')
    p.add_argument('--synthetic', type=int, default=0, help='run on a synthetic VOC-shaped pool of this many images')
    p.add_argument('--synthetic-size', type=int, default=default_size)
    p.add_argument('--cycles', type=int, default=None, help='override the number of AL cycles')
    p.add_argument('--samples-per-gpu', type=int, default=None)
    p.add_argument('--log-interval', type=int, default=None, help='iterations between two lines of the text log (config key log_config.interval)')
    p.add_argument('--hua-estimator', choices=['mc', 'closed'], default=None,
                   help='HUA estimator of the pool scoring pass: Monte-Carlo (default) or the closed form of its limit (config key model.test_cfg.hua_estimator)')
    p.add_argument('--device-transforms', action='store_true',
                   help='run Resize / RandomFlip / Normalize / Pad of the VOC pipelines as one HIP kernel per batch (config key data.device_transforms)')
    p.add_argument('--device-metric', action='store_true',
                   help='EvalHook computes mAP on the device: padded detections -> aod_eval_match -> one D2H copy, the test set sharded over '
                        'the ranks (config key evaluation.device_metric); same numbers as the host metric.  With metric=\'bbox\' (COCO '
                        'configs): padded detections -> aod_coco_match, the dict of CocoDataset.evaluate')
    args = p.parse_args()
    try:            # (at start-up: a malformed value must not surface after a whole training cycle)
        args.noise_sigmas = tuple(float(s) for s in args.noise_levels.split(',') if s.strip())
    except ValueError:
        p.error(f'--noise-levels: {args.noise_levels!r} is not a comma-separated list of numbers')
    from aod_meh_hua_amd.scoring import LOCSTAB_MAX_LEVELS
    if not 1 <= len(args.noise_sigmas) <= LOCSTAB_MAX_LEVELS or not all(0.0 <= s < float('inf') for s in args.noise_sigmas):
        p.error(f'--noise-levels: 1..{LOCSTAB_MAX_LEVELS} finite values >= 0 are needed, got {args.noise_levels!r}')
    from aod_meh_hua_amd.scoring import CONSISTENCY_MODES, consistency_views
    args.consistency_view_names = tuple(s.strip() for s in args.consistency_views.split(',') if s.strip())
    try:
        consistency_views(args.consistency_view_names, '--consistency-views')
    except ValueError as e:
        p.error(str(e))
    for flag, v in (('--minority-alpha', args.minority_alpha), ('--minority-beta', args.minority_beta)):
        if not 0 < v <= 1:
            p.error(f'{flag}: a share in (0, 1] is needed, got {v}')
    for flag, v in (('--enms-thr', args.enms_thr), ('--intra-thr', args.intra_thr), ('--inter-thr', args.inter_thr)):
        if v != v:
            p.error(f'{flag} is NaN')
    if args.consistency_mode not in CONSISTENCY_MODES:
        p.error(f"--consistency-mode: {args.consistency_mode!r} is none of 'both', 'box', 'cls'")
    os.environ.setdefault('LOCAL_RANK', str(args.local_rank))
    return args


def init_dist(launcher, backend='nccl', **kwargs):
    """mmcv.runner.init_dist as the reference calls it (tools/train_RetinaNet.py:119-121): one process per GPU; 'nccl' is RCCL over xGMI on
    ROCm.  pytorch: the environment of torch.distributed.run; slurm: rank / size from SLURM_PROCID / SLURM_NTASKS, the first host of
    SLURM_NODELIST as the rendezvous address (mmcv: `scontrol show hostname`), local rank = rank modulo the visible devices; mpi: the
    OMPI_COMM_WORLD_* variables."""
    import subprocess
    import torch.distributed as dist
    if launcher == 'slurm':
        rank, world = int(os.environ['SLURM_PROCID']), int(os.environ['SLURM_NTASKS'])
        if 'MASTER_ADDR' not in os.environ:
            try:
                os.environ['MASTER_ADDR'] = subprocess.getoutput(f"scontrol show hostname {os.environ['SLURM_NODELIST']} | head -n1").strip() or '127.0.0.1'
            except KeyError:
                os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ.setdefault('MASTER_PORT', str(kwargs.pop('port', 29500)))
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank % max(torch.cuda.device_count(), 1)))
    elif launcher == 'mpi':
        os.environ.update(RANK=os.environ['OMPI_COMM_WORLD_RANK'], WORLD_SIZE=os.environ['OMPI_COMM_WORLD_SIZE'],
                          LOCAL_RANK=os.environ.get('OMPI_COMM_WORLD_LOCAL_RANK', '0'))
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', str(kwargs.pop('port', 29500)))
    elif launcher != 'pytorch':
        raise ValueError(f'Invalid launcher type: {launcher}')
    kwargs.pop('port', None)
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', 0)))
    dist.init_process_group(backend=backend, **kwargs)


def set_loss_bbox(cfg, loss_bbox, loss_weight=None):
    """--loss-bbox / --loss-bbox-weight: the box loss and the space it is taken in are one choice -- L1 reads the encoded deltas,
    IoU / GIoU the decoded boxes -- so model.bbox_head.loss_bbox and model.bbox_head.reg_decoded_bbox are written together."""
    head = cfg.model.bbox_head
    if loss_bbox:
        head.loss_bbox = dict(type=loss_bbox + 'Loss', loss_weight=1.0 if loss_weight is None else float(loss_weight))
        head.reg_decoded_bbox = loss_bbox != 'L1'
    elif loss_weight is not None:
        head.loss_bbox.loss_weight = float(loss_weight)
    return cfg


def main(default_config='configs/_base_/Config_RetinaNet.py', default_size=512):
    args = parse_args(default_config, default_size)
    cfg = Config.fromfile(args.config)
    seed = 20
    torch.manual_seed(seed), np.random.seed(seed), random.seed(seed)
    cfg.seed, cfg.onlyEval = seed, onlyEval
    if args.bbox_head:
        cfg.model.bbox_head.type = args.bbox_head
    set_loss_bbox(cfg, args.loss_bbox, args.loss_bbox_weight)
    if args.uncertainty_pool == 'PPAL' or args.class_difficulty:
        cfg.model.bbox_head.class_difficulty = dict(CLASS_DIFFICULTY)
    str2unc = {'SACA': 'scaleAvg_classAvg', 'SSCS': 'scaleSum_classSum', 'SACS': 'scaleAvg_classSum', 'SSCA': 'scaleSum_classAvg'}
    if args.Unc_type:
        cfg.uncertainty_pool2 = str2unc[args.Unc_type]
    if args.uncertainty_pool:
        cfg.uncertainty_pool = args.uncertainty_pool
        cfg.model.test_cfg.uncertainty_pool = args.uncertainty_pool
    base_dir = osp.dirname(osp.dirname(osp.abspath(__file__)))
    cfg.work_dir = osp.join(base_dir, 'work_dirs', args.work_dir)
    mkdir_or_exist(cfg.work_dir)
    cfg.save_dir = osp.join(cfg.work_dir, 'model_save')
    mkdir_or_exist(cfg.save_dir)
    # train_RetinaNet.py:107-110: --gpu-ids wins, else range(--gpus) (default: one device)
    cfg.gpu_ids = args.gpu_ids if args.gpu_ids is not None else list(range(args.gpus or 1))
    if args.precision:
        from aod_meh_hua_amd import functional as AF
        AF.set_precision(args.precision)
    distributed = args.launcher != 'none'
    if distributed:
        init_dist(args.launcher, **cfg.dist_params)                          # (sets RANK / LOCAL_RANK / WORLD_SIZE for slurm and mpi)
    local = int(os.environ.get('LOCAL_RANK', 0))
    torch.cuda.set_device(local)
    if distributed:
        import torch.distributed as dist
        cfg.gpu_ids = list(range(dist.get_world_size()))
    rank = int(os.environ.get('RANK', 0))
    if editCfg:
        EditCfg(cfg, editCfg)
    cfg.model.backbone.pop('init_cfg', None) if args.synthetic else None
    if args.synthetic:            # the pool is N deterministic synthetic images
        n = args.synthetic
        ann = osp.join(cfg.work_dir, 'synthetic_all.txt')
        if rank == 0:
            np.savetxt(ann, np.array([f'synthetic_{i}' for i in range(n)]), fmt='%s')
        if distributed:
            torch.distributed.barrier()
        ds = dict(type='SyntheticVOCDataset', size=(args.synthetic_size, args.synthetic_size), ann_file=[ann])
        cfg.data.train = dict(type='RepeatDataset', times=cfg.X_L_repeat, dataset=dict(ds))
        cfg.data.test = dict(ds)
        cfg.data.val = dict(ds, ann_file=None, indices=list(range(min(n, 8))))        # (no VOC2007 test split offline: a few pool images)
        cfg.X_L_0_size, cfg.X_S_size = max(n // 8, 1), max(n // 16, 1)
    if args.cycles is not None:
        cfg.cycles = list(range(args.cycles))
    if args.samples_per_gpu:
        cfg.data.samples_per_gpu = args.samples_per_gpu
    if args.log_interval:
        cfg.log_config.interval = args.log_interval
    if args.device_transforms:
        cfg.data.device_transforms = True
    if args.hua_estimator:
        cfg.model.test_cfg.hua_estimator = args.hua_estimator
    if args.device_metric:
        cfg.evaluation.device_metric = True
    cfg.dump(osp.join(cfg.work_dir, osp.basename(args.config)))
    timestamp = time.strftime('%Y%m%d_%H%M%S', time.localtime())
    logger = get_root_logger(log_file=osp.join(cfg.work_dir, f'{timestamp}.log'), log_level=cfg.log_level)
    meta = dict(exp_name=osp.basename(args.config))
    if args.deterministic:
        from aod_meh_hua_amd import functional as _AF
        _AF.set_deterministic(True)
        logger.info('--deterministic: weight gradients and split-K sums are reduced in a fixed order by construction; bias / BN-shift column sums '
                    'now as ordered partial sums too (aod_set_deterministic)')
    # train_RetinaNet.py:139-141: 8 loader workers when started from a shell, else 0; here: 8 for real image data (AOD_WORKERS overrides), 0 for
    # the synthetic pool (its samples are generated in-process)
    cfg.data.workers_per_gpu = 0 if args.synthetic else int(os.environ.get('AOD_WORKERS', 8))

    X_L, X_U, X_all, all_anns = get_X_L_0_prev(cfg)
    if rank == 0:
        np.save(cfg.work_dir + '/X_L_0.npy', X_L), np.save(cfg.work_dir + '/X_U_0.npy', X_U)
    notResumed = True
    for cycle in cfg.cycles:
        if resume_cycle >= 0 and notResumed:
            X_L, X_U = ResumeCycle(cfg, cycle, resume_cycle)
            if not isinstance(X_L, np.ndarray):
                continue
            notResumed = False
        logger.info(f'Current cycle is {cycle} cycle.  len of X_U:{len(X_U)}, X_L:{len(X_L)}')
        cfg = create_X_L_file(cfg, X_L, all_anns, cycle)
        apply_device_transforms(cfg.data)
        model = build_detector(cfg.model)
        model.init_weights()
        if cfg.model.train_cfg.get('bias') == 'uniform':                     # :158-162
            head = model.bbox_head
            if hasattr(head, 'retina_cls'):
                N, k = head.num_anchors, head.retina_cls.bias.numel()
                torch.nn.init.uniform_(head.retina_cls.bias, -math.sqrt(1 / (N * k)), math.sqrt(1 / (N * k)))
            else:                                                             # tools/train_SSD.py:172-178
                for conv in head.cls_convs:
                    torch.nn.init.uniform_(conv[-1].bias, -math.sqrt(1 / 2000), math.sqrt(1 / 2000))
        if load_cycle >= 0:
            from aod_meh_hua_amd.mmcv_lite import load_checkpoint
            cfg_name = osp.splitext(osp.basename(args.config))[0]
            load_checkpoint(model, f'{cfg.save_dir}/{cfg_name}_Cycle{load_cycle}_Epoch{cfg.runner.max_epochs}_mycode.pth')
        datasets = [build_dataset(cfg.data.train)]
        model.CLASSES = datasets[0].CLASSES
        validate = not args.no_validate                                       # :60,193,210 (the reference evaluates unless told not to)
        for epoch in range(cfg.outer_epoch):
            cfg.lr_config.step = [1000]
            if epoch != cfg.outer_epoch - 1:                                  # :179-183
                cfg.evaluation.interval = 100
            cfg.optimizer['lr'] = 0.001
            if epoch == 0:
                logger.info(f'Epoch = {epoch}, First Label Set Training')
                cfg.total_epochs = cfg.epoch_ratio[0]
                train_detector_SSL(model, [build_dataset(cfg.data.train)], cfg, distributed=distributed, validate=validate, timestamp=timestamp, meta=meta)
            cfg.evaluation.interval = 100                                     # :198-201: evaluate only at the end of the last outer epoch
            if epoch == cfg.outer_epoch - 1:
                cfg.lr_config.step = [2]
                cfg.evaluation.interval = cfg.epoch_ratio[0]
            logger.info(f'Epoch = {epoch}, Fully-Supervised Learning')
            cfg.total_epochs = cfg.epoch_ratio[0]
            train_detector_SSL(model, [build_dataset(cfg.data.train)], cfg, distributed=distributed, validate=validate, timestamp=timestamp, meta=meta)
        if isSave and rank == 0:
            for f in os.listdir(cfg.save_dir):
                if '_mycode' not in f:
                    os.remove(osp.join(cfg.save_dir, f))
            cfg_name = osp.splitext(osp.basename(args.config))[0]
            torch.save(model.state_dict(), f'{cfg.save_dir}/{cfg_name}_Cycle{cycle}_Epoch{cfg.runner.max_epochs}_mycode.pth')
        if cycle != cfg.cycles[-1]:
            dataset_al = build_dataset(cfg.data.test)
            data_loader = build_dataloader(dataset_al, samples_per_gpu=cfg.data.samples_per_gpu, workers_per_gpu=cfg.data.workers_per_gpu,
                                           dist=False, shuffle=False)
            poolModel = MMDataParallel(model, device_ids=cfg.gpu_ids)
            # Coreset and CDAL take the labelled set (their initial centers) and select by rank, not by score: their vector marks exactly
            # X_S_size images, so the zero-score share of update_X_L is switched off for it; every other pool keeps its kwargs
            # CCMS (uncertainty pre-selection, then k-center greedy under the object-matching distance) is handled like them
            # PPAL is CCMS with the class-weighted first stage
            # DivProto (sweep by ENMS score, progressive prototype pick) likewise; ENMS alone is an ordinary score
            # BADGE and KMeansPP (k-means++ seeding on gradient embeddings / on the Coreset descriptors) likewise
            coreset = (cfg.uncertainty_pool in ('Coreset', 'CDAL') or cfg.uncertainty_pool == 'CCMS' or cfg.uncertainty_pool == 'PPAL'
                       or cfg.uncertainty_pool == 'DivProto' or cfg.uncertainty_pool in ('BADGE', 'KMeansPP'))
            pool_kw = dict(X_L=X_L) if coreset else {}
            if cfg.uncertainty_pool in ('BADGE', 'KMeansPP'):                 # k-means++ seeding: the draws must not repeat from cycle to cycle
                pool_kw.update(seed=args.selection_seed + cycle)
            if cfg.uncertainty_pool == 'BADGE':
                pool_kw.update(max_obj=args.max_objects)
            if cfg.uncertainty_pool in ('CCMS', 'PPAL'):
                pool_kw.update(candidate_factor=args.candidate_factor, max_obj=args.max_objects)
            if cfg.uncertainty_pool in ('ENMS', 'DivProto'):
                pool_kw.update(max_obj=args.max_objects, t_enms=args.enms_thr)
            if cfg.uncertainty_pool == 'DivProto':
                pool_kw.update(t_intra=args.intra_thr, t_inter=args.inter_thr, alpha=args.minority_alpha, beta=args.minority_beta,
                               class_balance=not args.no_class_balance)
            if cfg.uncertainty_pool in ('Entropy', 'Margin', 'LeastConf'):    # the posterior pools: ordinary scores, zeroRate stays on
                pool_kw = dict(unc_aggregate=args.unc_aggregate)
            if args.class_difficulty and cfg.uncertainty_pool in ('Entropy', 'Margin', 'LeastConf', 'CCMS'):
                pool_kw['class_weighted'] = True                              # (PPAL sets it itself)
            if cfg.uncertainty_pool in ('LocStability', 'LocStability_C'):    # localization stability: ordinary scores too
                pool_kw = dict(sigmas=args.noise_sigmas, seed=args.noise_seed)
            if cfg.uncertainty_pool == 'Consistency':                         # prediction consistency under mirroring: ordinary scores too
                pool_kw = dict(views=args.consistency_view_names, mode=args.consistency_mode, unc_aggregate=args.unc_aggregate)
            if coreset and zeroRate and cycle == cfg.cycles[0]:
                logger.info(f'uncertainty_pool={cfg.uncertainty_pool}: zeroRate {zeroRate} -> 0 (the picks are the selection)')
            with torch.no_grad():
                uncertainty = calculate_uncertainty(cfg, poolModel, data_loader, return_box=False, showNMS=False, saveUnc=False,
                                                    saveMaxConf=saveMaxConf, clsW=clsW, scaleUnc=False, score_thr=args.hua_score_thr,
                                                    iou_thr=args.hua_iou_thr, **pool_kw)
            maxconf = None
            if saveMaxConf and not coreset:                                   # :236-240
                uncertainty, maxconf = uncertainty
                maxconf = maxconf.cpu().numpy() if torch.is_tensor(maxconf) else np.asarray(maxconf)
            uncertainty = uncertainty.cpu().numpy() if torch.is_tensor(uncertainty) else np.asarray(uncertainty)
            X_L, X_U = update_X_L(uncertainty, X_all, X_L, cfg.X_S_size, zeroRate=0 if coreset else zeroRate, maxconf=maxconf,
                                  useMaxConf=useMaxConf)
            if rank == 0:
                np.save(cfg.work_dir + f'/X_L_{cycle + 1}.npy', X_L), np.save(cfg.work_dir + f'/X_U_{cycle + 1}.npy', X_U)
                np.save(cfg.work_dir + f'/Unc_{cycle + 1}.npy', uncertainty)
            logger.info(f'cycle {cycle}: scored {len(uncertainty)} images, {int((uncertainty > 0).sum())} non-zero, selected {cfg.X_S_size}')
        if rank == 0:
            DelJunkSave(cfg.work_dir)


if __name__ == '__main__':
    main()
