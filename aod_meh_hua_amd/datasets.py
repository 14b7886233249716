"""Data side of the boundary (SURVEY 8b "Data contract"): the synthetic VOC-shaped dataset the benchmarks and the AL-loop plumbing use
 and the real VOC path: XMLDataset / VOCDataset (datasets/xml_style.py:13-170, voc.py:11-94,
custom.py:56-363), ConcatDataset / RepeatDataset (dataset_wrappers.py), GroupSampler (samplers/group_sampler.py:9-50), mmcv collate
with padding, build_dataset / build_dataloader (builder.py:40-147).  Transforms live in pipelines.py."""
import os.path as osp
import xml.etree.ElementTree as ET

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .mmcv_lite import DataContainer, Registry, build_from_cfg
from .pipelines import DeferredImage

DATASETS = Registry('dataset')
VOC_CLASSES = ('aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog', 'horse',
               'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')


@DATASETS.register_module()
class SyntheticVOCDataset(Dataset):
    """Deterministic per-index samples: img ~ N(0,1) [3,H,W] (already 'normalised'), G ~ U{1..5} boxes with
    w,h ~ U(H/16, 3H/4) clipped inside, labels ~ U{0..19}.  `indices` (or ann_file of integer ids) selects a subset."""
    CLASSES = VOC_CLASSES

    def __init__(self, num_images=64, size=(512, 512), seed=20, indices=None, ann_file=None, test_mode=False, **kw):
        self.size, self.seed, self.test_mode = tuple(size), seed, test_mode
        if ann_file is not None:
            files = ann_file if isinstance(ann_file, (list, tuple)) else [ann_file]
            ids = np.concatenate([np.atleast_1d(np.loadtxt(f, dtype=str)) for f in files]) if len(files) else np.zeros(0, str)
            self.indices = np.array([int(str(i).split('_')[-1]) for i in ids], dtype=np.int64)
        else:
            self.indices = np.arange(num_images) if indices is None else np.asarray(indices)
        self.flag = np.zeros(len(self.indices), dtype=np.uint8)

    def __len__(self):
        return len(self.indices)

    def get_ann_info(self, i):
        """XMLDataset.get_ann_info format (xml_style.py:95-160): numpy boxes / labels (+ empty ignore sets)."""
        d = self[i]
        return dict(bboxes=d['gt_bboxes'].numpy().astype(np.float32), labels=d['gt_labels'].numpy().astype(np.int64),
                    bboxes_ignore=np.zeros((0, 4), np.float32), labels_ignore=np.zeros((0,), np.int64))

    def evaluate(self, results, metric='mAP', logger=None, proposal_nums=(100, 300, 1000), iou_thr=0.5, scale_ranges=None, **kwargs):
        """VOCDataset.evaluate (datasets/voc.py:37-94), VOC07 11-point mode; extra EvalHook kwargs (show, isUnc, out_dir) are ignored
        like the reference's signature swallows them."""
        from .core.evaluation import evaluate_voc
        return evaluate_voc(results, [self.get_ann_info(i) for i in range(len(self))], year=2007, classes=self.CLASSES, metric=metric,
                            logger=logger, iou_thr=iou_thr)

    def __getitem__(self, i):
        idx = int(self.indices[i])
        H, W = self.size
        g = torch.Generator().manual_seed(self.seed * 1000003 + idx)
        img = torch.randn(3, H, W, generator=g)
        G = int(torch.randint(1, 6, (1,), generator=g))
        wh = torch.rand(G, 2, generator=g) * torch.tensor([W * 0.6875, H * 0.6875]) + torch.tensor([W / 16., H / 16.])
        xy = torch.rand(G, 2, generator=g) * (torch.tensor([float(W), float(H)]) - wh)
        meta = dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), ori_shape=(H, W, 3), scale_factor=np.ones(4, np.float32), flip=False,
                    flip_direction=None, filename=f'synthetic_{idx}', ori_filename=f'synthetic_{idx}', image_id=idx)
        return dict(img=img, img_metas=meta, gt_bboxes=torch.cat([xy, xy + wh], 1), gt_labels=torch.randint(0, 20, (G,), generator=g))


@DATASETS.register_module()
class DevicePhiloxPool(Dataset):
    """Unlabeled pool whose images are generated ON the device ('pool of 10 000 synthetic 512^2 images generated on-device
    from Philox(seed=20, image_id)'): image i is a pure function of (seed, i), so any sharding over ranks / batches scores the same pool.
    `device_batch(idxs, device)` is the hook apis/test.py single_gpu_uncertainty uses instead of host collate + H2D copy; `__getitem__`
    gives the same image on the host for small cross-checks."""
    CLASSES = VOC_CLASSES

    def __init__(self, num_images=10000, size=(512, 512), seed=20, **kw):
        self.num_images, self.size, self.seed = int(num_images), tuple(size), int(seed)
        self.flag = np.zeros(self.num_images, dtype=np.uint8)
        self._buf = {}

    def __len__(self):
        return self.num_images

    def _meta(self, idx):
        H, W = self.size
        return dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), ori_shape=(H, W, 3), scale_factor=np.ones(4, np.float32), flip=False,
                    flip_direction=None, filename=f'philox_{idx}', ori_filename=f'philox_{idx}', image_id=idx)

    def device_batch(self, idxs, device, image_ids=None, out=None):
        """-> dict(img=[tensor [B,3,H,W] on device], img_metas=[list of dicts]).  The image tensor is `out` when given (the scoring graph's
        input buffer, graphs.GraphedScore.static_image: nothing is copied afterwards), else a per-batch-size static buffer; one kernel launch."""
        from . import _C
        H, W = self.size
        B = len(idxs)
        if out is not None and tuple(out.shape) == (B, 3, H, W) and out.dtype == torch.float32 and out.is_contiguous():
            img = out
        else:
            key = (B, str(device))
            if key not in self._buf:
                self._buf[key] = torch.empty(B, 3, H, W, device=device)
            img = self._buf[key]
        ids = image_ids if image_ids is not None else torch.tensor(list(idxs), dtype=torch.int64).to(device, non_blocking=True)
        _C.call('aod_synth_normal_images', _C.ptr(img), B, 3 * H * W, self.seed, _C.ptr(ids), _C.stream())
        return dict(img=[img], img_metas=[[self._meta(int(i)) for i in idxs]])

    def __getitem__(self, i):
        dev = torch.device('cuda', torch.cuda.current_device())
        d = self.device_batch([int(i)], dev)
        return dict(img=d['img'][0][0].cpu(), img_metas=d['img_metas'][0][0])


@DATASETS.register_module()
class RepeatDataset(Dataset):
    """mmdet/datasets/dataset_wrappers.py:128-170."""

    def __init__(self, dataset, times):
        self.dataset = build_dataset(dataset) if isinstance(dataset, dict) else dataset
        self.times, self.CLASSES = times, self.dataset.CLASSES
        self._ori_len = len(self.dataset)
        self.flag = np.tile(self.dataset.flag, times) if hasattr(self.dataset, 'flag') else None

    def __getitem__(self, idx):
        return self.dataset[idx % self._ori_len]

    def __len__(self):
        return self.times * self._ori_len


class CustomDataset(Dataset):
    """custom.py:56-363 (detection subset): annotation list -> filtered infos -> aspect-ratio group flag -> pipeline."""
    CLASSES = None

    def __init__(self, ann_file, pipeline, classes=None, data_root=None, img_prefix='', seg_prefix=None, proposal_file=None,
                 test_mode=False, filter_empty_gt=True, device_transforms=False):
        from .pipelines import Compose
        # device_transforms: Resize / RandomFlip / Normalize / Pad leave the pixels to one aod_image_xform launch per batch (pipelines.py)
        self.device_transforms = bool(device_transforms)
        self.ann_file, self.data_root, self.img_prefix = ann_file, data_root, img_prefix
        self.test_mode, self.filter_empty_gt, self.proposals = test_mode, filter_empty_gt, None
        self.CLASSES = self.get_classes(classes)
        if self.data_root is not None:
            if not osp.isabs(self.ann_file):
                self.ann_file = osp.join(self.data_root, self.ann_file)
            if not (self.img_prefix is None or osp.isabs(self.img_prefix)):
                self.img_prefix = osp.join(self.data_root, self.img_prefix)
        self.data_infos = self.load_annotations(self.ann_file)
        if not test_mode:
            valid_inds = self._filter_imgs()
            self.data_infos = [self.data_infos[i] for i in valid_inds]
            self._set_group_flag()
        else:
            self.flag = np.zeros(len(self.data_infos), dtype=np.uint8)
        self.pipeline = Compose(pipeline)

    def __len__(self):
        return len(self.data_infos)

    @classmethod
    def get_classes(cls, classes=None):
        if classes is None:
            return cls.CLASSES
        if isinstance(classes, str):
            return [ln.strip() for ln in open(classes) if ln.strip()]
        if isinstance(classes, (tuple, list)):
            return classes
        raise ValueError(f'Unsupported type {type(classes)} of classes.')

    def pre_pipeline(self, results):
        results['img_prefix'], results['seg_prefix'], results['proposal_file'] = self.img_prefix, None, None
        results['bbox_fields'], results['mask_fields'], results['seg_fields'] = [], [], []
        if self.device_transforms:
            results['device_transforms'] = True

    def _filter_imgs(self, min_size=32):
        return [i for i, info in enumerate(self.data_infos) if min(info['width'], info['height']) >= min_size]

    def _set_group_flag(self):
        self.flag = np.zeros(len(self), dtype=np.uint8)
        for i in range(len(self)):
            info = self.data_infos[i]
            if info['width'] / info['height'] > 1:
                self.flag[i] = 1

    def _rand_another(self, idx):
        return np.random.choice(np.where(self.flag == self.flag[idx])[0])

    def __getitem__(self, idx):
        if self.test_mode:
            return self.prepare_test_img(idx)
        while True:
            data = self.prepare_train_img(idx)
            if data is None:
                idx = self._rand_another(idx)
                continue
            return data

    def prepare_train_img(self, idx):
        results = dict(img_info=self.data_infos[idx], ann_info=self.get_ann_info(idx))
        self.pre_pipeline(results)
        return self.pipeline(results)

    def prepare_test_img(self, idx):
        results = dict(img_info=self.data_infos[idx])
        self.pre_pipeline(results)
        return self.pipeline(results)


@DATASETS.register_module()
class XMLDataset(CustomDataset):
    """xml_style.py:13-170: PASCAL-VOC style `ImageSets/Main/*.txt` id list + one `Annotations/<id>.xml` per image."""

    def __init__(self, min_size=None, **kwargs):
        assert self.CLASSES or kwargs.get('classes', None), 'CLASSES in `XMLDataset` can not be None.'
        self.min_size = min_size
        super().__init__(**kwargs)
        self.cat2label = {cat: i for i, cat in enumerate(self.CLASSES)}

    def _xml(self, img_id):
        return ET.parse(osp.join(self.img_prefix, 'Annotations', f'{img_id}.xml')).getroot()

    def load_annotations(self, ann_file):
        data_infos = []
        for img_id in [ln.strip() for ln in open(ann_file) if ln.strip()]:
            size = self._xml(img_id).find('size')
            if size is not None:
                width, height = int(size.find('width').text), int(size.find('height').text)
            else:
                from PIL import Image
                with Image.open(osp.join(self.img_prefix, 'JPEGImages', f'{img_id}.jpg')) as im:
                    width, height = im.size
            data_infos.append(dict(id=img_id, filename=f'JPEGImages/{img_id}.jpg', width=width, height=height))
        return data_infos

    def _filter_imgs(self, min_size=32):
        valid = []
        for i, info in enumerate(self.data_infos):
            if min(info['width'], info['height']) < min_size:
                continue
            if self.filter_empty_gt:
                if any(obj.find('name').text in self.CLASSES for obj in self._xml(info['id']).findall('object')):
                    valid.append(i)
            else:
                valid.append(i)
        return valid

    def get_ann_info(self, idx):
        """:95-160: 1-based VOC coordinates -> 0-based (bbox - 1); `difficult` objects and (min_size) tiny ones go to the ignore set."""
        cat2label = {cat: i for i, cat in enumerate(self.CLASSES)}
        bboxes, labels, bboxes_ignore, labels_ignore = [], [], [], []
        for obj in self._xml(self.data_infos[idx]['id']).findall('object'):
            name = obj.find('name').text
            if name not in self.CLASSES:
                continue
            label = cat2label[name]
            difficult = obj.find('difficult')
            difficult = 0 if difficult is None else int(difficult.text)
            bb = obj.find('bndbox')
            bbox = [int(float(bb.find(k).text)) for k in ('xmin', 'ymin', 'xmax', 'ymax')]
            ignore = False
            if self.min_size:
                assert not self.test_mode
                if bbox[2] - bbox[0] < self.min_size or bbox[3] - bbox[1] < self.min_size:
                    ignore = True
            if difficult or ignore:
                bboxes_ignore.append(bbox), labels_ignore.append(label)
            else:
                bboxes.append(bbox), labels.append(label)
        bboxes = np.array(bboxes, ndmin=2) - 1 if bboxes else np.zeros((0, 4))
        labels = np.array(labels) if labels else np.zeros((0,))
        bboxes_ignore = np.array(bboxes_ignore, ndmin=2) - 1 if bboxes_ignore else np.zeros((0, 4))
        labels_ignore = np.array(labels_ignore) if labels_ignore else np.zeros((0,))
        return dict(bboxes=bboxes.astype(np.float32), labels=labels.astype(np.int64), bboxes_ignore=bboxes_ignore.astype(np.float32),
                    labels_ignore=labels_ignore.astype(np.int64))

    def get_cat_ids(self, idx):
        cat2label = {cat: i for i, cat in enumerate(self.CLASSES)}
        return [cat2label[o.find('name').text] for o in self._xml(self.data_infos[idx]['id']).findall('object')
                if o.find('name').text in self.CLASSES]


@DATASETS.register_module()
class VOCDataset(XMLDataset):
    """voc.py:11-94."""
    CLASSES = VOC_CLASSES

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if 'VOC2007' in self.img_prefix:
            self.year = 2007
        elif 'VOC2012' in self.img_prefix:
            self.year = 2012
        else:
            raise ValueError('Cannot infer dataset year from img_prefix')

    def evaluate(self, results, metric='mAP', logger=None, proposal_nums=(100, 300, 1000), iou_thr=0.5, scale_ranges=None, **kwargs):
        from .core.evaluation import evaluate_voc
        return evaluate_voc(results, [self.get_ann_info(i) for i in range(len(self))], year=self.year, classes=self.CLASSES, metric=metric,
                            logger=logger, iou_thr=iou_thr)


COCO_CLASSES = ('person', 'bicycle', 'car', 'motorcycle', 'airplane', 'bus', 'train', 'truck', 'boat', 'traffic light', 'fire hydrant',
                'stop sign', 'parking meter', 'bench', 'bird', 'cat', 'dog', 'horse', 'sheep', 'cow', 'elephant', 'bear', 'zebra', 'giraffe',
                'backpack', 'umbrella', 'handbag', 'tie', 'suitcase', 'frisbee', 'skis', 'snowboard', 'sports ball', 'kite', 'baseball bat',
                'baseball glove', 'skateboard', 'surfboard', 'tennis racket', 'bottle', 'wine glass', 'cup', 'fork', 'knife', 'spoon', 'bowl',
                'banana', 'apple', 'sandwich', 'orange', 'broccoli', 'carrot', 'hot dog', 'pizza', 'donut', 'cake', 'chair', 'couch',
                'potted plant', 'bed', 'dining table', 'toilet', 'tv', 'laptop', 'mouse', 'remote', 'keyboard', 'cell phone', 'microwave',
                'oven', 'toaster', 'sink', 'refrigerator', 'book', 'clock', 'vase', 'scissors', 'teddy bear', 'hair drier', 'toothbrush')
_COCO_JSON = {}           # absolute path -> parsed annotation file (per process: the splits of one pool share it)


def load_coco_json(path):
    """A COCO annotation file parsed once per path and process: dict(images = the image records in file order, by_id = image id -> record,
    anns = image id -> its annotations in file order, categories)."""
    import json
    key = osp.abspath(path)
    parsed = _COCO_JSON.get(key)
    if parsed is None:
        with open(key) as f:
            raw = json.load(f)
        images = list(raw.get('images', []))
        anns = {im['id']: [] for im in images}
        for ann in raw.get('annotations', []):
            anns.setdefault(ann['image_id'], []).append(ann)
        parsed = _COCO_JSON[key] = dict(images=images, by_id={im['id']: im for im in images}, anns=anns,
                                        categories=list(raw.get('categories', [])))
    return parsed


@DATASETS.register_module()
class CocoDataset(CustomDataset):
    """COCO detection annotations read with plain json (mmdet/datasets/coco.py's behaviour, restated; no pycocotools).  `ann_file` is the
    annotation json itself (all of its images) or, with `coco_json=` naming the json, a text list of image ids, one per line: the form
    the active-learning bookkeeping reads and rewrites (utils/active_datasets.py).  Category ids need not be contiguous: cat_ids lists the
    ids of the categories named in CLASSES, in CLASSES order, and cat2label enumerates them."""
    CLASSES = COCO_CLASSES

    def __init__(self, coco_json=None, **kwargs):
        self.coco_json = coco_json
        super().__init__(**kwargs)

    def load_annotations(self, ann_file):
        path = ann_file if str(ann_file).endswith('.json') else self.coco_json
        if path is None:
            raise ValueError(f'CocoDataset: ann_file {ann_file!r} is an image-id list; coco_json= must name the annotation file')
        if self.data_root is not None and not osp.isabs(path):
            path = osp.join(self.data_root, path)
        self.coco = load_coco_json(path)
        by_name = {c['name']: c['id'] for c in self.coco['categories']}
        self.cat_ids = [by_name[n] for n in self.CLASSES if n in by_name]
        self.cat2label = {cid: i for i, cid in enumerate(self.cat_ids)}
        if str(ann_file).endswith('.json'):
            records = self.coco['images']
        else:
            by_str = {str(k): v for k, v in self.coco['by_id'].items()}
            records = []
            for img_id in [ln.strip() for ln in open(ann_file) if ln.strip()]:
                if img_id not in by_str:
                    raise KeyError(f'CocoDataset: image id {img_id} of {ann_file} is not in {path}')
                records.append(by_str[img_id])
        self.img_ids = [im['id'] for im in records]
        return [dict(id=im['id'], filename=im['file_name'], width=im['width'], height=im['height']) for im in records]

    def _anns(self, idx):
        return self.coco['anns'].get(self.data_infos[idx]['id'], [])

    def _filter_imgs(self, min_size=32):
        valid = []
        for i, info in enumerate(self.data_infos):
            if min(info['width'], info['height']) < min_size:
                continue
            if self.filter_empty_gt and not any(a['category_id'] in self.cat2label for a in self._anns(i)):
                continue
            valid.append(i)
        self.img_ids = [self.img_ids[i] for i in valid]
        return valid

    def get_cat_ids(self, idx):
        return [a['category_id'] for a in self._anns(idx)]

    def get_ann_info(self, idx):
        """The training view: an annotation is dropped when it is marked `ignore`, lies outside the image, has area <= 0 or a side below
        one pixel, or belongs to no kept category; xywh -> [x, y, x + w, y + h]; `iscrowd` boxes go to the ignore set."""
        info = self.data_infos[idx]
        bboxes, labels, bboxes_ignore, labels_ignore = [], [], [], []
        for ann in self._anns(idx):
            if ann.get('ignore', False):
                continue
            x1, y1, w, h = ann['bbox']
            inter_w = max(0, min(x1 + w, info['width']) - max(x1, 0))
            inter_h = max(0, min(y1 + h, info['height']) - max(y1, 0))
            if inter_w * inter_h == 0:
                continue
            if ann['area'] <= 0 or w < 1 or h < 1:
                continue
            if ann['category_id'] not in self.cat2label:
                continue
            bbox = [x1, y1, x1 + w, y1 + h]
            if ann.get('iscrowd', False):
                bboxes_ignore.append(bbox), labels_ignore.append(self.cat2label[ann['category_id']])
            else:
                bboxes.append(bbox), labels.append(self.cat2label[ann['category_id']])
        return dict(bboxes=np.array(bboxes, dtype=np.float32).reshape(-1, 4), labels=np.array(labels, dtype=np.int64),
                    bboxes_ignore=np.array(bboxes_ignore, dtype=np.float32).reshape(-1, 4), labels_ignore=np.array(labels_ignore, dtype=np.int64))

    def get_eval_info(self, idx):
        """The evaluation view, untouched by the training filters: every annotation of a kept category in file order --
        boxes [G, 4] float64 xywh as written, area [G] float64 (the file's), iscrowd [G] uint8, labels [G] int64."""
        anns = [a for a in self._anns(idx) if a['category_id'] in self.cat2label]
        return dict(boxes=np.array([a['bbox'] for a in anns], dtype=np.float64).reshape(-1, 4),
                    area=np.array([a['area'] for a in anns], dtype=np.float64),
                    iscrowd=np.array([1 if a.get('iscrowd', 0) else 0 for a in anns], dtype=np.uint8),
                    labels=np.array([self.cat2label[a['category_id']] for a in anns], dtype=np.int64))

    def eval_infos(self):
        """[get_eval_info(i)] built once per dataset object"""
        infos = getattr(self, '_eval_infos', None)
        if infos is None or len(infos) != len(self):
            infos = self._eval_infos = [self.get_eval_info(i) for i in range(len(self))]
        return infos

    def evaluate(self, results, metric='bbox', logger=None, proposal_nums=(100, 300, 1000), iou_thrs=None, classwise=False,
                 metric_items=None, **kwargs):
        """COCO bbox AP (core/coco_eval.py) with mmdet's keys: bbox_mAP, _50, _75, _s, _m, _l and bbox_mAP_copypaste.  The arrays
        go straight to the evaluator; extra EvalHook kwargs (show, isUnc, out_dir) are ignored like the reference's signature swallows them."""
        from .core.coco_eval import check_metric, evaluate_bbox
        check_metric(metric)
        return evaluate_bbox(results, self.eval_infos(), self.CLASSES, iou_thrs=iou_thrs, proposal_nums=proposal_nums, classwise=classwise,
                             metric_items=metric_items, logger=logger)


class ConcatDataset(torch.utils.data.ConcatDataset):
    """dataset_wrappers.py:12-125 (VOC07+12 trainval): concatenated flags; evaluation is per-dataset in the reference and unused here."""

    def __init__(self, datasets, separate_eval=True):
        super().__init__(datasets)
        self.CLASSES = datasets[0].CLASSES
        self.flag = np.concatenate([d.flag for d in datasets]) if hasattr(datasets[0], 'flag') else None

    def get_ann_info(self, idx):
        import bisect
        d = bisect.bisect_right(self.cumulative_sizes, idx)
        return self.datasets[d].get_ann_info(idx if d == 0 else idx - self.cumulative_sizes[d - 1])


def build_dataset(cfg, default_args=None):
    """builder.py:40-73: list of cfgs or list-valued ann_file -> ConcatDataset; RepeatDataset wrapper; registry otherwise.
    A `device_transforms` key on a RepeatDataset config reaches the dataset it wraps; SyntheticVOCDataset (already normalised tensors)
    ignores it."""
    if isinstance(cfg, (list, tuple)):
        return ConcatDataset([build_dataset(c, default_args) for c in cfg])
    if cfg['type'] == 'RepeatDataset':
        inner = dict(cfg['dataset'])
        if 'device_transforms' in cfg:
            inner['device_transforms'] = cfg['device_transforms']
        return RepeatDataset(build_dataset(inner, default_args), cfg['times'])
    if cfg['type'] != 'SyntheticVOCDataset' and isinstance(cfg.get('ann_file'), (list, tuple)):
        ann_files, prefixes = cfg['ann_file'], cfg.get('img_prefix')
        parts = []
        for i, af in enumerate(ann_files):
            c = dict(cfg)
            c['ann_file'] = af
            if isinstance(prefixes, (list, tuple)):
                c['img_prefix'] = prefixes[i]
            parts.append(build_dataset(c, default_args))
        return ConcatDataset(parts)
    return build_from_cfg(cfg, DATASETS, default_args)


def apply_device_transforms(data_cfg):
    """`data.device_transforms = True` in a config -> the switch in the train / val / test dataset configs (and every entry of a list of
    them).  Idempotent; returns the switch."""
    on = bool(data_cfg.get('device_transforms', False))
    if on:
        for key in ('train', 'val', 'test'):
            sub = data_cfg.get(key)
            for c in (sub if isinstance(sub, (list, tuple)) else [sub]):
                if isinstance(c, dict):
                    c['device_transforms'] = True
    return on


class GroupSampler(torch.utils.data.Sampler):
    """samplers/group_sampler.py:9-50: batches never mix the two aspect-ratio groups; each group is padded (by repetition) to a multiple
    of samples_per_gpu, shuffled inside the group, and the batches of both groups are shuffled together (np.random like the reference)."""

    def __init__(self, dataset, samples_per_gpu=1):
        assert hasattr(dataset, 'flag')
        self.dataset, self.samples_per_gpu = dataset, samples_per_gpu
        self.flag = dataset.flag.astype(np.int64)
        self.group_sizes = np.bincount(self.flag)
        self.num_samples = sum(int(np.ceil(s / samples_per_gpu)) * samples_per_gpu for s in self.group_sizes)

    def __iter__(self):
        indices = []
        for i, size in enumerate(self.group_sizes):
            if size == 0:
                continue
            indice = np.where(self.flag == i)[0]
            np.random.shuffle(indice)
            num_extra = int(np.ceil(size / self.samples_per_gpu)) * self.samples_per_gpu - len(indice)
            indice = np.concatenate([indice, np.random.choice(indice, num_extra)])
            indices.append(indice)
        indices = np.concatenate(indices)
        indices = [indices[i * self.samples_per_gpu:(i + 1) * self.samples_per_gpu]
                   for i in np.random.permutation(range(len(indices) // self.samples_per_gpu))]
        return iter(np.concatenate(indices).astype(np.int64).tolist())

    def __len__(self):
        return self.num_samples


class DistributedGroupSampler(torch.utils.data.Sampler):
    """mmdet/datasets/samplers/group_sampler.py:53-148: per epoch (seed + epoch) every aspect-ratio group is shuffled and padded to a
    multiple of samples_per_gpu * world, whole batches are shuffled, and rank r takes the r-th contiguous share -- so a batch never mixes
    portrait and landscape images and every rank draws a different, epoch-dependent share.  `set_epoch` is called by the runner at the
    start of every training epoch (mmcv's DistSamplerSeedHook)."""

    def __init__(self, dataset, samples_per_gpu=1, num_replicas=None, rank=None, seed=0):
        import math
        import torch.distributed as tdist
        if num_replicas is None or rank is None:
            ok = tdist.is_available() and tdist.is_initialized()
            num_replicas = tdist.get_world_size() if ok else 1
            rank = tdist.get_rank() if ok else 0
        self.dataset, self.samples_per_gpu, self.num_replicas, self.rank, self.seed, self.epoch = dataset, samples_per_gpu, num_replicas, rank, seed or 0, 0
        self.flag = np.asarray(dataset.flag).astype(np.int64)
        self.group_sizes = np.bincount(self.flag)
        self.num_samples = sum(int(math.ceil(sz * 1.0 / samples_per_gpu / num_replicas)) * samples_per_gpu for sz in self.group_sizes)
        self.total_size = self.num_samples * num_replicas

    def __iter__(self):
        import math
        g = torch.Generator()
        g.manual_seed(self.epoch + self.seed)
        indices = []
        for i, size in enumerate(self.group_sizes):
            if size > 0:
                indice = np.where(self.flag == i)[0]
                indice = indice[list(torch.randperm(int(size), generator=g).numpy())].tolist()
                extra = int(math.ceil(size * 1.0 / self.samples_per_gpu / self.num_replicas)) * self.samples_per_gpu * self.num_replicas - len(indice)
                tmp = indice.copy()
                for _ in range(extra // size):
                    indice.extend(tmp)
                indice.extend(tmp[:extra % size])
                indices.extend(indice)
        assert len(indices) == self.total_size
        indices = [indices[j] for i in list(torch.randperm(len(indices) // self.samples_per_gpu, generator=g))
                   for j in range(i * self.samples_per_gpu, (i + 1) * self.samples_per_gpu)]
        offset = self.num_samples * self.rank
        return iter(indices[offset:offset + self.num_samples])

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch


class DeviceImageBatch:
    """A collated batch of deferred images (pipelines.DeferredImage, device_transforms=True): ONE uint8 host buffer holding the B
    aod_image_xform_item_t records (first, 256-B aligned block) and the packed BGR HWC sources behind them, so that the batch travels in
    one H2D copy; `shape` = (B, 3, Hp, Wp) is the float32 batch eager collate would have produced.  Picklable (loader workers) and
    pinnable (DataLoader pin_memory).  `to_device` uploads it and runs one aod_image_xform launch on the current stream."""
    ITEM = np.dtype([('src_off', '<i8'), ('h', '<i4'), ('w', '<i4'), ('oh', '<i4'), ('ow', '<i4'), ('ph', '<i4'), ('pw', '<i4'),
                     ('sy', '<f4'), ('sx', '<f4'), ('flip', '<i4'), ('to_rgb', '<i4'), ('pad_val', '<f4'), ('mean', '<f4', (3,)),
                     ('std', '<f4', (3,)), ('reserved', '<i4')])
    assert ITEM.itemsize == 80
    dtype = torch.float32          # of the batch it becomes; with `shape`, what graph signatures and static-buffer allocation read

    def __init__(self, buf, shape, src_off):
        self.buf, self.shape, self.src_off = buf, tuple(shape), int(src_off)

    @classmethod
    def pack(cls, images):
        B = len(images)
        Hp, Wp = max(im.ph for im in images), max(im.pw for im in images)
        items = np.zeros(B, cls.ITEM)
        src_off = -(-B * cls.ITEM.itemsize // 256) * 256
        sizes = [im.src.nbytes for im in images]
        buf = np.empty(src_off + sum(sizes), np.uint8)
        off = 0
        for b, im in enumerate(images):
            h, w = im.src.shape[:2]
            buf[src_off + off:src_off + off + sizes[b]] = im.src.reshape(-1)
            items[b] = (off, h, w, im.oh, im.ow, im.ph, im.pw, np.float32(h / im.oh), np.float32(w / im.ow), im.flip, int(im.to_rgb),
                        im.pad_val, im.mean, im.std, 0)
            off += sizes[b]
        buf[:B * cls.ITEM.itemsize] = items.view(np.uint8)
        buf[B * cls.ITEM.itemsize:src_off] = 0
        return cls(torch.from_numpy(buf), (B, 3, Hp, Wp), src_off)

    def items(self):
        """the item records as a numpy structured array (host view)"""
        return self.buf[:self.shape[0] * self.ITEM.itemsize].numpy().view(self.ITEM)

    def sources(self):
        """the packed sources as a flat uint8 numpy array (host view)"""
        return self.buf[self.src_off:].numpy()

    def pin_memory(self):
        return self if self.buf.is_pinned() else DeviceImageBatch(self.buf.pin_memory(), self.shape, self.src_off)

    def __getstate__(self):
        return dict(buf=self.buf, shape=self.shape, src_off=self.src_off)

    def __setstate__(self, st):
        self.buf, self.shape, self.src_off = st['buf'], st['shape'], st['src_off']

    def to_device(self, device, out=None):
        """-> float32 [B, 3, Hp, Wp] on `device`: `out` when given (a graph's static image buffer: the kernel writes it directly), else a
        new tensor.  Fresh pinned staging for every call that was not handed a pinned buffer (see graphs.GraphedTrainStep._load)."""
        from . import hipops
        B, _, Hp, Wp = self.shape
        it = self.items()
        end = it['src_off'] + it['h'].astype(np.int64) * it['w'] * 3
        if len(it) != B or (it['h'] < 1).any() or (it['w'] < 1).any() or (it['src_off'] < 0).any() or int(end.max()) > self.buf.numel() - self.src_off:
            raise ValueError('DeviceImageBatch: an item points outside the packed sources')
        host = self.buf if self.buf.is_pinned() else self.buf.pin_memory()
        dev = torch.empty(host.numel(), dtype=torch.uint8, device=device)
        dev.copy_(host, non_blocking=True)
        if out is None:
            out = torch.empty(self.shape, dtype=torch.float32, device=device)
        return hipops.image_xform(dev[self.src_off:], dev[:self.src_off], B, Hp, Wp, out)


def _collate_dc(items, samples_per_gpu):
    """mmcv.parallel.collate for a list of DataContainers (one GPU per process: a single chunk)."""
    first = items[0]
    if first.cpu_only:
        return DataContainer([[d.data for d in items]], first.stack, cpu_only=True)
    if first.stack and isinstance(first.data, DeferredImage):
        # deferred images (device_transforms=True): padded to the batch maximum by the kernel itself
        return DataContainer([DeviceImageBatch.pack([d.data for d in items])], True)
    if first.stack:
        # pad the last `pad_dims` = 2 dims to the batch maximum (bottom / right, like F.pad in mmcv), then stack
        h = max(d.data.shape[-2] for d in items)
        w = max(d.data.shape[-1] for d in items)
        out = []
        for d in items:
            t = d.data
            out.append(torch.nn.functional.pad(t, (0, w - t.shape[-1], 0, h - t.shape[-2]), value=0))
        return DataContainer([torch.stack(out)], True)
    return DataContainer([[d.data for d in items]], False)


def collate(batch, samples_per_gpu=1):
    """mmcv.parallel.collate: pipeline samples (dicts of DataContainers; test mode: lists per augmentation) or the plain tensors of
    SyntheticVOCDataset -> one dict of DataContainers with a single per-device chunk."""
    first = batch[0]
    if isinstance(first.get('img'), DataContainer):
        return {k: _collate_dc([b[k] for b in batch], samples_per_gpu) for k in first}
    if isinstance(first.get('img'), (list, tuple)):              # MultiScaleFlipAug: [aug][...] -> list over augmentations
        n_aug = len(first['img'])
        out = {}
        for k in first:
            # plain tensors (ImageToTensor): mmcv would refuse unequal shapes (its configs switch to DefaultFormatBundle for
            # samples_per_gpu > 1, train_Lambda.py:61-63); pad bottom / right like a stacked DataContainer instead
            out[k] = [(_collate_dc([b[k][a] for b in batch], samples_per_gpu) if isinstance(first[k][a], DataContainer)
                       else _collate_dc([DataContainer(b[k][a], stack=True) for b in batch], samples_per_gpu).data[0]) for a in range(n_aug)]
        return out
    return dict(img=DataContainer([torch.stack([b['img'] for b in batch])], stack=True),
                img_metas=DataContainer([[b['img_metas'] for b in batch]], cpu_only=True),
                gt_bboxes=DataContainer([[b['gt_bboxes'] for b in batch]]),
                gt_labels=DataContainer([[b['gt_labels'] for b in batch]]))


def build_dataloader(dataset, samples_per_gpu, workers_per_gpu, num_gpus=1, dist=True, shuffle=True, seed=None, **kwargs):
    """mmdet/datasets/builder.py:76-139: dist=True -> this rank's strided share of a seeded permutation
    (DistributedGroupSampler semantics, samplers/group_sampler.py:101-142)."""
    import torch.distributed as tdist
    sampler = None
    if dist and tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
        if shuffle and getattr(dataset, 'flag', None) is not None:
            sampler = DistributedGroupSampler(dataset, samples_per_gpu, seed=seed or 0)          # builder.py:105-108
        else:
            sampler = torch.utils.data.distributed.DistributedSampler(dataset, shuffle=shuffle, seed=seed or 0)
        shuffle = False
    if sampler is None and shuffle and getattr(dataset, 'flag', None) is not None and len(np.unique(dataset.flag)) > 1:
        sampler, shuffle = GroupSampler(dataset, samples_per_gpu), False          # builder.py:113-115 (aspect-ratio groups)
    g = torch.Generator()
    g.manual_seed(seed or 0)
    return DataLoader(dataset, batch_size=samples_per_gpu, sampler=sampler, shuffle=shuffle, num_workers=workers_per_gpu,
                      collate_fn=lambda b: collate(b, samples_per_gpu), generator=g, drop_last=False, **kwargs)
