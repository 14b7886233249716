"""GPU: the COCO evaluation pass end to end -- apis.single_gpu_coco_map (padded detections -> aod_coco_match -> DeviceCocoAccumulator)
against CocoDataset.evaluate(single_gpu_test(...), metric='bbox') on the same model and loader: the same dict key for key, under graph
replay and eagerly, at batch sizes 1, 2 and 3, for RetinaNet and SSD300, through EvalHook with and without device_metric, and the
active-learning driver on a COCO pool."""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import model as omodel
from tests.coco_util import VOC_NAMES, write_coco_images, write_coco_json

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _coco_tree(root, num_images, size, names=VOC_NAMES):
    """images + annotation json + id list of a synthetic pool; image 0's first box becomes a crowd, image 1 gains a tiny box"""
    from aod_meh_hua_amd.datasets import SyntheticVOCDataset
    src = SyntheticVOCDataset(num_images=num_images, size=size)
    os.makedirs(root, exist_ok=True)
    write_coco_images(os.path.join(root, 'images'), src)
    path, lst = os.path.join(root, 'instances.json'), os.path.join(root, 'ids.txt')
    ids = write_coco_json(path, src, names=names, crowd=((0, 0),), extra=((1, dict(bbox=[3.0, 3.0, 2.0, 2.0], label=5)),))
    np.savetxt(lst, np.array(ids), fmt='%s')
    return path, lst, os.path.join(root, 'images') + '/'


def _dataset(config, tree, size):
    from aod_meh_hua_amd.datasets import build_dataset
    from aod_meh_hua_amd.mmcv_lite import Config
    cfg = Config.fromfile(os.path.join(ROOT, config))
    cfg.model.backbone.pop('init_cfg', None)
    pipeline = cfg.test_pipeline
    pipeline[1]['img_scale'] = size
    path, lst, prefix = tree
    ds = build_dataset(dict(type='CocoDataset', ann_file=lst, coco_json=path, img_prefix=prefix, pipeline=pipeline, classes=VOC_NAMES),
                       dict(test_mode=True))
    return cfg, ds


def _loader(ds, bs):
    from aod_meh_hua_amd.datasets import build_dataloader
    return build_dataloader(ds, samples_per_gpu=bs, workers_per_gpu=0, dist=False, shuffle=False)


def _build(cfg, state):
    from aod_meh_hua_amd.mmcv_lite import MMDataParallel
    from aod_meh_hua_amd.models import build_detector
    model = build_detector(cfg.model)
    model.load_state_dict(state, strict=True)
    return MMDataParallel(model.cuda()).eval()


def _host(model, ds, bs, **kw):
    from aod_meh_hua_amd.apis.test import single_gpu_test
    return ds.evaluate(single_gpu_test(model, _loader(ds, bs), isUnc=False), metric='bbox', logger='silent', **kw)


def _host_precision(model, ds, bs, iou_thrs=None):
    from aod_meh_hua_amd.apis.test import single_gpu_test
    from aod_meh_hua_amd.core import coco_eval as CE
    results = single_gpu_test(model, _loader(ds, bs), isUnc=False)
    infos, K = ds.eval_infos(), len(ds.CLASSES)
    thrs = CE.default_iou_thrs() if iou_thrs is None else np.asarray(iou_thrs, np.float64)
    parts = [CE.image_states(r[:K], i, thrs, 1000) for r, i in zip(results, infos)]
    return CE.accumulate(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts], 2),
                         CE.count_npig(infos, K), K)


@pytest.fixture(scope='module')
def retina(tmp_path_factory):
    """a small RetinaNet and 12 synthetic images at 128 x 128 as a COCO pool.  retina_cls's weights are scaled (x 1, 2, 4, ...) until the
    metric is not vacuous (bbox_mAP_50 > 0)"""
    tree = _coco_tree(str(tmp_path_factory.mktemp('coco')), 12, (128, 128))
    cfg, ds = _dataset('configs/_base_/Config_RetinaNet.py', tree, (128, 128))
    assert len(ds) == 12 and ds.get_eval_info(0)['iscrowd'][0] == 1 and ds.get_eval_info(1)['area'][-1] == 4.0
    sd = omodel.seeded_state_dict(cls_bias=1.0)
    for scale in (1, 2, 4, 8, 16, 32):
        state = dict(sd)
        state['bbox_head.retina_cls.weight'] = sd['bbox_head.retina_cls.weight'] * scale
        model = _build(cfg, state)
        want = {2: _host(model, ds, 2)}
        print(f'retina fixture: retina_cls x {scale}: {want[2]}')
        if want[2]['bbox_mAP_50'] > 0:
            break
    return model, ds, want


def _want(retina, bs):
    model, ds, want = retina
    if bs not in want:
        want[bs] = _host(model, ds, bs)
    return want[bs]


def test_fixture_is_not_vacuous(retina):
    assert retina[2][2]['bbox_mAP_50'] > 0


@pytest.mark.parametrize('graph', ['replayed', 'eager'])
@pytest.mark.parametrize('bs', [1, 2, 3])
def test_single_gpu_coco_map_equals_the_host_dict(retina, bs, graph, monkeypatch):
    from aod_meh_hua_amd import apis
    from aod_meh_hua_amd.apis import test as apis_test
    model, ds, _ = retina
    if graph == 'eager':
        monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    else:
        monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    want = _want(retina, bs)
    tm = {}
    got = apis.single_gpu_coco_map(model, _loader(ds, bs), isUnc=False, _timing=tm)
    assert got == want and list(got) == list(want), (got, want)
    # the unrounded precision array [T, 101, K, A] too, not only the dict's three digits
    prec = _host_precision(model, ds, bs)
    assert (prec > 0).any() and np.array_equal(tm['accumulator'].precision(), prec)
    if graph == 'replayed':          # it did replay: the captured evaluation graph holds this batch shape
        gs = [v for k, v in apis_test._GSCORE.get(model).items() if k[0] == 'eval_padded']
        assert len(gs) == 1 and len(gs[0].cache) >= 1 and not gs[0].pipe


def test_options_reach_the_device_path(retina):
    from aod_meh_hua_amd import apis
    model, ds, _ = retina
    # loose thresholds: many matches, per-class numbers well above zero
    kw = dict(iou_thrs=[0.05, 0.1, 0.3, 0.5], classwise=True, metric_items=['mAP', 'mAP_50', 'mAP_s'])
    want = _host(model, ds, 2, **kw)
    got = apis.single_gpu_coco_map(model, _loader(ds, 2), isUnc=False, **kw)
    print('loose thresholds:', got)
    assert got == want and list(got) == list(want) and 'bbox_AP_aeroplane' in got and 'bbox_mAP_75' not in got
    assert got['bbox_mAP'] > 0 and sum(v > 0 for k, v in got.items() if k.startswith('bbox_AP_')) >= 2
    with pytest.raises(ValueError, match='detUnc'):
        apis.single_gpu_coco_map(model, _loader(ds, 2), detUnc=True)
    with pytest.raises(KeyError, match='is not supported'):
        apis.single_gpu_coco_map(model, _loader(ds, 2), metric='segm')


def test_accumulator_update_on_detections_seeded_from_the_gts():
    """DeviceCocoAccumulator.update (H2D pack, aod_coco_match, store) and finalize on the quantised draw, whose detections are copies,
    halves and shifts of the gts: every summary number is well above zero, and dict and precision array equal the host evaluator's."""
    from aod_meh_hua_amd.core import coco_eval as CE
    from aod_meh_hua_amd.core.coco_eval_device import DeviceCocoAccumulator
    from tests.coco_util import padded_batch, quantised_draw
    results, infos = quantised_draw()
    K, M, N = len(results[0]), 16, len(results)
    names = [str(c) for c in range(K)]
    want = CE.evaluate_bbox(results, infos, names, classwise=True, logger='silent')
    assert all(want[f'bbox_{k}'] > 0.01 for k in CE.METRIC_ITEMS), want          # (0.037 .. 0.221: far from the rounding step)
    acc = DeviceCocoAccumulator(K, None, M, N, 'cuda')
    rng = np.random.RandomState(2)
    for s in range(0, N, 12):
        d, l, n = padded_batch(results[s:s + 12], M, rng)
        acc.update(list(range(s, min(s + 12, N))), torch.from_numpy(d).cuda(), torch.from_numpy(l).cuda(), torch.from_numpy(n).cuda(),
                   infos[s:s + 12])
    got = acc.finalize(names, classwise=True, logger='silent')
    assert got == want and list(got) == list(want), (got, want)
    parts = [CE.image_states(r, i, CE.default_iou_thrs(), 1000) for r, i in zip(results, infos)]
    prec = CE.accumulate(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts], 2),
                         CE.count_npig(infos, K), K)
    assert np.array_equal(acc.precision(), prec)


def test_eval_hook_bbox_with_and_without_device_metric(retina):
    from aod_meh_hua_amd.mmcv_lite import EvalHook, LogBuffer
    model, ds, _ = retina
    want = _want(retina, 2)

    class R:
        epoch, logger = 2, 'silent'
    R.model = model
    out = []
    for extra in (dict(), dict(device_metric=True)):
        R.log_buffer = LogBuffer()
        hook = EvalHook(_loader(ds, 2), interval=3, metric='bbox', show=False, isUnc=False, out_dir=None, **extra)
        res = hook.after_train_epoch(R)
        assert R.log_buffer.ready and R.log_buffer.output['eval_iter_num'] == 6
        assert all(R.log_buffer.output[k] == v for k, v in res.items())
        out.append(res)
    assert out[0] == out[1] == want and list(out[0]) == list(out[1])
    R.log_buffer = LogBuffer()
    with pytest.raises(KeyError, match='is not supported'):
        EvalHook(_loader(ds, 2), interval=3, metric='segm', device_metric=True).after_train_epoch(R)


def test_ssd300_coco_device_metric_equals_the_host_dict(tmp_path):
    from aod_meh_hua_amd import apis
    from oracle import model_ssd as ossd
    tree = _coco_tree(str(tmp_path / 'coco'), 4, (300, 300))
    cfg, ds = _dataset('configs/_base_/Config_SSD.py', tree, (300, 300))
    model = _build(cfg, ossd.seeded_state_dict())
    assert model.module.bbox_head.test_cfg.max_per_img == 200
    from aod_meh_hua_amd.apis.test import single_gpu_test
    results = single_gpu_test(model, _loader(ds, 2), isUnc=False)
    assert sum(a.shape[0] for img in results for a in img) > 0
    want = ds.evaluate(results, metric='bbox', logger='silent')
    got = apis.single_gpu_coco_map(model, _loader(ds, 2), isUnc=False)
    assert got == want and list(got) == list(want), (got, want)


def test_al_driver_two_cycles_on_a_coco_pool(tmp_path):
    from aod_meh_hua_amd.datasets import COCO_CLASSES
    from aod_meh_hua_amd.mmcv_lite import Config
    path, lst, prefix = _coco_tree(str(tmp_path / 'coco'), 12, (128, 128), names=COCO_CLASSES[:20])
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/_base_/Config_RetinaNet_COCO.py'))
    cfg.model.backbone.pop('init_cfg')                       # no pretrained weights: nothing is fetched
    for split in (cfg.data.train.dataset, cfg.data.test, cfg.data.val):
        split.coco_json, split.img_prefix = path, prefix
        split.ann_file = [lst] if isinstance(split.ann_file, (list, tuple)) else lst
        for step in split.pipeline:
            if 'img_scale' in step:
                step['img_scale'] = (128, 128)
    cfg.X_L_0_size, cfg.X_S_size, cfg.epoch_ratio, cfg.outer_epoch = 4, 2, [1, 1], 1
    cfg.runner.max_epochs = 1
    cfg.evaluation.interval = 1
    cfg.log_config.interval = 1
    patched = str(tmp_path / 'Config_RetinaNet_COCO.py')
    cfg.dump(patched)
    wd = f'pytest_coco_driver_{os.getpid()}'
    cmd = [sys.executable, os.path.join(ROOT, 'tools/train_RetinaNet.py'), '--config', patched, '--cycles', '2', '--work-dir', wd,
           '--samples-per-gpu', '2', '--device-metric']
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=dict(os.environ, AOD_WORKERS='0'))
    out = os.path.join(ROOT, 'work_dirs', wd)
    try:
        assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
        xl0, xl1 = np.load(os.path.join(out, 'X_L_0.npy')), np.load(os.path.join(out, 'X_L_1.npy'))
        unc = np.load(os.path.join(out, 'Unc_1.npy'))
        assert len(xl0) == 4 and len(xl1) == 6 and set(xl0) <= set(xl1) and unc.shape == (12,) and np.isfinite(unc).all()
        log = ''.join(open(f).read() for f in glob.glob(os.path.join(out, '*.log'))) + p.stdout + p.stderr
        assert 'bbox_mAP' in log
    finally:
        shutil.rmtree(out, ignore_errors=True)
