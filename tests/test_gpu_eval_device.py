"""GPU: the device evaluation pass end to end -- apis.test.single_gpu_map (padded detections -> aod_eval_match -> DeviceMapAccumulator)
against eval_map(single_gpu_test(...)) on the same model and loader: the same mean_ap float and every per-class array equal, under graph
replay and eagerly, for RetinaNet and SSD300, and through EvalHook(device_metric=True)."""
import os

import numpy as np
import pytest
import torch

from oracle import model as omodel
from tests.eval_device_util import assert_same_eval

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(config, state_dict, num_images, size, bs):
    from aod_meh_hua_amd.datasets import build_dataloader, build_dataset
    from aod_meh_hua_amd.mmcv_lite import Config, MMDataParallel
    from aod_meh_hua_amd.models import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, config))
    cfg.model.backbone.pop('init_cfg')
    model = build_detector(cfg.model)
    model.load_state_dict(state_dict, strict=True)
    model = MMDataParallel(model.cuda())
    ds = build_dataset(dict(type='SyntheticVOCDataset', num_images=num_images, size=size), dict(test_mode=True))
    dl = build_dataloader(ds, samples_per_gpu=bs, workers_per_gpu=0, dist=False, shuffle=False)
    return model, ds, dl


def _host(model, ds, dl, thrs, dataset='voc07'):
    from aod_meh_hua_amd.apis.test import single_gpu_test
    from aod_meh_hua_amd.core.evaluation import eval_map
    results = single_gpu_test(model, dl, isUnc=False)
    anns = [ds.get_ann_info(i) for i in range(len(ds))]
    n_det = sum(a.shape[0] for img in results for a in img)
    return [eval_map(results, anns, iou_thr=t, dataset=dataset, logger='silent') for t in thrs], n_det


@pytest.fixture(scope='module')
def retina():
    model, ds, dl = _setup('configs/_base_/Config_RetinaNet.py', omodel.seeded_state_dict(cls_bias=1.0), 6, (128, 128), 2)
    want, n_det = _host(model, ds, dl, [0.5, 0.75])
    assert n_det > 0                                   # the comparison is not vacuous
    return model, ds, dl, want


def test_single_gpu_map_equals_the_host_metric_under_graph_replay(retina, monkeypatch):
    from aod_meh_hua_amd.apis import test as apis_test
    model, ds, dl, want = retina
    monkeypatch.delenv('AOD_HIP_GRAPH', raising=False)
    got = apis_test.single_gpu_map(model, dl, iou_thr=[0.5, 0.75], dataset='voc07', isUnc=False)
    assert isinstance(got, list) and len(got) == 2
    for g, w in zip(got, want):
        assert_same_eval(g, w)
    assert sum(r['num_dets'] for r in got[0][1]) > 0
    # it did replay: one captured eval graph for the 2-image batch shape
    cache = apis_test._GSCORE.get(model)
    gs = [v for k, v in cache.items() if k[0] == 'eval_padded']
    assert len(gs) == 1 and len(gs[0].cache) == 1 and not gs[0].pipe
    # a float threshold gives the pair itself; a second pass replays the same graph
    one = apis_test.single_gpu_map(model, dl, iou_thr=0.5, dataset='voc07', isUnc=False)
    assert isinstance(one, tuple)
    assert_same_eval(one, want[0])
    assert len(gs[0].cache) == 1


def test_single_gpu_map_equals_the_host_metric_eagerly(retina, monkeypatch):
    from aod_meh_hua_amd.apis import test as apis_test
    model, ds, dl, want = retina
    monkeypatch.setenv('AOD_HIP_GRAPH', '0')
    got = apis_test.single_gpu_map(model, dl, iou_thr=[0.5, 0.75], dataset='voc07', isUnc=False)
    for g, w in zip(got, want):
        assert_same_eval(g, w)
    # area-mode AP with class names, as a non-2007 dataset asks for it
    from aod_meh_hua_amd.core.evaluation import eval_map
    from aod_meh_hua_amd.apis.test import single_gpu_test
    res = single_gpu_test(model, dl, isUnc=False)
    anns = [ds.get_ann_info(i) for i in range(len(ds))]
    assert_same_eval(apis_test.single_gpu_map(model, dl, iou_thr=0.5, dataset=ds.CLASSES, isUnc=False),
                     eval_map(res, anns, iou_thr=0.5, dataset=ds.CLASSES, logger='silent'))


def test_eval_hook_device_metric_returns_the_host_dict(retina):
    from aod_meh_hua_amd.mmcv_lite import EvalHook, LogBuffer
    model, ds, dl, want = retina

    class R:
        epoch, logger = 4, 'silent'
    R.model = model
    out = []
    for extra in (dict(), dict(device_metric=True)):
        R.log_buffer = LogBuffer()
        hook = EvalHook(dl, interval=5, metric='mAP', show=False, isUnc=False, out_dir=None, **extra)
        res = hook.after_train_epoch(R)
        assert R.log_buffer.output['mAP'] == res['mAP'] and R.log_buffer.output['eval_iter_num'] == 3 and R.log_buffer.ready
        out.append(res)
    assert out[0] == out[1] and list(out[0]) == list(out[1]) and out[1]['AP50'] == round(want[0][0], 3)


def test_ssd300_device_metric_equals_the_host_metric():
    from aod_meh_hua_amd.apis import test as apis_test
    from oracle import model_ssd as ossd
    model, ds, dl = _setup('configs/_base_/Config_SSD.py', ossd.seeded_state_dict(), 4, (300, 300), 2)
    assert model.module.bbox_head.test_cfg.max_per_img == 200
    want, n_det = _host(model, ds, dl, [0.5])
    assert n_det > 0
    assert_same_eval(apis_test.single_gpu_map(model, dl, iou_thr=0.5, dataset='voc07', isUnc=False), want[0])


def test_detunc_is_refused(retina):
    from aod_meh_hua_amd.apis.test import single_gpu_map
    model, ds, dl, want = retina
    with pytest.raises(ValueError, match='detUnc'):
        single_gpu_map(model, dl, detUnc=True)
