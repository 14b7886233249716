"""CPU tests of the COCO data path on small annotation files written to tmp_path: CocoDataset's two ann_file forms, category-id mapping,
the training view (get_ann_info) against the evaluation view (get_eval_info), the image filters, and the active-learning bookkeeping
(text id lists) on it."""
import json
import os

import numpy as np
import pytest

from aod_meh_hua_amd import datasets as D
from aod_meh_hua_amd.datasets import build_dataset
from tests.coco_util import category_ids, write_coco_json

NAMES = ('person', 'car', 'dog', 'boat')


def _anns():
    """image 0: one annotation of every kind; image 1: plain; image 2: only a foreign category; image 3: too small; image 4: empty"""
    img0 = [dict(bbox=[10, 20, 30, 40], label=1),                               # kept
            dict(bbox=[5, 5, 50, 60], label=0, iscrowd=1),                      # crowd -> ignore set
            dict(bbox=[1, 1, 10, 10], label=2, ignore=1),                       # `ignore` -> dropped
            dict(bbox=[2, 2, 10, 10], category_id=999),                         # foreign category -> dropped
            dict(bbox=[3, 3, 0.5, 10], label=2),                                # w < 1 -> dropped
            dict(bbox=[4, 4, 10, 0.25], label=2),                               # h < 1 -> dropped
            dict(bbox=[6, 6, 10, 10], label=3, area=0.0),                       # area <= 0 -> dropped
            dict(bbox=[300, 10, 20, 20], label=3),                              # outside the 200-wide image -> dropped
            dict(bbox=[100.5, 50.25, 20, 30], label=3, area=123.0)]             # kept; area differs from w * h
    return [img0, [dict(bbox=[0, 0, 64, 64], label=2)], [dict(bbox=[7, 7, 20, 20], category_id=999)], [dict(bbox=[1, 1, 8, 8], label=0)], []]


SIZES = [(100, 200), (64, 64), (80, 80), (20, 300), (50, 50)]          # (h, w)


@pytest.fixture()
def coco(tmp_path):
    path = str(tmp_path / 'instances.json')
    ids = write_coco_json(path, _anns(), names=NAMES + ('unused',), size=SIZES)
    raw = json.load(open(path))
    raw['categories'].append(dict(id=999, name='foreign'))
    json.dump(raw, open(path, 'w'))
    D._COCO_JSON.clear()
    return path, ids


def test_json_form_and_id_list_form_give_the_same_infos(coco, tmp_path):
    path, ids = coco
    a = build_dataset(dict(type='CocoDataset', ann_file=path, pipeline=[], classes=NAMES), dict(test_mode=True))
    lst = str(tmp_path / 'all.txt')
    np.savetxt(lst, np.array(ids), fmt='%s')
    b = build_dataset(dict(type='CocoDataset', ann_file=lst, coco_json=path, pipeline=[], classes=NAMES), dict(test_mode=True))
    assert a.data_infos == b.data_infos and a.img_ids == b.img_ids == ids and len(a) == 5
    assert a.data_infos[0] == dict(id=ids[0], filename='img_0.png', width=200, height=100)
    for i in range(5):
        for k, v in a.get_eval_info(i).items():
            assert np.array_equal(v, b.get_eval_info(i)[k])
    # a subset, in the list's order
    np.savetxt(lst, np.array([ids[3], ids[1]]), fmt='%s')
    c = build_dataset(dict(type='CocoDataset', ann_file=lst, coco_json=path, pipeline=[], classes=NAMES), dict(test_mode=True))
    assert c.img_ids == [ids[3], ids[1]] and c.get_eval_info(1)['labels'].tolist() == [2]
    # data_root joins both paths
    d = build_dataset(dict(type='CocoDataset', ann_file='all.txt', coco_json='instances.json', data_root=str(tmp_path), pipeline=[],
                           classes=NAMES), dict(test_mode=True))
    assert d.img_ids == c.img_ids


def test_category_ids_with_gaps(coco):
    path, _ = coco
    ds = build_dataset(dict(type='CocoDataset', ann_file=path, pipeline=[], classes=NAMES), dict(test_mode=True))
    want = category_ids(5)[:4]
    assert want == [1, 2, 4, 5] and ds.cat_ids == want and ds.cat2label == {1: 0, 2: 1, 4: 2, 5: 3}
    # CLASSES order wins over the file's category order
    rev = build_dataset(dict(type='CocoDataset', ann_file=path, pipeline=[], classes=NAMES[::-1]), dict(test_mode=True))
    assert rev.cat_ids == want[::-1] and rev.get_eval_info(1)['labels'].tolist() == [1]
    assert ds.get_cat_ids(0) == [2, 1, 4, 999, 4, 4, 5, 5, 5]
    assert len(D.CocoDataset.CLASSES) == 80 and len(set(D.CocoDataset.CLASSES)) == 80 and 'CocoDataset' in D.DATASETS.module_dict


def test_training_view_drops_and_ignores_evaluation_view_keeps(coco):
    path, _ = coco
    ds = build_dataset(dict(type='CocoDataset', ann_file=path, pipeline=[], classes=NAMES), dict(test_mode=True))
    a = ds.get_ann_info(0)
    assert a['bboxes'].tolist() == [[10, 20, 40, 60], [100.5, 50.25, 120.5, 80.25]] and a['labels'].tolist() == [1, 3]
    assert a['bboxes_ignore'].tolist() == [[5, 5, 55, 65]] and a['labels_ignore'].tolist() == [0]
    assert (a['bboxes'].dtype, a['labels'].dtype, a['bboxes_ignore'].dtype, a['labels_ignore'].dtype) == (np.float32, np.int64, np.float32, np.int64)
    e = ds.get_ann_info(4)
    assert e['bboxes'].shape == (0, 4) and e['labels'].shape == (0,) and e['bboxes_ignore'].shape == (0, 4) and e['labels_ignore'].shape == (0,)
    assert list(a) == ['bboxes', 'labels', 'bboxes_ignore', 'labels_ignore']
    from aod_meh_hua_amd.core.evaluation_device import pack_annotations
    assert pack_annotations([a, e])[3].tolist() == [3, 0]
    v = ds.get_eval_info(0)                          # everything of a kept category, file order, as written
    assert v['labels'].tolist() == [1, 0, 2, 2, 2, 3, 3, 3] and v['iscrowd'].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    assert v['boxes'][-1].tolist() == [100.5, 50.25, 20, 30] and v['area'].tolist() == [1200, 3000, 100, 5, 2.5, 0, 400, 123]
    assert (v['boxes'].dtype, v['area'].dtype, v['iscrowd'].dtype, v['labels'].dtype) == (np.float64, np.float64, np.uint8, np.int64)
    z = ds.get_eval_info(4)
    assert z['boxes'].shape == (0, 4) and z['area'].shape == (0,)


def test_filter_imgs_and_filter_empty_gt(coco):
    path, ids = coco
    ds = build_dataset(dict(type='CocoDataset', ann_file=path, pipeline=[], classes=NAMES))
    assert ds.img_ids == [ids[0], ids[1]] and ds.flag.tolist() == [1, 0]          # 2: foreign only, 3: 20 px high, 4: empty
    keep = build_dataset(dict(type='CocoDataset', ann_file=path, pipeline=[], classes=NAMES, filter_empty_gt=False))
    assert keep.img_ids == [ids[0], ids[1], ids[2], ids[4]]


def test_unknown_id_raises(coco, tmp_path):
    path, ids = coco
    lst = str(tmp_path / 'bad.txt')
    np.savetxt(lst, np.array([ids[0], 424242]), fmt='%s')
    with pytest.raises(KeyError, match='424242'):
        build_dataset(dict(type='CocoDataset', ann_file=lst, coco_json=path, pipeline=[], classes=NAMES))
    with pytest.raises(ValueError, match='coco_json'):
        build_dataset(dict(type='CocoDataset', ann_file=lst, pipeline=[], classes=NAMES))


def test_unsupported_metrics_raise(coco):
    path, _ = coco
    ds = build_dataset(dict(type='CocoDataset', ann_file=path, pipeline=[], classes=NAMES), dict(test_mode=True))
    empty = [[np.zeros((0, 5), np.float32) for _ in NAMES] for _ in range(len(ds))]
    for m in ('segm', 'proposal', 'proposal_fast', ['bbox', 'segm']):
        with pytest.raises(KeyError, match='is not supported'):
            ds.evaluate(empty, metric=m)
    assert ds.evaluate(empty, metric='bbox', logger='silent')['bbox_mAP'] == 0.0


def test_active_learning_split_round_trip_and_one_parse(tmp_path, monkeypatch):
    from aod_meh_hua_amd.datasets import SyntheticVOCDataset
    from aod_meh_hua_amd.mmcv_lite import Config
    from aod_meh_hua_amd.utils.active_datasets import create_X_L_file, create_X_U_file, get_X_L_0_prev
    src = SyntheticVOCDataset(num_images=12, size=(64, 64))
    path, lst = str(tmp_path / 'pool.json'), str(tmp_path / 'pool.txt')
    ids = write_coco_json(path, src)
    np.savetxt(lst, np.array(ids), fmt='%s')
    from tests.coco_util import VOC_NAMES
    inner = dict(type='CocoDataset', ann_file=[lst], coco_json=path, pipeline=[], classes=VOC_NAMES)
    cfg = Config(dict(data=dict(train=dict(type='RepeatDataset', times=1, dataset=inner)), X_L_0_size=4, X_S_size=2, X_L_repeat=2, X_U_repeat=2,
                      work_dir=str(tmp_path / 'work')))
    np.random.seed(5)
    X_L, X_U, X_all, anns = get_X_L_0_prev(cfg)
    assert len(X_all) == 12 and len(X_L) == 4 and len(X_U) == 4 and not set(X_L) & set(X_U)
    D._COCO_JSON.clear()
    loads = []
    real = json.load
    monkeypatch.setattr(json, 'load', lambda f, *a, **k: (loads.append(1), real(f, *a, **k))[1])
    cfg = create_X_L_file(cfg, X_L, anns, 0)
    ds = build_dataset(cfg.data.train)
    assert len(ds) == 8 and ds.dataset.datasets[0].img_ids == [ids[i] for i in X_L]
    for k, i in enumerate(X_L):
        assert np.allclose(ds.dataset.get_ann_info(k)['bboxes'], src.get_ann_info(int(i))['bboxes'], atol=1e-4)
        assert ds.dataset.get_ann_info(k)['labels'].tolist() == src.get_ann_info(int(i))['labels'].tolist()
    cfg = create_X_U_file(cfg, X_U, anns, 0)
    du = build_dataset(cfg.data.train)
    assert du.dataset.datasets[0].img_ids == [ids[i] for i in X_U]
    # two splits of one pool in one ConcatDataset: the json was parsed once for all of the above
    both = build_dataset(dict(inner, ann_file=[cfg.work_dir + '/cycle0/trainval_X_L_07.txt', cfg.work_dir + '/cycle0/trainval_X_U_07.txt']))
    assert len(both) == 8 and len(loads) == 1
    assert both.datasets[0].coco is both.datasets[1].coco


def test_coco_id_list_tool_writes_what_the_dataset_keeps(coco, tmp_path):
    import importlib.util
    path, ids = coco
    spec = importlib.util.spec_from_file_location('coco_id_list', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                               'tools', 'coco_id_list.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    names = str(tmp_path / 'names.txt')
    open(names, 'w').write('\n'.join(NAMES) + '\n')
    out_all, out_train = str(tmp_path / 'all_ids.txt'), str(tmp_path / 'train_ids.txt')
    assert tool.main([path, out_all, '--classes', names]) == 0 and tool.main([path, out_train, '--classes', names, '--train']) == 0
    assert [int(x) for x in open(out_all).read().split()] == ids
    assert [int(x) for x in open(out_train).read().split()] == [ids[0], ids[1]]          # what _filter_imgs keeps
    # the n-th line of the --train list is the n-th image of the training dataset built from it, so pool indices are list indices
    ds = build_dataset(dict(type='CocoDataset', ann_file=out_train, coco_json=path, pipeline=[], classes=NAMES))
    assert ds.img_ids == [ids[0], ids[1]] and len(ds) == len(open(out_train).read().split())


def test_pool_inputs_of_a_test_mode_batch(tmp_path):
    """apis.test._inputs on a collated MultiScaleFlipAug batch: one entry per augmentation, the image batch as a tensor and the metas as a
    plain list -- the form a SyntheticVOCDataset batch has after it, and the form the captured evaluation graph takes"""
    import torch
    from aod_meh_hua_amd.apis.test import _inputs, _single, _unwrap
    from aod_meh_hua_amd.datasets import SyntheticVOCDataset, collate
    from aod_meh_hua_amd.mmcv_lite import DataContainer
    from tests.coco_util import VOC_NAMES, write_coco_images
    src = SyntheticVOCDataset(num_images=3, size=(64, 96))
    write_coco_images(str(tmp_path / 'images'), src)
    path = str(tmp_path / 'pool.json')
    write_coco_json(path, src)
    norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
    pipeline = [dict(type='LoadImageFromFile'),
                dict(type='MultiScaleFlipAug', img_scale=(96, 64), flip=False,
                     transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Normalize', **norm),
                                 dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]
    ds = build_dataset(dict(type='CocoDataset', ann_file=path, img_prefix=str(tmp_path / 'images'), pipeline=pipeline, classes=VOC_NAMES),
                       dict(test_mode=True))
    batch = collate([ds[0], ds[1], ds[2]], 3)
    assert isinstance(batch['img_metas'][0], DataContainer)          # what the collate hands over
    data = _inputs(batch)
    assert sorted(data) == ['img', 'img_metas'] and _single(data)
    assert torch.is_tensor(data['img'][0]) and tuple(data['img'][0].shape) == (3, 3, 64, 96)
    metas = data['img_metas'][0]
    assert isinstance(metas, list) and len(metas) == 3 and all(isinstance(m, dict) for m in metas)
    assert [m['ori_filename'] for m in metas] == ['img_0.png', 'img_1.png', 'img_2.png'] and metas[0]['img_shape'] == (64, 96, 3)
    # a batch of the synthetic dataset (containers at the top level) keeps the form it always had
    syn = _inputs(collate([src[0], src[1]], 2))
    assert torch.is_tensor(syn['img'][0]) and tuple(syn['img'][0].shape) == (2, 3, 64, 96) and [m['image_id'] for m in syn['img_metas'][0]] == [0, 1]
    # containers and plain values outside lists are unwrapped as before
    dc = DataContainer([[1, 2]], cpu_only=True)
    assert _unwrap(dc) == [[1, 2]] and _unwrap(5) == 5 and _unwrap([dc, 7]) == [[1, 2], 7]
