#!/usr/bin/env python
"""Write the image-id list of a COCO annotation file, one id per line: the `ann_file` form CocoDataset takes next to `coco_json=`, and the
form the active-learning bookkeeping reads and rewrites (configs/_base_/Config_RetinaNet_COCO.py).

    python tools/coco_id_list.py data/coco/annotations/instances_val2017.json data/coco/annotations/val2017_ids.txt
    python tools/coco_id_list.py data/coco/annotations/instances_train2017.json data/coco/annotations/train2017_ids.txt --train

--train keeps only the images that pass the training filters (at least 32 pixels on the short side, at least one annotation of a kept
category), so that the n-th line of the list is the n-th image of the training dataset built from it."""
import argparse
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('json')
    p.add_argument('out')
    p.add_argument('--train', action='store_true', help='only the images that pass CocoDataset._filter_imgs')
    p.add_argument('--classes', default=None, help='file with one class name per line (default: the 80 COCO classes)')
    a = p.parse_args(argv)
    from aod_meh_hua_amd.datasets import CocoDataset
    ds = CocoDataset(ann_file=a.json, pipeline=[], classes=a.classes, test_mode=not a.train)
    with open(a.out, 'w') as f:
        f.writelines(f'{i}\n' for i in ds.img_ids)
    print(f'{a.out}: {len(ds.img_ids)} image ids')
    return 0


if __name__ == '__main__':
    sys.exit(main())
