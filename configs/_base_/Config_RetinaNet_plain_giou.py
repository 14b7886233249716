# The plain RetinaNet-R50-FPN baseline (Config_RetinaNet_plain.py) trained with the GIoU box loss on the decoded boxes instead of L1 on
# the encoded deltas: loss_bbox and reg_decoded_bbox go together.  Everything else is the plain baseline.
_base_ = './Config_RetinaNet_plain.py'
model = dict(bbox_head=dict(reg_decoded_bbox=True, loss_bbox=dict(type='GIoULoss', loss_weight=2.0)))
