# r50_ycbv_pbr.py with the box regression loss swapped for CIoULoss (centre distance and aspect-ratio terms on top of
# IoU): the first knob to turn for small or elongated BOP objects.  loss_weight=2.0 is GIoU's value carried over as a
# starting point; nobody has trained with this file yet.
_base_ = ['./r50_ycbv_pbr.py']

model = dict(bbox_head=dict(loss_bbox=dict(_delete_=True, type='CIoULoss', loss_weight=2.0)))
