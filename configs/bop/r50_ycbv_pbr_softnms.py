# r50_ycbv_pbr.py with Soft-NMS at test time (mmcv.ops.batched_nms, nms.type='soft_nms'): overlapping detections of one
# class have their scores decayed instead of being deleted, for bins that hold many heavily overlapping instances of one
# object (T-LESS, ITODD, IC-BIN).  The values are mmcv's defaults, a starting point; nobody has evaluated with this file yet.
_base_ = ['./r50_ycbv_pbr.py']

test_cfg = dict(nms=dict(_delete_=True, type='soft_nms', iou_threshold=0.3, sigma=0.5, min_score=1e-3, method='linear'))
