# r50_ycbv_pbr.py trained with CutOut occlusion: the model, losses and schedule of that file, the data pipeline of
# base/datasets/bop_detection_cutout.py (AutoAugment over [Rotate, CutOut], [CutOut], [Translate] directly after Resize:
# constant 480 x 640 batches).
_base_ = ['./r50_ycbv_pbr.py', '../base/datasets/bop_detection_cutout.py']

data = dict(samples_per_gpu=16, workers_per_gpu=8)
