# r50_ycbv_pbr.py trained with scale jitter: the model, losses and schedule of that file, the data pipeline of
# base/datasets/bop_detection_jitter.py (Resize(ratio_range) + RandomCrop + Pad(size): constant 480 x 640 batches).
_base_ = ['./r50_ycbv_pbr.py', '../base/datasets/bop_detection_jitter.py']

data = dict(samples_per_gpu=16, workers_per_gpu=8)
