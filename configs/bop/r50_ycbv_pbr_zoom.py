# r50_ycbv_pbr.py trained with zoom augmentation: the model, losses and schedule of that file, the data pipeline of
# base/datasets/bop_detection_zoom.py (Expand + MinIoURandomCrop in front of Resize(keep_ratio=False): constant 480 x 640 batches).
_base_ = ['./r50_ycbv_pbr.py', '../base/datasets/bop_detection_zoom.py']

data = dict(samples_per_gpu=16, workers_per_gpu=8)
