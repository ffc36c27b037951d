# r50_ycbv_pbr.py trained with AutoAugment's colour stages: the model, losses and schedule of that file, the data pipeline of
# base/datasets/bop_detection_color.py (AutoAugment over [Rotate, ColorTransform], [EqualizeTransform], [BrightnessTransform,
# ContrastTransform], [CutOut] directly after Resize: constant 480 x 640 batches).  The levels and probabilities are a
# starting point nobody has trained with.
_base_ = ['./r50_ycbv_pbr.py', '../base/datasets/bop_detection_color.py']

data = dict(samples_per_gpu=16, workers_per_gpu=8)
