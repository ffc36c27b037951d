# r50_ycbv_pbr.py with an exponential moving average of the trainable weights: mmcv's EMAHook at its defaults.  Every
# evaluation during training and every checkpoint sees the EMA weights (a checkpoint's parameters ARE the EMA weights; the
# raw ones ride along as its `ema_*` entries, so a resume is exact).  A starting point: nobody has trained with this file
# yet.  With few optimizer steps (r50_ycbv_pbr_accum.py) a larger momentum and a shorter warm_up are the knobs to try.
_base_ = ['./r50_ycbv_pbr.py']

custom_hooks = [dict(type='EMAHook', momentum=0.0002, interval=1, warm_up=100)]
