# r50_ycbv_pbr.py on ONE GPU at the reference's effective batch: 8 accumulated micro-batches of 16 images per optimizer
# step (the reference trains on 8 GPUs x 16), with weight decay kept off the BN / GN affine parameters.  A starting point:
# nobody has trained with this file yet.  max_iters, the OneCycle horizon and the checkpoint / evaluation intervals count
# micro-iterations (multiply the base file's by 8 for the same number of optimizer steps).
_base_ = ['./r50_ycbv_pbr.py']

optimizer = dict(paramwise_cfg=dict(norm_decay_mult=0.))
optimizer_config = dict(type='GradientCumulativeOptimizerHook', cumulative_iters=8, grad_clip=dict(max_norm=35, norm_type=2))
