# Zoom training from BOP images: Expand places the frame on a mean-filled canvas of up to 2x its size (zoom-out, objects get
# smaller), MinIoURandomCrop cuts a random patch with an IoU floor against the gt boxes (zoom-in), and Resize brings
# whatever came out to 640 x 480 (keep_ratio=False: the SSD form, so every batch has one tensor shape and the engine's
# per-shape plan and launch tape keep replaying).  On the device no canvas is made: the resize and the mask kernels sample
# the planned window of the source directly.
# ratio_range=(1, 2), prob=0.5, the min_ious and min_crop_size=0.3 are a starting point, not tuned values: nobody has
# trained with them yet.
dataset_type = 'BOPDataset'
data_root = 'data/bop/ycbv/'
background_dir = 'data/backgrounds/'
img_norm_cfg = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
label_assignment = dict(
    type='LabelAssignment',
    anchor_generator_cfg=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                              strides=[8, 16, 32, 64, 128]),
    neg_threshold=0.2, positive_num=10, adapt_positive_num=False, balance_sample=True)
train_pipeline = [
    dict(type='LoadImageFromFile'),
    dict(type='LoadAnnotations', with_bbox=True, with_bop_mask=True),
    dict(type='Expand', mean=img_norm_cfg['mean'], to_rgb=img_norm_cfg['to_rgb'], ratio_range=(1, 2), prob=0.5),
    dict(type='MinIoURandomCrop', min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3),
    dict(type='Resize', img_scale=(640, 480), keep_ratio=False),
    dict(type='RandomBackground', background_dir=background_dir, prob=0.3),
    dict(type='CosyPoseAug', p=0.8, pipelines=[
        dict(type='PillowBlur', p=1., factor_interval=(1, 3)),
        dict(type='PillowSharpness', p=0.3, factor_interval=(0., 50.)),
        dict(type='PillowContrast', p=0.3, factor_interval=(0.2, 50.)),
        dict(type='PillowBrightness', p=0.5, factor_interval=(0.1, 6.0)),
        dict(type='PillowColor', p=0.3, factor_interval=(0., 20.))]),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='GenerateDistanceMap'),
    label_assignment,
    dict(type='Normalize', **img_norm_cfg),
    dict(type='Pad', size_divisor=16),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels', 'points_to_gt_index', 'points_weight']),
]
data = dict(
    samples_per_gpu=16, workers_per_gpu=4,
    train=dict(type=dataset_type, ann_file=data_root + 'annotations/train_pbr.json', img_prefix=data_root + 'train_pbr/',
               seg_prefix=data_root + 'train_pbr/', pipeline=train_pipeline))
