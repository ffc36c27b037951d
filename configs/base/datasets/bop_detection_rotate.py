# In-plane rotation training from BOP images: the pbr pipeline with Rotate directly after Resize.  Half of the samples are
# turned by 30 degrees, the sign drawn per sample, about the centre of the resized frame; what the turn uncovers is filled
# with grey (128), which a drawn RandomBackground then replaces like the rest of the scene outside the masks.  Boxes become
# the extent of their turned corners, clipped to the frame; masks are warped with the frame.  Every batch stays 480 x 640.
# On the device the turn is one warp launch on the resized frames and one on the resized masks (cv2.warpAffine's classic
# fixed-point bilinear arithmetic).
# level=10, max_rotate_angle=30 and prob=0.5 are a starting point, not tuned values: nobody has trained with them yet.
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
    dict(type='Resize', img_scale=(640, 480), keep_ratio=True),
    dict(type='Rotate', level=10, max_rotate_angle=30, prob=0.5, img_fill_val=128),
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
