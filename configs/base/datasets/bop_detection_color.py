# Colour and occlusion training from BOP images: the pbr pipeline with one AutoAugment directly after Resize whose four
# policies are [Rotate, ColorTransform], [EqualizeTransform], [BrightnessTransform, ContrastTransform] and [CutOut]: the mix of
# geometric and colour stages of the AutoAugment-for-detection policies.  A colour stage changes pixels only; boxes, labels
# and masks stay as they are, as in the reference.  The ColorTransform behind the Rotate of its policy sees the warp's fill
# pixels, as in the reference.  The colour stages run in front of RandomBackground, so where a background is drawn they
# survive on the objects only (the merge pastes background everywhere else).
# On the device a policy's entries run in order, per entry rank: a warp launch, a CutOut launch, a histogram launch
# (Equalize / Contrast) and an apply launch, each only when some sample of the batch has such an entry at that rank.
# color_stages=True is this project's switch for colour stages inside policies: without it AutoAugment keeps refusing them.
# The levels and probabilities are a starting point, not tuned values: nobody has trained with them yet.
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
    dict(type='AutoAugment', policies=[
        [dict(type='Rotate', level=10, max_rotate_angle=30, prob=0.5, img_fill_val=128),
         dict(type='ColorTransform', level=6, prob=0.6)],
        [dict(type='EqualizeTransform', prob=0.8)],
        [dict(type='BrightnessTransform', level=3, prob=0.6), dict(type='ContrastTransform', level=7, prob=0.6)],
        [dict(type='CutOut', n_holes=(1, 4), cutout_ratio=[(0.1, 0.1), (0.2, 0.15)], fill_in=(0, 0, 0))]],
         color_stages=True),
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
