"""What the mask-free sampler tests share: the train pipelines with a chosen GenerateDistanceMap, and a set of boxes
that touch every border and corner of an image."""
import numpy as np

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
COSY = [dict(type="PillowBlur", p=1., factor_interval=(1, 3)),
        dict(type="PillowSharpness", p=0.3, factor_interval=(0., 50.)),
        dict(type="PillowContrast", p=0.3, factor_interval=(0.2, 50.)),
        dict(type="PillowBrightness", p=0.5, factor_interval=(0.1, 6.0)),
        dict(type="PillowColor", p=0.3, factor_interval=(0., 20.))]
MIX = [dict(type="RandomHSV", h_ratio=0.2, s_ratio=0.5, v_ratio=0.5, prob=1.0),
       dict(type="RandomNoise", noise_ratio=0.1, prob=1.0),
       dict(type="RandomSmooth", max_kernel_size=7, prob=1.0)]
ASSIGNER = dict(type="LabelAssignment",
                anchor_generator_cfg=dict(type="AnchorGenerator", ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                          strides=[8, 16, 32, 64, 128]),
                neg_threshold=0.2, positive_num=10, adapt_positive_num=False, balance_sample=True)
DM = dict(gdt=dict(type="GenerateDistanceMap", with_gt_mask=False, distance_transform="gdt", edge_mode="sobel"),
          mbd=dict(type="GenerateDistanceMap", with_gt_mask=False, distance_transform="mbd"),
          mask=dict(type="GenerateDistanceMap"))


def train_pipeline(background_dir, dm, mix=False, bg_prob=0.3, cosy_p=0.8):
    """the r50_ycbv_pbr train pipeline (mix: the mixpbr stages in place of CosyPoseAug) with the given GenerateDistanceMap"""
    return [
        dict(type="LoadImageFromFile"),
        dict(type="LoadAnnotations", with_bbox=True, with_bop_mask=True),
        dict(type="Resize", img_scale=(640, 480), keep_ratio=True),
        dict(type="RandomBackground", background_dir=background_dir, prob=bg_prob),
        *(MIX if mix else [dict(type="CosyPoseAug", p=cosy_p, pipelines=COSY)]),
        dict(type="RandomFlip", flip_ratio=0.5),
        DM[dm],
        ASSIGNER,
        dict(type="Normalize", **NORM),
        dict(type="Pad", size_divisor=16),
        dict(type="DefaultFormatBundle"),
        dict(type="Collect", keys=["img", "gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight"]),
    ]


def boxes_on_borders(rs, H, W, n):
    """random boxes plus boxes on every border, in every corner and below small_object_size (clipped like Resize does)"""
    x0, y0 = rs.uniform(0, W - 40, n), rs.uniform(0, H - 40, n)
    b = np.stack([x0, y0, x0 + rs.uniform(2, W / 2, n), y0 + rs.uniform(2, H / 2, n)], axis=1)
    fixed = [[0, 100.5, 90.2, 260.7], [W - 120.3, 50.1, W, 300.9], [200.4, 0, 420.6, 130.2], [150.2, H - 99.6, 333.3, H],
             [0, 0, 150.7, 140.1], [W - 200.5, 0, W, 99.9], [0, H - 150.2, 80.8, H], [W - 77.7, H - 210.1, W, H],
             [0, 0, W, H], [300.2, 200.9, 320.1, 225.5], [10.9, 10.1, 12.2, 40.0], [W - 9.5, H - 30.5, W, H]]
    b = np.concatenate([b, np.array(fixed)]).astype(np.float32)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, W)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, H)
    return b
