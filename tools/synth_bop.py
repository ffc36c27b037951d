"""Writes a small synthetic BOP tree from a seed (used by tests and tools/bench_pipeline.py):

    <root>/train_pbr/000000/rgb/000000.jpg ...                   images (JPEG)
    <root>/train_pbr/000000/mask_visib/000000_000000.png ...     visible masks (PNG, 0 / 255)
    <root>/detector_annotations/train_pbr.json                   COCO-style annotations, as tools/bop_to_coco.py writes them
    <root>/train_pbr/000000/scene_gt.json, scene_gt_info.json    the BOP ground truth tools/bop_to_coco.py reads
    <root>/image_lists/train_pbr.txt                             the image list it reads
    <root>/backgrounds/*.jpg                                     background images of several sizes
"""
import json
import os

import numpy as np

YCBV_NAMES = ("master_chef_can", "cracker_box", "sugar_box", "tomato_soup_can", "mustard_bottle", "tuna_fish_can",
              "pudding_box", "gelatin_box", "potted_meat_can", "banana", "pitcher_base", "bleach_cleanser", "bowl", "mug",
              "power_drill", "wood_block", "scissors", "large_marker", "large_clamp", "extra_large_clamp", "foam_brick")


def _image(rng, h, w):
    """smooth colour gradients plus noise: JPEG-friendly, but every stage changes it"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([np.sin(x / rng.uniform(20, 80) + rng.uniform(0, 6)) * 90 + 128,
                     np.cos(y / rng.uniform(20, 80) + rng.uniform(0, 6)) * 90 + 128,
                     np.sin((x + y) / rng.uniform(30, 90)) * 90 + 128], axis=2)
    return np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)


def write_tree(root, n_frames=8, objects=(3, 6), size=(640, 480), n_backgrounds=3, seed=0, quality=90, sizes=None,
               empty_frames=(), small_frames=()):
    """sizes: (w, h) per frame, cycled (default: `size` for all); empty_frames: frames without objects; small_frames: frames
    whose objects are 8 .. 20 pixels wide and high (below GenerateDistanceMap's small_object_size)"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    scene = os.path.join(root, "train_pbr", "000000")
    os.makedirs(os.path.join(scene, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(scene, "mask_visib"), exist_ok=True)
    images, anns = [], []
    for f in range(n_frames):
        w, h = sizes[f % len(sizes)] if sizes else size
        Image.fromarray(_image(rng, h, w)).save(os.path.join(scene, "rgb", f"{f:06d}.jpg"), quality=quality)
        images.append(dict(id=f + 1, file_name=f"000000/rgb/{f:06d}.jpg", width=w, height=h))
        for i in range(0 if f in empty_frames else rng.randint(objects[0], objects[1] + 1)):
            bw, bh = (rng.randint(8, 21), rng.randint(8, 21)) if f in small_frames else \
                (rng.randint(w // 10, w // 3), rng.randint(h // 10, h // 3))
            x0, y0 = rng.randint(0, w - bw), rng.randint(0, h - bh)
            yy, xx = np.mgrid[0:h, 0:w]
            inside = ((xx - x0 - bw / 2) / (bw / 2)) ** 2 + ((yy - y0 - bh / 2) / (bh / 2)) ** 2 <= 1.0
            mask = np.where(inside, 255, 0).astype(np.uint8)
            Image.fromarray(mask).save(os.path.join(scene, "mask_visib", f"{f:06d}_{i:06d}.png"))
            ys, xs = np.nonzero(inside)
            box = [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]
            anns.append(dict(id=len(anns) + 1, image_id=f + 1, category_id=int(rng.randint(1, 22)), bbox=box,
                             area=box[2] * box[3], iscrowd=0, ignore=False, visib_fract=float(rng.uniform(0.3, 1.0))))
    cats = [dict(id=i + 1, name=n) for i, n in enumerate(YCBV_NAMES)]
    os.makedirs(os.path.join(root, "detector_annotations"), exist_ok=True)
    ann_file = os.path.join(root, "detector_annotations", "train_pbr.json")
    with open(ann_file, "w") as fh:
        json.dump(dict(images=images, annotations=anns, categories=cats), fh)
    # the same records as BOP ground truth (scene_gt / scene_gt_info) and the image list, for the converter
    gt, info = {}, {}
    for a in anns:
        f = str(a["image_id"] - 1)
        gt.setdefault(f, []).append(dict(obj_id=a["category_id"], cam_R_m2c=[1, 0, 0, 0, 1, 0, 0, 0, 1], cam_t_m2c=[0, 0, 500]))
        info.setdefault(f, []).append(dict(bbox_obj=a["bbox"], bbox_visib=a["bbox"], visib_fract=a["visib_fract"]))
    for f in range(n_frames):
        gt.setdefault(str(f), [])
        info.setdefault(str(f), [])
    order = sorted(info, key=int)
    with open(os.path.join(scene, "scene_gt.json"), "w") as fh:
        json.dump({k: gt[k] for k in order}, fh)
    with open(os.path.join(scene, "scene_gt_info.json"), "w") as fh:
        json.dump({k: info[k] for k in order}, fh)
    os.makedirs(os.path.join(root, "image_lists"), exist_ok=True)
    image_list = os.path.join(root, "image_lists", "train_pbr.txt")
    with open(image_list, "w") as fh:
        fh.write("".join(im["file_name"] + "\n" for im in images))
    bg_dir = os.path.join(root, "backgrounds")
    os.makedirs(bg_dir, exist_ok=True)
    for b in range(n_backgrounds):
        bw, bh = [(320, 240), (700, 500), (640, 480), (500, 375)][b % 4]
        Image.fromarray(_image(rng, bh, bw)).save(os.path.join(bg_dir, f"bg{b:03d}.jpg"), quality=quality)
    return dict(ann_file=ann_file, img_prefix=os.path.join(root, "train_pbr"), seg_prefix=os.path.join(root, "train_pbr"),
                background_dir=bg_dir, image_list=image_list)


def pipelines(background_dir, bg_prob=0.3, cosy_p=0.8):
    """the RADet r50_ycbv_pbr train / test pipelines as config dicts"""
    norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
    train = [
        dict(type="LoadImageFromFile"),
        dict(type="LoadAnnotations", with_bbox=True, with_bop_mask=True),
        dict(type="Resize", img_scale=(640, 480), keep_ratio=True),
        dict(type="RandomBackground", background_dir=background_dir, prob=bg_prob),
        dict(type="CosyPoseAug", p=cosy_p, pipelines=[
            dict(type="PillowBlur", p=1., factor_interval=(1, 3)),
            dict(type="PillowSharpness", p=0.3, factor_interval=(0., 50.)),
            dict(type="PillowContrast", p=0.3, factor_interval=(0.2, 50.)),
            dict(type="PillowBrightness", p=0.5, factor_interval=(0.1, 6.0)),
            dict(type="PillowColor", p=0.3, factor_interval=(0., 20.))]),
        dict(type="RandomFlip", flip_ratio=0.5),
        dict(type="GenerateDistanceMap"),
        dict(type="LabelAssignment",
             anchor_generator_cfg=dict(type="AnchorGenerator", ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                       strides=[8, 16, 32, 64, 128]),
             neg_threshold=0.2, positive_num=10, adapt_positive_num=False, balance_sample=True),
        dict(type="Normalize", **norm),
        dict(type="Pad", size_divisor=16),
        dict(type="DefaultFormatBundle"),
        dict(type="Collect", keys=["img", "gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight"]),
    ]
    test = [
        dict(type="LoadImageFromFile"),
        dict(type="MultiScaleFlipAug", img_scale=(640, 480), flip=False, transforms=[
            dict(type="Resize", keep_ratio=True),
            dict(type="RandomFlip"),
            dict(type="Normalize", **norm),
            dict(type="Pad", size_divisor=32),
            dict(type="ImageToTensor", keys=["img"]),
            dict(type="Collect", keys=["img"])]),
    ]
    return train, test
