"""Image side of the BOP data pipeline, host parts: the NumPy restatement of the CosyPose Pillow stages against live Pillow,
the per-sample random draws against a literal restatement of the reference's stage order, pipeline / loader construction
from the RADet config dicts, and the group sampler."""
import os
import random
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _augment_ref as R  # noqa: E402

PIL = pytest.importorskip("PIL")
from PIL import Image, ImageEnhance, ImageFilter  # noqa: E402

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
COSY = [dict(type="PillowBlur", p=1., factor_interval=(1, 3)),
        dict(type="PillowSharpness", p=0.3, factor_interval=(0., 50.)),
        dict(type="PillowContrast", p=0.3, factor_interval=(0.2, 50.)),
        dict(type="PillowBrightness", p=0.5, factor_interval=(0.1, 6.0)),
        dict(type="PillowColor", p=0.3, factor_interval=(0., 20.))]


def train_pipeline(background_dir):
    return [
        dict(type="LoadImageFromFile"),
        dict(type="LoadAnnotations", with_bbox=True, with_bop_mask=True),
        dict(type="Resize", img_scale=(640, 480), keep_ratio=True),
        dict(type="RandomBackground", background_dir=background_dir, prob=0.3),
        dict(type="CosyPoseAug", p=0.8, pipelines=COSY),
        dict(type="RandomFlip", flip_ratio=0.5),
        dict(type="GenerateDistanceMap"),
        dict(type="LabelAssignment",
             anchor_generator_cfg=dict(type="AnchorGenerator", ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                       strides=[8, 16, 32, 64, 128]),
             neg_threshold=0.2, positive_num=10, adapt_positive_num=False, balance_sample=True),
        dict(type="Normalize", **NORM),
        dict(type="Pad", size_divisor=16),
        dict(type="DefaultFormatBundle"),
        dict(type="Collect", keys=["img", "gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight"]),
    ]


TEST_PIPELINE = [
    dict(type="LoadImageFromFile"),
    dict(type="MultiScaleFlipAug", img_scale=(640, 480), flip=False, transforms=[
        dict(type="Resize", keep_ratio=True),
        dict(type="RandomFlip"),
        dict(type="Normalize", **NORM),
        dict(type="Pad", size_divisor=32),
        dict(type="ImageToTensor", keys=["img"]),
        dict(type="Collect", keys=["img"])]),
]

SIZES = [(1, 1), (1, 3), (3, 1), (2, 2), (3, 3), (2, 7), (7, 2), (5, 13), (37, 61), (64, 97)]
FACTORS = [0.0, 0.37, 1.0, float(np.nextafter(np.float32(1), np.float32(2))), 1.5, 6.0, 20.0, 50.0]


@pytest.mark.parametrize("hw", SIZES)
def test_restated_pillow_ops_equal_pillow(hw):
    rng = np.random.RandomState(hw[0] * 131 + hw[1])
    img = rng.randint(0, 256, (*hw, 3)).astype(np.uint8)
    im = Image.fromarray(img)
    for k in (1, 2, 3):
        np.testing.assert_array_equal(R.gaussian_blur(img, k), np.asarray(im.filter(ImageFilter.GaussianBlur(k))), err_msg=f"blur {k}")
    for f in FACTORS:
        for name, fn in (("Sharpness", R.sharpness), ("Contrast", R.contrast), ("Brightness", R.brightness), ("Color", R.color)):
            np.testing.assert_array_equal(fn(img, f), np.asarray(getattr(ImageEnhance, name)(im).enhance(f)), err_msg=f"{name} {f}")


def test_restated_chain_equals_pillow_chain():
    rng = np.random.RandomState(7)
    img = rng.randint(0, 256, (45, 71, 3)).astype(np.uint8)
    im = Image.fromarray(img).filter(ImageFilter.GaussianBlur(2))
    for name, f in (("Sharpness", 12.5), ("Contrast", 0.7), ("Brightness", 2.25), ("Color", 3.0)):
        im = getattr(ImageEnhance, name)(im).enhance(f)
    np.testing.assert_array_equal(R.cosypose(img, 2, 12.5, 0.7, 2.25, 3.0), np.asarray(im))


def test_package_blur_params_equal_restatement():
    from radet_amd.datasets.loading import blur_params
    for k in (1, 2, 3):
        assert blur_params(k) == R.blur_params(k)


def test_merge_and_normalize_restatements():
    rng = np.random.RandomState(1)
    img = rng.randint(0, 256, (6, 9, 3)).astype(np.uint8)
    bg = rng.randint(0, 256, (6, 9, 3)).astype(np.uint8)
    masks = np.zeros((2, 6, 9), np.uint8)
    masks[0, 1:3, 2:5] = 1
    masks[1, 4:, 6:] = 2                                  # not 1: background
    fg = np.zeros((6, 9), bool)
    fg[1:3, 2:5] = True
    np.testing.assert_array_equal(R.merge_background(img, bg, masks), np.where(fg[..., None], img, bg))
    x = R.normalize(img, NORM["mean"], NORM["std"])
    assert x.shape == (3, 6, 9) and x.dtype == np.float32
    assert x[0, 0, 0] == (np.float32(img[0, 0, 2]) - np.float32(123.675)) * np.float32(1 / np.float64(np.float32(58.395)))


def _stages(bg_dir):
    from radet_amd.utils import build_from_cfg
    from radet_amd.datasets import PIPELINES
    return (build_from_cfg(dict(type="RandomBackground", background_dir=bg_dir, prob=0.5), PIPELINES),
            build_from_cfg(dict(type="CosyPoseAug", p=0.6, pipelines=COSY), PIPELINES),
            build_from_cfg(dict(type="RandomFlip", flip_ratio=0.5), PIPELINES))


def _reference_draws(rnd, nprnd, bgs):
    """the reference's order of draws, restated literally: RandomBackground, CosyPoseAug (+ its five stages), RandomFlip"""
    out = {}
    if not rnd.random() > 0.5:
        out["background"] = rnd.choice(bgs)
    if not rnd.random() > 0.6:
        out["aug_blur"] = rnd.randint(1, 3)
        for key, (p, iv) in zip(("aug_sharpness", "aug_contrast", "aug_brightness", "aug_color"),
                                ((0.3, (0., 50.)), (0.3, (0.2, 50.)), (0.5, (0.1, 6.0)), (0.3, (0., 20.)))):
            if rnd.random() <= p:
                out[key] = rnd.uniform(*iv)
    out["flip"] = nprnd.choice(["horizontal", None], p=[0.5, 0.5]) is not None
    return out


def test_draw_plan_consumes_generators_like_the_reference(tmp_path, monkeypatch):
    from radet_amd.datasets import loading
    for i in range(3):
        Image.fromarray(np.full((4, 5, 3), 40 * i, np.uint8)).save(tmp_path / f"b{i}.png")
    decoded = []
    monkeypatch.setattr(loading, "decode_bgr", lambda p: decoded.append(p) or np.zeros((4, 5, 3), np.uint8))
    stages = _stages(str(tmp_path))
    bgs = stages[0].background_images
    assert bgs == sorted(bgs)
    a, b = random.Random(5), random.Random(5)
    na, nb = np.random.RandomState(5), np.random.RandomState(5)
    seen = set()
    for _ in range(200):
        s = dict(img_shape=(4, 5, 3), bbox_fields=[])
        for st in stages:
            st.plan(s, a, na)
        ref = _reference_draws(b, nb, bgs)
        if "background" in ref:
            assert decoded.pop() == ref.pop("background")
        got = {k: v for k, v in s.items() if k.startswith("aug_") or k == "flip"}
        assert got == ref
        seen.update(ref)
        seen.add(("flip", ref["flip"]))
        assert a.getstate() == b.getstate()
        sa, sb = na.get_state(), nb.get_state()
        assert sa[2] == sb[2] and np.array_equal(sa[1], sb[1])
    assert seen >= {"aug_blur", "aug_sharpness", "aug_contrast", "aug_brightness", "aug_color", ("flip", True), ("flip", False)}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=8, seed=3)


def test_build_dataset_and_loader_from_radet_configs(tree):
    from radet_amd.datasets import build_dataloader, build_dataset
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.datasets.loading import ImagePipeline
    train = build_dataset(dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"],
                               seg_prefix=tree["seg_prefix"], pipeline=train_pipeline(tree["background_dir"])))
    test = build_dataset(dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"],
                              pipeline=TEST_PIPELINE, test_mode=True))
    assert isinstance(train.pipeline, ImagePipeline) and isinstance(test.pipeline, ImagePipeline)
    assert len(train) == 8 and len(test) == 8
    loader = build_dataloader(train, samples_per_gpu=4, workers=64, seed=0)
    assert loader.workers == 16 and len(loader) == 2
    assert len(build_dataloader(test, samples_per_gpu=4, workers=2, seed=0, shuffle=False)) == 2
    # the host part of a sample: decoded BGR image, boxes / labels / masks of the annotation file, the resize plan
    s = train.plan_sample(0, *sample_generators(0, 0, 0))
    ann = train.get_ann_info(0)
    assert s["img"].shape == (480, 640, 3) and s["img"].dtype == np.uint8
    assert s["gt_masks"].shape == (len(ann["labels"]), 480, 640)
    b = ann["bboxes"].copy()
    if s["flip"]:
        b = np.stack([640 - b[:, 2], b[:, 1], 640 - b[:, 0], b[:, 3]], axis=1)
    np.testing.assert_array_equal(s["gt_bboxes"], b)
    np.testing.assert_array_equal(s["gt_labels"], ann["labels"])
    assert s["pad_shape"] == (480, 640, 3) and s["img_shape"] == (480, 640, 3)
    t = test.plan_sample(0, *sample_generators(0, 0, 0))
    assert t["pad_shape"] == (480, 640, 3) and t["flip"] is False


def test_unused_options_are_refused(tree):
    from radet_amd.datasets import build_dataset
    bad = [dict(TEST_PIPELINE[0]), dict(TEST_PIPELINE[1], flip=True)]
    with pytest.raises(NotImplementedError):
        build_dataset(dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"], pipeline=bad,
                           test_mode=True))
    with pytest.raises(NotImplementedError):
        build_dataset(dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"], test_mode=True,
                           pipeline=[dict(type="LoadImageFromFile", to_float32=True), dict(type="Normalize", **NORM),
                                     dict(type="Collect", keys=["img"])]))


def test_group_sampler_shards():
    from radet_amd.datasets.loader import group_batches
    flag = np.array([0, 1] * 12 + [1] * 8, np.uint8)        # 12 portrait + 20 landscape
    world, bs = 2, 2
    shards = [group_batches(flag, bs, seed=9, epoch=3, rank=r, world=world) for r in range(world)]
    flat = [i for sh in shards for b in sh for i in b]
    assert sorted(flat) == list(range(len(flag)))              # disjoint and covering (no padding needed here)
    for sh in shards:
        assert len(sh) == len(shards[0])
        for b in sh:
            assert len(b) == bs and len(set(flag[b])) == 1
    assert shards == [group_batches(flag, bs, seed=9, epoch=3, rank=r, world=world) for r in range(world)]
    assert shards != [group_batches(flag, bs, seed=9, epoch=4, rank=r, world=world) for r in range(world)]
    odd = np.array([0] * 5 + [1] * 3, np.uint8)                # groups padded with repeats of their own members
    b = [x for r in range(2) for x in group_batches(odd, 2, seed=1, epoch=0, rank=r, world=2)]
    assert set(i for x in b for i in x) == set(range(8)) and all(len(set(odd[x])) == 1 for x in b)
