"""Zoom augmentation, host side: the planning of Expand + MinIoURandomCrop (+ Resize) against the reference's stages run under
the same seeds (tests/golden/zoom_aug.npz, made by tests/golden/gen_zoom_aug.py), the source window they leave behind, the
refusals and the zoom configs."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _zoom_cfg import zoom_train_cfg  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden", "zoom_aug.npz")
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def _args(d):
    """the tuples that JSON made lists of"""
    return None if d is None else {k: tuple(v) if isinstance(v, list) else v for k, v in d.items()}


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    g["cases"] = [(_args(a), _args(b), c) for a, b, c in json.loads(str(g["cases"]))]
    g["resizes"] = [_args(r) for r in json.loads(str(g["resizes"]))]
    return g


def test_fixture_holds_the_edge_cases(gold):
    g = gold
    H, W = (int(v) for v in g["src_hw"])
    n = len(g["seed"])
    per_case = np.bincount(g["case"])
    assert len(per_case) == len(g["cases"]) and (per_case >= 2 * 8).all()          # >= 8 seeds, both Resize forms
    has_e = np.array([g["cases"][c][0] is not None for c in g["case"]])
    has_c = np.array([g["cases"][c][1] is not None for c in g["case"]])
    with_boxes = np.array([g["cases"][c][2] for c in g["case"]])
    assert (has_e & ~g["applied"]).any() and g["applied"].any()                     # Expand skipped, Expand applied
    assert (g["mode"] == 1).any() and (g["modes"] > 1).any()                        # mode 1; a mode abandoned after 50 trials
    assert (with_boxes & (g["n_boxes"] < len(g["boxes"]))).any()                    # a box dropped
    assert (with_boxes & (g["n_boxes"] == 0) & (g["n_ignore"] > 0)).any()           # gt emptied, an ignore box survives
    x0, y0, x1, y1 = g["patch"].T
    cropped = has_c & (g["mode"] != 1)
    assert (cropped & g["applied"] & ((x0 < g["left"]) | (y0 < g["top"]) | (x1 > g["left"] + W) | (y1 > g["top"] + H))).any()   # fill
    assert (~with_boxes & cropped).any() and (has_e & has_c).any()
    e_args = [a for a, _, _ in g["cases"] if a is not None]
    assert {a["prob"] for a in e_args} >= {0, 0.5, 1} and {a["to_rgb"] for a in e_args} == {True, False}
    assert any(len(set(a["mean"])) == 1 for a in e_args) and any(len(set(a["mean"])) == 3 for a in e_args)
    c_args = [b for a, b, _ in g["cases"] if b is not None and a is None]
    assert dict() in c_args and dict(min_ious=(0.9,)) in c_args and dict(bbox_clip_border=False) in c_args
    assert dict(min_crop_size=0.9) in c_args
    assert {r["keep_ratio"] for r in g["resizes"]} == {True, False}
    assert n == len(g["next"])


@pytest.mark.parametrize("masks_as", ["bitmap", "runs"])
def test_planning_reproduces_the_reference(gold, masks_as):
    from radet_amd.datasets.loading import Expand, MinIoURandomCrop, Resize
    g = gold
    H, W = (int(v) for v in g["src_hw"])
    ob = oi = zb = zi = 0
    for n in range(len(g["seed"])):
        ea, ca, with_boxes = g["cases"][g["case"][n]]
        ra = g["resizes"][g["resize"][n]]
        rs = np.random.RandomState(int(g["seed"][n]))
        nb0 = len(g["boxes"]) if with_boxes else 0
        s = dict(img=np.zeros((H, W, 3), np.uint8), img_shape=(H, W, 3), bbox_fields=["gt_bboxes_ignore", "gt_bboxes"],
                 mask_fields=["gt_masks"], gt_bboxes=g["boxes"][:nb0].copy(), gt_bboxes_ignore=g["ignore"][:nb0 and 2].copy(),
                 gt_labels=g["labels"][:nb0].copy())
        if masks_as == "bitmap":                 # mask k is filled with k: the surviving rows name themselves
            s["gt_masks"] = np.arange(nb0, dtype=np.uint8)[:, None, None] * np.ones((1, H, W), np.uint8)
        else:
            s["gt_masks_rle"] = (list(range(nb0)), (H, W))
        what = f"sample {n}: {ea} {ca} {ra} seed {g['seed'][n]}"
        y0 = x0 = 0
        wh, ww = H, W
        if ea is not None:
            Expand(**ea).plan(s, None, rs)
            assert ("src_window" in s) == bool(g["applied"][n]), what
            if g["applied"][n]:
                left, top = int(g["left"][n]), int(g["top"][n])
                fill = tuple(int(v) for v in np.asarray(ea["mean"][::-1] if ea["to_rgb"] else ea["mean"]).astype(np.uint8))
                assert s["src_window"] == (-top, -left, *(int(v) for v in g["canvas"][n]), fill), what
                y0, x0, wh, ww = s["src_window"][:4]
        if ca is not None:
            MinIoURandomCrop(**ca).plan(s, None, rs)
            assert s["crop_mode"] == g["mode"][n], what
            if g["mode"][n] != 1:
                px0, py0, px1, py1 = (int(v) for v in g["patch"][n])
                assert s["crop_patch"] == (px0, py0, px1, py1), what
                y0, x0, wh, ww = y0 + py0, x0 + px0, py1 - py0, px1 - px0
                assert s["src_window"][:4] == (y0, x0, wh, ww), what
        if (wh, ww) != (H, W):
            assert s["src_window"][:4] == (y0, x0, wh, ww) and s["resize_hw"] == (wh, ww), what
        assert (wh, ww) == tuple(g["zoom_hw"][n]) and tuple(s["img_shape"]) == tuple(g["zoom_img_shape"][n]), what
        nb, ni = int(g["n_boxes"][n]), int(g["n_ignore"][n])
        for key, want in (("gt_bboxes", g["zoom_boxes"][zb:zb + nb]), ("gt_bboxes_ignore", g["zoom_ignore"][zi:zi + ni])):
            assert s[key].dtype == want.dtype and np.array_equal(s[key], want), f"{what}: {key} before Resize"
        Resize(**ra).plan(s, None, rs)
        assert rs.random_sample() == g["next"][n], what                  # the generator stands where the reference's does
        assert tuple(s["img_shape"]) == tuple(g["img_shape"][n]) and s["resize_hw"] == tuple(g["img_shape"][n][:2]), what
        assert s["scale_factor"].dtype == np.float32 and np.array_equal(s["scale_factor"], g["scale_factor"][n]), what
        for key, want in (("gt_bboxes", g["gt_bboxes"][ob:ob + nb]), ("gt_bboxes_ignore", g["gt_bboxes_ignore"][oi:oi + ni]),
                          ("gt_labels", g["gt_labels"][ob:ob + nb])):
            assert s[key].dtype == want.dtype and np.array_equal(s[key], want), f"{what}: {key}"
        kept = s["gt_masks"][:, 0, 0] if masks_as == "bitmap" else s["gt_masks_rle"][0]
        assert list(kept) == list(g["kept"][ob:ob + nb]), what
        if masks_as == "bitmap":
            assert s["gt_masks"].shape == (nb, H, W)                     # planned only: rows dropped, no pixel touched
        ob, oi, zb, zi = ob + nb, oi + ni, zb + nb, zi + ni
    assert ob == len(g["gt_bboxes"]) and oi == len(g["gt_bboxes_ignore"])


def test_patch_overlaps_is_the_references_iou():
    """float32 throughout with the union raised to eps, one patch against k boxes; no boxes -> an empty result"""
    from radet_amd.datasets.loading import patch_overlaps
    patch = np.array([10, 20, 50, 60])
    boxes = np.array([[10, 20, 50, 60], [0, 0, 5, 5], [30, 40, 70, 80], [20, 30, 20, 30]], np.float32)
    got = patch_overlaps(patch, boxes)
    f = np.float32
    inter = f(20) * f(20)
    want = np.array([1, 0, inter / (f(1600) + f(1600) - inter), 0], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert patch_overlaps(patch, boxes[:0]).shape == (0,)
    # a degenerate box against a degenerate patch: 0 / eps, not 0 / 0
    assert patch_overlaps(np.array([20, 30, 20, 30]), boxes[3:])[0] == 0


def test_resize_without_a_source_window_is_unchanged():
    from radet_amd.datasets.loading import Resize
    s = dict(img=np.zeros((60, 80, 3), np.uint8), bbox_fields=[])
    Resize(img_scale=(64, 48), keep_ratio=True).plan(s, None, None)
    assert s["resize_hw"] == (48, 64) and "src_window" not in s
    s = dict(img=np.zeros((60, 80, 3), np.uint8), bbox_fields=[], src_window=(-3, -4, 30, 80, (1, 2, 3)))
    Resize(img_scale=(64, 48), keep_ratio=True).plan(s, None, None)
    assert s["resize_hw"] == (24, 64) and s["img_shape"] == (24, 64, 3)


def _pipeline(*middle, first="LoadImageFromFile"):
    return [dict(type=first), *middle, dict(type="Normalize", **NORM), dict(type="Pad", size_divisor=32),
            dict(type="Collect", keys=["img"])]


def test_refusals():
    from radet_amd.datasets.loading import Expand, ImagePipeline
    expand, crop = dict(type="Expand", mean=NORM["mean"], ratio_range=(1, 2)), dict(type="MinIoURandomCrop")
    resize = dict(type="Resize", img_scale=(640, 480), keep_ratio=False)
    ann = dict(type="LoadAnnotations")
    for middle in ((ann, expand, crop, resize), (ann, expand, resize), (ann, crop, resize), (ann, expand, crop)):
        ImagePipeline(_pipeline(*middle))
    for stage in (expand, crop):
        with pytest.raises(NotImplementedError, match="after Resize"):
            ImagePipeline(_pipeline(ann, resize, stage))
        with pytest.raises(NotImplementedError, match="RandomCrop"):
            ImagePipeline(_pipeline(ann, stage, resize, dict(type="RandomCrop", crop_size=(480, 640))))
        with pytest.raises(NotImplementedError, match="LoadImageFromWebcam"):
            ImagePipeline(_pipeline(stage, resize, first="LoadImageFromWebcam"))
        with pytest.raises(NotImplementedError, match="MultiScaleFlipAug"):
            ImagePipeline([dict(type="LoadImageFromFile"), stage,
                           dict(type="MultiScaleFlipAug", img_scale=(640, 480), flip=False,
                                transforms=[dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", **NORM),
                                            dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]),
                                            dict(type="Collect", keys=["img"])])])
    with pytest.raises(NotImplementedError, match="Expand"):                    # the stages stand in the reference's order
        ImagePipeline(_pipeline(ann, crop, expand, resize))
    with pytest.raises(NotImplementedError):
        Expand(seg_ignore_label=255)
    with pytest.raises(NotImplementedError):
        Expand(prob=1).plan(dict(img=np.zeros((4, 4, 3), np.uint8), seg_fields=["gt_semantic_seg"]), None, np.random.RandomState(0))
    with pytest.raises(ValueError):
        Expand(mean=(300, 0, 0))
    with pytest.raises(ValueError):
        Expand(ratio_range=(0.5, 2))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL writes and decodes the generated JPEG / PNG files")
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=8, seed=3)


def test_zoom_configs_build(tree):
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.datasets.loading import ImagePipeline
    from radet_amd.utils import Config
    base = Config.fromfile(os.path.join(REPO, "configs", "base", "datasets", "bop_detection_zoom.py"))
    cfg, train = zoom_train_cfg(tree)
    plain = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    assert cfg.model == plain.model and cfg.train_cfg == plain.train_cfg and cfg.test_cfg == plain.test_cfg
    assert cfg.data.train.pipeline == base.data.train.pipeline == base.train_pipeline
    names = [t["type"] for t in cfg.data.train.pipeline]
    assert names[2:5] == ["Expand", "MinIoURandomCrop", "Resize"]
    stages = {t["type"]: t for t in cfg.data.train.pipeline}
    assert list(stages["Expand"]["mean"]) == NORM["mean"] and stages["Expand"]["to_rgb"] and stages["Expand"]["prob"] == 0.5
    assert tuple(stages["Expand"]["ratio_range"]) == (1, 2)
    assert tuple(stages["MinIoURandomCrop"]["min_ious"]) == (0.1, 0.3, 0.5, 0.7, 0.9) and stages["MinIoURandomCrop"]["min_crop_size"] == 0.3
    assert stages["Resize"]["img_scale"] == (640, 480) and not stages["Resize"]["keep_ratio"]
    ds = build_dataset(train)
    assert isinstance(ds.pipeline, ImagePipeline) and len(ds) == 8
    kinds = set()
    for epoch in range(3):
        for i in range(8):
            s = ds.plan_sample(i, *sample_generators(0, epoch, i))
            assert s["img_shape"] == s["pad_shape"] == (480, 640, 3) and s["resize_hw"] == (480, 640)    # one tensor shape
            assert len(s["gt_bboxes"]) == len(s["gt_labels"]) == len(s["gt_masks"]) > 0
            assert s["gt_masks"].shape[1:] == (480, 640)                    # the source masks: their window is cut on the device
            if "src_window" in s:
                y0, x0, h, w, fill = s["src_window"]
                assert fill in ((103, 116, 123), (0, 0, 0))                 # the mean in BGR order, truncated
                kinds.add("out" if (y0 < 0 or x0 < 0 or y0 + h > 480 or x0 + w > 640) else "in")
            else:
                kinds.add("whole")
    assert kinds == {"out", "in", "whole"}
