"""Scale-jitter training, host side: the planning of Resize (random scales) + RandomCrop against the reference's stages run
under the same seeds (tests/golden/scale_jitter.npz, made by tests/golden/gen_scale_jitter.py), Pad(size=), the refusals,
the jitter configs and the re-draw of a sample whose crop holds no box."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _jitter_cfg import jitter_train_cfg  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden", "scale_jitter.npz")
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def _args(d):
    """the tuples that JSON made lists of"""
    d = dict(d)
    for k in ("img_scale", "crop_size", "ratio_range"):
        if k in d:
            d[k] = [tuple(v) for v in d[k]] if isinstance(d[k][0], list) else tuple(d[k])
    return d


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    g["cases"] = [(_args(a), _args(b)) for a, b in json.loads(str(g["cases"]))]
    return g


def test_fixture_holds_the_edge_cases(gold):
    g = gold
    n = len(g["none"])
    assert n == len(g["cases"]) * 8 and g["none"].sum() >= 1
    assert ((g["n_boxes"] < len(g["boxes"])) & ~g["none"]).any()                                   # a dropped box
    absolute = np.array([g["cases"][c][1].get("crop_type", "absolute") == "absolute" for c in g["case"]])
    want = np.array([g["cases"][c][1]["crop_size"] for c in g["case"]], np.float64)
    assert (absolute & ((want[:, 0] > g["resized_hw"][:, 0]) | (want[:, 1] > g["resized_hw"][:, 1]))).any()   # crop > image
    ratio = np.array(["ratio_range" in g["cases"][c][0] for c in g["case"]])
    assert (ratio & (g["scale"][:, 0] < 80)).any()                                                  # a ratio below 1
    y0, x0, ch, cw = g["window"].T
    assert ((y0 + ch == g["resized_hw"][:, 0]) & (x0 + cw == g["resized_hw"][:, 1]) & ((y0 > 0) | (x0 > 0))).any()   # the corner
    modes = {(a.get("multiscale_mode"), "ratio_range" in a, isinstance(a["img_scale"], list)) for a, _ in g["cases"]}
    assert {("range", False, True), ("value", False, True), (None, True, False)} <= modes
    assert {b.get("crop_type", "absolute") for _, b in g["cases"]} == {"absolute", "absolute_range", "relative", "relative_range"}
    assert {b.get("bbox_clip_border", True) for _, b in g["cases"]} == {True, False}


@pytest.mark.parametrize("masks_as", ["bitmap", "runs"])
def test_planning_reproduces_the_reference(gold, masks_as):
    from radet_amd.datasets.loading import RandomCrop, Resize
    g = gold
    H, W = (int(v) for v in g["src_hw"])
    ob = oi = 0
    for n in range(len(g["none"])):
        ra, ca = g["cases"][g["case"][n]]
        rs = np.random.RandomState(int(g["seed"][n]))
        s = dict(img=np.zeros((H, W, 3), np.uint8), img_shape=(H, W, 3), bbox_fields=["gt_bboxes_ignore", "gt_bboxes"],
                 mask_fields=["gt_masks"], gt_bboxes=g["boxes"].copy(), gt_bboxes_ignore=g["ignore"].copy(),
                 gt_labels=g["labels"].copy())
        if masks_as == "bitmap":                 # mask k is filled with k: the surviving rows name themselves
            s["gt_masks"] = np.arange(4, dtype=np.uint8)[:, None, None] * np.ones((1, H, W), np.uint8)
        else:
            s["gt_masks_rle"] = ([0, 1, 2, 3], (H, W))
        Resize(**ra).plan(s, None, rs)
        what = f"sample {n}: {ra} {ca} seed {g['seed'][n]}"
        assert tuple(s["scale"]) == tuple(g["scale"][n]), what
        assert (-1 if s["scale_idx"] is None else s["scale_idx"]) == g["scale_idx"][n], what
        assert tuple(s["resize_hw"]) == tuple(g["resized_hw"][n]) and s["img_shape"] == (*g["resized_hw"][n], 3), what
        assert s["scale_factor"].dtype == np.float32 and np.array_equal(s["scale_factor"], g["scale_factor"][n]), what
        res = RandomCrop(**ca).plan(s, None, rs)
        assert rs.random_sample() == g["next"][n], what                  # the generator stands where the reference's does
        nb, ni = int(g["n_boxes"][n]), int(g["n_ignore"][n])
        assert (res is False) == bool(g["none"][n]), what
        if res is not False:
            assert tuple(s["crop_window"]) == tuple(g["window"][n]) and tuple(s["resize_hw"]) == tuple(g["resized_hw"][n]), what
            assert tuple(s["img_shape"]) == tuple(g["img_shape"][n]), what
            for key, want in (("gt_bboxes", g["gt_bboxes"][ob:ob + nb]), ("gt_bboxes_ignore", g["gt_bboxes_ignore"][oi:oi + ni]),
                              ("gt_labels", g["gt_labels"][ob:ob + nb])):
                assert s[key].dtype == want.dtype and np.array_equal(s[key], want), f"{what}: {key}"
            kept = s["gt_masks"][:, 0, 0] if masks_as == "bitmap" else s["gt_masks_rle"][0]
            assert list(kept) == list(g["kept"][ob:ob + nb]), what
            if masks_as == "bitmap":
                assert s["gt_masks"].shape == (nb, H, W)                 # planned only: rows dropped, no pixel touched
        ob, oi = ob + nb, oi + ni
    assert ob == len(g["gt_bboxes"]) and oi == len(g["gt_bboxes_ignore"])


def test_pad_size_metas():
    from radet_amd.datasets.loading import Pad
    s = dict(img_shape=(300, 640, 3))
    Pad(size=(480, 640)).plan(s, None, None)
    assert s["pad_shape"] == (480, 640, 3) and s["pad_fixed_size"] == (480, 640) and s["pad_size_divisor"] is None
    assert s["img_shape"] == (300, 640, 3)
    s = dict(img_shape=(300, 630, 3))
    Pad(size_divisor=32).plan(s, None, None)
    assert s["pad_shape"] == (320, 640, 3) and s["pad_fixed_size"] is None and s["pad_size_divisor"] == 32
    for shape in ((481, 640, 3), (480, 641, 3)):
        with pytest.raises(ValueError):
            Pad(size=(480, 640)).plan(dict(img_shape=shape), None, None)
    with pytest.raises(ValueError):
        Pad()
    with pytest.raises(ValueError):
        Pad(size=(480, 640), size_divisor=32)


def _pipeline(*middle, first="LoadImageFromFile"):
    return [dict(type=first), *middle, dict(type="Normalize", **NORM), dict(type="Pad", size=(480, 640)),
            dict(type="Collect", keys=["img"])]


def test_refusals():
    from radet_amd.datasets.loading import ImagePipeline, Pad, RandomCrop, Resize
    resize, crop = dict(type="Resize", img_scale=(640, 480), ratio_range=(0.6, 1.6)), dict(type="RandomCrop", crop_size=(480, 640))
    ImagePipeline(_pipeline(resize, crop))
    ImagePipeline(_pipeline(crop))                                       # (no Resize: the crop of the image as loaded)
    # wrong position: the message names the accepted one
    for middle in ((crop, resize), (resize, dict(type="RandomFlip", flip_ratio=0.5), crop),
                   (dict(type="LoadAnnotations"), resize, dict(type="RandomHSV", h_ratio=0.1, s_ratio=0.1, v_ratio=0.1), crop)):
        with pytest.raises(NotImplementedError, match="directly after Resize"):
            ImagePipeline(_pipeline(*middle))
    with pytest.raises(NotImplementedError, match="LoadImageFromWebcam"):
        ImagePipeline(_pipeline(resize, crop, first="LoadImageFromWebcam"))
    with pytest.raises(NotImplementedError):
        Resize(img_scale=(640, 480), override=True)
    with pytest.raises(NotImplementedError):
        Resize(img_scale=(640, 480), backend="pillow")
    with pytest.raises(NotImplementedError):
        Pad(size=(480, 640), pad_val=1)
    with pytest.raises(NotImplementedError):
        Pad(size_divisor=32, pad_val=114)
    with pytest.raises(ValueError):
        RandomCrop(crop_size=(480, 640), crop_type="centre")
    with pytest.raises(ValueError):
        RandomCrop(crop_size=(0.5, 0.5))
    with pytest.raises(ValueError):
        Resize(img_scale=[(640, 480), (800, 600)], ratio_range=(0.5, 2.0))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL writes and decodes the generated JPEG / PNG files")
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=8, seed=3)


def test_jitter_configs_build(tree):
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.datasets.loading import ImagePipeline
    from radet_amd.utils import Config
    base = Config.fromfile(os.path.join(REPO, "configs", "base", "datasets", "bop_detection_jitter.py"))
    cfg, train = jitter_train_cfg(tree)
    plain = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    assert cfg.model == plain.model and cfg.train_cfg == plain.train_cfg and cfg.test_cfg == plain.test_cfg
    assert cfg.data.train.pipeline == base.data.train.pipeline == base.train_pipeline
    stages = {t["type"]: t for t in cfg.data.train.pipeline}
    assert stages["Resize"]["img_scale"] == (640, 480) and stages["Resize"]["ratio_range"] == (0.6, 1.6) and stages["Resize"]["keep_ratio"]
    assert stages["RandomCrop"]["crop_size"] == (480, 640) and stages["Pad"]["size"] == (480, 640)
    ds = build_dataset(train)
    assert isinstance(ds.pipeline, ImagePipeline) and len(ds) == 8
    kinds = set()
    for i in range(8):
        s = ds.plan_sample(i, *sample_generators(0, 0, i))
        y0, x0, ch, cw = s["crop_window"]
        Hr, Wr = s["resize_hw"]
        assert s["pad_shape"] == (480, 640, 3) and s["img_shape"] == (ch, cw, 3) == (min(Hr, 480), min(Wr, 640), 3)
        assert 0 <= y0 <= Hr - ch and 0 <= x0 <= Wr - cw and len(s["gt_bboxes"]) == len(s["gt_labels"]) == len(s["gt_masks"]) > 0
        assert s["gt_masks"].shape[1:] == (480, 640)                    # the source masks: their window is cut on the device
        kinds.add("up" if Hr > 480 else "down")
    assert kinds == {"up", "down"}


def test_dataset_redraws_on_an_empty_crop(tree):
    """a crop of 4 x 4 pixels seldom holds a box: plan_sample (the loader's path) and __getitem__ take another image"""
    import random
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    _, train = jitter_train_cfg(tree)
    train["pipeline"] = [dict(t, crop_size=(4, 4)) if t["type"] == "RandomCrop" else t for t in train["pipeline"]]
    ds = build_dataset(train)
    plan, outcomes = ds.pipeline.plan, []

    def counted(results, rnd, nprnd):
        outcomes.append(plan(results, rnd, nprnd))
        return outcomes[-1]
    ds.pipeline.plan = counted
    first = [ds.plan_sample(i, *sample_generators(1, 0, i)) for i in range(8)]
    for s in first:
        assert s is not None and len(s["gt_bboxes"]) > 0 and s["img_shape"] == (4, 4, 3)
    assert sum(o is None for o in outcomes) >= 1 and sum(o is not None for o in outcomes) == 8
    # the same seeds again: the same samples (the re-draw uses the sample's own generators)
    again = [ds.plan_sample(i, *sample_generators(1, 0, i)) for i in range(8)]
    assert [(a["filename"], a["crop_window"]) for a in again] == [(a["filename"], a["crop_window"]) for a in first]
    # __getitem__ on the global generators; the device part is not what is tested here
    ds.pipeline.run = lambda planned, collate=False: planned
    del outcomes[:]
    random.seed(0)
    np.random.seed(0)
    got = [ds[i] for i in range(8)]
    assert all(s is not None and len(s["gt_bboxes"]) > 0 for s in got) and sum(o is None for o in outcomes) >= 1
