"""Test-time augmentation, host side: the NumPy restatement of the map-back against the reference's bbox_mapping_back
(tests/golden/tta_views.npz), MultiScaleFlipAug's view order and metas against the reference's, the descriptor rows of a
multi-view batch, and the refusals."""
import os
import random
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _tta_ref as R  # noqa: E402

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
DIRS = {0: None, 1: "horizontal", 2: "vertical", 3: "diagonal"}


def _pipe(loader, transforms=None, **msfa):
    inner = [dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", **NORM),
             dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])]
    return [dict(type=loader), dict(type="MultiScaleFlipAug", transforms=inner if transforms is None else transforms, **msfa)]


def _plan(pipeline, img):
    return pipeline.plan(dict(img=img, bbox_fields=[], mask_fields=[], seg_fields=[]), random, np.random)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(REPO, "tests", "golden", "tta_views.npz"), allow_pickle=False)


def test_map_back_restatement_equals_reference(fixture):
    f = fixture
    assert f["a_boxes"].shape[1] >= 200 and set(f["a_flip"].tolist()) == {0, 1, 2, 3}
    assert any(sf[0] != sf[1] for sf in f["a_sf"])                # (w_scale != h_scale from keep_ratio rounding)
    assert any(h % 2 and w % 2 for h, w in f["a_hw"])
    for boxes, want, hw, sf, flip in zip(f["a_boxes"], f["a_out"], f["a_hw"], f["a_sf"], f["a_flip"]):
        got = R.map_back(boxes, hw, sf, int(flip))
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(R.map_back(boxes, hw, sf, DIRS[int(flip)]), got)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_view_order_and_metas_equal_reference(fixture, k):
    from radet_amd.datasets.loading import ImagePipeline
    f = fixture
    scales = [tuple(int(v) for v in s) for s in f[f"b{k}_img_scale"]]
    dirs = [DIRS[int(c)] for c in f[f"b{k}_cfg_dir"]]
    msfa = dict(img_scale=scales if len(scales) > 1 else scales[0], flip=bool(f[f"b{k}_cfg_flip"]),
                flip_direction=dirs if len(dirs) > 1 else dirs[0])
    p = ImagePipeline(_pipe("LoadImageFromWebcam", **msfa))
    V = len(f[f"b{k}_flip"])
    assert p.views == V and p.frames
    img = np.zeros((37, 53, 3), np.uint8)
    s = _plan(p, img)
    views = s["_views"]
    assert [tuple(v["scale"]) for v in views] == [tuple(int(x) for x in sc) for sc in f[f"b{k}_scale"]]
    assert [bool(v["flip"]) for v in views] == [bool(x) for x in f[f"b{k}_flip"]]
    assert [v["flip_direction"] for v in views] == [DIRS[int(c)] for c in f[f"b{k}_dir"]]
    for key in ("scale", "flip", "flip_direction", "img_shape", "pad_shape"):
        assert s[key] == views[0][key]                            # (the sample itself is its first view)
    # each view's geometry is the single-view plan's at that scale
    for v in views:
        one = _plan(ImagePipeline(_pipe("LoadImageFromWebcam", img_scale=tuple(v["scale"]), flip=False)), img)
        assert "_views" not in one
        assert v["img_shape"] == one["img_shape"] and v["pad_shape"] == one["pad_shape"] and v["ori_shape"] == one["ori_shape"]
        assert np.array_equal(v["scale_factor"], one["scale_factor"]) and v["scale_factor"].dtype == np.float32
        assert v["resize_hw"] == one["resize_hw"]


def test_descriptor_rows_of_a_multi_view_batch():
    from radet_amd import kernels as K
    from radet_amd.datasets.loading import ImagePipeline, frame_desc_rows
    p = ImagePipeline(_pipe("LoadImageFromWebcam", img_scale=[(64, 48), (96, 80)], flip=True,
                            flip_direction=["horizontal", "vertical", "diagonal"]))
    rng = np.random.RandomState(3)
    frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (48, 64), (5, 7))]
    planned = [_plan(p, f) for f in frames]
    V, B = p.views, len(frames)
    assert V == 8
    every = [s["_views"][v] for v in range(V) for s in planned]
    hw = [s["resize_hw"] for s in every]
    flips = [K.PREP_FLIP[s["flip_direction"]] if s["flip"] else 0 for s in every]
    base = 0x7F1200003000
    rows, offs, nbytes = frame_desc_rows(frames, hw, True, base, views=V, flips=flips)
    assert rows.shape == (V * B, K.PREP_DESC_INTS) and rows.dtype == np.int32
    assert nbytes == sum(f.size for f in frames) and offs == [0, frames[0].size, frames[0].size + frames[1].size]   # each frame once
    want_flags = [0, K.PREP_FLIP_H, K.PREP_FLIP_V, K.PREP_FLIP_H | K.PREP_FLIP_V] * 2
    assert (K.PREP_FLIP_H, K.PREP_FLIP_V) == (2, 4)
    for v in range(V):
        for b, f in enumerate(frames):
            row = rows[v * B + b]
            addr = int(row[:2].view(np.uint32)[0]) | int(row[:2].view(np.uint32)[1]) << 32
            assert addr == base + offs[b]                         # the views of a frame share its address ...
            assert tuple(row[2:5]) == (3 * f.shape[1], f.shape[0], f.shape[1])     # ... its stride and its source h, w
            assert tuple(row[5:7]) == tuple(hw[v * B + b])
            assert row[7] == (K.PREP_TO_RGB | want_flags[v])
    # a single view builds the rows it built before
    one, _, _ = frame_desc_rows(frames, hw[:B], True, base)
    assert np.array_equal(one, rows[:B])


def test_refusals():
    from radet_amd import kernels as K
    from radet_amd.datasets.loading import ImagePipeline
    assert K.TTA_MAX_VIEWS == 16
    with pytest.raises(NotImplementedError):                      # a file pipeline with views
        ImagePipeline(_pipe("LoadImageFromFile", img_scale=(64, 48), flip=True))
    with pytest.raises(NotImplementedError):
        ImagePipeline(_pipe("LoadImageFromFile", img_scale=[(64, 48), (96, 80)], flip=False))
    with pytest.raises(NotImplementedError):                      # scale_factor=
        ImagePipeline(_pipe("LoadImageFromWebcam", scale_factor=[0.5, 1.0], flip=False))
    no_flip = [dict(type="Resize", keep_ratio=True), dict(type="Normalize", **NORM), dict(type="Pad", size_divisor=32),
               dict(type="Collect", keys=["img"])]
    with pytest.raises(ValueError, match="RandomFlip"):           # flip=True without RandomFlip
        ImagePipeline(_pipe("LoadImageFromWebcam", transforms=no_flip, img_scale=(64, 48), flip=True))
    ImagePipeline(_pipe("LoadImageFromWebcam", transforms=no_flip, img_scale=(64, 48), flip=False))
    with pytest.raises(ValueError, match="flip_direction"):       # a bad direction
        ImagePipeline(_pipe("LoadImageFromWebcam", img_scale=(64, 48), flip=True, flip_direction="sideways"))
    with pytest.raises(ValueError, match="flip_direction"):
        ImagePipeline(_pipe("LoadImageFromWebcam", img_scale=(64, 48), flip=True, flip_direction=["horizontal", "up"]))
    scales = [(64 + 2 * k, 48) for k in range(5)]
    ok = ImagePipeline(_pipe("LoadImageFromWebcam", img_scale=scales[:4], flip=True, flip_direction=["horizontal", "vertical", "diagonal"]))
    assert ok.views == 16
    with pytest.raises(ValueError, match="16"):                   # more than 16 views
        ImagePipeline(_pipe("LoadImageFromWebcam", img_scale=scales, flip=True, flip_direction=["horizontal", "vertical", "diagonal"]))


def test_tta_override_with_file_names_is_refused():
    from radet_amd.apis import inference as I, set_tta
    from radet_amd.utils import Config

    class Model:
        cfg = Config(dict(data=dict(test=dict(pipeline=_pipe("LoadImageFromFile", img_scale=(64, 48), flip=False)))))
    tta = dict(img_scale=[(64, 48), (96, 80)], flip=True, flip_direction="horizontal")
    m = set_tta(Model(), tta)
    assert m.tta == tta
    for names in ("a.png", ["a.png", "b.png"]):
        with pytest.raises(NotImplementedError, match="file names"):
            I.inference_detector(m, names)
    with pytest.raises(ValueError):
        set_tta(m, dict(scales=[(64, 48)]))
    assert set_tta(m, None).tta is None
    # the override replaces the three view arguments and keeps the transforms; pipelines are cached per (pipeline, tta)
    p = I._frame_pipeline(m, tta)
    assert p.views == 4 and p.frames and I._frame_pipeline(m, dict(tta)) is p
    assert I._frame_pipeline(m).views == 1 and I._frame_pipeline(m) is not p and I._frame_pipeline(m, tta) is p
    with pytest.raises(ValueError):
        I._frame_pipeline(m, dict(scales=[(64, 48)]))
