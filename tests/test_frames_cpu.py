"""Frames in memory, host parts: the LoadImageFromWebcam stage, the metas a frame pipeline plans against the file pipeline's,
the inputs and pipelines it refuses, and the descriptor rows of radet_preprocess_frames.  No device is touched."""
import os
import random
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def _pipeline(loader, scale=(64, 48)):
    return [dict(type=loader),
            dict(type="MultiScaleFlipAug", img_scale=scale, flip=False, transforms=[
                dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", **NORM),
                dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])])]


def _frame(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _plan(pipeline, **sample):
    return pipeline.plan(dict(bbox_fields=[], mask_fields=[], seg_fields=[], **sample), random, np.random)


def test_webcam_stage_sets_the_reference_keys():
    from radet_amd.datasets import PIPELINES
    from radet_amd.utils import build_from_cfg
    stage = build_from_cfg(dict(type="LoadImageFromWebcam", to_float32=False, color_type="color",
                                file_client_args=dict(backend="disk")), PIPELINES)
    img = _frame(37, 53)
    s = dict(img=img)
    stage.plan(s, random, np.random)
    assert s["filename"] is None and s["ori_filename"] is None and s["img"] is img
    assert s["img_shape"] == s["ori_shape"] == s["pad_shape"] == (37, 53, 3)
    assert all(type(s[k]) is tuple for k in ("img_shape", "ori_shape", "pad_shape")) and s["img_fields"] == ["img"]
    # a torch uint8 tensor of that shape, strided views included
    big = torch.zeros(40, 200, dtype=torch.uint8)
    view = big.as_strided((37, 53, 3), (200, 3, 1), 207)
    s = dict(img=view)
    stage.plan(s, random, np.random)
    assert s["img_shape"] == (37, 53, 3) and s["img"].shape == (37, 53, 3)
    with pytest.raises(NotImplementedError):
        build_from_cfg(dict(type="LoadImageFromWebcam", to_float32=True), PIPELINES)


@pytest.mark.parametrize("hw", [(37, 53), (48, 64), (100, 75)])
def test_frame_metas_equal_file_metas(hw, tmp_path):
    from PIL import Image
    from radet_amd.datasets.loading import ImagePipeline
    img = _frame(*hw, seed=hw[0])
    path = str(tmp_path / "f.png")
    Image.fromarray(img[..., ::-1]).save(path)
    files, frames = ImagePipeline(_pipeline("LoadImageFromFile")), ImagePipeline(_pipeline("LoadImageFromWebcam"))
    assert frames.frames and not files.frames
    a = _plan(files, img_info=dict(filename=path), img_prefix=None)
    b = _plan(frames, img=img)
    np.testing.assert_array_equal(a["img"], b["img"])
    for key in ("ori_shape", "img_shape", "pad_shape", "flip", "flip_direction", "keep_ratio", "resize_hw", "scale"):
        assert a[key] == b[key], key
    np.testing.assert_array_equal(a["scale_factor"], b["scale_factor"])
    for key in ("mean", "std", "to_rgb"):
        np.testing.assert_array_equal(a["img_norm_cfg"][key], b["img_norm_cfg"][key])
    assert a["filename"] == path and b["filename"] is None and b["ori_filename"] is None


@pytest.mark.parametrize("bad", [np.zeros((8, 9, 3), np.float32), np.zeros((8, 9), np.uint8), np.zeros((8, 9, 4), np.uint8),
                                 torch.zeros(8, 9, 3), torch.zeros(8, 9, dtype=torch.uint8),
                                 torch.zeros(8, 9, 4, dtype=torch.uint8), "frame.png"],
                         ids=["float_hwc", "2d", "4ch", "float_tensor", "2d_tensor", "4ch_tensor", "str"])
def test_wrong_inputs_raise_value_error(bad):
    from radet_amd.datasets.loading import ImagePipeline
    p = ImagePipeline(_pipeline("LoadImageFromWebcam"))
    with pytest.raises(ValueError) as e:
        _plan(p, img=bad)
    what = "str" if isinstance(bad, str) else str(tuple(bad.shape))
    assert what in str(e.value)                               # (the message names what was given)


def test_webcam_pipeline_must_be_a_test_pipeline():
    from radet_amd.datasets.loading import ImagePipeline
    flat = [dict(type="LoadImageFromWebcam"), dict(type="Resize", img_scale=(64, 48), keep_ratio=True),
            dict(type="Normalize", **NORM), dict(type="Pad", size_divisor=32), dict(type="Collect", keys=["img"])]
    assert ImagePipeline(flat).frames

    def with_stage(stage, at):
        return flat[:at] + [stage] + flat[at:]
    assigner = dict(type="LabelAssignment",
                    anchor_generator_cfg=dict(type="AnchorGenerator", ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                              strides=[8, 16, 32, 64, 128]),
                    neg_threshold=0.2, positive_num=10, adapt_positive_num=False, balance_sample=True)
    for bad in (with_stage(dict(type="RandomHSV", h_ratio=0.1, s_ratio=0.1, v_ratio=0.1), 2),
                with_stage(dict(type="CosyPoseAug", p=0.8, pipelines=[dict(type="PillowBlur")]), 2),
                with_stage(dict(type="RandomFlip", flip_ratio=0.5), 2),
                with_stage(dict(type="LoadAnnotations", with_bbox=True), 1),
                with_stage(dict(type="GenerateDistanceMap"), 2),
                with_stage(assigner, 2),
                with_stage(dict(type="GenerateDistanceMap"), 2)[:3] + [assigner] + flat[2:],
                flat[1:2] + flat[:1] + flat[2:],                                   # the loader is not the first stage
                [dict(type="LoadImageFromFile")] + flat):                          # two loaders
        with pytest.raises(NotImplementedError):
            ImagePipeline(bad)
    with pytest.raises(NotImplementedError):
        ImagePipeline(flat, sample_cache="device", cache_bytes=1 << 20)


def test_descriptor_rows_of_host_frames_and_a_strided_view():
    from radet_amd import kernels as K
    from radet_amd.datasets.loading import frame_desc_rows
    a, b = _frame(37, 53, 1), _frame(100, 75, 2)
    big = torch.zeros(60, 400, dtype=torch.uint8)
    view = big.as_strided((48, 64, 3), (400, 3, 1), 5 * 400 + 7)          # rows 400 bytes apart, an odd start address
    col = big.as_strided((1, 9, 3), (12345, 3, 1), 3)                     # one row: its stride has no meaning
    frames = [a, view, b, col]
    dst = [(45, 64), (48, 64), (48, 36), (7, 64)]
    base = (5 << 32) + 0xFFFFFF00                                         # the low word has its top bit set
    rows, offs, nbytes = frame_desc_rows(frames, dst, True, base)
    assert rows.dtype == np.int32 and rows.shape == (4, K.PREP_DESC_INTS) and K.PREP_DESC_INTS == 8
    assert offs == [0, None, a.size, None] and nbytes == a.size + b.size

    def addr(r):
        lo, hi = r[0:2].view(np.uint32)
        return int(lo) | int(hi) << 32
    assert addr(rows[0]) == base and addr(rows[2]) == base + a.size
    assert addr(rows[1]) == big.data_ptr() + 5 * 400 + 7 == view.data_ptr()
    assert addr(rows[3]) == col.data_ptr()
    assert rows[:, 2].tolist() == [53 * 3, 400, 75 * 3, 9 * 3]           # row strides in bytes
    assert rows[:, 3:5].tolist() == [[37, 53], [48, 64], [100, 75], [1, 9]]
    assert rows[:, 5:7].tolist() == [list(d) for d in dst]
    assert (rows[:, 7] == K.PREP_TO_RGB).all()
    assert (frame_desc_rows(frames, dst, False, base)[0][:, 7] == 0).all()
    # the header and the Python mirror name the same constants
    hdr = open(os.path.join(REPO, "include", "radet_hip.h")).read()
    assert f"#define PREP_DESC_INTS {K.PREP_DESC_INTS}\n" in hdr and f"#define PREP_TO_RGB {K.PREP_TO_RGB}\n" in hdr


def test_inference_detector_routes_frames_and_keeps_the_old_forms():
    """ndarray / uint8 HWC tensor -> the frame path (built once per model and test pipeline); a float tensor still means
    normalised NCHW"""
    from radet_amd.apis import inference as I
    from radet_amd.utils import Config
    assert I._is_frame(np.zeros((4, 5, 3), np.uint8)) and I._is_frame(torch.zeros(4, 5, 3, dtype=torch.uint8))
    assert not I._is_frame(torch.zeros(1, 3, 4, 3)) and not I._is_frame("a.png")

    class Model:
        cfg = Config(dict(data=dict(test=dict(pipeline=[dict(type="LoadImageFromFile", decode="device")]
                                              + _pipeline("LoadImageFromFile")[1:]))))
    m = Model()
    p = I._frame_pipeline(m)
    assert p.frames and I._frame_pipeline(m) is p
    m.cfg = Config(dict(data=dict(test=dict(pipeline=_pipeline("LoadImageFromFile", scale=(32, 24))))))
    q = I._frame_pipeline(m)
    assert q is not p and q.frames
    with pytest.raises(ValueError):
        I._frame_pipeline(object())
