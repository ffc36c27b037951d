"""RoI crops of detections, host side: the constants against the header, the NumPy restatement of the window rule
(tests/_crops_ref.py) on a hand-made table with hand-computed windows, every refusal of the crop request, and the public
signatures."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _crops_ref as R  # noqa: E402


def test_crop_constants_match_the_header():
    from radet_amd import _lib, kernels as K
    hdr = open(os.path.join(REPO, "include", "radet_hip.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)\n", hdr).group(1))
    assert define("CROP_ROW_INTS") == K.CROP_ROW_INTS == R.ROW_INTS == 6
    assert define("CROP_MAX_SIDE") == K.CROP_MAX_SIDE == R.MAX_SIDE == 16384
    assert (define("CROP_TO_RGB"), define("CROP_F32")) == (K.CROP_TO_RGB, K.CROP_F32) == (1, 2)
    assert len(_lib.SIGNATURES["radet_crop_plan"][1]) == 13 and len(_lib.SIGNATURES["radet_crop_frames"][1]) == 17
    from radet_amd import ops
    assert "crop_detections" in ops.__all__ and ops.Crops._fields == ("images", "windows", "index", "n_total")


NAN, INF = float("nan"), float("inf")
# (box, score) -> the window (wx0, wy0, ww, wh) worked out by hand, or None; size (Ho, Wo) = (8, 12): a = 1.5; scale 1;
# score_thr 0.3
TABLE_8x12 = [
    ((10, 10, 25, 20), 0.9, (10, 10, 15, 10)),          # w / a == h == 10: the tie, hs = 10, ws = 15; centre (17.5, 15)
    ((10, 10, 22, 20), 0.9, (8, 10, 15, 10)),           # w / a = 8 < h: the height decides; cx = 16 -> 16 - 7.5 = 8.5 -> 8
    ((10, 10, 40, 20), 0.9, (10, 5, 30, 20)),           # w / a = 20 > h: the width decides; cy = 15 -> 15 - 10 = 5
    ((5, 5, 5.25, 5.5), 0.9, (4, 4, 1, 1)),             # thinner than a pixel: hs = 0.5 -> 1, ws = 0.75 -> 1; centre (5.125, 5.25)
    ((-50000, -50000, 50000, 50000), 0.9, (-8192, -8192, 16384, 16384)),       # both sides beyond CROP_MAX_SIDE
    ((0, 0, 60000, 10), 0.9, (21808, -8187, 16384, 16384)),                    # w / a = 40000: both sides clamped; centre (30000, 5)
    ((NAN, 0, 10, 10), 0.9, None), ((0, 0, INF, 10), 0.9, None), ((0, -INF, 10, 10), 0.9, None),
    ((10, 10, 10, 20), 0.9, None),                      # zero area
    ((10, 10, 5, 20), 0.9, None), ((10, 20, 15, 10), 0.9, None),               # negative width / height
    ((2.0 ** 21, 0, 2.0 ** 21 + 10, 10), 0.9, None),    # centre beyond 2^20
    ((10, 10, 25, 20), 0.29, None),                     # below the threshold
    ((10, 10, 25, 20), 0.3, (10, 10, 15, 10)),          # equal to it: kept
    ((10, 10, 25, 20), 0.31, (10, 10, 15, 10)),
    ((10, 10, 25, 20), NAN, None),                      # a NaN score compares false
]

# size 16 x 16 (a = 1), scale 1: half-integer centres
TABLE_16 = [
    ((10, 10, 20, 20), 0.9, (10, 10, 10, 10)),          # centre (15, 15), side 10
    ((10, 10, 21, 20), 0.9, (10, 9, 11, 11)),           # centre (15.5, 15): 15.5 - 5.5 = 10, 15 - 5.5 = 9.5 -> 9
    ((-3, -4, 0, 1), 0.9, (-4, -4, 5, 5)),              # centre (-1.5, -1.5): -1.5 - 2.5 = -4
    ((0.5, 0.5, 3.5, 4.0), 0.9, (0, 0, 4, 4)),          # side ceil(3.5) = 4; centre (2, 2.25): 0, 0.25 -> 0
]


@pytest.mark.parametrize("size,table", [((8, 12), TABLE_8x12), ((16, 16), TABLE_16)])
def test_window_rule_on_a_hand_made_table(size, table):
    for box, score, want in table:
        assert R.window(box, score, size, 1.0, 0.3) == want, (box, score)
    boxes = np.array([t[0] for t in table], np.float32)[None]
    scores = np.array([t[1] for t in table], np.float32)[None]
    keep = [(0, j) + t[2] for j, t in enumerate(table) if t[2] is not None]
    rows, n_out, n_total = R.plan(boxes, scores, [len(table)], size, 1.0, 0.3, 1000)
    assert n_out == n_total == len(keep) and rows.dtype == np.int32 and rows.tolist() == [list(k) for k in keep]
    # a cap below the count keeps the first ones, in order; counts cut the walk; ranks at or beyond counts are not looked at
    rows, n_out, n_total = R.plan(boxes, scores, [len(table)], size, 1.0, 0.3, 2)
    assert (n_out, n_total) == (2, len(keep)) and rows.tolist() == [list(k) for k in keep[:2]]
    rows, n_out, n_total = R.plan(boxes, scores, [3], size, 1.0, 0.3, 1000)
    assert n_total == 3 and rows[:, 1].tolist() == [0, 1, 2]


def test_window_rule_scale_and_float32_rounding():
    # scale 1.2 on a side of 10: f32(1.2) = 1.2000000477, the product 12.000000477 is a tie that rounds to 12 in float32 (in
    # double it would be above 12 and the side 13): the rule is float32, every step rounded
    assert np.float32(10) * np.float32(1.2) == 12 and 10 * float(np.float32(1.2)) > 12
    assert R.window((10, 10, 20, 20), 1.0, (16, 16), 1.2, 0.0) == (9, 9, 12, 12)
    assert R.window((10, 10, 20, 20), 1.0, (16, 16), 1.5, 0.0) == (7, 7, 15, 15)       # 15 - 7.5 = 7.5 -> 7
    # a = 12 / 8 = 1.5 exactly; a = 8 / 12 rounds: w / a is the float32 quotient
    a = np.float32(8) / np.float32(12)
    assert R.window((0, 0, 10, 1), 1.0, (12, 8), 1.0, 0.0)[3] == int(np.ceil(np.float32(10) / a))


def test_pixel_restatement_on_a_constant_frame():
    """inside the frame the crop of a constant frame is that constant; outside it is the fill, in the frame's channel order"""
    frame = np.empty((20, 30, 3), np.uint8)
    frame[:] = (7, 8, 9)
    got = R.crop_u8(frame, (5, 5, 10, 10), (4, 4), (1, 2, 3))
    assert (got == (7, 8, 9)).all()
    got = R.crop_u8(frame, (40, 40, 6, 6), (4, 4), (1, 2, 3))
    assert (got == (1, 2, 3)).all()
    got = R.crops([frame], np.array([[0, 0, 40, 40, 6, 6]], np.int32), (4, 4), (1, 2, 3), dict(mean=[0, 0, 0], std=[1, 1, 1], to_rgb=True))
    assert got.shape == (1, 3, 4, 4) and (got[0, 0] == 3).all() and (got[0, 2] == 1).all()


FRAMES = [np.zeros((8, 9, 3), np.uint8)]
DETS = [(torch.zeros(0, 5), torch.zeros(0, dtype=torch.long))]


@pytest.mark.parametrize("kw", [
    dict(size=0), dict(size=(8, 0)), dict(size=(8, -1)), dict(size=(8, 8, 8)), dict(size=()), dict(size=8.0), dict(size=(8, 2.5)),
    dict(size="8"), dict(size=None), dict(size=(True, 8)), dict(size=5000),
    dict(size=8, scale=0), dict(size=8, scale=-1.0), dict(size=8, scale=float("nan")), dict(size=8, scale=float("inf")),
    dict(size=8, fill=(0, 0)), dict(size=8, fill=(0, 0, 256)), dict(size=8, fill=(0, -1, 0)), dict(size=8, fill=(0.5, 0, 0)),
    dict(size=8, fill=7), dict(size=8, max_crops=65536), dict(size=8, max_crops=-1),
    dict(size=8, normalize=dict(mean=[0, 0, 0])), dict(size=8, normalize=dict(mean=[0, 0, 0], std=[1, 0, 1])),
])
def test_bad_crop_requests_are_refused_before_any_device_work(kw):
    from radet_amd import ops
    from radet_amd.ops.crops import crop_spec
    with pytest.raises(ValueError):
        crop_spec(**kw)
    with pytest.raises(ValueError):
        ops.crop_detections(FRAMES, DETS, **kw)                    # (no GPU here: a request that got further would not raise this)


def test_accepted_requests():
    from radet_amd.ops.crops import crop_spec
    s = crop_spec(8)
    assert s.size == (8, 8) and s.scale == 1.2 and s.score_thr == 0.0 and s.max_crops is None and s.fill == 0 and s.mean is None
    s = crop_spec([np.int64(8), 12], scale=2, fill=np.array([1, 2, 3]), max_crops=65535,
                  normalize=dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=False))
    assert s.size == (8, 12) and s.fill == 1 | 2 << 8 | 3 << 16 and s.max_crops == 65535 and not s.to_rgb
    mean, stdinv = R.norm_consts([123.675, 116.28, 103.53], [58.395, 57.12, 57.375])
    assert np.array_equal(s.mean, mean) and np.array_equal(s.stdinv, stdinv) and s.mean.dtype == s.stdinv.dtype == np.float32


def test_crops_need_loaded_frames():
    """file names and normalised NCHW tensors are refused with a message that says what to pass"""
    from radet_amd import ops
    from radet_amd.apis import detect_frames, inference_detector
    from radet_amd.runtime import DetectorRuntime
    crops = dict(size=8, normalize=None)
    for bad in ("a.png", ["a.png", "b.png"], torch.zeros(1, 3, 8, 8), torch.zeros(3, 8, 8), [torch.zeros(3, 8, 8)],
                [np.zeros((8, 8, 3), np.float32)], []):
        with pytest.raises(ValueError, match="loaded frames"):
            inference_detector(None, bad, crops=crops)
    with pytest.raises(ValueError, match="loaded frames"):
        ops.crop_detections(["a.png"], DETS, 8)
    with pytest.raises(ValueError):
        inference_detector(None, FRAMES, crops=dict(scale=1.0))                   # no size
    with pytest.raises(ValueError):
        inference_detector(None, FRAMES, crops=dict(size=8, normalize=None, zoom=2))
    with pytest.raises(ValueError):
        inference_detector(None, FRAMES, crops=dict(size=8, normalize=None, scale=0))
    with pytest.raises(NotImplementedError, match="detect_graph"):
        DetectorRuntime.detect_graph(None, None, None, None, crops=crops)

    # detect_frames: the refusal comes with the first batch (it is a generator)
    from test_frames_cpu import _pipeline
    from radet_amd.utils import Config

    class Model:
        cfg = Config(dict(data=dict(test=dict(pipeline=_pipeline("LoadImageFromFile")))))
        training = False
        test_cfg = None

        class bbox_head:
            num_classes = 1

        class _Rt:
            @staticmethod
            def detect_stream(batches, *a, **k):
                return (b for b in batches)

        def runtime(self):
            return self._Rt
    with pytest.raises(ValueError, match="loaded frames"):
        next(detect_frames(Model(), ["a.png"], crops=crops))
    with pytest.raises(ValueError):
        next(detect_frames(Model(), FRAMES, crops=dict(size=8, normalize=None, max_crops=70000)))


def test_default_normalize_is_the_test_pipelines():
    from radet_amd.apis.inference import _crop_request
    from radet_amd.utils import Config
    from test_frames_cpu import _pipeline

    class Model:
        cfg = Config(dict(data=dict(test=dict(pipeline=_pipeline("LoadImageFromFile")))))
    norm = [t for t in Model.cfg.data.test.pipeline[1]["transforms"] if t["type"] == "Normalize"][0]
    s = _crop_request(Model(), dict(size=(8, 12)))
    mean, stdinv = R.norm_consts(norm["mean"], norm["std"])
    assert np.array_equal(s.mean, mean) and np.array_equal(s.stdinv, stdinv) and s.to_rgb == norm["to_rgb"]
    assert s.max_crops is None and s.fill == 0 and s.scale == 1.2
    assert _crop_request(Model(), dict(size=8, normalize=None)).mean is None


def test_public_signatures_keep_their_parameters_in_place():
    from radet_amd import ops
    from radet_amd.apis import detect_frames, inference_detector
    assert list(inspect.signature(inference_detector).parameters) == ["model", "imgs", "scale_factor", "crops"]
    assert list(inspect.signature(detect_frames).parameters) == ["model", "frames", "batch_size", "on_device", "crops"]
    p = inspect.signature(detect_frames).parameters
    assert p["batch_size"].default == 8 and p["on_device"].default is False and p["crops"].default is None
    assert inspect.signature(inference_detector).parameters["crops"].default is None
    sig = inspect.signature(ops.crop_detections)
    assert list(sig.parameters) == ["frames", "dets", "size", "scale", "score_thr", "max_crops", "fill", "normalize"]
    assert [sig.parameters[k].default for k in ("scale", "score_thr", "max_crops", "fill", "normalize")] == [1.2, 0.0, None, (0, 0, 0), None]
    assert "x_frame = x0 + (u + 0.5) * w / Wo - 0.5" in ops.Crops.__doc__
