"""RoI crops of detections on the device (radet_crop_plan / radet_crop_frames): the plan against the NumPy float32
restatement exactly, the pixels bit-equal to the chain of existing kernels (radet_resize_linear_u8 with view rows built on
the host from the same plan, then radet_preprocess_frames' Normalize on the resized bytes) and to the NumPy restatement, the
slots beyond n_out untouched, truncation, edge shapes, and the public interface on a synth-initialised detector."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _crops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
NAN, INF = float("nan"), float("inf")
FILL = (17, 130, 241)
THR = 0.25
COUNTS = (0, 5, 2)
# frame 1 is 64 x 48 (h x w), frame 2 is 40 x 50.  Frame 0 has no detections: its slots hold valid-looking boxes that must be
# ignored, like every slot at or beyond a frame's count.
IGNORED = [(2, 3, 20, 30, 0.9)] * 5
TABLES = {
    # an interior box, one box over each of the four edges; wholly outside the frame (all fill), thinner than a pixel
    "edges": [IGNORED,
              [(16, 24, 28, 36, 0.9), (-6, 20, 9, 33, 0.8), (15, -9, 30, 8, 0.7), (40, 30, 55, 44, 0.6), (12, 55, 29, 70, 0.5)],
              [(70, 60, 90, 85, 0.9), (20.25, 10.5, 20.5, 10.75, 0.8), (1, 1, 9, 9, 0.9), (1, 1, 9, 9, 0.9), (1, 1, 9, 9, 0.9)]],
    # the whole frame (at scale 1.5 it overhangs all four edges), below the threshold, NaN, a valid one behind the invalid
    # ones, inf; a zero-area box, a score equal to the threshold
    "invalid": [IGNORED,
                [(0, 0, 48, 64, 0.9), (10, 10, 30, 30, 0.2), (NAN, 10, 30, 30, 0.9), (5.5, 7.5, 33, 29, 0.6), (10, 10, INF, 30, 0.9)],
                [(10, 10, 10, 30, 0.9), (8, 9, 31, 22, THR), (1, 1, 9, 9, 0.9), (1, 1, 9, 9, 0.9), (1, 1, 9, 9, 0.9)]],
}
SIZES = [(16, 16), (8, 12)]


@pytest.fixture(scope="module")
def scene():
    """three frames: 37 x 53 and 64 x 48 host arrays, and a 40 x 50 device view into a larger tensor (rows 401 bytes apart, an
    odd byte address); `host` = all three as host arrays"""
    rng = np.random.RandomState(5)
    f0, f1 = (rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (64, 48)))
    g = torch.Generator().manual_seed(3)
    big = torch.randint(0, 256, (60, 401), dtype=torch.uint8, generator=g).cuda()
    view = big.as_strided((40, 50, 3), (401, 3, 1), 5 * 401 + 8)
    assert view.data_ptr() % 2 == 1 and view.stride(0) != 3 * 50 and not view.is_contiguous()
    return dict(frames=[f0, f1, view], host=[f0, f1, view.cpu().numpy().copy()], big=big, before=big.clone())


def _dets(name):
    t = np.array(TABLES[name], np.float32)
    return np.ascontiguousarray(t[..., :4]), np.ascontiguousarray(t[..., 4]), np.array(COUNTS, np.int32)


def _spec(size, normalize, scale=1.5, fill=FILL, thr=THR):
    from radet_amd.ops.crops import crop_spec
    return crop_spec(size, scale=scale, score_thr=thr, fill=fill, normalize=normalize)


def _run(frames, boxes, scores, counts, spec, cap, canary=None):
    """the two launches -> (images, rows, counters) as host arrays; canary: the byte every output is filled with before.
    counters: i32 [2 + B] = {n_out, n_total, where each frame's rows end}"""
    from radet_amd import kernels as K
    from radet_amd.ops.crops import frame_table
    dev = torch.device("cuda", torch.cuda.current_device())
    desc, keep = frame_table(frames, dev)
    b, s, c = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (boxes, scores, counts))
    Ho, Wo = spec.size
    f32 = spec.mean is not None
    fillb = 0 if canary is None else canary
    rows = torch.full((max(cap, 1), K.CROP_ROW_INTS * 4), fillb, dtype=torch.uint8, device=dev).view(torch.int32)
    images = torch.full((cap, 3 * Ho * Wo * (4 if f32 else 1)), fillb, dtype=torch.uint8, device=dev)
    images = images.view(torch.float32).view(cap, 3, Ho, Wo) if f32 else images.view(cap, Ho, Wo, 3)
    counters = torch.full((2 + len(frames),), -7, dtype=torch.int32, device=dev)
    K.crop_plan(b, s, c, spec.size, spec.scale, spec.score_thr, cap, rows, counters)
    K.crop_frames(rows, counters, desc, len(frames), cap, spec.size, images, spec.fill, spec.mean, spec.stdinv, spec.to_rgb)
    torch.cuda.synchronize()
    del keep
    return images.cpu().numpy(), rows.cpu().numpy(), counters.cpu().numpy()


def _counters(n_out, n_total, rows, B):
    """what the plan leaves in its counters for these rows: frame b's rows are those before ends[b] and not before ends[b - 1]"""
    return [n_out, n_total] + np.searchsorted(rows[:n_out, 0], np.arange(B), side="right").tolist()


def _chain(host_frames, rows, size, fill_word, normalize):
    """the same crops from the existing kernels: radet_resize_linear_u8 with one view row {Ho, Wo, wy0, wx0, wh, ww, 0, 0, Ho,
    Wo, 0, fill} per plan row over the packed frames, then (f32) radet_preprocess_frames at identity size on the resized bytes"""
    from radet_amd import kernels as K
    from radet_amd.datasets.loading import frame_desc_rows
    dev = torch.device("cuda", torch.cuda.current_device())
    Ho, Wo = size
    n = len(rows)
    offs = np.cumsum([0] + [f.shape[0] * f.shape[1] for f in host_frames])
    src = torch.from_numpy(np.concatenate([f.reshape(-1) for f in host_frames])).to(dev)
    sdesc = np.array([[offs[r[0]], *host_frames[r[0]].shape[:2]] for r in rows], np.int32)
    ddesc = np.array([[i * Ho * Wo, Ho, Wo] for i in range(n)], np.int32)
    views = np.array([[Ho, Wo, r[3], r[2], r[5], r[4], 0, 0, Ho, Wo, 0, fill_word] for r in rows], np.int32)
    dst = torch.full((n, Ho, Wo, 3), 99, dtype=torch.uint8, device=dev)
    K.resize_linear_u8(src, torch.from_numpy(sdesc).to(dev), dst, torch.from_numpy(ddesc).to(dev), n, Ho * Wo, 3,
                       views=torch.from_numpy(views).to(dev))
    if normalize is None:
        torch.cuda.synchronize()
        return dst.cpu().numpy()
    crops = [dst[i] for i in range(n)]
    prow, _, _ = frame_desc_rows(crops, [(Ho, Wo)] * n, normalize["to_rgb"], 0)
    out = torch.full((n, 3, Ho, Wo), float("nan"), device=dev)
    K.preprocess_frames(torch.from_numpy(prow).to(dev), n, Ho, Wo, *R.norm_consts(normalize["mean"], normalize["std"]), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------- 1. mixed frames, both references
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("table", sorted(TABLES))
def test_mixed_frames_plan_and_pixels(scene, table, size):
    boxes, scores, counts = _dets(table)
    cap = 15
    want_rows, n_out, n_total = R.plan(boxes, scores, counts, size, 1.5, THR, cap)
    assert n_out == n_total == {"edges": 7, "invalid": 3}[table]                 # (what the table is built to give)
    assert _counters(n_out, n_total, want_rows, 3)[2:] == {"edges": [0, 5, 7], "invalid": [0, 2, 3]}[table]
    if table == "invalid":
        assert want_rows[:, :2].tolist() == [[1, 0], [1, 3], [2, 1]]
    for normalize in (NORM, dict(NORM, to_rgb=False), None):
        spec = _spec(size, normalize)
        images, rows, counters = _run(scene["frames"], boxes, scores, counts, spec, cap)
        assert counters.tolist() == _counters(n_out, n_total, want_rows, 3)
        assert np.array_equal(rows[:n_out], want_rows)
        chain = _chain(scene["host"], want_rows, size, spec.fill, normalize)
        assert images.dtype == chain.dtype and np.array_equal(images[:n_out], chain)
        assert np.array_equal(images[:n_out], R.crops(scene["host"], want_rows, size, FILL, normalize))
    assert torch.equal(scene["big"], scene["before"])
    if table == "edges":                                    # the wholly outside box is all fill, the others are not
        u8 = _run(scene["frames"], boxes, scores, counts, _spec(size, None), cap)[0]
        assert (u8[5] == np.array(FILL, np.uint8)).all() and not (u8[0] == np.array(FILL, np.uint8)).all(axis=-1).any()
        assert want_rows[6, 4:].tolist() == [1, 1]          # the sub-pixel box: a 1 x 1 window


# ------------------------------------------------------------------------------------------- 2. slots beyond n_out / 3. truncation
@pytest.mark.parametrize("normalize", [NORM, None], ids=["f32", "u8"])
def test_slots_beyond_n_out_keep_the_canary(scene, normalize):
    boxes, scores, counts = _dets("invalid")
    spec = _spec((8, 12), normalize)
    images, rows, counters = _run(scene["frames"], boxes, scores, counts, spec, 6, canary=0xA5)
    assert counters.tolist() == [3, 3, 0, 2, 3]
    assert (rows[3:].view(np.uint8) == 0xA5).all() and (images[3:].view(np.uint8) == 0xA5).all()
    want_rows = R.plan(boxes, scores, counts, (8, 12), 1.5, THR, 6)[0]
    assert np.array_equal(rows[:3], want_rows)
    assert np.array_equal(images[:3], R.crops(scene["host"], want_rows, (8, 12), FILL, normalize))


def test_truncation_keeps_the_first_cap_in_order(scene):
    boxes, scores, counts = _dets("edges")
    spec = _spec((16, 16), None)
    full = R.plan(boxes, scores, counts, (16, 16), 1.5, THR, 15)[0]
    images, rows, counters = _run(scene["frames"], boxes, scores, counts, spec, 4, canary=0x5A)
    assert counters.tolist() == [4, 7, 0, 4, 4] and rows.shape[0] == 4          # (the ends count the rows that were kept)
    assert np.array_equal(rows, full[:4])
    assert np.array_equal(images, R.crops(scene["host"], full[:4], (16, 16), FILL, None))
    # through the public entry point: the record says what was left out
    from radet_amd import ops
    got = ops.crop_detections(scene["frames"], tuple(torch.from_numpy(a) for a in (boxes, scores, counts)), 16, scale=1.5,
                              score_thr=THR, max_crops=4, fill=FILL)
    assert got.n_total == 7 and got.images.shape == (4, 16, 16, 3) and np.array_equal(got.images.cpu().numpy(), images)
    assert np.array_equal(got.index.cpu().numpy(), full[:4, :2]) and np.array_equal(got.windows.cpu().numpy(), full[:4, 2:])


# ------------------------------------------------------------------------------------------- 4. edge shapes
def test_all_counts_zero_writes_nothing(scene):
    boxes, scores, _ = _dets("edges")
    for normalize in (NORM, None):
        images, rows, counters = _run(scene["frames"], boxes, scores, np.zeros(3, np.int32), _spec((8, 12), normalize), 5, canary=0xA5)
        assert counters.tolist() == [0, 0, 0, 0, 0]
        assert (rows.view(np.uint8) == 0xA5).all() and (images.view(np.uint8) == 0xA5).all()
    from radet_amd import ops
    got = ops.crop_detections(scene["frames"], [torch.zeros(0, 5)] * 3, (8, 12), normalize=NORM)
    assert got.images.shape == (0, 3, 8, 12) and got.windows.shape == (0, 4) and got.index.shape == (0, 2) and got.n_total == 0


# 20 x 20: two trips of a block, the second partly filled; 40 x 30 and 33 x 35: two blocks; 5 x 7, 1 x 1, 3 x 90, 33 x 35: planes
# that are no multiple of four pixels (the u8 mode's byte stores)
@pytest.mark.parametrize("size", [(20, 20), (40, 30), (5, 7), (1, 1), (3, 90), (33, 35)])
def test_one_frame_one_detection_and_the_fill_colour(size):
    rng = np.random.RandomState(size[0])
    frame = rng.randint(0, 256, (21, 30, 3)).astype(np.uint8)
    boxes, scores, counts = np.array([[[20, 12, 36, 25]]], np.float32), np.array([[0.5]], np.float32), np.array([1], np.int32)
    want_rows, n_out, _ = R.plan(boxes, scores, counts, size, 1.2, 0.0, 1)
    assert n_out == 1
    for normalize in (NORM, None):
        spec = _spec(size, normalize, scale=1.2, thr=0.0)
        images, rows, counters = _run([frame], boxes, scores, counts, spec, 1)
        assert counters.tolist() == [1, 1, 1] and np.array_equal(rows, want_rows)
        assert np.array_equal(images, R.crops([frame], want_rows, size, FILL, normalize))
    # the window overhangs the frame's right edge: the last column is fill, in the frame's (BGR) channel order before the swap
    if size == (1, 1):
        return
    x0, _, ww, _ = (int(v) for v in want_rows[0, 2:])
    assert x0 + int(np.floor((size[1] - 0.5) * ww / size[1] - 0.5)) >= 30      # (the last column's left tap is beyond the frame)
    u8 = _run([frame], boxes, scores, counts, _spec(size, None, scale=1.2, thr=0.0), 1)[0]
    assert u8[0, :, -1].tolist() == [list(FILL)] * size[0]
    f32 = _run([frame], boxes, scores, counts, _spec(size, NORM, scale=1.2, thr=0.0), 1)[0]
    mean, stdinv = R.norm_consts(NORM["mean"], NORM["std"])
    for plane, c in enumerate((2, 1, 0)):                   # to_rgb: plane 0 holds the fill's third (R) byte
        assert (f32[0, plane, :, -1] == (np.float32(FILL[c]) - mean[plane]) * stdinv[plane]).all()


def test_bad_arguments_are_refused_before_any_launch():
    from radet_amd import _lib, kernels as K
    dev = torch.device("cuda", torch.cuda.current_device())
    boxes, scores = torch.zeros(1, 1, 4, device=dev), torch.zeros(1, 1, device=dev)
    counts, counters = torch.zeros(1, dtype=torch.int32, device=dev), torch.full((3,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((1, K.CROP_ROW_INTS), -7, dtype=torch.int32, device=dev)
    desc = torch.zeros(1, K.PREP_DESC_INTS, dtype=torch.int32, device=dev)
    out = torch.full((1, 8, 8, 3), 7, dtype=torch.uint8, device=dev)

    def plan(B=1, Kd=1, Ho=8, Wo=8, scale=1.0, cap=1):
        _lib.call("radet_crop_plan", boxes.data_ptr(), scores.data_ptr(), counts.data_ptr(), B, Kd, Ho, Wo, scale, 0.0, cap,
                  rows.data_ptr(), counters.data_ptr(), None)

    def frames(B=1, cap=1, Ho=8, Wo=8, flags=0):
        _lib.call("radet_crop_frames", rows.data_ptr(), counters.data_ptr(), desc.data_ptr(), B, cap, Ho, Wo, flags, 0, 0.0, 0.0,
                  0.0, 1.0, 1.0, 1.0, out.data_ptr(), None)
    for kw in (dict(B=-1), dict(Kd=-1), dict(Kd=0), dict(cap=-1), dict(cap=65536), dict(Ho=0), dict(Wo=0), dict(Ho=4097),
               dict(Wo=4097), dict(scale=0.0), dict(scale=-1.0), dict(scale=NAN), dict(scale=INF), dict(B=65536, Kd=32768)):
        with pytest.raises(_lib.RadetHipError):
            plan(**kw)
    for kw in (dict(B=-1), dict(cap=-1), dict(cap=65536), dict(Ho=0), dict(Wo=4097), dict(flags=4)):
        with pytest.raises(_lib.RadetHipError):
            frames(**kw)
    plan(B=0)                                               # no frames, no slots: OK, no launch
    plan(cap=0)
    frames(B=0)
    frames(cap=0)
    torch.cuda.synchronize()
    assert (counters == -7).all() and (rows == -7).all() and (out == 7).all()


def test_crop_detections_takes_per_frame_detections(scene):
    """the list form, as detect_frames(on_device=True) yields it, equals the padded triple"""
    from radet_amd import ops
    boxes, scores, counts = _dets("edges")
    per = [(torch.from_numpy(np.concatenate([boxes[b, :c], scores[b, :c, None]], -1)).cuda(), torch.zeros(c, dtype=torch.long))
           for b, c in enumerate(COUNTS)]
    a = ops.crop_detections(scene["frames"], per, (8, 12), scale=1.5, score_thr=THR, fill=FILL, normalize=NORM)
    b = ops.crop_detections(scene["host"], tuple(torch.from_numpy(x) for x in (boxes, scores, counts)), (8, 12), scale=1.5,
                            score_thr=THR, fill=FILL, normalize=NORM)
    want_rows = R.plan(boxes, scores, counts, (8, 12), 1.5, THR, 15)[0]
    for got in (a, b):
        assert got.n_total == 7 and got.images.is_cuda and got.images.dtype == torch.float32
        assert np.array_equal(got.index.cpu().numpy(), want_rows[:, :2]) and np.array_equal(got.windows.cpu().numpy(), want_rows[:, 2:])
        assert np.array_equal(got.images.cpu().numpy(), R.crops(scene["host"], want_rows, (8, 12), FILL, NORM))
    with pytest.raises(ValueError):
        ops.crop_detections(scene["frames"][:2], per, 8)


# ------------------------------------------------------------------------------------------- 5. / 6. the public interface
def _pipe(loader, scale):
    return [dict(type=loader),
            dict(type="MultiScaleFlipAug", img_scale=scale, flip=False, transforms=[
                dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", **NORM),
                dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])])]


@pytest.fixture(scope="module")
def det():
    """the detector of tests/test_gpu_frames.py: img_scale (640, 480) on small landscape frames, batches of 2 and 1 images
    padded to 480 x 640 are geometries whose conv tile picks are pinned, so nothing is tuned while the tests run"""
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    d = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().eval()
    synth_fill(d, seed=0)
    with torch.no_grad():
        d.bbox_head.atss_cls.bias += 2.0                       # (scores above the threshold: the comparisons are not vacuous)
    d.cfg = Config(dict(data=dict(test=dict(pipeline=_pipe("LoadImageFromFile", (640, 480))))))
    return d


@pytest.fixture(scope="module")
def det_frames():
    rng = np.random.RandomState(11)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (48, 64), (60, 80), (30, 40), (75, 100))]


def _log_calls(fn):
    from radet_amd import _lib
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        return seen, fn()
    finally:
        _lib.call = call


def _same_crops(a, b):
    assert a.n_total == b.n_total
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)


def test_detect_frames_with_crops(det, det_frames):
    from radet_amd import ops
    from radet_amd.apis import detect_frames, inference_detector
    req = dict(size=(16, 12), scale=1.3, fill=(5, 6, 7))
    list(detect_frames(det, det_frames, batch_size=2))     # (weight fold, plans of both batch sizes: not part of the logs below)
    plain_log, plain = _log_calls(lambda: list(detect_frames(det, det_frames, batch_size=2, on_device=True)))
    crop_log, both = _log_calls(lambda: list(detect_frames(det, det_frames, batch_size=2, on_device=True, crops=req)))
    assert len(plain) == len(both) == 5 and sum(int(b.shape[0]) for b, _ in plain) > 0
    # three batches (2, 2, 1 frames); each frame's crops are cut from that frame: equal to the stand-alone op on it
    for k, (frame, (b0, l0), ((b1, l1), crops)) in enumerate(zip(det_frames, plain, both)):
        assert torch.equal(b0, b1) and torch.equal(l0, l1)                        # detections: bit-equal to the call without
        want = ops.crop_detections([frame], [(b1, l1)], (16, 12), scale=1.3, fill=(5, 6, 7), normalize=NORM)
        assert 0 < want.images.shape[0] == crops.images.shape[0] <= b1.shape[0] and crops.images.shape[1:] == (3, 16, 12)
        assert torch.equal(crops.images, want.images) and torch.equal(crops.windows, want.windows)
        assert torch.equal(crops.index[:, 1], want.index[:, 1]) and (crops.index[:, 0] == k % 2).all()   # (its place in its batch)
    # without crops= a batch issues the launches it issued before: the whole sequence of each of the three batches, name by
    # name, is that of the same frames through inference_detector -- the path without a crops= branch that the frame tests
    # run -- which is one frame preparation, the forward pass, one decode and one NMS
    def per_batch(log):
        starts = [i for i, n in enumerate(log) if n == "radet_preprocess_frames"]
        return [log[a:b] for a, b in zip(starts, starts[1:] + [len(log)])]
    assert plain_log[0] == "radet_preprocess_frames" and len(per_batch(plain_log)) == 3
    for k, got in enumerate(per_batch(plain_log)):
        want_log, _ = _log_calls(lambda: inference_detector(det, det_frames[2 * k:2 * k + 2]))
        assert got == want_log, (k, got, want_log)
        assert got[-2:] == ["radet_decode_candidates", "radet_nms"] and not [n for n in got if "crop" in n]
        assert [got.count(n) for n in ("radet_preprocess_frames", "radet_decode_candidates", "radet_nms")] == [1, 1, 1]
    # with crops= exactly the two launches more per batch, behind its NMS
    assert [b[:-2] for b in per_batch(crop_log)] == per_batch(plain_log)
    assert all(b[-2:] == ["radet_crop_plan", "radet_crop_frames"] for b in per_batch(crop_log))
    # inference_detector: one batch, (results, crops of the batch); u8 crops on request
    res, crops = inference_detector(det, det_frames[:2], crops=dict(size=8, normalize=None))
    want = inference_detector(det, det_frames[:2])
    assert len(res) == 2 and all(np.array_equal(x, y) for ra, rb in zip(res, want) for x, y in zip(ra, rb))
    raw = list(detect_frames(det, det_frames[:2], batch_size=2, on_device=True))
    _same_crops(crops, ops.crop_detections(det_frames[:2], raw, 8))
    assert crops.images.dtype == torch.uint8 and crops.images.shape[1:] == (8, 8, 3) and crops.n_total == crops.images.shape[0] > 0
    one, c1 = inference_detector(det, det_frames[1], crops=dict(size=8, normalize=None))
    assert len(one) == det.bbox_head.num_classes and 0 < c1.images.shape[0] <= sum(len(c) for c in one)
    # the runtime stays usable, and a frame source on the device takes the same path
    dev_frames = [torch.from_numpy(f).cuda() for f in det_frames[:2]]
    _, c2 = inference_detector(det, dev_frames, crops=dict(size=8, normalize=None))
    _same_crops(c2, crops)


def _sync_warnings(fn):
    """the number of synchronising calls PyTorch reports while fn runs (a blocking device-to-host copy, .item(), a stream or
    device synchronize; waiting for an event is not one)"""
    import warnings
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return len([w for w in seen if "synchroniz" in str(w.message).lower()])


def test_detect_frames_with_crops_adds_no_synchronisation(det, det_frames):
    """the host stays one batch behind the device: the crops' counters and the per-frame split come in the pinned copy that
    brings the detection counts, behind an event on the stream that made them.  A blocking copy on the caller's stream would
    wait for the NEXT batch's forward pass, which is already enqueued there when a batch is handed out; PyTorch reports every
    such call, and the stream with crops= makes as many of them as the stream without."""
    from radet_amd.apis import detect_frames
    req = dict(size=(16, 12), scale=1.3)
    list(detect_frames(det, det_frames, batch_size=2, on_device=True, crops=req))         # (plans, allocator pools)
    got = []
    assert _sync_warnings(lambda: torch.zeros(3, device="cuda").cpu()) >= 1               # (the count sees a blocking copy)
    plain = _sync_warnings(lambda: list(detect_frames(det, det_frames, batch_size=2, on_device=True)))
    with_crops = _sync_warnings(lambda: got.extend(detect_frames(det, det_frames, batch_size=2, on_device=True, crops=req)))
    print(f"synchronising calls: {plain} without crops=, {with_crops} with")
    assert with_crops == plain
    assert len(got) == 5 and sum(int(c.images.shape[0]) for _, c in got) > 0              # (crops were cut and split per frame)
