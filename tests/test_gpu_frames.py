"""Frames in memory on the device: radet_preprocess_frames against the file pipeline's chain and a NumPy restatement bit for
bit, its edge shapes, device frames read in place, inference_detector on arrays against files, and detect_frames."""
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
SIZES = [(37, 53), (48, 64), (100, 75)]          # under (64, 48): an upscale, the identity, a downscale by 0.64


def _pipe(loader, scale, to_rgb=True):
    return [dict(type=loader),
            dict(type="MultiScaleFlipAug", img_scale=scale, flip=False, transforms=[
                dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", to_rgb=to_rgb, **NORM),
                dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])])]


def _plan(pipeline, **sample):
    return pipeline.plan(dict(bbox_fields=[], mask_fields=[], seg_fields=[], **sample), random, np.random)


@pytest.fixture(scope="module")
def frames():
    rng = np.random.RandomState(11)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES + [(60, 80), (30, 40), (75, 100)]]


@pytest.fixture(scope="module")
def pngs(frames, tmp_path_factory):
    """the frames as PNG files (lossless): what the file pipeline decodes is the frame"""
    from PIL import Image
    d = tmp_path_factory.mktemp("frames")
    paths = []
    for k, f in enumerate(frames):
        paths.append(str(d / f"{k}.png"))
        Image.fromarray(f[..., ::-1]).save(paths[-1])
    return paths


def _file_batch(cfg, paths):
    from radet_amd.datasets.loading import ImagePipeline
    p = ImagePipeline(cfg)
    return p.run([_plan(p, img_info=dict(filename=n), img_prefix=None) for n in paths], collate=True)


def _frame_batch(cfg, imgs):
    from radet_amd.datasets.loading import ImagePipeline
    p = ImagePipeline(cfg)
    return p.run([_plan(p, img=f) for f in imgs], collate=True)


def _norm_consts():
    mean = np.array(NORM["mean"], np.float32)
    stdinv = (1.0 / np.array(NORM["std"], np.float32).astype(np.float64)).astype(np.float32)
    return mean, stdinv


def _restate(imgs, dst_hw, Hp, Wp, to_rgb):
    """oracle.imgproc.resize_linear_u8, then (q - mean) * f32(1 / f64(std)) in fp32 (NumPy rounds after each operation, as
    the kernels do without contraction), zero padding"""
    from oracle.imgproc import resize_linear_u8
    mean, stdinv = _norm_consts()
    out = np.zeros((len(imgs), 3, Hp, Wp), np.float32)
    for o, img, (h, w) in zip(out, imgs, dst_hw):
        q = resize_linear_u8(np.ascontiguousarray(img), (w, h))
        q = q[..., ::-1] if to_rgb else q
        o[:, :h, :w] = ((q.astype(np.float32) - mean) * stdinv).transpose(2, 0, 1)
    return out


def _scaled(imgs, scale, divisor=32):
    from radet_amd.core.mask import rescale_size
    hw = []
    for f in imgs:
        nw, nh = rescale_size((f.shape[1], f.shape[0]), scale)
        hw.append((nh, nw))
    Hp = max(int(math.ceil(h / divisor)) * divisor for h, _ in hw)
    Wp = max(int(math.ceil(w / divisor)) * divisor for _, w in hw)
    return hw, Hp, Wp


def _same_metas(a, b):
    assert len(a) == len(b)
    for ma, mb in zip(a, b):
        assert ma.keys() == mb.keys()
        for k in ma:
            if k in ("filename", "ori_filename"):
                assert mb[k] is None
            elif k == "img_norm_cfg":
                assert all(np.array_equal(ma[k][j], mb[k][j]) for j in ("mean", "std", "to_rgb"))
            elif k == "scale_factor":
                assert np.array_equal(ma[k], mb[k]) and ma[k].dtype == mb[k].dtype
            else:
                assert ma[k] == mb[k], k


# ------------------------------------------------------------------------------------------- 1. against the existing chain
@pytest.mark.parametrize("to_rgb", [True, False])
def test_frame_batch_equals_file_batch_and_restatement(frames, pngs, to_rgb):
    imgs, paths = frames[:3], pngs[:3]
    hw, Hp, Wp = _scaled(imgs, (64, 48))
    assert hw == [(45, 64), (48, 64), (64, 48)] and (Hp, Wp) == (64, 64)
    want = _restate(imgs, hw, Hp, Wp, to_rgb)
    files = _file_batch(_pipe("LoadImageFromFile", (64, 48), to_rgb), paths)
    # the restatement against the existing pipeline first: a mismatch below then points at the new kernel
    assert np.array_equal(files["img"][0].cpu().numpy(), want)
    got = _frame_batch(_pipe("LoadImageFromWebcam", (64, 48), to_rgb), imgs)
    assert got["img"][0].shape == (3, 3, 64, 64) and got["img"][0].dtype == torch.float32
    assert torch.equal(got["img"][0], files["img"][0])
    assert np.array_equal(got["img"][0].cpu().numpy(), want)
    _same_metas(files["img_metas"][0], got["img_metas"][0])
    # per-sample form: each sample's view is cut to its own pad_shape, as in the file path
    from radet_amd.datasets.loading import ImagePipeline
    p = ImagePipeline(_pipe("LoadImageFromWebcam", (64, 48), to_rgb))
    one = p(dict(img=imgs[0], bbox_fields=[], mask_fields=[], seg_fields=[]))
    assert torch.equal(one["img"][0], files["img"][0][0])


# ------------------------------------------------------------------------------------------- 2. edge shapes
def _launch(imgs, dst_hw, Hp, Wp, to_rgb, out=None):
    """radet_preprocess_frames on host frames uploaded back to back; `out` is pre-filled with NaN so that every element the
    kernel does not write shows"""
    from radet_amd import kernels as K
    from radet_amd.datasets.loading import frame_desc_rows
    dev = torch.device("cuda")
    buf = torch.from_numpy(np.concatenate([f.reshape(-1) for f in imgs])).to(dev)
    rows, offs, nbytes = frame_desc_rows(imgs, dst_hw, to_rgb, buf.data_ptr())
    assert nbytes == buf.numel()
    desc = torch.from_numpy(rows).to(dev)
    if out is None:
        out = torch.full((len(imgs), 3, Hp, Wp), float("nan"), device=dev)
    K.preprocess_frames(desc, len(imgs), Hp, Wp, *_norm_consts(), out)
    torch.cuda.synchronize()
    return out


EDGES = {
    "1x1_identity": ([(1, 1)], [(1, 1)], 8, 8),                     # destination smaller than one 256-thread block
    "1x1_upscaled": ([(1, 1)], [(5, 7)], 8, 8),
    "column_w1": ([(9, 1)], [(13, 1)], 16, 4),
    "column_widened": ([(9, 1)], [(13, 4)], 16, 4),
    "row_h1": ([(1, 9)], [(1, 13)], 2, 16),
    "plane_not_multiple_of_256": ([(11, 23), (30, 7)], [(17, 19), (16, 5)], 17, 19),      # 323 pixels: two blocks
    "b1_two_blocks": ([(20, 33)], [(15, 25)], 16, 32),
    "full_plane_no_padding": ([(6, 10)], [(16, 16)], 16, 16),
}


@pytest.mark.parametrize("case", sorted(EDGES))
def test_edge_shapes(case):
    src, dst, Hp, Wp = EDGES[case]
    rng = np.random.RandomState(len(case))
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in src]
    for to_rgb in (True, False):
        got = _launch(imgs, dst, Hp, Wp, to_rgb).cpu().numpy()
        assert np.array_equal(got, _restate(imgs, dst, Hp, Wp, to_rgb))          # (NaN left anywhere fails this)
        for g, (h, w) in zip(got, dst):
            assert (g[:, h:, :] == 0.0).all() and (g[:, :, w:] == 0.0).all()


def test_no_frames_no_launch_and_bad_sizes():
    from radet_amd import _lib, kernels as K
    out = torch.full((1, 3, 8, 8), 7.0, device="cuda")
    desc = torch.zeros(1, K.PREP_DESC_INTS, dtype=torch.int32, device="cuda")
    K.preprocess_frames(desc, 0, 8, 8, *_norm_consts(), out)                      # nimg = 0: OK, nothing written
    K.preprocess_frames(desc, 1, 0, 8, *_norm_consts(), out)                      # an empty plane: OK
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    for n, Hp, Wp in ((-1, 8, 8), (1, -8, 8), (1, 8, -8)):
        with pytest.raises(_lib.RadetHipError):
            _lib.call("radet_preprocess_frames", desc.data_ptr(), n, Hp, Wp, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ------------------------------------------------------------------------------------------- 3. device sources in place
def test_device_view_is_read_in_place(frames):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    big = torch.randint(0, 256, (60, 401), dtype=torch.uint8, generator=g).to(dev)
    view = big.as_strided((48, 64, 3), (401, 3, 1), 5 * 401 + 8)          # rows 401 bytes apart (> 3 * 64), an odd address
    assert view.data_ptr() % 2 == 1 and view.stride(0) > 3 * 64 and not view.is_contiguous()
    host = view.cpu().numpy().copy()
    before = big.clone()
    cfg = _pipe("LoadImageFromWebcam", (64, 48))
    a = _frame_batch(cfg, [view])
    b = _frame_batch(cfg, [host])
    torch.cuda.synchronize()
    assert torch.equal(a["img"][0], b["img"][0]) and torch.equal(big, before)
    _same_metas(b["img_metas"][0], a["img_metas"][0])
    # a batch that mixes host frames and device frames, the view resized this time
    cfg = _pipe("LoadImageFromWebcam", (40, 30))
    mixed = _frame_batch(cfg, [frames[0], view, torch.from_numpy(frames[2]).to(dev)])
    hosts = _frame_batch(cfg, [frames[0], host, frames[2]])
    torch.cuda.synchronize()
    assert torch.equal(mixed["img"][0], hosts["img"][0]) and torch.equal(big, before)


# ------------------------------------------------------------------------------------------- 4. / 5. the public interface
# The detector runs at img_scale (640, 480) on the landscape frames: the frames stay tiny (they resize to 447 x 640 and
# 480 x 640), and batches of 4, 2 and 1 images padded to 480 x 640 are geometries whose conv tile picks are pinned
# (radet_amd/tune_gfx950.json), so nothing is tuned while the tests run.
DET_FRAMES = (0, 1, 3, 4, 5)


@pytest.fixture(scope="module")
def det():
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


def _same_results(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert len(ra) == len(rb)
        for ca, cb in zip(ra, rb):
            assert ca.dtype == cb.dtype and np.array_equal(ca, cb)


def test_inference_detector_on_arrays_equals_files(det, frames, pngs):
    from radet_amd.apis import inference_detector
    imgs, paths = [frames[k] for k in DET_FRAMES[:4]], [pngs[k] for k in DET_FRAMES[:4]]
    batch = _file_batch(det.cfg.data.test.pipeline, paths)
    assert batch["img"][0].shape == (4, 3, 480, 640)
    with torch.no_grad():
        want = det(return_loss=False, rescale=True, **batch)
    got = inference_detector(det, imgs)
    n = sum(len(c) for r in want for c in r)
    print("detections:", n)
    assert len(got) == 4 and n > 0
    _same_results(got, want)
    # a single array is a batch of one and returns that frame's result
    one, as_list = inference_detector(det, imgs[1]), inference_detector(det, [imgs[1]])
    assert len(as_list) == 1 and len(one) == det.bbox_head.num_classes
    _same_results([one], as_list)
    # a device tensor takes the same path; the existing forms behave as before
    _same_results([inference_detector(det, torch.from_numpy(imgs[1]).cuda())], as_list)
    _same_results([inference_detector(det, paths[1])], as_list)
    _same_results(inference_detector(det, batch["img"][0][1:2, :, :480, :640], scale_factor=batch["img_metas"][0][1]["scale_factor"]),
                  as_list)
    assert det._frame_pipeline[1].frames                       # (built once, cached on the model)
    with pytest.raises(ValueError):
        inference_detector(det, imgs[1].astype(np.float32))


def test_detect_frames(det, frames):
    from radet_amd.apis import detect_frames, inference_detector
    from radet_amd.core.bbox import bbox2result
    frames = [frames[k] for k in DET_FRAMES]
    want = [r for lo in (0, 2, 4) for r in inference_detector(det, frames[lo:lo + 2])]
    assert len(want) == 5 and sum(len(c) for r in want for c in r) > 0
    got = list(detect_frames(det, iter(frames), batch_size=2))
    _same_results(got, want)
    raw = list(detect_frames(det, frames, batch_size=2, on_device=True))
    assert len(raw) == 5 and all(b.is_cuda and b.dtype == torch.float32 and l.dtype == torch.int64 for b, l in raw)
    _same_results([bbox2result(b, l, det.bbox_head.num_classes) for b, l in raw], want)
    # a generator dropped after its first result: the second batch is in flight; the runtime stays usable
    inference_detector(det, frames[0:2])                       # (makes the plan of two images the current one)
    own = {k: det.runtime().engine.buf[k].data_ptr() for k in ("cls", "reg_u", "iou")}
    it = detect_frames(det, frames, batch_size=2)
    _same_results([next(it)], want[:1])
    it.close()
    assert own == {k: det.runtime().engine.buf[k].data_ptr() for k in own}
    _same_results(inference_detector(det, frames[0:2]), want[0:2])
