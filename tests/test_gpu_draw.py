"""Detections drawn on frames on the device (radet_draw_detections): the kernel bit-equal to the NumPy restatement
(tests/_draw_ref.py) out of place and in place for every table of tests/_draw_cases.py at thickness 1, 2, 3 and 5, on the
scene of tests/test_gpu_crops.py (two host frames, a device view at an odd byte address with rows 401 bytes apart); canaries
around and under the destinations; the stand-alone op's two detection forms; the streaming API, show_result and
imshow_det_bboxes on a synth-initialised detector."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _draw_cases as C  # noqa: E402
import _draw_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
VIEW = ((40, 50, 3), (401, 3, 1), 5 * 401 + 8)          # the device view of the crops scene: shape, strides, offset
CANARY = 0xA5


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def scene():
    """frames: 37 x 53 and 64 x 48 host arrays and a 40 x 50 device view into a larger tensor (rows 401 bytes apart, an odd
    byte address); view_mask: the bytes of `big` that the view shows"""
    host, big = C.frames_host()
    big = big.cuda()
    view = big.as_strided(*VIEW)
    assert view.data_ptr() % 2 == 1 and view.stride(0) != 3 * 50 and not view.is_contiguous()
    mask = torch.zeros(big.numel(), dtype=torch.bool)
    mask.as_strided(*VIEW)[:] = True
    return dict(frames=[host[0], host[1], view], host=host, big=big, before=big.cpu().clone(), view_mask=mask.view(big.shape))


def _painter(case, thickness):
    from radet_amd.ops.draw import Painter
    return Painter(_dev(), **C.api_kwargs(case, thickness))


def _launch(painter, srcs, dsts, case, inplace):
    """one launch over the tables of srcs / dsts (device tensors), the detections of `case`"""
    from radet_amd import kernels as K
    from radet_amd.ops.crops import frame_table
    dev = _dev()
    b, s, l, c = (torch.from_numpy(a).to(dev) for a in C.padded(case))
    table, keep = frame_table(list(srcs) + list(dsts), dev)
    n = len(srcs) * K.PREP_DESC_INTS
    painter.launch(table[:n], table[n:] if not inplace else table[:n], len(srcs), max(f.shape[0] for f in srcs),
                   max(f.shape[1] for f in srcs), b, s, l, c, inplace)
    torch.cuda.synchronize()
    del keep


def _device_scene(scene, fill=None):
    """fresh device tensors shaped like the scene: frames 0 and 1 contiguous, frame 2 the strided view of a larger tensor;
    fill: a byte instead of the scene's pixels"""
    dev = _dev()
    if fill is None:
        big = scene["big"].clone()
        f = [torch.from_numpy(scene["host"][0]).to(dev), torch.from_numpy(scene["host"][1]).to(dev)]
    else:
        big = torch.full_like(scene["big"], fill)
        f = [torch.full(scene["host"][i].shape, fill, dtype=torch.uint8, device=dev) for i in (0, 1)]
    return f + [big.as_strided(*VIEW)], big


@pytest.mark.parametrize("thickness", C.THICKNESSES)
@pytest.mark.parametrize("case", sorted(C.CASES))
def test_kernel_is_the_restatement(scene, case, thickness):
    want = C.expected(case, thickness)
    painter = _painter(case, thickness)
    assert any((w != f).any() for w, f in zip(want, scene["host"]))                # (pixels do change)
    # out of place: host and device sources, destinations pre-filled with a canary come back fully written; the strided
    # destination's enclosing tensor keeps its canary everywhere else, the source's enclosing tensor is unchanged
    srcs, _ = _device_scene(scene)
    srcs[2] = scene["frames"][2]
    dsts, dbig = _device_scene(scene, fill=CANARY)
    _launch(painter, srcs, dsts, case, False)
    for b in range(3):
        assert np.array_equal(dsts[b].cpu().numpy(), want[b]), (case, thickness, b, "out of place")
    assert torch.equal(scene["big"].cpu(), scene["before"])
    assert (dbig.cpu()[~scene["view_mask"]] == CANARY).all()
    # in place: the same bytes; the enclosing tensor's other bytes unchanged
    frames, big = _device_scene(scene)
    _launch(painter, frames, frames, case, True)
    for b in range(3):
        assert np.array_equal(frames[b].cpu().numpy(), want[b]), (case, thickness, b, "in place")
    assert torch.equal(big.cpu()[~scene["view_mask"]], scene["before"][~scene["view_mask"]])
    # a table that mixes both without the flag: frame 1 in place (its destination row names its source), the others not
    frames, big = _device_scene(scene)
    dsts, dbig = _device_scene(scene, fill=CANARY)
    dsts[1] = frames[1]
    _launch(painter, frames, dsts, case, False)
    for b in range(3):
        assert np.array_equal(dsts[b].cpu().numpy(), want[b]), (case, thickness, b, "mixed")
    assert np.array_equal(frames[0].cpu().numpy(), scene["host"][0]) and torch.equal(big.cpu(), scene["before"])


def test_draw_detections_takes_both_forms_and_host_frames(scene):
    from radet_amd.ops import draw_detections
    case, t = "edges", 2
    want = C.expected(case, t)
    b, s, l, c = C.padded(case)
    kw = C.api_kwargs(case, t)
    host_before = [f.copy() for f in scene["host"]]
    out = draw_detections(scene["frames"], tuple(torch.from_numpy(a) for a in (b, s, l, c)), **kw)
    per_frame = [(torch.from_numpy(np.concatenate([b[i, :c[i]], s[i, :c[i], None]], 1)), torch.from_numpy(l[i, :c[i]]))
                 for i in range(3)]
    out2 = draw_detections(scene["frames"], per_frame, **kw)
    base = out[0].untyped_storage().data_ptr()
    for i in range(3):
        assert out[i].is_cuda and out[i].dtype == torch.uint8 and tuple(out[i].shape) == scene["host"][i].shape
        assert out[i].untyped_storage().data_ptr() == base                         # views of one allocation
        assert np.array_equal(out[i].cpu().numpy(), want[i]) and torch.equal(out[i], out2[i])
        assert np.array_equal(scene["host"][i], host_before[i])
    assert torch.equal(scene["big"].cpu(), scene["before"])
    # in place: device tensors only, and they are the frames themselves
    frames, big = _device_scene(scene)
    got = draw_detections(frames, per_frame, inplace=True, **kw)
    torch.cuda.synchronize()
    assert all(g is f for g, f in zip(got, frames)) and all(np.array_equal(f.cpu().numpy(), w) for f, w in zip(frames, want))
    with pytest.raises(ValueError, match="in place"):
        draw_detections(scene["frames"], per_frame, inplace=True, **kw)
    with pytest.raises(ValueError):
        draw_detections(scene["frames"][:2], per_frame, **kw)
    with pytest.raises(ValueError):
        draw_detections([scene["frames"][2].permute(1, 0, 2)], per_frame[:1], **kw)     # pixels not contiguous


def test_bad_arguments_are_refused_before_any_launch(scene):
    from radet_amd import kernels as K
    from radet_amd._lib import RadetHipError
    from radet_amd.ops.crops import frame_table
    dev = _dev()
    frames, _ = _device_scene(scene)
    before = [f.clone() for f in frames]
    b, s, l, c = (torch.from_numpy(a).to(dev) for a in C.padded("edges"))
    table, keep = frame_table(frames, dev)
    cov, widths = (torch.from_numpy(a).to(dev) for a in C.atlas_for("edges"))
    pal = torch.zeros(5, 3, dtype=torch.uint8, device=dev)

    def call(**kw):
        a = dict(thickness=2, box_colour=255, palette=None, text_colour=255, a_bg=204, score_thr=0.3, max_dets=256, n_names=5, pad=2,
                 inplace=True, atlas=cov, widths=widths)
        a.update(kw)
        K.draw_detections(table, table, 3, 64, 53, b, s, l, c, **a)
    for kw in (dict(thickness=0), dict(thickness=K.DRAW_MAX_THICKNESS + 1), dict(max_dets=K.DRAW_MAX_DETS + 1), dict(a_bg=256),
               dict(text_colour=1 << 24), dict(pad=K.DRAW_MAX_PAD + 1), dict(n_names=cov.shape[0]), dict(score_thr=float("nan"))):
        with pytest.raises(RadetHipError):
            call(**kw)
    with pytest.raises(AssertionError):
        call(box_colour=None)                                    # neither a colour nor a palette
    call(box_colour=None, palette=pal, max_dets=0)               # nothing drawn, in place: nothing stored
    torch.cuda.synchronize()
    assert all(torch.equal(f, g) for f, g in zip(frames, before))
    del keep


# --------------------------------------------------------------------------------------------------- the public interface
def _pipe(loader, scale):
    return [dict(type=loader),
            dict(type="MultiScaleFlipAug", img_scale=scale, flip=False, transforms=[
                dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", **NORM),
                dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])])]


@pytest.fixture(scope="module")
def det():
    """the detector of tests/test_gpu_crops.py: batches of 2 and 1 small landscape frames padded to 480 x 640"""
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


def test_draw_frames_streams_detections_and_overlays(det):
    from radet_amd.apis import detect_frames, draw_frames
    from radet_amd.ops import draw_detections
    rng = np.random.RandomState(11)
    frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (48, 64), (60, 80))]
    before = [f.copy() for f in frames]
    n_cls = det.bbox_head.num_classes
    names = [f"c{i}" for i in range(n_cls)]
    atlas = R.synthetic_atlas(n_cls)
    thr = 0.1
    style = dict(class_names=names, score_thr=thr, bbox_color="class", text_color=(10, 200, 250), thickness=2, font_size=13,
                 atlas=atlas)
    from radet_amd.ops.draw import class_palette
    st = R.Style(2, None, class_palette(n_cls), (10, 200, 250), 204, thr, 256, n_cls, 2)
    plain = list(detect_frames(det, frames, batch_size=2, on_device=True))
    plain_host = list(detect_frames(det, frames, batch_size=2))
    both = list(draw_frames(det, frames, batch_size=2, on_device=True, **style))
    both_host = list(draw_frames(det, frames, batch_size=2, **style))
    assert len(both) == len(both_host) == 3
    drawn = 0
    for i, f in enumerate(frames):
        (b0, l0), ((b1, l1), img) = plain[i], both[i]
        assert torch.equal(b0, b1) and torch.equal(l0, l1)                          # detections: bit-equal to detect_frames'
        res_h, img_h = both_host[i]
        assert len(res_h) == n_cls and all(np.array_equal(x, y) for x, y in zip(res_h, plain_host[i]))
        assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == f.shape
        assert isinstance(img_h, np.ndarray) and np.array_equal(img_h, img.cpu().numpy())
        want_op = draw_detections([f], [(b1, l1)], **style)[0]
        assert torch.equal(img, want_op)                                            # == the stand-alone op on the yielded dets
        k = int(b1.shape[0])
        boxes = b1.cpu().numpy()
        want = R.gather_frame(f, boxes[:, :4], boxes[:, 4], l1.cpu().numpy(), k, st, atlas)
        assert np.array_equal(img_h, want)                                          # == the restatement
        assert np.array_equal(R.painter_frame(f, boxes[:, :4], boxes[:, 4], l1.cpu().numpy(), k, st, atlas), want)
        drawn += int((boxes[:, 4] > np.float32(thr)).sum())
        assert np.array_equal(f, before[i])                                         # the caller's arrays are unchanged
    assert drawn >= 1 and any((img_h != f).any() for (_, img_h), f in zip(both_host, frames))
    # device frames from the caller: copied unless inplace=True
    dev_frames = [torch.from_numpy(f).cuda() for f in frames]
    out = list(draw_frames(det, dev_frames, batch_size=2, on_device=True, **style))
    for i, ((b1, l1), img) in enumerate(out):
        assert torch.equal(img, both[i][1]) and torch.equal(dev_frames[i].cpu(), torch.from_numpy(frames[i]))
    out = list(draw_frames(det, dev_frames, batch_size=2, on_device=True, inplace=True, **style))
    for i, ((b1, l1), img) in enumerate(out):
        assert img is dev_frames[i] and torch.equal(img, both[i][1])
    with pytest.raises(ValueError, match="in place"):
        list(draw_frames(det, frames, batch_size=2, inplace=True, **style))
    with pytest.raises(TypeError):
        list(draw_frames(det, frames, colour="red"))


def test_show_result_and_imshow_write_what_they_return(det, tmp_path):
    from PIL import Image
    from radet_amd.apis import inference_detector
    from radet_amd.core.visualization import imshow_det_bboxes, result_to_dets
    rng = np.random.RandomState(11)
    frame = rng.randint(0, 256, (60, 80, 3)).astype(np.uint8)
    result = inference_detector(det, frame)
    bboxes, labels = result_to_dets(result)
    assert (bboxes[:, 4] > 0.1).any()
    out = det.show_result(frame, result, score_thr=0.1, out_file=str(tmp_path / "a" / "shown.png"))
    back = np.asarray(Image.open(tmp_path / "a" / "shown.png").convert("RGB"))[..., ::-1]
    assert out.shape == frame.shape and out.dtype == np.uint8 and np.array_equal(back, out) and (out != frame).any()
    out2 = imshow_det_bboxes(frame, bboxes, labels, class_names=None, score_thr=0.1, bbox_color=(72, 101, 241),
                             text_color=(72, 101, 241), show=False, out_file=str(tmp_path / "b.png"))
    back2 = np.asarray(Image.open(tmp_path / "b.png").convert("RGB"))[..., ::-1]
    assert np.array_equal(back2, out2) and np.array_equal(out2, out)
    # img may be a file name
    Image.fromarray(np.ascontiguousarray(frame[..., ::-1])).save(tmp_path / "in.png")
    assert np.array_equal(det.show_result(str(tmp_path / "in.png"), result, score_thr=0.1), out)
