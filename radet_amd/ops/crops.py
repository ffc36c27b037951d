"""Detections -> a packed batch of RoI crops on the device (radet_amd/csrc/crops.hip): what a downstream pose network
consumes -- one window per detection, cut from the original frame, resized to one fixed size and normalised -- without
pulling boxes to the host.  `crop_detections` is the stand-alone entry point; DetectorRuntime runs the same two launches
behind decode + NMS (`inference_detector(..., crops=...)`, `detect_frames(..., crops=...)`)."""
import logging
import numbers
from collections import namedtuple

import numpy as np
import torch

from .. import kernels as K

Crops = namedtuple("Crops", "images windows index n_total")
Crops.__doc__ = """images: f32 [n,3,Ho,Wo] (normalised) or u8 [n,Ho,Wo,3] (raw BGR) on the device; windows i32 [n,4] = (x0, y0,
w, h) of each crop's source window in frame pixels (it may overhang the frame: the fill colour shows there); index i32 [n,2]
= (frame, rank of the detection in that frame); n_total: the number of valid detections, > n when max_crops cut the list.

Crop pixel (u, v) shows the frame at  x_frame = x0 + (u + 0.5) * w / Wo - 0.5,  y_frame = y0 + (v + 0.5) * h / Ho - 0.5
(pixel centres at integers): a pose network moves its intrinsics with  fx' = fx * Wo / w,  cx' = (cx - x0 + 0.5) * Wo / w -
0.5, and likewise for y.  w / h == Wo / Ho up to the rounding of the sides to whole pixels."""

CropSpec = namedtuple("CropSpec", "size scale score_thr max_crops fill mean stdinv to_rgb")


def crop_spec(size, scale=1.2, score_thr=0.0, max_crops=None, fill=(0, 0, 0), normalize=None):
    """the checked arguments of a crop request (nothing is approximated: what the kernels do not do is refused)"""
    def _int(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool)
    hw = (size, size) if _int(size) else tuple(size) if isinstance(size, (tuple, list)) else None
    if hw is None or len(hw) != 2 or not all(_int(v) and v > 0 for v in hw):
        raise ValueError(f"crops: size={size!r} is not one or two positive ints (Ho, Wo)")
    if max(hw) > K.CROP_MAX_OUT:
        raise ValueError(f"crops: size={size!r} exceeds the kernel's largest side ({K.CROP_MAX_OUT})")
    if not isinstance(scale, numbers.Real) or not np.isfinite(scale) or not scale > 0:
        raise ValueError(f"crops: scale={scale!r} must be a finite number > 0")
    if not isinstance(score_thr, numbers.Real) or np.isnan(score_thr):
        raise ValueError(f"crops: score_thr={score_thr!r}")
    fill = tuple(fill) if isinstance(fill, (tuple, list, np.ndarray)) else None
    if fill is None or len(fill) != 3 or not all(_int(v) and 0 <= v <= 255 for v in fill):
        raise ValueError("crops: fill must be three integers in [0, 255] (the frames' channel order, BGR)")
    if max_crops is not None and (not _int(max_crops) or max_crops < 0):
        raise ValueError(f"crops: max_crops={max_crops!r}")
    if max_crops is not None and max_crops > K.CROP_MAX_SLOTS:
        raise ValueError(f"crops: max_crops={max_crops} exceeds the kernel's {K.CROP_MAX_SLOTS} slots; crop in several calls")
    mean = stdinv = None
    to_rgb = False
    if normalize is not None:
        cfg = dict(normalize)
        if set(cfg) - {"mean", "std", "to_rgb"} or "mean" not in cfg or "std" not in cfg:
            raise ValueError(f"crops: normalize={normalize!r} is not dict(mean, std, to_rgb)")
        m, s = np.asarray(cfg["mean"], np.float32).reshape(-1), np.asarray(cfg["std"], np.float32).reshape(-1)
        if m.size != 3 or s.size != 3 or not np.isfinite(m).all() or not (np.isfinite(s) & (s != 0)).all():
            raise ValueError(f"crops: normalize={normalize!r} needs three finite means and three finite non-zero stds")
        # Normalize's constants as the frame pipeline rounds them (datasets/loading.py)
        mean, stdinv = m.astype(np.float64).astype(np.float32), (1.0 / s.astype(np.float64)).astype(np.float32)
        to_rgb = bool(cfg.get("to_rgb", True))
    return CropSpec(tuple(int(v) for v in hw), float(scale), float(score_thr), None if max_crops is None else int(max_crops),
                    int(fill[0]) | int(fill[1]) << 8 | int(fill[2]) << 16, mean, stdinv, to_rgb)


def check_frames(frames):
    """crops are cut from loaded frames (HxWx3 uint8, host arrays or device tensors): file names and normalised NCHW
    tensors have no source pixels on the device in frame coordinates"""
    ok = isinstance(frames, (list, tuple)) and len(frames) > 0
    for f in frames if ok else ():
        if isinstance(f, np.ndarray):
            ok = ok and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3
        else:
            ok = ok and isinstance(f, torch.Tensor) and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3
    if not ok:
        raise ValueError("crops are cut from loaded frames: pass a list of HxWx3 uint8 frames (ndarrays or device tensors), not "
                         "file names or a normalised NCHW tensor")


def frame_table(frames, dev):
    """-> (desc i32 [B, PREP_DESC_INTS] on the device, what keeps its addresses valid): host frames go up packed behind the
    table in one pinned copy, device frames are read where they are (ImagePipeline._run_frames' upload)"""
    from ..datasets.loading import upload_frames
    for f in frames:
        if isinstance(f, torch.Tensor) and (f.device != dev or f.stride(2) != 1 or f.stride(1) != 3):
            raise ValueError(f"a frame on {f.device} with strides {tuple(f.stride())}: frames are on {dev}, pixels contiguous")
    table = upload_frames(frames, [tuple(int(v) for v in f.shape[:2]) for f in frames], False, dev)
    return table, (table, list(frames))


def launch_crops(spec, boxes, scores, counts, desc, cap, counters):
    """the two launches on the current stream: -> (images [cap, ...], rows i32 [cap, CROP_ROW_INTS]); counters i32 [2 + B],
    zeroed, receives {n_out, n_total, where each frame's rows end}.  Nothing is read back."""
    dev = boxes.device
    B = int(boxes.shape[0])
    Ho, Wo = spec.size
    rows = torch.empty(max(cap, 1), K.CROP_ROW_INTS, dtype=torch.int32, device=dev)
    if spec.mean is not None:
        images = torch.empty(cap, 3, Ho, Wo, dtype=torch.float32, device=dev)
    else:
        images = torch.empty(cap, Ho, Wo, 3, dtype=torch.uint8, device=dev)
    if cap > 0 and B > 0 and boxes.shape[1] > 0:
        K.crop_plan(boxes, scores, counts, spec.size, spec.scale, spec.score_thr, cap, rows, counters)
        K.crop_frames(rows, counters, desc, B, cap, spec.size, images, spec.fill, spec.mean, spec.stdinv, spec.to_rgb)
    return images, rows


def collect_crops(images, rows, n_out, n_total):
    """the record of the first n_out slots (views, no copies of the pixels); says so when detections were left out"""
    n_out, n_total = int(n_out), int(n_total)
    if n_total > n_out:
        logging.getLogger("radet_amd").warning("crops: %d valid detections, %d slots: the last %d have no crop (max_crops)",
                                               n_total, n_out, n_total - n_out)
    r = rows[:n_out]
    return Crops(images[:n_out], r[:, 2:6].contiguous(), r[:, 0:2].contiguous(), n_total)


def split_crops(crops, ends):
    """the per-frame records of a batch's crops: ends[b] = where frame b's rows end (the plan's counters from the third on,
    already on the host -- nothing is read from the device here); views of the batch's tensors, n_total stays the batch's"""
    out, lo = [], 0
    for hi in ends:
        hi = int(hi)
        out.append(Crops(crops.images[lo:hi], crops.windows[lo:hi], crops.index[lo:hi], crops.n_total))
        lo = hi
    return out


def _padded(dets, dev):
    """list of (f32 [k,5], labels) per frame, or (boxes [B,K,4], scores [B,K], counts [B]) -> the padded triple on dev"""
    if isinstance(dets, (tuple, list)) and len(dets) == 3 and torch.is_tensor(dets[0]) and dets[0].dim() == 3:
        boxes, scores, counts = dets
        boxes, scores = boxes.to(dev, torch.float32).contiguous(), scores.to(dev, torch.float32).contiguous()
        counts = torch.as_tensor(counts).to(dev, torch.int32).contiguous()
        if boxes.shape[2] != 4 or tuple(scores.shape) != tuple(boxes.shape[:2]) or counts.numel() != boxes.shape[0]:
            raise ValueError(f"crops: boxes {tuple(boxes.shape)}, scores {tuple(scores.shape)}, counts {tuple(counts.shape)}")
        return boxes, scores, counts
    per = []
    for d in dets:
        d = d[0] if isinstance(d, (tuple, list)) else d
        d = torch.as_tensor(d).to(dev, torch.float32).reshape(-1, 5)
        per.append(d)
    Kd = max([int(d.shape[0]) for d in per] + [1])
    boxes = torch.zeros(len(per), Kd, 4, device=dev)
    scores = torch.zeros(len(per), Kd, device=dev)
    for i, d in enumerate(per):
        boxes[i, :d.shape[0]] = d[:, :4]
        scores[i, :d.shape[0]] = d[:, 4]
    counts = torch.tensor([int(d.shape[0]) for d in per], dtype=torch.int32).to(dev)
    return boxes, scores, counts


def crop_detections(frames, dets, size, scale=1.2, score_thr=0.0, max_crops=None, fill=(0, 0, 0), normalize=None):
    """One crop per detection, cut from its frame on the device and resized to `size` = (Ho, Wo) (an int: square).

    frames: list of HxWx3 uint8 BGR frames, ndarrays or device tensors (views into larger tensors are read in place), sizes
    may differ.  dets: per frame (dets f32 [k,5], labels) as `detect_frames(on_device=True)` yields them (or just the
    [k,5] tensors), or the padded NMS outputs (boxes [B,K,4], scores [B,K], counts [B]); boxes in frame pixels.
    The window of a detection is its box grown by `scale` and widened to the output's aspect ratio around the box centre
    (include/radet_hip.h, radet_crop_plan); outside the frame it shows `fill` (BGR).  Detections below score_thr, with a
    non-finite coordinate or an empty box get no crop; at most max_crops (default: all, at most 65535) are kept, in order.
    normalize=dict(mean, std, to_rgb) -> f32 [n,3,Ho,Wo] like the test pipeline's Normalize; None -> u8 [n,Ho,Wo,3], raw BGR.
    Pixels: the project's 8-bit INTER_LINEAR (cv2.resize restated; parity with cv2 itself unpinned).
    Returns a `Crops` record (see its docstring for the crop -> frame map).  One host synchronisation (the crop count).
    Memory: max_crops slots (default: every detection slot handed in, B * K) of 3 * Ho * Wo values are allocated before the
    count is known, and the record's views keep all of them alive: pass max_crops where the slots far outnumber the detections."""
    spec = crop_spec(size, scale, score_thr, max_crops, fill, normalize)
    check_frames(frames)
    from . import _dev
    dev = _dev()
    boxes, scores, counts = _padded(dets, dev)
    if boxes.shape[0] != len(frames):
        raise ValueError(f"crops: {len(frames)} frames, detections of {boxes.shape[0]}")
    B, Kd = int(boxes.shape[0]), int(boxes.shape[1])
    if B * Kd >= 2 ** 31:
        raise ValueError(f"crops: {B} x {Kd} detection slots")
    cap = spec.max_crops if spec.max_crops is not None else B * Kd
    if cap > K.CROP_MAX_SLOTS:
        raise ValueError(f"crops: {cap} detection slots exceed the kernel's {K.CROP_MAX_SLOTS}; pass max_crops or crop in "
                         "several calls")
    desc, keep = frame_table(frames, dev)
    counters = torch.zeros(2 + B, dtype=torch.int32, device=dev)
    images, rows = launch_crops(spec, boxes, scores, counts, desc, cap, counters)
    n_out, n_total = counters[:2].cpu().tolist()                    # (the host waits here: `keep` outlives the launches)
    del keep
    return collect_crops(images, rows, n_out, n_total)
