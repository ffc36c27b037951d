"""The image side of the reference's BOP data pipelines (radet/datasets/pipelines: loading.py, transforms.py,
color_aug.py, formating.py, test_time_aug.py) under the reference's stage names and constructor arguments.

Every stage has a host part, `plan(s, rnd, nprnd)`: file decoding (Pillow, into BGR u8 like mmcv.imfrombytes), box
arithmetic (NumPy, mmdet 2.x Resize / RandomFlip.bbox_flip) and every random draw, in the reference's order, on the
sample's own generators (`rnd`: a random.Random or the `random` module, `nprnd`: a RandomState or `np.random`).  Planning
touches no device, so the loader runs it on host threads.  `ImagePipeline.run(planned)` then does the device part of a
whole batch on the calling thread and stream: the resize of images and backgrounds (radet_resize_linear_u8), mask
normalisation / resize / flip (radet_mask_transform; radet_rle_masks for masks annotated as run lists or polygons), the four augmentation launches of csrc/augment.hip (a mixpbr
pipeline: merge, hsv_noise, box, finish), the box crops / distance maps of a mask-free GenerateDistanceMap
(radet_crop_canvases, the ops' packed GDT / MBD chain, radet_paste_maps) and the label assigner -- a fixed number of
launches whatever the batch size.  With decode="device" on LoadImageFromFile / RandomBackground the host reads the file,
its headers and its scan index (radet_amd/core/jpeg.py) and run() decodes the batch's baseline JPEGs in front of the
resize (radet_jpeg_decode, three launches); files outside the decoder's subset are decoded by Pillow as before.  With
sample_cache='device' decoded frames and backgrounds stay in HBM after their first visit and later batches gather them
with one radet_copy_segments launch (sample_cache.py).  A single sample (`BOPDataset.__getitem__`) is a batch
of one.  A pipeline whose first stage is LoadImageFromWebcam takes frames that are in memory already (ndarray or device
tensor): a test pipeline, whose run() is one pinned upload and one radet_preprocess_frames launch (_run_frames).
Windows: every sample has one view (sample_view; the view row of include/radet_hip.h) -- the window of the source that is
resized, the virtual resized size, and the window of that which is computed -- and the resize and both mask kernels take
one such row per image or mask.  Scale jitter (Resize with random scales, RandomCrop, Pad(size=)): RandomCrop plans the
output window (s["crop_window"]) and run() computes that window only, so a batch keeps one tensor shape at the cost of the
crop's pixels.  Zoom (Expand, MinIoURandomCrop, in front of Resize): the stages plan the source window in image coordinates,
which may overhang the image (s["src_window"]); run() resizes that window straight from the image, the canvas fill where
it overhangs; no canvas is ever made.
Affine augmentation (Rotate, Shear, Translate, or one AutoAugment over them, directly after Resize): the stages plan boxes
and leave forward matrices in s["affine"]; run() warps the resized frames and the resized, unflipped masks once per
entry (radet_warp_affine_u8: cv2.warpAffine's classic fixed-point bilinear path), in front of the merge and the flip.
CutOut (in that block, bare or in AutoAugment policies, or behind the photometric stages in front of RandomFlip): the stage
plans its holes; run() fills them per entry rank on the packed u8 frames (radet_cutout_u8, next to the warp launch of that
rank) or, for the late position, in the finished f32 batch (radet_cutout_f32 after radet_augment_finish).
Colour stages (ColorTransform, EqualizeTransform, BrightnessTransform, ContrastTransform, in that block, bare or in the
policies of an AutoAugment(color_stages=True)): the stage plans its gate and factor; run() maps the packed u8 frames at the entry's rank
(radet_color_stats_u8 for the histograms Equalize and Contrast need, radet_color_apply_u8 in place).
Options the RADet configs do not use raise NotImplementedError."""
import collections
import glob
import math
import os
import struct
import threading

import numpy as np
import torch

from .. import kernels as K
from ..core import jpeg, rle
from ..core.mask import rescale_size
from ..utils import build_from_cfg
from .pipelines import PIPELINES, GenerateDistanceMap, LabelAssignment
from .sample_cache import CachedImage, SampleCache, cache_args, normalised_runs

osp = os.path
DEFAULT_META_KEYS = ("filename", "ori_filename", "ori_shape", "img_shape", "pad_shape", "scale_factor", "flip",
                     "flip_direction", "img_norm_cfg")
# stage order of the device part (a pipeline lists a subsequence of it; MultiScaleFlipAug's transforms sit in its place)
_ORDER = ("LoadImageFromFile", "LoadAnnotations", "MultiScaleFlipAug", "Expand", "MinIoURandomCrop", "Resize", "RandomCrop", "Affine", "RandomBackground", "CosyPoseAug", "RandomHSV",
          "RandomNoise", "RandomSmooth", "CutOut", "RandomFlip", "GenerateDistanceMap", "LabelAssignment", "Normalize", "Pad",
          "DefaultFormatBundle", "ImageToTensor", "Collect")
_ZOOM = ("Expand", "MinIoURandomCrop")                       # the source-window stages
_AFFINE = ("Rotate", "Shear", "Translate", "AutoAugment")    # the warp stages: one block in the "Affine" slot of _ORDER
# what may stand in that block (a CutOut elsewhere is a late one; a colour stage elsewhere is refused)
_BLOCK = _AFFINE + ("CutOut", "ColorTransform", "EqualizeTransform", "BrightnessTransform", "ContrastTransform")
_MIX = ("RandomHSV", "RandomNoise", "RandomSmooth")          # the mixpbr stages: aug_hsv_noise + aug_box
_COSY_ORDER = ("PillowBlur", "PillowSharpness", "PillowContrast", "PillowBrightness", "PillowColor")
# flags of a params row (include/radet_hip.h)
F_MERGE, F_BLUR, F_SHARP, F_CONTRAST, F_BRIGHT, F_COLOR, F_FLIP, F_TO_RGB = 1, 2, 4, 8, 16, 32, 64, 128
# flags of a params2 row (the mixpbr stages)
F2_HSV, F2_NOISE, F2_BOX = 1, 2, 4


def _refuse(what):
    raise NotImplementedError(f"{what} is not used by the RADet configs and is not implemented")


def decode_bgr(path):
    """mmcv.imfrombytes(flag='color') with Pillow: 3-channel BGR u8"""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[..., ::-1])


def _decode_arg(decode):
    if decode not in ("host", "device"):
        raise ValueError(f"decode is 'host' or 'device', got {decode!r}")
    return decode


_CACHE_LOCK = threading.Lock()


def _plan_image(path, stage):
    """the image of a decode='device' stage: a jpeg.DeviceJpeg (bytes, header, scan index; nothing decoded), or the host's
    pixels for a file the device decoder does not take"""
    if stage.cache is None:                      # (a stage used outside an ImagePipeline; the pipeline sets a shared cache)
        with _CACHE_LOCK:
            if stage.cache is None:
                stage.cache = jpeg.IndexCache(stage.index_cache)
    item = jpeg.plan_file(path, stage.cache, stage.seg_mcus)
    return decode_bgr(path) if item is None else item


def _plan_pixels(path, stage, s, field):
    """s[field] of a LoadImageFromFile / RandomBackground stage: with a sample cache, the placeholder of a cached file (one
    stat, the file is not opened) or the file's key in s["_cache_keys"][field] for run() to enter it; then the stage's decode"""
    if stage.sample_cache is not None:
        hit, key = stage.sample_cache.lookup(path)
        if hit is not None:
            return hit
        s.setdefault("_cache_keys", {})[field] = key
    return decode_bgr(path) if stage.decode == "host" else _plan_image(path, stage)


def decode_unchanged(path):
    """mmcv.imfrombytes(flag='unchanged') of an 8-bit single-channel mask PNG"""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im) if im.mode in ("L", "P", "1") else np.asarray(im.convert("L"))


def blur_params(k):
    """PIL ImagingGaussianBlur(radius k, 3 passes) -> (box radius, ww, fw) of ImagingHorizontalBoxBlur: the box length of
    the extended box blur in float32 (sqrt and floor in double, as the C code promotes them), then 24-bit fixed-point weights"""
    f = np.float32
    sigma2 = f(f(k) * f(k)) / f(3)
    L = f(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f(math.floor((float(L) - 1.0) / 2.0))
    a = f(f(f(2) * l + f(1)) * f(l * f(l + f(1)) - f(3) * sigma2))
    a = f(a / f(f(6) * f(sigma2 - f(l + f(1)) * f(l + f(1)))))
    radius = f(l + a)
    ww = int(f(1 << 24) / f(radius * f(2) + f(1)))
    return int(radius), ww, ((1 << 24) - (2 * int(radius) + 1) * ww) // 2


def _f32_bits(v):
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


# ---------------------------------------------------------------------------------------------------- loading
@PIPELINES.register_module()
class LoadImageFromFile:
    def __init__(self, to_float32=False, color_type="color", file_client_args=None, decode="host", index_cache=None,
                 seg_mcus=jpeg.DEFAULT_SEG_MCUS):
        """decode='device': plan() reads the file and its scan index, ImagePipeline.run decodes the batch on the GPU
        (baseline JPEG; any other file is decoded here as with 'host'); index_cache: a directory for the scan indexes"""
        self.decode, self.index_cache, self.seg_mcus, self.cache = _decode_arg(decode), index_cache, seg_mcus, None
        self.sample_cache = None                      # (an ImagePipeline with sample_cache='device' sets its cache here)
        if to_float32:
            _refuse("LoadImageFromFile(to_float32=True)")
        if color_type != "color":
            _refuse(f"LoadImageFromFile(color_type={color_type!r})")
        if file_client_args not in (None, dict(backend="disk")):
            _refuse(f"LoadImageFromFile(file_client_args={file_client_args})")

    def plan(self, s, rnd, nprnd):
        name = s["img_info"]["filename"]
        s["filename"] = osp.join(s["img_prefix"], name) if s.get("img_prefix") is not None else name
        s["ori_filename"] = name
        s["img"] = _plan_pixels(s["filename"], self, s, "img")
        s["img_shape"] = s["ori_shape"] = s["pad_shape"] = s["img"].shape
        s["img_fields"] = ["img"]


@PIPELINES.register_module()
class LoadImageFromWebcam:
    """The frame is in results["img"] already (radet/datasets/pipelines/loading.py:88): an ndarray HxWx3 uint8 in BGR order, as
    mmcv.imread gives, or a torch.uint8 tensor of that shape -- on the device it is read in place by ImagePipeline.run,
    also as a view into a larger tensor (rows may be strided; the 3 bytes of a pixel and the pixels of a row are contiguous)"""

    def __init__(self, to_float32=False, color_type="color", file_client_args=None):
        if to_float32:
            _refuse("LoadImageFromWebcam(to_float32=True)")
        if color_type != "color":
            _refuse(f"LoadImageFromWebcam(color_type={color_type!r})")
        if file_client_args not in (None, dict(backend="disk")):
            _refuse(f"LoadImageFromWebcam(file_client_args={file_client_args})")

    def plan(self, s, rnd, nprnd):
        img = s["img"]
        if isinstance(img, torch.Tensor) and not img.is_cuda and img.dtype == torch.uint8:
            img = img.numpy()                                   # (a host tensor is a host frame)
        if not isinstance(img, (np.ndarray, torch.Tensor)):
            raise ValueError(f"LoadImageFromWebcam takes an ndarray or a torch tensor HxWx3 uint8, got {type(img).__name__}")
        u8 = img.dtype == (np.uint8 if isinstance(img, np.ndarray) else torch.uint8)
        if not u8 or len(img.shape) != 3 or img.shape[2] != 3 or 0 in img.shape:
            raise ValueError(f"LoadImageFromWebcam takes a frame HxWx3 uint8 (BGR), got {img.dtype} of shape {tuple(img.shape)}")
        if isinstance(img, torch.Tensor):
            h, w = img.shape[:2]
            sy, sx, sc = img.stride()
            if sc != 1 or (w > 1 and sx != 3) or (h > 1 and sy >= 2 ** 31):
                raise ValueError(f"LoadImageFromWebcam reads a device frame in place: its pixels must be 3 contiguous bytes and "
                                 f"the pixels of a row contiguous, got strides {tuple(img.stride())} for shape {tuple(img.shape)}")
        s["filename"] = s["ori_filename"] = None
        s["img"] = img
        s["img_shape"] = s["ori_shape"] = s["pad_shape"] = tuple(img.shape)
        s["img_fields"] = ["img"]


@PIPELINES.register_module()
class LoadAnnotations:
    def __init__(self, with_bbox=True, with_label=True, with_mask=False, with_seg=False, with_bop_mask=False, poly2mask=True,
                 file_client_args=None):
        if with_seg:
            _refuse("LoadAnnotations(with_seg)")
        if with_mask and not poly2mask:
            _refuse("LoadAnnotations(with_mask=True, poly2mask=False) (PolygonMasks)")
        if with_mask and with_bop_mask:
            _refuse("LoadAnnotations(with_mask=True, with_bop_mask=True) (two sources for gt_masks)")
        self.with_bbox, self.with_label, self.with_bop_mask, self.with_mask = with_bbox, with_label, with_bop_mask, with_mask
        self.sample_cache = None

    def plan(self, s, rnd, nprnd):
        ann = s["ann_info"]
        if self.with_bbox:
            s["gt_bboxes"] = np.asarray(ann["bboxes"], np.float32).reshape(-1, 4).copy()
            if ann.get("bboxes_ignore") is not None:
                s["gt_bboxes_ignore"] = np.asarray(ann["bboxes_ignore"], np.float32).reshape(-1, 4).copy()
                s["bbox_fields"].append("gt_bboxes_ignore")
            s["bbox_fields"].append("gt_bboxes")
        if self.with_label:
            s["gt_labels"] = np.asarray(ann["labels"], np.int64).copy()
        if self.with_bop_mask:
            h, w = s["img_info"]["height"], s["img_info"]["width"]
            paths = [osp.join(s["seg_prefix"], p) for p in ann["masks"]]
            cache = self.sample_cache
            looked = [cache.mask_lookup(p, (h, w)) for p in paths] if cache is not None else None
            if looked is not None and all(runs is not None for runs, _ in looked):
                # every mask file was seen before: their run lists (sample_cache.normalised_runs) take the radet_rle_masks path
                s["gt_masks_rle"] = ([[runs] for runs, _ in looked], (h, w))
                cache.count_mask_hits(len(looked))
            else:
                masks = [decode_unchanged(p) for p in paths]
                for m in masks:
                    if m.shape != (h, w):
                        raise ValueError(f"mask of shape {m.shape} for an image of {h} x {w}")
                for m, (runs, key) in zip(masks, looked or ()):
                    if runs is None:
                        cache.mask_insert(key, normalised_runs(m), (h, w))
                s["gt_masks"] = np.stack(masks) if masks else np.zeros((0, h, w), np.uint8)
            s["mask_fields"].append("gt_masks")
        if self.with_mask:
            # the `segmentation` objects of the annotation file (polygons, run lists, compressed run lists) as run lists:
            # nothing is decoded to pixels here, radet_rle_masks does that for the whole batch (ImagePipeline._masks)
            h, w = s["img_info"]["height"], s["img_info"]["width"]
            ids = ann.get("ann_ids") or range(len(ann["masks"]))
            name = s["img_info"].get("filename", s["img_info"].get("file_name"))
            s["gt_masks_rle"] = ([rle.parts_from_segmentation(seg, h, w, f"{name}, record {k}") for seg, k in zip(ann["masks"], ids)],
                                 (h, w))
            s["mask_fields"].append("gt_masks")


# ---------------------------------------------------------------------------------------------------- geometry
@PIPELINES.register_module()
class Resize:
    """One scale, or the reference's random scales (transforms.py:97-200), drawn from the sample's NumPy generator with the
    reference's calls in its order: ratio_range -> random_sample(); several img_scale values with multiscale_mode 'range'
    -> randint for the long edge, then the short edge; 'value' -> randint(len(img_scale))."""

    def __init__(self, img_scale=None, multiscale_mode="range", ratio_range=None, keep_ratio=True, bbox_clip_border=True,
                 backend="cv2", override=False):
        if override or backend != "cv2":
            _refuse("Resize(override / backend)")
        if img_scale is None:
            self.img_scale = None
        else:
            scales = img_scale if isinstance(img_scale, list) else [img_scale]
            if not scales or not all(isinstance(v, (tuple, list)) and len(v) == 2 for v in scales):
                raise TypeError(f"Resize: img_scale is a tuple or a list of tuples, got {img_scale!r}")
            self.img_scale = [tuple(v) for v in scales]
        if ratio_range is not None:
            if self.img_scale is None or len(self.img_scale) != 1:
                raise ValueError("Resize(ratio_range=...) takes exactly one img_scale")
            if len(ratio_range) != 2 or not ratio_range[0] <= ratio_range[1]:
                raise ValueError(f"Resize: ratio_range is (min_ratio, max_ratio), got {ratio_range!r}")
        elif multiscale_mode not in ("value", "range"):
            raise ValueError(f"Resize: multiscale_mode is 'value' or 'range', got {multiscale_mode!r}")
        elif multiscale_mode == "range" and self.img_scale is not None and len(self.img_scale) not in (1, 2):
            raise ValueError("Resize(multiscale_mode='range') takes two img_scale values: the bounds of the range")
        self.multiscale_mode, self.ratio_range = multiscale_mode, None if ratio_range is None else tuple(ratio_range)
        self.keep_ratio, self.bbox_clip_border = keep_ratio, bbox_clip_border

    def _random_scale(self, nprnd):
        """(scale, scale_idx) as Resize._random_scale of the reference sets them"""
        if self.ratio_range is not None:
            lo, hi = self.ratio_range
            ratio = nprnd.random_sample() * (hi - lo) + lo
            return (int(self.img_scale[0][0] * ratio), int(self.img_scale[0][1] * ratio)), None
        if len(self.img_scale) == 1:
            return self.img_scale[0], 0
        if self.multiscale_mode == "range":
            long_, short = [max(v) for v in self.img_scale], [min(v) for v in self.img_scale]
            long_edge = nprnd.randint(min(long_), max(long_) + 1)
            short_edge = nprnd.randint(min(short), max(short) + 1)
            return (long_edge, short_edge), None
        idx = nprnd.randint(len(self.img_scale))
        return self.img_scale[idx], idx

    def plan(self, s, rnd, nprnd):
        if "scale" not in s:
            if self.img_scale is None:
                raise KeyError("Resize: no img_scale given and no 'scale' in the results")
            s["scale"], s["scale_idx"] = self._random_scale(nprnd)
        # (after Expand / MinIoURandomCrop the image is the source window they planned)
        h, w = s["src_window"][2:4] if "src_window" in s else s["img"].shape[:2]
        if self.keep_ratio:
            nw, nh = rescale_size((w, h), s["scale"])
        else:
            nw, nh = int(s["scale"][0]), int(s["scale"][1])
        s["resize_hw"] = (nh, nw)
        sf = np.array([nw / w, nh / h, nw / w, nh / h], dtype=np.float32)
        s["img_shape"] = s["pad_shape"] = (nh, nw, 3)
        s["scale_factor"], s["keep_ratio"] = sf, self.keep_ratio
        for key in s.get("bbox_fields", []):
            b = s[key] * sf
            if self.bbox_clip_border:
                b[:, 0::2] = np.clip(b[:, 0::2], 0, nw)
                b[:, 1::2] = np.clip(b[:, 1::2], 0, nh)
            s[key] = b


def _zoom_size(s):
    """the size of the image that Expand / MinIoURandomCrop see: the source window planned so far, or the image as loaded"""
    return tuple(s["src_window"][2:4]) if "src_window" in s else tuple(int(v) for v in s["img"].shape[:2])


def _set_src_window(s, y0, x0, h, w, fill):
    s["src_window"] = (int(y0), int(x0), int(h), int(w), tuple(fill))
    # (without a Resize the window is the output; pad_shape follows it so that a pipeline without Pad collects the window)
    s["resize_hw"] = (int(h), int(w))
    s["pad_shape"] = (int(h), int(w), 3)


def sample_view(s, src_hw=None):
    """A planned sample's view row {Hr, Wr, wy0, wx0, wh, ww, oy, ox, h, w, flip = 0, fill} (include/radet_hip.h
    RADET_VIEW_INTS): s["src_window"] is the window of the source that is resized (without one: the whole source, which is
    the image, or src_hw for a mask of that size), s["resize_hw"] the virtual resized size, s["crop_window"] the window of
    that which is computed (without one: all of it)."""
    Hs, Ws = s["img"].shape[:2] if src_hw is None else src_hw
    wy0, wx0, wh, ww, fill = s.get("src_window", (0, 0, Hs, Ws, (0, 0, 0)))
    Hr, Wr = s.get("resize_hw", (wh, ww))
    oy, ox, h, w = s.get("crop_window", (0, 0, Hr, Wr))
    return tuple(int(v) for v in (Hr, Wr, wy0, wx0, wh, ww, oy, ox, h, w, 0, fill[0] | fill[1] << 8 | fill[2] << 16))


@PIPELINES.register_module()
class Expand:
    """The reference's Expand (transforms.py:914-996), planned: zoom-out.  The image is placed at (left, top) of a canvas of
    int(h * ratio) x int(w * ratio) filled with `mean`; draws on the sample's NumPy generator in the reference's order:
    uniform(0, 1) against prob, the ratio, left, top.  Boxes shift by (left, top).  No pixel is touched and no canvas is
    made: s["src_window"] = (y0, x0, h, w, fill_bgr), the canvas as a window of the image in image coordinates (its origin
    is negative), which ImagePipeline.run samples directly.  img_shape stays what it was, as in the reference.  The draws
    are kept in s["expand"] = (ratio, left, top)."""

    def __init__(self, mean=(0, 0, 0), to_rgb=True, ratio_range=(1, 4), seg_ignore_label=None, prob=0.5):
        if seg_ignore_label is not None:
            _refuse("Expand(seg_ignore_label=...) (semantic segmentation maps)")
        if len(mean) != 3:
            raise ValueError(f"Expand: mean is one value per channel of a 3-channel image, got {mean!r}")
        if len(ratio_range) != 2 or not 1 <= ratio_range[0] <= ratio_range[1]:
            raise ValueError(f"Expand: ratio_range is (min_ratio, max_ratio) with 1 <= min_ratio <= max_ratio, got {ratio_range!r}")
        self.to_rgb, self.ratio_range, self.prob = to_rgb, tuple(ratio_range), prob
        # the image is BGR where Expand stands, so a mean given in RGB order is reversed
        self.mean = tuple(mean)[::-1] if to_rgb else tuple(mean)
        self.min_ratio, self.max_ratio = self.ratio_range
        if not all(0 <= v < 256 for v in self.mean):
            raise ValueError(f"Expand: mean {mean!r} does not fit the uint8 image")
        # what NumPy's cast of the mean to the uint8 canvas stores: truncated, not rounded
        self.fill = tuple(int(v) for v in np.asarray(self.mean, np.float64).astype(np.uint8))

    def plan(self, s, rnd, nprnd):
        if nprnd.uniform(0, 1) > self.prob:
            return
        if s.get("seg_fields"):
            _refuse("Expand on a sample with seg_fields")
        if "src_window" in s:
            _refuse("Expand after another source-window stage")
        h, w = _zoom_size(s)
        ratio = nprnd.uniform(self.min_ratio, self.max_ratio)
        left = int(nprnd.uniform(0, w * ratio - w))
        top = int(nprnd.uniform(0, h * ratio - h))
        for key in s.get("bbox_fields", []):
            s[key] = s[key] + np.tile((left, top), 2).astype(s[key].dtype)
        _set_src_window(s, -top, -left, int(h * ratio), int(w * ratio), self.fill)
        s["expand"] = (ratio, left, top)


def patch_overlaps(patch, boxes, eps=1e-6):
    """bbox_overlaps (radet/core/evaluation/bbox_overlaps.py, mode 'iou') of one patch against k boxes, float32 [k]: the
    areas, the intersection and the union in float32, the union raised to eps before the division.  (cocoeval.box_iou_matrix
    computes in float64 and has no eps: not bit-equal, so it is not used here.)"""
    p, b = np.asarray(patch).astype(np.float32), boxes.astype(np.float32).reshape(-1, 4)
    if not len(b):
        return np.zeros(0, np.float32)
    area_p = (p[2] - p[0]) * (p[3] - p[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.maximum(np.minimum(p[2], b[:, 2]) - np.maximum(p[0], b[:, 0]), 0)
    ih = np.maximum(np.minimum(p[3], b[:, 3]) - np.maximum(p[1], b[:, 1]), 0)
    overlap = iw * ih
    union = np.maximum(area_p + area_b - overlap, eps)
    return (overlap / union).astype(np.float32)


def _centres_in_patch(boxes, patch):
    centre = (boxes[:, :2] + boxes[:, 2:]) / 2
    return (centre[:, 0] > patch[0]) & (centre[:, 1] > patch[1]) & (centre[:, 0] < patch[2]) & (centre[:, 1] < patch[3])


@PIPELINES.register_module()
class MinIoURandomCrop:
    """The reference's MinIoURandomCrop (transforms.py:1006-1136), planned: zoom-in.  Draws on the sample's NumPy generator
    in the reference's order: choice over (1, *min_ious, 0) -- mode 1 leaves the sample as it is -- then up to 50 trials of
    new_w, new_h, (aspect test), left, top, where left and top are uniform(w - new_w) and uniform(h - new_h) with NumPy's
    high = 1.0, as the reference calls them; after 50 failed trials a new mode.  A patch passes when its IoU with every
    box of every bbox field reaches the mode and the centre of at least one box lies inside it; per field the boxes whose
    centre lies inside are kept, clipped to the patch and shifted, labels and masks with them.  No pixel is touched: the
    patch goes into s["src_window"] (composed with Expand's, when that came first).  The draws are kept in s["crop_mode"]
    and s["crop_patch"] = (x0, y0, x1, y1) in the coordinates of the image the stage saw."""
    bbox2label = {"gt_bboxes": "gt_labels", "gt_bboxes_ignore": "gt_labels_ignore"}
    bbox2mask = {"gt_bboxes": "gt_masks", "gt_bboxes_ignore": "gt_masks_ignore"}

    def __init__(self, min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3, bbox_clip_border=True):
        self.min_ious, self.sample_mode = tuple(min_ious), (1, *min_ious, 0)
        self.min_crop_size, self.bbox_clip_border = min_crop_size, bbox_clip_border

    def plan(self, s, rnd, nprnd):
        if s.get("seg_fields"):
            _refuse("MinIoURandomCrop on a sample with seg_fields")
        if "bbox_fields" not in s:
            raise KeyError("MinIoURandomCrop needs bbox_fields (LoadAnnotations before it)")
        all_boxes = np.concatenate([s[key] for key in s["bbox_fields"]], 0) if s["bbox_fields"] else np.zeros((0, 4), np.float32)
        h, w = _zoom_size(s)
        while True:
            mode = nprnd.choice(self.sample_mode)
            s["crop_mode"] = float(mode)
            if mode == 1:
                return
            for _ in range(50):
                new_w = nprnd.uniform(self.min_crop_size * w, w)
                new_h = nprnd.uniform(self.min_crop_size * h, h)
                if new_h / new_w < 0.5 or new_h / new_w > 2:
                    continue
                left = nprnd.uniform(w - new_w)                 # (one argument: low; high is NumPy's 1.0)
                top = nprnd.uniform(h - new_h)
                patch = np.array((int(left), int(top), int(left + new_w), int(top + new_h)))
                if patch[2] == patch[0] or patch[3] == patch[1]:
                    continue
                overlaps = patch_overlaps(patch, all_boxes)
                if len(overlaps) > 0 and overlaps.min() < mode:
                    continue
                if len(overlaps) > 0:
                    if not _centres_in_patch(all_boxes, patch).any():
                        continue
                    for key in s["bbox_fields"]:
                        b = s[key].copy()
                        keep = _centres_in_patch(b, patch)
                        b = b[keep]
                        if self.bbox_clip_border:
                            b[:, 2:] = b[:, 2:].clip(max=patch[2:])
                            b[:, :2] = b[:, :2].clip(min=patch[:2])
                        b -= np.tile(patch[:2], 2)
                        s[key] = b
                        label_key, mask_key = self.bbox2label.get(key), self.bbox2mask.get(key)
                        if label_key in s:
                            s[label_key] = s[label_key][keep]
                        if mask_key in s:
                            s[mask_key] = s[mask_key][keep.nonzero()[0]]
                        if mask_key is not None and mask_key + "_rle" in s:
                            parts, src_hw = s[mask_key + "_rle"]
                            s[mask_key + "_rle"] = ([parts[k] for k in keep.nonzero()[0]], src_hw)
                # (left <= max(w - new_w, 1), so int(left + new_w) <= w: the patch lies inside the image it is cut from)
                px0, py0, px1, py1 = (int(v) for v in patch)
                ph, pw = py1 - py0, px1 - px0
                y0, x0, fill = (*s["src_window"][:2], s["src_window"][4]) if "src_window" in s else (0, 0, (0, 0, 0))
                _set_src_window(s, y0 + py0, x0 + px0, ph, pw, fill)
                s["crop_patch"] = (px0, py0, px1, py1)
                s["img_shape"] = (ph, pw, 3)
                return


@PIPELINES.register_module()
class RandomCrop:
    """The reference's RandomCrop (transforms.py:587-770), planned: the crop-size draws of _get_crop_size, then offset_h,
    then offset_w, on the sample's NumPy generator; boxes shifted, clipped and filtered, the labels and masks of dropped
    boxes dropped with them.  No pixel is touched: s["crop_window"] = (y0, x0, h, w) inside the virtual resized image
    s["resize_hw"]; ImagePipeline.run computes that window only.  plan() returns False for a crop without a gt box
    (allow_negative_crop=False): the reference's None, ImagePipeline.plan returns None then."""
    bbox2label = {"gt_bboxes": "gt_labels", "gt_bboxes_ignore": "gt_labels_ignore"}
    bbox2mask = {"gt_bboxes": "gt_masks", "gt_bboxes_ignore": "gt_masks_ignore"}

    def __init__(self, crop_size, crop_type="absolute", allow_negative_crop=False, bbox_clip_border=True):
        if crop_type not in ("relative_range", "relative", "absolute", "absolute_range"):
            raise ValueError(f"Invalid crop_type {crop_type}.")
        if crop_type in ("absolute", "absolute_range"):
            if not (isinstance(crop_size[0], int) and isinstance(crop_size[1], int) and crop_size[0] > 0 and crop_size[1] > 0):
                raise ValueError(f"RandomCrop(crop_type={crop_type!r}): crop_size is two positive ints, got {crop_size!r}")
            if crop_type == "absolute_range" and crop_size[0] > crop_size[1]:
                raise ValueError(f"RandomCrop(crop_type='absolute_range'): crop_size is (min, max), got {crop_size!r}")
        elif not (0 < crop_size[0] <= 1 and 0 < crop_size[1] <= 1):
            raise ValueError(f"RandomCrop(crop_type={crop_type!r}): crop_size is two ratios in (0, 1], got {crop_size!r}")
        self.crop_size, self.crop_type = tuple(crop_size), crop_type
        self.allow_negative_crop, self.bbox_clip_border = allow_negative_crop, bbox_clip_border

    def _get_crop_size(self, h, w, nprnd):
        if self.crop_type == "absolute":
            return min(self.crop_size[0], h), min(self.crop_size[1], w)
        if self.crop_type == "absolute_range":
            crop_h = nprnd.randint(min(h, self.crop_size[0]), min(h, self.crop_size[1]) + 1)
            crop_w = nprnd.randint(min(w, self.crop_size[0]), min(w, self.crop_size[1]) + 1)
            return crop_h, crop_w
        if self.crop_type == "relative":
            crop_h, crop_w = self.crop_size
        else:
            size = np.asarray(self.crop_size, dtype=np.float32)
            crop_h, crop_w = size + nprnd.rand(2) * (1 - size)
        return int(h * crop_h + 0.5), int(w * crop_w + 0.5)

    def plan(self, s, rnd, nprnd):
        h, w = (int(v) for v in s["img_shape"][:2])
        ch, cw = self._get_crop_size(h, w, nprnd)
        if ch <= 0 or cw <= 0:
            raise ValueError(f"RandomCrop: a crop of {ch} x {cw} from an image of {h} x {w}")
        y0 = int(nprnd.randint(0, max(h - ch, 0) + 1))
        x0 = int(nprnd.randint(0, max(w - cw, 0) + 1))
        ch, cw = min(ch, h - y0), min(cw, w - x0)
        offset = np.array([x0, y0, x0, y0], dtype=np.float32)
        for key in s.get("bbox_fields", []):
            b = s[key] - offset
            if self.bbox_clip_border:
                b[:, 0::2] = np.clip(b[:, 0::2], 0, cw)
                b[:, 1::2] = np.clip(b[:, 1::2], 0, ch)
            valid = (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])
            if key == "gt_bboxes" and not valid.any() and not self.allow_negative_crop:
                return False
            s[key] = b[valid, :]
            label_key, mask_key = self.bbox2label.get(key), self.bbox2mask.get(key)
            if label_key in s:
                s[label_key] = s[label_key][valid]
            if mask_key in s:
                s[mask_key] = s[mask_key][valid.nonzero()[0]]
            if mask_key is not None and mask_key + "_rle" in s:
                parts, src_hw = s[mask_key + "_rle"]
                s[mask_key + "_rle"] = ([parts[k] for k in valid.nonzero()[0]], src_hw)
        s.setdefault("resize_hw", (h, w))
        s["crop_window"] = (y0, x0, ch, cw)
        # (pad_shape follows the crop, so that a pipeline without Pad collects the cropped image)
        s["img_shape"] = s["pad_shape"] = (ch, cw, 3)


# ---------------------------------------------------------------------------------------------------- affine
_MAX_LEVEL = 10
_AFFINE_MAX_ENTRIES = 4
CUTOUT_MAX_HOLES = 64


CutHoles = collections.namedtuple("CutHoles", "rects fill")   # one fired CutOut: int32 [n, 4] rows {x1, y1, x2, y2}, fill bytes (BGR)


def _block_entries(s):
    """the number of entries (fired warp and CutOut stages) of the sample's block so far"""
    return len(s["block_ops"]) if "block_ops" in s else len(s.get("affine", ()))


# one fired colour stage: a key of K.COLOR_KINDS and the factor (float64; 1.0 for "equalize", which has none)
ColorOp = collections.namedtuple("ColorOp", "kind factor")
_BLOCK_KEYS = dict(warp="affine", cutout="cutout", color="color")


def _block_list(s):
    """the entries of the sample's block in the order they ran: (matrix, fill) of s["affine"], CutHoles of s["cutout"] and
    ColorOp of s["color"]"""
    if "block_ops" not in s:
        return list(s.get("affine", ()))
    return [s[_BLOCK_KEYS[kind]][j] for kind, j in s["block_ops"]]


def rotation_matrix(center, angle, scale):
    """cv2.getRotationMatrix2D(center, angle, scale): float64 [2, 3]"""
    a = math.radians(angle)
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = float(center[0]), float(center[1])
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], np.float64)


def shear_matrix(magnitude, direction):
    """mmcv.imshear's matrix: float32 entries, widened to float64 as cv2.warpAffine does"""
    m = np.float32([[1, magnitude, 0], [0, 1, 0]]) if direction == "horizontal" else np.float32([[1, 0, 0], [magnitude, 1, 0]])
    return m.astype(np.float64)


def translate_matrix(offset, direction):
    """mmcv.imtranslate's matrix: float32 entries, widened to float64"""
    m = np.float32([[1, 0, offset], [0, 1, 0]]) if direction == "horizontal" else np.float32([[1, 0, 0], [0, 1, offset]])
    return m.astype(np.float64)


def _fill_arg(name, img_fill_val):
    """img_fill_val as the reference takes it -> the three bytes cv2 stores for that borderValue (rounded half to even)"""
    if isinstance(img_fill_val, (float, int)):
        vals = (float(img_fill_val),) * 3
    elif isinstance(img_fill_val, tuple) and len(img_fill_val) == 3:
        vals = tuple(float(v) for v in img_fill_val)
    else:
        raise ValueError(f"{name}: img_fill_val is a number or a tuple of 3, got {img_fill_val!r}")
    if not all(0 <= v <= 255 for v in vals):
        raise ValueError(f"{name}: img_fill_val {img_fill_val!r} outside [0, 255]")
    return vals, tuple(int(np.rint(v)) for v in vals)


class _AffineStage:
    """What Rotate, Shear and Translate share: the gate and sign draws on the sample's NumPy generator (rand() > prob,
    then rand() < random_negative_prob, the reference's calls in its order), the filter of boxes that the move left
    without extent, and the record: a stage that fires appends (forward 2 x 3 matrix float64, fill bytes in the image's
    channel order) to s["affine"] and (stage name, signed angle / magnitude / offset) to s["affine_draws"];
    ImagePipeline.run warps the resized frame and its masks once per entry."""
    bbox2label = {"gt_bboxes": "gt_labels", "gt_bboxes_ignore": "gt_labels_ignore"}
    bbox2mask = {"gt_bboxes": "gt_masks", "gt_bboxes_ignore": "gt_masks_ignore"}

    def _common(self, level, img_fill_val, seg_ignore_label, prob, random_negative_prob):
        name = type(self).__name__
        if not isinstance(level, (int, float)) or not 0 <= level <= _MAX_LEVEL:
            raise ValueError(f"{name}: level is a number in [0, {_MAX_LEVEL}], got {level!r}")
        if not 0 <= prob <= 1.0:
            raise ValueError(f"{name}: prob is in [0, 1], got {prob!r}")
        self.level, self.prob, self.random_negative_prob = level, prob, random_negative_prob
        self.img_fill_val, self.fill = _fill_arg(name, img_fill_val)
        self.seg_ignore_label = seg_ignore_label

    def _negative(self, value, nprnd):
        return -value if nprnd.rand() < self.random_negative_prob else value

    def _size(self, s):
        if s.get("seg_fields"):
            _refuse(f"{type(self).__name__} on a sample with seg_fields (semantic segmentation maps)")
        return int(s["img_shape"][0]), int(s["img_shape"][1])

    def _record(self, s, matrix, h, w):
        entries = s.setdefault("affine", [])
        if _block_entries(s) >= _AFFINE_MAX_ENTRIES:
            _refuse(f"more than {_AFFINE_MAX_ENTRIES} affine stages firing on one sample")
        if "block_ops" in s:                             # (a CutOut fired before this stage: the order across kinds counts)
            s["block_ops"].append(("warp", len(entries)))
        if not K.warp_fits(K.invert_affine(matrix), h, w):
            _refuse(f"{type(self).__name__}: matrix {matrix.tolist()} on an image of {h} x {w} (its inverse leaves the warp "
                    f"kernel's 32-bit fixed point)")
        entries.append((np.asarray(matrix, np.float64), self.fill))

    def _filter_invalid(self, s, min_size=0):
        for key in s.get("bbox_fields", []):
            b = s[key]
            keep = np.nonzero((b[:, 2] - b[:, 0] > min_size) & (b[:, 3] - b[:, 1] > min_size))[0]
            s[key] = b[keep]
            label_key, mask_key = self.bbox2label.get(key), self.bbox2mask.get(key)
            if label_key in s:
                s[label_key] = s[label_key][keep]
            if mask_key in s:
                s[mask_key] = s[mask_key][keep]
            if mask_key is not None and mask_key + "_rle" in s:
                parts, src_hw = s[mask_key + "_rle"]
                s[mask_key + "_rle"] = ([parts[k] for k in keep], src_hw)

    def worst_matrices(self, h, w):
        """the matrices of both signs on an h x w image (the build-time check of the fixed-point range)"""
        raise NotImplementedError


def _box_corners(b):
    """[4, 2, n, 1]: the corners (min, min), (max, min), (min, max), (max, max) of n boxes, in the boxes' dtype"""
    x0, y0, x1, y1 = np.split(b, b.shape[-1], axis=-1)
    return np.stack([[x0, y0], [x1, y0], [x0, y1], [x1, y1]])


def _corner_extent(xs, ys, h, w, dtype):
    """the box around moved corners (xs, ys: [n, 4]), clipped to the image as the reference clips it"""
    x0, y0 = np.clip(np.min(xs, axis=-1), a_min=0, a_max=w), np.clip(np.min(ys, axis=-1), a_min=0, a_max=h)
    x1, y1 = np.clip(np.max(xs, axis=-1), a_min=x0, a_max=w), np.clip(np.max(ys, axis=-1), a_min=y0, a_max=h)
    return np.stack([x0, y0, x1, y1], axis=-1).astype(dtype)


@PIPELINES.register_module()
class Rotate(_AffineStage):
    """The reference's Rotate (auto_augment.py:329-540), planned: angle = level / 10 * max_rotate_angle, negated by the sign
    draw; matrix cv2.getRotationMatrix2D(center, -angle, scale) about ((w - 1) / 2, (h - 1) / 2) of the image as it is at
    that point unless `center` is given; boxes: the float64 matrix times the homogeneous corners, the extent, clipped."""

    def __init__(self, level, scale=1, center=None, img_fill_val=128, seg_ignore_label=255, prob=0.5, max_rotate_angle=30,
                 random_negative_prob=0.5):
        self._common(level, img_fill_val, seg_ignore_label, prob, random_negative_prob)
        if not isinstance(scale, (int, float)):
            raise ValueError(f"Rotate: scale is a number, got {scale!r}")
        if scale == 0:
            _refuse("Rotate(scale=0) (a singular matrix: nothing of the image is left)")
        if isinstance(center, (int, float)):
            center = (center, center)
        elif center is not None and not (isinstance(center, tuple) and len(center) == 2):
            raise ValueError(f"Rotate: center is None, a number or a tuple of 2, got {center!r}")
        if not isinstance(max_rotate_angle, (int, float)):
            raise ValueError(f"Rotate: max_rotate_angle is a number, got {max_rotate_angle!r}")
        self.scale, self.center, self.max_rotate_angle = scale, center, max_rotate_angle
        self.angle = (level / _MAX_LEVEL) * max_rotate_angle

    def _matrix(self, angle, h, w):
        center = self.center if self.center is not None else ((w - 1) * 0.5, (h - 1) * 0.5)
        return rotation_matrix(center, -angle, self.scale)

    def worst_matrices(self, h, w):
        return [self._matrix(self.angle, h, w), self._matrix(-self.angle, h, w)]

    def plan(self, s, rnd, nprnd):
        if nprnd.rand() > self.prob:
            return
        h, w = self._size(s)
        angle = self._negative(self.angle, nprnd)
        matrix = self._matrix(angle, h, w)
        self._record(s, matrix, h, w)
        for key in s.get("bbox_fields", []):
            c = _box_corners(s[key])
            c = np.concatenate((c, np.ones((4, 1, c.shape[2], 1), c.dtype)), axis=1).transpose((2, 0, 1, 3))
            moved = np.matmul(matrix, c)[..., 0]                              # [n, 4, 2], float64
            s[key] = _corner_extent(moved[:, :, 0], moved[:, :, 1], h, w, s[key].dtype)
        self._filter_invalid(s)
        s.setdefault("affine_draws", []).append(("Rotate", float(angle)))


@PIPELINES.register_module()
class Shear(_AffineStage):
    """The reference's Shear (auto_augment.py:112-325), planned: magnitude = level / 10 * max_shear_magnitude, negated by
    the sign draw; boxes: a float32 2 x 2 matrix times the corners, the extent, clipped"""

    def __init__(self, level, img_fill_val=128, seg_ignore_label=255, prob=0.5, direction="horizontal", max_shear_magnitude=0.3,
                 random_negative_prob=0.5, interpolation="bilinear"):
        self._common(level, img_fill_val, seg_ignore_label, prob, random_negative_prob)
        if direction not in ("horizontal", "vertical"):
            raise ValueError(f"Shear: direction is 'horizontal' or 'vertical', got {direction!r}")
        if not isinstance(max_shear_magnitude, float) or not 0. <= max_shear_magnitude <= 1.:
            raise ValueError(f"Shear: max_shear_magnitude is a float in [0, 1], got {max_shear_magnitude!r}")
        if interpolation != "bilinear":
            _refuse(f"Shear(interpolation={interpolation!r}) (the warp kernel is cv2's bilinear one)")
        self.direction, self.max_shear_magnitude, self.interpolation = direction, max_shear_magnitude, interpolation
        self.magnitude = (level / _MAX_LEVEL) * max_shear_magnitude

    def worst_matrices(self, h, w):
        return [shear_matrix(self.magnitude, self.direction), shear_matrix(-self.magnitude, self.direction)]

    def plan(self, s, rnd, nprnd):
        if nprnd.rand() > self.prob:
            return
        h, w = self._size(s)
        magnitude = self._negative(self.magnitude, nprnd)
        self._record(s, shear_matrix(magnitude, self.direction), h, w)
        m22 = np.stack([[1, magnitude], [0, 1]] if self.direction == "horizontal" else [[1, 0], [magnitude, 1]]).astype(np.float32)
        for key in s.get("bbox_fields", []):
            c = _box_corners(s[key])[..., 0].transpose((2, 1, 0)).astype(np.float32)      # [n, 2, 4]
            moved = np.matmul(m22[None, :, :], c)
            s[key] = _corner_extent(moved[:, 0, :], moved[:, 1, :], h, w, s[key].dtype)
        self._filter_invalid(s)
        s.setdefault("affine_draws", []).append(("Shear", float(magnitude)))


@PIPELINES.register_module()
class Translate(_AffineStage):
    """The reference's Translate (auto_augment.py:543-705), planned: offset = int(level / 10 * max_translate_offset) pixels,
    negated by the sign draw; boxes shifted and cut at the image's border, those left with an extent of at most min_size
    dropped"""

    def __init__(self, level, prob=0.5, img_fill_val=128, seg_ignore_label=255, direction="horizontal", max_translate_offset=250.,
                 random_negative_prob=0.5, min_size=0):
        self._common(level, img_fill_val, seg_ignore_label, prob, random_negative_prob)
        if direction not in ("horizontal", "vertical"):
            raise ValueError(f"Translate: direction is 'horizontal' or 'vertical', got {direction!r}")
        if not isinstance(max_translate_offset, (int, float)):
            raise ValueError(f"Translate: max_translate_offset is a number, got {max_translate_offset!r}")
        self.direction, self.max_translate_offset, self.min_size = direction, max_translate_offset, min_size
        self.offset = int((level / _MAX_LEVEL) * max_translate_offset)

    def worst_matrices(self, h, w):
        return [translate_matrix(self.offset, self.direction), translate_matrix(-self.offset, self.direction)]

    def plan(self, s, rnd, nprnd):
        if nprnd.rand() > self.prob:
            return
        h, w = self._size(s)
        offset = self._negative(self.offset, nprnd)
        self._record(s, translate_matrix(offset, self.direction), h, w)
        for key in s.get("bbox_fields", []):
            x0, y0, x1, y1 = np.split(s[key], s[key].shape[-1], axis=-1)
            if self.direction == "horizontal":
                x0, x1 = np.maximum(0, x0 + offset), np.minimum(w, x1 + offset)
            else:
                y0, y1 = np.maximum(0, y0 + offset), np.minimum(h, y1 + offset)
            s[key] = np.concatenate([x0, y0, x1, y1], axis=-1)
        self._filter_invalid(s, self.min_size)
        s.setdefault("affine_draws", []).append(("Translate", int(offset)))


_AFFINE_STAGES = ("Rotate", "Shear", "Translate")
_COLOR_STAGES = ("ColorTransform", "EqualizeTransform", "BrightnessTransform", "ContrastTransform")
_POLICY_STAGES = _AFFINE_STAGES + ("CutOut",)       # (+ _COLOR_STAGES in an AutoAugment(color_stages=True))


def _fill_in_arg(fill_in):
    """fill_in of CutOut -> three bytes: the reference assigns it into the u8 image, which would wrap or truncate silently
    anything that is not an integer in [0, 255]"""
    ok = isinstance(fill_in, (tuple, list)) and len(fill_in) == 3 and all(
        isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and 0 <= v <= 255 and v == int(v) for v in fill_in)
    if not ok:
        raise ValueError(f"CutOut: fill_in is three integers in [0, 255] in the image's channel order (BGR), got {fill_in!r}")
    return tuple(int(v) for v in fill_in)


@PIPELINES.register_module()
class CutOut:
    """The reference's CutOut (transforms.py:1734-1804), planned: the draws on the sample's NumPy generator in the reference's
    order -- randint(n_holes[0], n_holes[1] + 1) holes, per hole randint(0, w), randint(0, h), randint(0, len(candidates)) --
    on the h x w of s["img_shape"]; a hole is the candidate as given (cutout_shape: (w, h) in pixels) or int(ratio * w),
    int(ratio * h) (cutout_ratio), from (x1, y1) to clip(x1 + cw, 0, w), clip(y1 + ch, 0, h).  Boxes, labels and masks are
    untouched, as in the reference.  No pixel is touched here.  In the block after Resize (next to Rotate / Shear /
    Translate, bare or in an AutoAugment policy) a stage that drew holes is one entry of the block: it appends CutHoles(int32
    [n, 4] rows {x1, y1, x2, y2}, fill bytes in BGR) to s["cutout"] and ("cutout", its index there) to s["block_ops"], the
    list of the block's entries in the order they ran (("warp", index into s["affine"]) for the warp stages; s["affine"]
    itself keeps holding the warp entries only).  Behind the photometric stages (`late`, set by ImagePipeline) the holes go
    to s["cutout_late"] = (rows, fill) and are cut into the finished batch.  A stage that drew no hole records nothing."""
    late = False

    def __init__(self, n_holes, cutout_shape=None, cutout_ratio=None, fill_in=(0, 0, 0)):
        if (cutout_shape is None) == (cutout_ratio is None):
            raise ValueError("CutOut: either cutout_shape or cutout_ratio is given, not both")
        if isinstance(n_holes, (tuple, list)):
            if not (len(n_holes) == 2 and all(isinstance(v, (int, np.integer)) for v in n_holes) and 0 <= n_holes[0] < n_holes[1]):
                raise ValueError(f"CutOut: n_holes is an int or (min, max) with 0 <= min < max, got {n_holes!r}")
            n_holes = (int(n_holes[0]), int(n_holes[1]))
        elif isinstance(n_holes, (int, np.integer)) and not isinstance(n_holes, bool) and n_holes >= 0:
            n_holes = (int(n_holes), int(n_holes))
        else:
            raise ValueError(f"CutOut: n_holes is an int or (min, max) with 0 <= min < max, got {n_holes!r}")
        if n_holes[1] > CUTOUT_MAX_HOLES:
            _refuse(f"CutOut(n_holes={n_holes}) (more than CUTOUT_MAX_HOLES = {CUTOUT_MAX_HOLES} holes per stage)")
        self.with_ratio = cutout_ratio is not None
        given = cutout_ratio if self.with_ratio else cutout_shape
        if not isinstance(given, (list, tuple)):
            raise ValueError(f"CutOut: cutout_shape / cutout_ratio is a tuple of 2 or a list of such tuples, got {given!r}")
        candidates = given if isinstance(given, list) else [given]
        kinds = (int, float, np.integer, np.floating) if self.with_ratio else (int, np.integer)
        if not candidates or not all(isinstance(c, (tuple, list)) and len(c) == 2 and all(
                isinstance(v, kinds) and not isinstance(v, bool) for v in c) for c in candidates):
            raise ValueError(f"CutOut: each candidate is (w, h), {'two numbers' if self.with_ratio else 'two ints'}, got {given!r}")
        self.n_holes, self.candidates, self.fill_in = n_holes, [tuple(c) for c in candidates], fill_in
        self.fill = _fill_in_arg(fill_in)

    def draw(self, h, w, nprnd):
        """the reference's draws on an h x w image -> int32 [n, 4] rows {x1, y1, x2, y2}"""
        n = nprnd.randint(self.n_holes[0], self.n_holes[1] + 1)
        rects = np.zeros((n, 4), np.int32)
        for r in rects:
            x1 = nprnd.randint(0, w)
            y1 = nprnd.randint(0, h)
            cw, ch = self.candidates[nprnd.randint(0, len(self.candidates))]
            if self.with_ratio:
                cw, ch = int(cw * w), int(ch * h)
            r[:] = [x1, y1, np.clip(x1 + cw, 0, w), np.clip(y1 + ch, 0, h)]
        return rects

    def plan(self, s, rnd, nprnd):
        if s.get("seg_fields"):
            _refuse("CutOut on a sample with seg_fields (semantic segmentation maps)")
        rects = self.draw(int(s["img_shape"][0]), int(s["img_shape"][1]), nprnd)
        if not len(rects):
            return
        if self.late:
            s["cutout_late"] = CutHoles(rects, self.fill)
            return
        if _block_entries(s) >= _AFFINE_MAX_ENTRIES:
            _refuse(f"more than {_AFFINE_MAX_ENTRIES} affine stages firing on one sample")
        ops = s.setdefault("block_ops", [("warp", k) for k in range(len(s.get("affine", ())))])
        holes = s.setdefault("cutout", [])
        ops.append(("cutout", len(holes)))
        holes.append(CutHoles(rects, self.fill))


def enhance_level_to_value(level, a=1.8, b=0.1):
    """auto_augment.py:18-20: the factor of a colour stage, in Python floats"""
    return (level / _MAX_LEVEL) * a + b


class _ColorStage:
    """What ColorTransform, EqualizeTransform, BrightnessTransform and ContrastTransform (auto_augment.py:709-890) share,
    planned: one nprnd.rand() per call, the stage is skipped when it is > prob, no other draw; factor =
    enhance_level_to_value(level).  A stage that fires is one entry of the block after Resize: it appends ColorOp(kind,
    factor as float64) to s["color"] and ("color", its index there) to s["block_ops"] (created as CutOut.plan creates it).
    No pixel is touched here and boxes, labels and masks never are; ImagePipeline.run maps the packed u8 frame at the
    entry's rank (radet_color_stats_u8 / radet_color_apply_u8), so a stage behind a warp sees the warp's fill pixels."""
    kind = None

    def _common(self, level, prob):
        name = type(self).__name__
        if self.kind != "equalize" and (isinstance(level, bool) or not isinstance(level, (int, float)) or not 0 <= level <= _MAX_LEVEL):
            raise ValueError(f"{name}: level is a number in [0, {_MAX_LEVEL}], got {level!r}")
        if isinstance(prob, bool) or not isinstance(prob, (int, float)) or not 0 <= prob <= 1.0:
            raise ValueError(f"{name}: prob is in [0, 1], got {prob!r}")
        self.level, self.prob = level, prob
        self.factor = 1.0 if self.kind == "equalize" else enhance_level_to_value(level)

    def plan(self, s, rnd, nprnd):
        if s.get("seg_fields"):
            _refuse(f"{type(self).__name__} on a sample with seg_fields (semantic segmentation maps; drop the stage or the "
                    f"seg fields)")
        if nprnd.rand() > self.prob:
            return
        if _block_entries(s) >= _AFFINE_MAX_ENTRIES:
            _refuse(f"more than {_AFFINE_MAX_ENTRIES} affine stages firing on one sample")
        ops = s.setdefault("block_ops", [("warp", k) for k in range(len(s.get("affine", ())))])
        fired = s.setdefault("color", [])
        ops.append(("color", len(fired)))
        fired.append(ColorOp(self.kind, float(self.factor)))


@PIPELINES.register_module()
class ColorTransform(_ColorStage):
    """mmcv.adjust_color(img, factor): every pixel blended with its gray value"""
    kind = "color"

    def __init__(self, level, prob=0.5):
        self._common(level, prob)


@PIPELINES.register_module()
class EqualizeTransform(_ColorStage):
    """mmcv.imequalize(img): every channel mapped through its own histogram"""
    kind = "equalize"

    def __init__(self, prob=0.5):
        self._common(None, prob)


@PIPELINES.register_module()
class BrightnessTransform(_ColorStage):
    """mmcv.adjust_brightness(img, factor): the image blended with black"""
    kind = "brightness"

    def __init__(self, level, prob=0.5):
        self._common(level, prob)


@PIPELINES.register_module()
class ContrastTransform(_ColorStage):
    """mmcv.adjust_contrast(img, factor): the image blended with the mean of its gray image"""
    kind = "contrast"

    def __init__(self, level, prob=0.5):
        self._common(level, prob)


@PIPELINES.register_module()
class AutoAugment:
    """The reference's AutoAugment (auto_augment.py:45-108) over the affine stages and CutOut: np.random.choice over the
    policies on the sample's NumPy generator, then the stages of the chosen policy in order.  s["policy"] = the index drawn.
    color_stages=True (this project's argument, the reference has none) lets policies hold ColorTransform, EqualizeTransform,
    BrightnessTransform and ContrastTransform too; without it a policy that names one is refused, as it was before these
    stages were built (the existing tests hold that refusal), and the message names the argument."""

    def __init__(self, policies, color_stages=False):
        if not isinstance(color_stages, bool):
            raise ValueError(f"AutoAugment: color_stages is a bool, got {color_stages!r}")
        allowed = _POLICY_STAGES + (_COLOR_STAGES if color_stages else ())
        if not isinstance(policies, list) or not policies or not all(isinstance(p, list) and p for p in policies):
            raise ValueError("AutoAugment: policies is a non-empty list of non-empty lists")
        for policy in policies:
            for t in policy:
                if not isinstance(t, dict) or "type" not in t:
                    raise ValueError("AutoAugment: each augmentation is a dict with the key 'type'")
                if t["type"] not in allowed:
                    hint = "; pass color_stages=True to AutoAugment for the colour stages" if t["type"] in _COLOR_STAGES else ""
                    _refuse(f"AutoAugment policy stage {t['type']} (policies hold {allowed} only{hint})")
            if len(policy) > _AFFINE_MAX_ENTRIES:
                _refuse(f"an AutoAugment policy of {len(policy)} stages (at most {_AFFINE_MAX_ENTRIES} affine entries per sample)")
        self.policies, self.color_stages = [[dict(t) for t in policy] for policy in policies], color_stages
        self.transforms = [[build_from_cfg(t, PIPELINES) for t in policy] for policy in self.policies]

    def plan(self, s, rnd, nprnd):
        k = int(nprnd.choice(len(self.transforms)))
        s["policy"] = k
        for t in self.transforms[k]:
            t.plan(s, rnd, nprnd)


@PIPELINES.register_module()
class RandomFlip:
    def __init__(self, flip_ratio=None, direction="horizontal"):
        if direction != "horizontal" or isinstance(flip_ratio, list):
            _refuse(f"RandomFlip(direction={direction!r}, list flip_ratio)")
        if flip_ratio is not None:
            assert 0 <= flip_ratio <= 1
        self.flip_ratio, self.direction = flip_ratio, direction

    def plan(self, s, rnd, nprnd):
        if "flip" not in s:
            if self.flip_ratio is None:
                raise TypeError("RandomFlip(flip_ratio=None) needs 'flip' in the results (MultiScaleFlipAug sets it)")
            cur = nprnd.choice([self.direction, None], p=[self.flip_ratio, 1 - self.flip_ratio])
            s["flip"] = cur is not None
        if "flip_direction" not in s:
            s["flip_direction"] = cur
        if s["flip"]:
            w = s["img_shape"][1]
            for key in s.get("bbox_fields", []):
                b = s[key].copy()
                b[..., 0::4] = w - s[key][..., 2::4]
                b[..., 2::4] = w - s[key][..., 0::4]
                s[key] = b


@PIPELINES.register_module()
class Normalize:
    def __init__(self, mean, std, to_rgb=True):
        self.mean, self.std, self.to_rgb = np.array(mean, np.float32), np.array(std, np.float32), to_rgb

    def plan(self, s, rnd, nprnd):
        s["img_norm_cfg"] = dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb)


@PIPELINES.register_module()
class Pad:
    def __init__(self, size=None, size_divisor=None, pad_val=0):
        if pad_val != 0:
            _refuse("Pad(pad_val != 0)")
        if (size is None) == (size_divisor is None):
            raise ValueError("Pad takes one of size and size_divisor")
        self.size = None if size is None else (int(size[0]), int(size[1]))
        self.size_divisor = None if size_divisor is None else int(size_divisor)

    def plan(self, s, rnd, nprnd):
        h, w = s["img_shape"][:2]
        if self.size is not None:
            if h > self.size[0] or w > self.size[1]:
                raise ValueError(f"Pad(size={self.size}): the image is {h} x {w}")
            s["pad_shape"] = (*self.size, 3)
            s["pad_fixed_size"], s["pad_size_divisor"] = self.size, None
            return
        d = self.size_divisor
        s["pad_shape"] = (int(math.ceil(h / d)) * d, int(math.ceil(w / d)) * d, 3)
        s["pad_fixed_size"], s["pad_size_divisor"] = None, d


# ---------------------------------------------------------------------------------------------------- photometric
@PIPELINES.register_module()
class RandomBackground:
    def __init__(self, background_dir, prob=0.8, file_client_args=None, flag="color", decode="host", index_cache=None,
                 seg_mcus=jpeg.DEFAULT_SEG_MCUS):
        self.decode, self.index_cache, self.seg_mcus, self.cache = _decode_arg(decode), index_cache, seg_mcus, None
        self.sample_cache = None
        if flag != "color":
            _refuse(f"RandomBackground(flag={flag!r})")
        # sorted: the reference's glob order depends on the file system
        self.background_images = sorted(glob.glob(osp.join(background_dir, "*.jpg")) + glob.glob(osp.join(background_dir, "*.png")))
        if not self.background_images:
            raise RuntimeError(f"No background images found in {background_dir}")
        self.background_dir, self.prob = background_dir, prob

    def plan(self, s, rnd, nprnd):
        if rnd.random() > self.prob:
            return
        path = rnd.choice(self.background_images)
        s["background"] = _plan_pixels(path, self, s, "background")


class _PillowStage:
    key = None

    def __init__(self, p, factor_interval):
        self.p, self.factor_interval = p, tuple(factor_interval)

    def draw(self, s, rnd):
        if rnd.random() <= self.p:
            s[self.key] = rnd.uniform(*self.factor_interval)


@PIPELINES.register_module()
class PillowSharpness(_PillowStage):
    key = "aug_sharpness"

    def __init__(self, p=0.3, factor_interval=(0., 50.)):
        super().__init__(p, factor_interval)


@PIPELINES.register_module()
class PillowContrast(_PillowStage):
    key = "aug_contrast"

    def __init__(self, p=0.3, factor_interval=(0.2, 50.)):
        super().__init__(p, factor_interval)


@PIPELINES.register_module()
class PillowBrightness(_PillowStage):
    key = "aug_brightness"

    def __init__(self, p=0.5, factor_interval=(0.1, 6.0)):
        super().__init__(p, factor_interval)


@PIPELINES.register_module()
class PillowColor(_PillowStage):
    key = "aug_color"

    def __init__(self, p=0.3, factor_interval=(0.0, 20.0)):
        super().__init__(p, factor_interval)


@PIPELINES.register_module()
class PillowBlur(_PillowStage):
    """GaussianBlur(k), k = random.randint(*factor_interval); `p` is ignored, as in the reference"""
    key = "aug_blur"

    def __init__(self, p=0.4, factor_interval=(1, 3)):
        super().__init__(p, factor_interval)

    def draw(self, s, rnd):
        s[self.key] = rnd.randint(*self.factor_interval)


@PIPELINES.register_module()
class CosyPoseAug:
    def __init__(self, p=0.8, pipelines=()):
        self.p = p
        self.pipelines = [build_from_cfg(c, PIPELINES) if isinstance(c, dict) else c for c in pipelines]
        names = [type(t).__name__ for t in self.pipelines]
        pos = [(_COSY_ORDER.index(n) if n in _COSY_ORDER else -1) for n in names]
        if -1 in pos or pos != sorted(set(pos)):
            _refuse(f"CosyPoseAug stages {names} (the device chain runs a subsequence of {_COSY_ORDER}, each at most once)")

    def plan(self, s, rnd, nprnd):
        if rnd.random() > self.p:
            return
        for t in self.pipelines:
            t.draw(s, rnd)


@PIPELINES.register_module()
class RandomHSV:
    """cv2 BGR -> HSV, each channel times uniform(-1, 1) * ratio + 1 (clipped only for factors >= 1), HSV -> BGR
    (aug_hsv_noise); factors stored in s["aug_hsv"]"""

    def __init__(self, h_ratio, s_ratio, v_ratio, prob=1.0):
        if not all(0 <= r <= 1 for r in (h_ratio, s_ratio, v_ratio)):
            _refuse("RandomHSV with a ratio outside [0, 1] (negative factors)")
        self.h_ratio, self.s_ratio, self.v_ratio, self.prob = h_ratio, s_ratio, v_ratio, prob

    def plan(self, s, rnd, nprnd):
        if rnd.random() > self.prob:
            return
        s["aug_hsv"] = tuple(rnd.uniform(-1, 1) * ratio + 1 for ratio in (self.h_ratio, self.s_ratio, self.v_ratio))


@PIPELINES.register_module()
class RandomNoise:
    """img + N(0, sigma) * 255, sigma = uniform(0, noise_ratio), clipped and truncated (aug_hsv_noise).  Where the
    reference draws np.random.normal, the sample's RandomState draws a Philox key instead (two uint64), which keeps every
    later draw at its place in the stream; the device makes the normals from Philox-4x64-10 under that key (DESIGN.md
    sections 2 and 9: the reference's distribution, not its stream).  s["aug_noise"] = (sigma, key)"""

    def __init__(self, noise_ratio, prob=1.0):
        self.noise_ratio, self.prob = noise_ratio, prob

    def plan(self, s, rnd, nprnd):
        if rnd.random() > self.prob:
            return
        sigma = rnd.uniform(0, self.noise_ratio)
        s["aug_noise"] = (sigma, nprnd.randint(0, 2 ** 64, size=2, dtype=np.uint64))


@PIPELINES.register_module()
class RandomSmooth:
    """cv2.blur(img, (k, k)), k = random.choice([1, 3, ..., max_kernel_size]) (aug_box); s["aug_smooth"] = k"""

    def __init__(self, max_kernel_size=7, prob=1.0):
        self.max_kernel_size = max_kernel_size
        self.kernel_sizes = [i * 2 + 1 for i in range(self.max_kernel_size // 2 + 1)]
        if max(self.kernel_sizes) > 7:
            _refuse(f"RandomSmooth(max_kernel_size={max_kernel_size}) (the box kernel takes k up to 7)")
        self.prob = prob

    def plan(self, s, rnd, nprnd):
        if rnd.random() > self.prob:
            return
        s["aug_smooth"] = rnd.choice(self.kernel_sizes)


# ---------------------------------------------------------------------------------------------------- formatting
@PIPELINES.register_module()
class DefaultFormatBundle:
    def plan(self, s, rnd, nprnd):
        pass


@PIPELINES.register_module()
class ImageToTensor:
    def __init__(self, keys):
        self.keys = list(keys)

    def plan(self, s, rnd, nprnd):
        pass


@PIPELINES.register_module()
class Collect:
    def __init__(self, keys, meta_keys=DEFAULT_META_KEYS):
        self.keys, self.meta_keys = list(keys), tuple(meta_keys)

    def plan(self, s, rnd, nprnd):
        s["_collect"] = self


@PIPELINES.register_module()
class MultiScaleFlipAug:
    """The views of test-time augmentation in the reference's order (radet/datasets/pipelines/test_time_aug.py:94-106):
    scales outermost; per scale the unflipped view, then one view per flip_direction.  Every view is planned as the single
    view at its scale is, with flip / flip_direction set, so img_shape, pad_shape and scale_factor are Resize's and Pad's.
    One view (a single img_scale, flip=False) is the plain test pipeline.  Several views are built for pipelines on frames
    in memory only (ImagePipeline refuses them behind LoadImageFromFile).  scale_factor= is refused (Resize has no such
    input here); flip=True without a RandomFlip among the transforms is an error -- the reference warns and then maps the
    boxes back with a flip that never happened."""

    def __init__(self, transforms, img_scale=None, scale_factor=None, flip=False, flip_direction="horizontal"):
        if scale_factor is not None or img_scale is None:
            _refuse("MultiScaleFlipAug(scale_factor=...) / without img_scale")
        scales = img_scale if isinstance(img_scale, list) else [img_scale]
        if not scales or not all(isinstance(v, (tuple, list)) and len(v) == 2 for v in scales):
            raise TypeError(f"MultiScaleFlipAug: img_scale is a tuple or a list of tuples, got {img_scale!r}")
        directions = list(flip_direction) if isinstance(flip_direction, (list, tuple)) else [flip_direction]
        for d in directions:
            if d not in K.PREP_FLIP:
                raise ValueError(f"MultiScaleFlipAug: flip_direction {d!r} (one of {sorted(K.PREP_FLIP)}, or a list of them)")
        self.transforms = [build_from_cfg(t, PIPELINES) if isinstance(t, dict) else t for t in transforms]
        if flip and not any(isinstance(t, RandomFlip) for t in self.transforms):
            raise ValueError("MultiScaleFlipAug(flip=True) without a RandomFlip among its transforms: the views would not be "
                             "flipped, and their boxes would be mapped back as if they were")
        self.flip, self.flip_direction = bool(flip), directions
        flips = [(False, None)] + ([(True, d) for d in directions] if flip else [])
        self.views = [(tuple(sc), f, d) for sc in scales for f, d in flips]
        if len(self.views) > K.TTA_MAX_VIEWS:
            raise ValueError(f"MultiScaleFlipAug: {len(self.views)} views ({len(scales)} scales x {len(flips)} flips), at most "
                             f"{K.TTA_MAX_VIEWS}")
        self.img_scale = self.views[0][0]

    def _plan_view(self, s, view, rnd, nprnd):
        s.update(scale=view[0], flip=view[1], flip_direction=view[2], _tta=True)
        for t in self.transforms:
            t.plan(s, rnd, nprnd)

    def plan(self, s, rnd, nprnd):
        if len(self.views) == 1:
            return self._plan_view(s, self.views[0], rnd, nprnd)
        views = []
        for view in self.views:                                 # (every view from the state in front of this stage)
            v = dict(s)
            self._plan_view(v, view, rnd, nprnd)
            views.append(v)
        s.update(views[0])                                      # the sample itself is its first view; the others ride along
        s["_views"] = views


# ---------------------------------------------------------------------------------------------------- the batched device part
def is_image_pipeline(transforms):
    return any((t.get("type") if isinstance(t, dict) else type(t).__name__) == "LoadImageFromFile" for t in transforms or ())


# the stages of a pipeline that starts from LoadImageFromWebcam: the reference's test pipeline, nothing else
_FRAME_STAGES = ("LoadImageFromWebcam", "MultiScaleFlipAug", "Resize", "RandomFlip", "Normalize", "Pad", "DefaultFormatBundle",
                 "ImageToTensor", "Collect")


def frame_desc_rows(frames, dst_hw, to_rgb, host_base, views=1, flips=None):
    """The descriptor rows of radet_preprocess_frames (include/radet_hip.h, PREP_DESC_INTS) for a batch of frames HxWx3 u8:
    an ndarray goes into the batch's upload buffer, packed, at the byte offset returned for it (its address: host_base +
    offset, the device address of that buffer's pixel part); a torch tensor is read where it is (data_ptr, row stride).
    views > 1 (test-time augmentation): views * B rows, view-major (row v * B + b), dst_hw and flips (PREP_FLIP_* bits) per
    row; the rows of a frame's views name the same address, and the frame is in the upload once.
    Host arithmetic only.  Returns (int32 [views * B, PREP_DESC_INTS], byte offset per frame or None, bytes of the upload)."""
    B = len(frames)
    rows = np.zeros((views * B, K.PREP_DESC_INTS), np.int32)
    offs, o = [], 0
    for b, f in enumerate(frames):
        h, w = int(f.shape[0]), int(f.shape[1])
        if isinstance(f, np.ndarray):
            addr, stride = host_base + o, 3 * w
            offs.append(o)
            o += 3 * h * w
        else:
            addr, stride = f.data_ptr(), (int(f.stride(0)) if h > 1 else 3 * w)
            offs.append(None)
        if not 0 <= stride < 2 ** 31:
            raise ValueError(f"frame of shape {tuple(f.shape)}: a row stride of {stride} bytes does not fit the descriptor")
        for r in range(b, views * B, B):
            row, (dh, dw) = rows[r], dst_hw[r]
            row[0:2] = np.array([addr & 0xFFFFFFFF, addr >> 32], np.uint32).view(np.int32)
            row[2:8] = [stride, h, w, dh, dw, (K.PREP_TO_RGB if to_rgb else 0) | (flips[r] if flips is not None else 0)]
    return rows, offs, o


def _upload_tables(frames, n_rows, build, dev):
    """[descriptor table of n_rows rows | host frames, packed, each once] into one device buffer in ONE pinned, non-blocking
    copy.  The table needs the buffer's address, so the buffer is allocated first (the host frames' bytes are known from their
    shapes) and build(address of the buffer's pixel part) -> (table i32 [n_rows, PREP_DESC_INTS], byte offset per frame or
    None, bytes of the pixel part) writes the rows against it; frames that are device tensors are not copied, the table holds
    their addresses.  Returns the table as i32 [n_rows * PREP_DESC_INTS]: a view of the buffer, which it keeps alive."""
    head = n_rows * K.PREP_DESC_INTS * 4
    nbytes = sum(f.size for f in frames if isinstance(f, np.ndarray))
    up = torch.empty(head + nbytes, dtype=torch.uint8, device=dev)
    table, offs, packed = build(up.data_ptr() + head)
    if packed != nbytes or table.size * 4 != head:
        raise RuntimeError(f"upload: a table of {table.size * 4} bytes and {packed} bytes of frames for {head} + {nbytes}")
    stage = torch.empty(head + nbytes, dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    host[:head] = table.reshape(-1).view(np.uint8)
    for f, o in zip(frames, offs):
        if o is not None:
            np.copyto(host[head + o:head + o + f.size].reshape(f.shape), f)
    up.copy_(stage, non_blocking=True)
    return up[:head].view(torch.int32)


def upload_frames(frames, dst_hw, to_rgb, dev, views=1, flips=None):
    """_upload_tables for a plain batch: the table of frame_desc_rows.  Returns it flat, i32 [views * B * PREP_DESC_INTS]."""
    return _upload_tables(frames, views * len(frames), lambda base: frame_desc_rows(frames, dst_hw, to_rgb, base, views, flips), dev)


def tile_desc_rows(frames, rects, row_start, dst_hw, to_rgb, host_base):
    """The descriptor rows of a TILED batch (tiled inference, ops/tiles.py): rects i32 [R, 4] (x0, y0, tw, th), image-major
    with row_start i32 [B + 1], are source rectangles inside the frames.  A row of radet_preprocess_frames' table names a byte
    address, a row stride and an h x w, so a rectangle of a frame is just another row: the frame's address shifted by
    y0 * stride + 3 * x0, the frame's stride, the rectangle's th x tw -- the kernel reads it where the frame lies.  Frames
    are placed as frame_desc_rows places them (host frames packed behind host_base, each ONCE; device tensors in place).
    dst_hw: the resized size per row.  Host arithmetic only.  Returns (int32 [B, PREP_DESC_INTS] the source frames as
    frame_desc_rows describes them at their own size -- what the RoI crops read --, int32 [R, PREP_DESC_INTS] the rows, byte
    offset per frame or None, bytes of the upload)."""
    B = len(frames)
    rects = np.asarray(rects, np.int64).reshape(-1, 4)
    if len(row_start) != B + 1 or int(row_start[0]) != 0 or int(row_start[-1]) != len(rects) or len(dst_hw) != len(rects):
        raise ValueError(f"tile_desc_rows: row_start {list(row_start)} for {B} frames and {len(rects)} rows")
    src, offs, nbytes = frame_desc_rows(frames, [tuple(int(v) for v in f.shape[:2]) for f in frames], to_rgb, host_base)
    rows = np.zeros((len(rects), K.PREP_DESC_INTS), np.int32)
    for b, f in enumerate(frames):
        h, w = int(f.shape[0]), int(f.shape[1])
        base = int(src[b, 0:2].view(np.uint32)[0]) | (int(src[b, 0:2].view(np.uint32)[1]) << 32)
        stride = int(src[b, 2])
        for r in range(int(row_start[b]), int(row_start[b + 1])):
            x0, y0, tw, th = (int(v) for v in rects[r])
            if not (0 <= x0 and 0 <= y0 and 1 <= tw and 1 <= th and x0 + tw <= w and y0 + th <= h):
                raise ValueError(f"row {r}: the rectangle {(x0, y0, tw, th)} leaves its {w} x {h} frame")
            addr = base + y0 * stride + 3 * x0
            rows[r, 0:2] = np.array([addr & 0xFFFFFFFF, addr >> 32], np.uint32).view(np.int32)
            rows[r, 2:8] = [stride, th, tw, dst_hw[r][0], dst_hw[r][1], K.PREP_TO_RGB if to_rgb else 0]
    return src, rows, offs, nbytes


def upload_tile_rows(frames, rects, row_start, dst_hw, to_rgb, dev):
    """[the B source frames' table | the R rows' table | host frames, packed, each once] into one device buffer in ONE pinned,
    non-blocking copy, as upload_frames does for a plain batch.  Returns (table i32 [B + R, PREP_DESC_INTS]: a view of the
    buffer, which it keeps alive; its first B rows are what crops= reads, the rows' table starts at row B)."""
    B, R = len(frames), len(rects)

    def build(base):
        src, rows, offs, nbytes = tile_desc_rows(frames, rects, row_start, dst_hw, to_rgb, base)
        return np.concatenate([src, rows]), offs, nbytes
    return _upload_tables(frames, B + R, build, dev).view(B + R, K.PREP_DESC_INTS)


class ImagePipeline:
    """A pipeline that starts from files: host planning per sample, one batched device pass per batch.  Or from frames in
    memory (LoadImageFromWebcam first): a test pipeline whose device pass is one upload and one launch (_run_frames)."""

    def __init__(self, transforms, image_decode=None, index_cache=None, seg_mcus=None, sample_cache=None, cache_bytes=None):
        """image_decode ('host' / 'device'), index_cache (a directory) and seg_mcus (MCUs per index segment, or 'row'),
        when given, are set on the pipeline's LoadImageFromFile and RandomBackground stages.
        sample_cache='device' with cache_bytes (the HBM budget for pixels, required): decoded frames and backgrounds stay
        in HBM and mask PNGs in host memory as run lists after their first visit (datasets/sample_cache.py)"""
        sample_cache, cache_bytes = cache_args(sample_cache, cache_bytes)
        given = image_decode is not None or index_cache is not None or seg_mcus is not None
        if given:
            extra = dict(**({} if image_decode is None else dict(decode=_decode_arg(image_decode))),
                         **({} if index_cache is None else dict(index_cache=index_cache)),
                         **({} if seg_mcus is None else dict(seg_mcus=seg_mcus)))
            transforms = [{**t, **extra} if isinstance(t, dict) and t.get("type") in ("LoadImageFromFile", "RandomBackground") else t
                          for t in transforms]
        self.cfg = list(transforms)                       # (wrapped datasets share one pipeline when their configs are equal)
        self.transforms = [build_from_cfg(t, PIPELINES) if isinstance(t, dict) else t for t in transforms]
        if given:
            for t in self.transforms:                     # (stages that were passed as objects)
                if isinstance(t, (LoadImageFromFile, RandomBackground)):
                    t.decode = t.decode if image_decode is None else image_decode
                    t.index_cache = t.index_cache if index_cache is None else index_cache
                    t.seg_mcus = t.seg_mcus if seg_mcus is None else seg_mcus
        # one index cache per pipeline (= per dataset), shared by the frames and the backgrounds
        shared = None
        for t in self.transforms:
            if isinstance(t, (LoadImageFromFile, RandomBackground)) and t.decode == "device":
                shared = shared or jpeg.IndexCache(t.index_cache)
                t.cache = shared
        self.device_decode = shared is not None
        # decode_stats: files decoded by the device decoder / files of a decode='device' stage that went to the host decoder.
        # cache_stats (a property): the sample cache's counters -- hits / misses (frame and background lookups), inserted /
        # bytes (entries and pixel bytes in the HBM arena), rejected_full (decoded files the budget or the chunk size did not
        # take), invalidated (entries dropped because the file changed), mask_hits / mask_bytes (masks served from, and
        # bytes of, the host run-list table); all zero without sample_cache='device'
        self.decode_stats = dict(device=0, fallback=0)
        self.sample_cache = None if sample_cache is None else SampleCache(cache_bytes)
        for t in self.transforms:
            if isinstance(t, (LoadImageFromFile, RandomBackground, LoadAnnotations)):
                t.sample_cache = self.sample_cache
        self._decode_pending = []
        flat = []
        for t in self.transforms:
            flat += [t] + (list(t.transforms) if isinstance(t, MultiScaleFlipAug) else [])
        names = [type(t).__name__ for t in flat]
        # frames in memory: LoadImageFromWebcam stands where LoadImageFromFile does, in front of a test pipeline
        self.frames = bool(names) and names[0] == "LoadImageFromWebcam"
        if "LoadImageFromWebcam" in names and (not self.frames or "LoadImageFromFile" in names):
            _refuse(f"pipeline {names} (LoadImageFromWebcam is the first stage and the only loader)")
        if self.frames:
            names[0] = "LoadImageFromFile"
            self._check_frame_pipeline(flat, sample_cache)
        # the block after Resize: the warp stages, and the CutOut stages that stand in one run with them from Resize on (or
        # from the RandomCrop behind it); a CutOut anywhere else is a late one, which has its own slot of the order
        start = names.index("Resize") + 1 if "Resize" in names else len(names)
        start += start < len(names) and names[start] == "RandomCrop"
        stop = start
        while stop < len(names) and names[stop] in _BLOCK:
            stop += 1
        block = [k for k, n in enumerate(names) if n in _AFFINE or (n in ("CutOut",) + _COLOR_STAGES and start <= k < stop)]
        late = [k for k, n in enumerate(names) if n == "CutOut" and k not in block]
        if "CutOut" in names and any(isinstance(t, MultiScaleFlipAug) for t in flat):
            _refuse("CutOut in a MultiScaleFlipAug (test) pipeline")
        # the colour stages work on the packed u8 frames of that block and nowhere else
        for k, n in enumerate(names):
            if n in _COLOR_STAGES and any(isinstance(t, MultiScaleFlipAug) for t in flat):
                _refuse(f"{n} in a MultiScaleFlipAug (test) pipeline (the colour stages are training augmentation: take it out "
                        f"of the test pipeline)")
            if n in _COLOR_STAGES and k not in block:
                _refuse(f"{n} at position {k} of {names} (the colour stages stand in the block directly after Resize -- or after "
                        f"the RandomCrop behind it --, bare next to Rotate / Shear / Translate / CutOut or inside one AutoAugment(color_stages=True): "
                        f"move it there)")
        for k in late:
            flat[k].late = True
        if block:
            self._check_affine(flat, names, block)
        # (the block counts as one stage, "Affine", of the order)
        slots = ["Affine" if k in block else n for k, n in enumerate(names) if k not in block[1:]]
        pos = [(_ORDER.index(n) if n in _ORDER else -1) for n in slots]
        for n in (n for n in names if n in _ZOOM):
            if "Resize" in names and names.index(n) > names.index("Resize"):
                _refuse(f"{n} after Resize in {names} (the zoom stages plan a window of the source image: they stand before Resize)")
            if "RandomCrop" in names:
                _refuse(f"{n} together with RandomCrop (a source window and a window of the resized image in one pipeline)")
            if any(isinstance(t, MultiScaleFlipAug) for t in flat):
                _refuse(f"{n} in a MultiScaleFlipAug (test) pipeline")
        if "RandomCrop" in names and (-1 not in pos and pos != sorted(set(pos)) or any(isinstance(t, MultiScaleFlipAug) for t in flat)):
            _refuse(f"RandomCrop at position {names.index('RandomCrop')} of {names} (it stands directly after Resize: after "
                    f"{_ORDER[:_ORDER.index('RandomCrop')][-3:]}, before every stage of {_ORDER[_ORDER.index('RandomCrop') + 1:]}; "
                    f"not in a MultiScaleFlipAug pipeline)")
        if -1 in pos or pos != sorted(set(pos)):
            _refuse(f"pipeline {names} (an image pipeline runs a subsequence of {_ORDER}, each stage once)")
        if "CosyPoseAug" in names and any(n in _MIX for n in names):
            _refuse("CosyPoseAug together with RandomHSV / RandomNoise / RandomSmooth")
        self.mix = any(n in _MIX for n in names)
        for need in ("LoadImageFromFile", "Normalize", "Collect"):
            if need not in names:
                _refuse(f"an image pipeline without {need}")
        self.assigner = next((t for t in flat if isinstance(t, LabelAssignment)), None)
        dm = next((t for t in flat if isinstance(t, GenerateDistanceMap)), None)
        if self.assigner is not None and dm is None:
            raise ValueError("LabelAssignment needs GenerateDistanceMap before it")
        # the mask-free sampler: box crops of the augmented image -> GDT / MBD maps (Sobel and MBD are the device paths)
        self.mask_free = dm if dm is not None and not dm.with_gt_mask else None
        if self.mask_free is not None and getattr(dm.distance_transform, "extract_edge_func", None) is not None:
            _refuse("GenerateDistanceMap(extract_edge_func=...) in an image pipeline (a host callback)")
        if late and self.mask_free is not None:
            _refuse("a CutOut behind the photometric stages together with GenerateDistanceMap(with_gt_mask=False) (the mask-free "
                    "crops are cut from the u8 image in front of the blends: they would not see the holes)")
        self.tta = any(isinstance(t, MultiScaleFlipAug) for t in self.transforms)
        # test-time augmentation: the number of views per sample (1: the plain test pipeline)
        self.views = max([len(t.views) for t in self.transforms if isinstance(t, MultiScaleFlipAug)] or [1])
        if self.views > 1 and not self.frames:
            raise NotImplementedError(
                f"MultiScaleFlipAug with {self.views} views (flip=True / several scales) behind LoadImageFromFile: test-time "
                "augmentation is built for frames in memory (LoadImageFromWebcam first; inference_detector / detect_frames on "
                "loaded images); file datasets, single_gpu_test and tools/test.py with several views are not implemented")

    @staticmethod
    def _check_affine(flat, names, block):
        """Rotate / Shear / Translate / CutOut (in any order, repeats allowed, at most 4) or one AutoAugment over them: one
        block directly after Resize.  A block without a warp stage is pointwise: it may follow RandomCrop and stand in a
        pipeline with the zoom stages.  (Seg fields need no check here: LoadAnnotations(with_seg=True) does not build.)"""
        where = f"{[names[k] for k in block]} at positions {block} of {names}"
        stages = []
        for t in (flat[k] for k in block):
            stages += [u for policy in t.transforms for u in policy] if isinstance(t, AutoAugment) else [t]
        warps = [k for k in block if isinstance(flat[k], _AffineStage)
                 or (isinstance(flat[k], AutoAugment) and any(isinstance(u, _AffineStage) for p in flat[k].transforms for u in p))]
        first = names[warps[0]] if warps else names[block[0]]
        if any(isinstance(t, MultiScaleFlipAug) for t in flat):
            _refuse(f"{first} in a MultiScaleFlipAug (test) pipeline")
        for other in ("RandomCrop", *_ZOOM) if warps else ():
            if other in names:
                _refuse(f"{first} together with {other} (a warp composed with a window is left out)")
        before = ("Resize",) if warps else ("Resize", "RandomCrop")
        if block != list(range(block[0], block[0] + len(block))) or block[0] == 0 or names[block[0] - 1] not in before:
            _refuse(f"{where} (the affine stages stand as one block directly after Resize, before RandomBackground)")
        kinds = [names[k] for k in block]
        if "AutoAugment" in kinds and len(kinds) > 1:
            _refuse(f"{where} (bare Rotate / Shear / Translate stages, or one AutoAugment)")
        if len(kinds) > _AFFINE_MAX_ENTRIES:
            _refuse(f"{where} (at most {_AFFINE_MAX_ENTRIES} affine entries per sample)")
        for t in (t for t in stages if isinstance(t, _AffineStage)):
            # the fixed-point range of the warp kernel, on the largest image the augmentation kernels take
            for m in t.worst_matrices(K.AUG_MAX_W, K.AUG_MAX_W):
                if not K.warp_fits(K.invert_affine(m), K.AUG_MAX_W, K.AUG_MAX_W):
                    _refuse(f"{type(t).__name__} with the matrix {m.tolist()} (its inverse leaves the warp kernel's 32-bit "
                            f"fixed point on an image of {K.AUG_MAX_W} x {K.AUG_MAX_W})")

    @staticmethod
    def _check_frame_pipeline(flat, sample_cache):
        """a pipeline on frames is a test pipeline: no annotations, background, augmentation stages or assigner"""
        for t in flat:
            n = type(t).__name__
            if n not in _FRAME_STAGES:
                _refuse(f"{n} in a pipeline that starts with LoadImageFromWebcam (a test pipeline: {_FRAME_STAGES})")
            if isinstance(t, RandomFlip) and t.flip_ratio:
                _refuse("RandomFlip(flip_ratio > 0) in a pipeline that starts with LoadImageFromWebcam")
        if sample_cache is not None:
            _refuse("sample_cache with a pipeline that starts with LoadImageFromWebcam (frames have no file to key them)")

    @property
    def cache_stats(self):
        from .sample_cache import COUNTERS
        return dict(self.sample_cache.stats) if self.sample_cache is not None else dict.fromkeys(COUNTERS, 0)

    def plan(self, results, rnd, nprnd):
        """host part of one sample (thread-safe for distinct generators): decoding, boxes, random draws"""
        s = dict(results)
        for t in self.transforms:
            if not isinstance(t, LabelAssignment):     # (device-only: run() does it; GenerateDistanceMap plans its crops)
                if t.plan(s, rnd, nprnd) is False:     # (RandomCrop left no gt box: the reference's pipeline returns None)
                    return None
        s["_nprnd"] = nprnd
        return s

    def __call__(self, results):
        """one sample on the global generators, like the reference (None when RandomCrop dropped it)"""
        import random
        s = self.plan(results, random, np.random)
        return None if s is None else self.run([s])[0]

    # --------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _dev():
        return torch.device("cuda", torch.cuda.current_device())

    def _decode_packed(self, sources, dev, align=1):
        """The packed u8 BGR source buffer of a batch whose images are jpeg.DeviceJpeg plans (and host arrays, for the files
        the device decoder does not take): one pinned non-blocking upload of the files, tables and index rows, then
        radet_jpeg_decode's three launches.  Returns (buffer, pixel offset per source); nothing waits for the device: the
        decoder's error words are copied to pinned memory and read by a later call (check_decode_errors)."""
        self.check_decode_errors()
        offs, o = [], 0
        for a in sources:
            offs.append(o)
            o += -(-a.shape[0] * a.shape[1] // align) * align
        src = torch.empty(o * 3, dtype=torch.uint8, device=dev)
        on_dev = [k for k, a in enumerate(sources) if isinstance(a, jpeg.DeviceJpeg)]
        on_host = [k for k, a in enumerate(sources) if not isinstance(a, jpeg.DeviceJpeg)]
        self.decode_stats["device"] += len(on_dev)
        self.decode_stats["fallback"] += len(on_host)
        if on_host:
            up = torch.from_numpy(np.concatenate([sources[k].reshape(-1) for k in on_host])).pin_memory().to(dev, non_blocking=True)
            u = 0
            for k in on_host:
                n = sources[k].size
                src[offs[k] * 3:offs[k] * 3 + n].copy_(up[u:u + n])
                u += n
        self._decode_into(src, [sources[k] for k in on_dev], [offs[k] for k in on_dev], dev)
        return src, offs

    def _decode_into(self, src, items, item_offs, dev):
        """radet_jpeg_decode of `items` to their pixel offsets of the packed buffer `src`; the error words go to the pending list"""
        blob, sections, sizes = jpeg.pack_batch(items, item_offs)
        blob = torch.from_numpy(blob).pin_memory().to(dev, non_blocking=True)
        err, _, _ = K.jpeg_decode(blob, sections, sizes, len(items), src)
        host_err = torch.empty(len(items), dtype=torch.int32).pin_memory()
        host_err.copy_(err, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._decode_pending.append((ev, host_err, [it.path for it in items]))

    def _cached_packed(self, planned, with_bg, sources, dev, align=1):
        """The packed u8 BGR source buffer of a batch under sample_cache='device', whose sources are host arrays, jpeg.DeviceJpeg
        plans and cache hits (CachedImage).  Host arrays go up in one pinned non-blocking copy; one radet_copy_segments
        launch moves them and every hit to their places; the JPEG plans are decoded in place.  Then the newly decoded files
        that the arena takes are copied into it by a second launch and entered in the table.  A batch of hits only uploads
        no pixels; nothing here waits for the device.  Returns (buffer, pixel offset per source)."""
        self.check_decode_errors()
        cache = self.sample_cache
        keys = ([s.get("_cache_keys", {}).get("img") for s in planned]
                + [planned[i].get("_cache_keys", {}).get("background") for i in with_bg])
        offs, o = [], 0
        for a in sources:
            offs.append(o)
            o += -(-a.shape[0] * a.shape[1] // align) * align
        src = torch.empty(o * 3, dtype=torch.uint8, device=dev)
        base = src.data_ptr()
        hits = [k for k, a in enumerate(sources) if isinstance(a, CachedImage)]
        on_dev = [k for k, a in enumerate(sources) if isinstance(a, jpeg.DeviceJpeg)]
        on_host = [k for k, a in enumerate(sources) if isinstance(a, np.ndarray)]
        if self.device_decode:
            self.decode_stats["device"] += len(on_dev)
            self.decode_stats["fallback"] += len(on_host)
        cache.wait_inserts()
        rows = [(sources[k].addr, base + offs[k] * 3, sources[k].nbytes) for k in hits]
        if on_host:
            up = torch.from_numpy(np.concatenate([sources[k].reshape(-1) for k in on_host])).pin_memory().to(dev, non_blocking=True)
            u = up.data_ptr()
            for k in on_host:
                rows.append((u, base + offs[k] * 3, sources[k].size))
                u += sources[k].size
        if rows:
            cache.copy(rows, dev)
        if on_dev:
            self._decode_into(src, [sources[k] for k in on_dev], [offs[k] for k in on_dev], dev)
        fresh = [k for k in on_host + on_dev if keys[k] is not None]
        taken = cache.reserve([(keys[k], sources[k].shape) for k in fresh])
        if taken:
            where = {keys[k][0]: base + offs[k] * 3 for k in reversed(fresh)}
            cache.copy([(where[key[0]], addr, nbytes) for key, _, addr, nbytes in taken], dev)
            cache.record_insert()
            cache.commit(taken)
        return src, offs

    def check_decode_errors(self, wait=False):
        """raise for a file whose device decode set an error word (the batches whose copy has arrived; wait=True: all)"""
        while self._decode_pending and (wait or self._decode_pending[0][0].query()):
            ev, host_err, paths = self._decode_pending.pop(0)
            if wait:
                ev.synchronize()
            bad = [(p, int(e)) for p, e in zip(paths, host_err.tolist()) if e]
            if bad and self.sample_cache is not None:
                for p, _ in bad:
                    self.sample_cache.drop(p)
            if bad:
                what = "; ".join(f"{p}: " + ", ".join(v for k, v in jpeg.ERRORS.items() if e & k) for p, e in bad)
                raise ValueError(f"device JPEG decode failed (the pixels of that batch are undefined): {what}")

    def _resize_packed(self, arrays, dst_hw, dev, align=1, src=None, views=None):
        """u8 HWC images of any sizes -> one packed device buffer of the dst sizes (one upload, one resize launch); every
        image starts at a multiple of `align` pixels.  src: (packed device buffer, pixel offsets) when the images are there
        already.  views: per image its view row (sample_view) -- dst_hw is then the size of the row's output window"""
        src, src_offs = src if src is not None else (torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays])).to(dev), None)
        sdesc, ddesc, so, do = [], [], 0, 0
        for k, (a, (h, w)) in enumerate(zip(arrays, dst_hw)):
            so = so if src_offs is None else src_offs[k]
            sdesc.append((so, a.shape[0], a.shape[1]))
            ddesc.append((do, h, w))
            so += a.shape[0] * a.shape[1]
            do += -(-h * w // align) * align
        dst = torch.empty(do * 3, dtype=torch.uint8, device=dev)
        n = len(arrays)
        desc = np.array(sdesc + ddesc, np.int32).reshape(-1)
        if views is not None:
            desc = np.concatenate([desc, np.array(views, np.int32).reshape(-1)])
        desc = torch.from_numpy(desc).to(dev)
        K.resize_linear_u8(src, desc[:3 * n].view(n, 3), dst, desc[3 * n:6 * n].view(n, 3), n, max(h * w for h, w in dst_hw), 3,
                           views=desc[6 * n:].view(n, K.VIEW_INTS) if views is not None else None)
        return dst, [d[0] for d in ddesc]

    @staticmethod
    def _warp_packed(img, entries, offs, hw, dev, channels=3):
        """The block entries of a batch applied to its packed images, rank by rank (k = 0 .. the longest list - 1).  entries:
        per image a list, in the order the entries ran, of (forward 2 x 3 matrix, fill) for a warp or CutHoles(rects, fill)
        for a CutOut; offs / hw: per image its pixel offset and size.  At rank k: one radet_warp_affine_u8 launch if any
        image's k-th entry is a warp, ping-ponging between `img` and one more buffer of its size -- an image whose k-th
        entry is not a warp is copied (WARP_SKIP) --, then one radet_cutout_u8 launch, in place, if any image's k-th entry
        is a CutOut (the other images are skip rows).  So a hole cut at a lower rank is warped with the image and one cut at
        a higher rank is axis-aligned.  One descriptor upload for all ranks: the warp rows, then (only when some entry is a
        CutOut) the CutOut rows and the hole table, then (only when some entry is a colour stage) the colour rows.  A ColorOp
        at rank k: after the warp and CutOut launches of that rank, one radet_color_stats_u8 launch if any image's k-th entry
        is 'equalize' or 'contrast' (into its own slice of one histogram buffer, zeroed once per batch by radet_fill_zero),
        then one radet_color_apply_u8 launch, in place (the other images are skip rows).  Returns the buffer that holds
        the result."""
        ranks, n = max(len(e) for e in entries), len(entries)
        if not ranks:
            return img
        cut = any(isinstance(x, CutHoles) for e in entries for x in e)
        col = any(isinstance(x, ColorOp) for e in entries for x in e)
        W = np.zeros((ranks, n, K.WARP_DESC_INTS), np.int32)
        D = np.zeros((ranks, n, K.CUTOUT_DESC_INTS), np.int32) if cut else None
        CD = np.zeros((ranks, n, K.COLOR_DESC_INTS), np.int32) if col else None
        holes, first, dims = [], 0, []
        for k in range(ranks):
            kth = [(e[k] if k < len(e) else None) for e in entries]
            for i, (x, o, (h, w)) in enumerate(zip(kth, offs, hw)):
                K.warp_desc_row(W[k, i], o, o, h, w, channels, *((None,) if x is None or isinstance(x, (CutHoles, ColorOp)) else x))
                if isinstance(x, CutHoles):
                    K.cutout_desc_row(D[k, i], o, h, w, x.fill, first, len(x.rects))
                    holes.append(np.asarray(x.rects, np.int32).reshape(-1, 4))
                    first += len(x.rects)
                elif cut:
                    K.cutout_desc_row(D[k, i], o, h, w, skip=True)
                if isinstance(x, ColorOp):
                    K.color_desc_row(CD[k, i], o, h, w, x.kind, x.factor)
                elif col:
                    K.color_desc_row(CD[k, i], o, h, w, skip=True)
            dims.append((any(x is not None and not isinstance(x, (CutHoles, ColorOp)) for x in kth),
                         *K.cutout_launch_dims([x.rects if isinstance(x, CutHoles) else None for x in kth], hw),
                         any(isinstance(x, ColorOp) for x in kth),
                         any(isinstance(x, ColorOp) and x.kind in K.COLOR_STATS_KINDS for x in kth)))
        parts = [W] + ([D, np.concatenate(holes)] if cut else []) + ([CD] if col else [])
        up = torch.from_numpy(np.concatenate([a.reshape(-1) for a in parts])).to(dev)
        wdesc = up[:W.size].view(ranks, n, K.WARP_DESC_INTS)
        if cut:
            cdesc = up[W.size:W.size + D.size].view(ranks, n, K.CUTOUT_DESC_INTS)
            table = up[W.size + D.size:up.numel() - (CD.size if col else 0)].view(-1, 4)
        hist = None
        if col:
            coldesc = up[up.numel() - CD.size:].view(ranks, n, K.COLOR_DESC_INTS)
            if any(d[4] for d in dims):
                hist = torch.empty((ranks, n, 4, 256), dtype=torch.int32, device=dev)
                K.fill_zero(hist)
        max_px = max(h * w for h, w in hw)
        cur, other = img, None
        for k, (warp, most, area, colour, stats) in enumerate(dims):
            if warp:
                other = torch.empty_like(img) if other is None else other
                K.warp_affine_u8(cur, other, wdesc[k], n, max_px, channels)
                cur, other = other, cur
            if most and area:
                K.cutout_u8(cur, cdesc[k], table, n, most, area)
            if stats:
                K.color_stats_u8(cur, coldesc[k], hist[k], n, max_px)
            if colour:
                K.color_apply_u8(cur, coldesc[k], hist[k] if stats else None, n, max_px)
        return cur

    @staticmethod
    def _cutout_late(out, planned, hw, dev, mean, stdinv):
        """the holes of the batch's late CutOut stages cut into the finished f32 batch: one upload, one radet_cutout_f32
        launch (none when no sample drew a hole of any area)"""
        B = len(planned)
        D = np.zeros((B, K.CUTOUT_DESC_INTS), np.int32)
        holes, first = [], 0
        for i, (s, (h, w)) in enumerate(zip(planned, hw)):
            rects, fill = s.get("cutout_late", (None, (0, 0, 0)))
            if rects is None:
                K.cutout_desc_row(D[i], i, h, w, skip=True)
                continue
            K.cutout_desc_row(D[i], i, h, w, fill, first, len(rects), flip=bool(s.get("flip")), to_rgb=bool(s["img_norm_cfg"]["to_rgb"]))
            holes.append(np.asarray(rects, np.int32).reshape(-1, 4))
            first += len(rects)
        most, area = K.cutout_launch_dims([s["cutout_late"][0] if "cutout_late" in s else None for s in planned], hw)
        if not (most and area):
            return
        up = torch.from_numpy(np.concatenate([D.reshape(-1), np.concatenate(holes).reshape(-1)])).to(dev)
        K.cutout_f32(out, up[:D.size].view(B, K.CUTOUT_DESC_INTS), up[D.size:].view(-1, 4), B, most, area, mean, stdinv)

    @staticmethod
    def _mask_groups(planned, keys):
        """the samples that carry masks, grouped by (kind: "bitmap" / "runs", source size, keys[i]), bitmaps first: per group
        (kind, source size, key, sample indices, masks per sample)"""
        groups = {}
        for i, s in enumerate(planned):
            if "gt_masks_rle" in s and "gt_masks" in s:
                raise ValueError("a sample carries both gt_masks and gt_masks_rle")
            if "gt_masks" in s:
                groups.setdefault(("bitmap", tuple(s["gt_masks"].shape[1:]), keys[i]), []).append(i)
            elif "gt_masks_rle" in s:
                groups.setdefault(("runs", tuple(s["gt_masks_rle"][1]), keys[i]), []).append(i)
        return [(*key, idx, [len(planned[i]["gt_masks"] if key[0] == "bitmap" else planned[i]["gt_masks_rle"][0]) for i in idx])
                for key, idx in sorted(groups.items(), key=lambda kv: kv[0][0] != "bitmap")]

    @staticmethod
    def _upload_runs(planned, idx, src_hw, flips, dev, rows=None):
        """the run lists of the samples idx (and their view rows) in one pinned upload: radet_rle_masks' three arrays, and
        the rows' device copy"""
        ends, prows, mrows = rle.pack_runs([m for i in idx for m in planned[i]["gt_masks_rle"][0]], *src_hw, flips)
        parts = [ends.view(np.int32), prows.reshape(-1), mrows.reshape(-1)] + ([] if rows is None else [rows.reshape(-1)])
        packed = torch.from_numpy(np.concatenate(parts)).pin_memory().to(dev, non_blocking=True)
        a, b, c = ends.size, ends.size + prows.size, ends.size + prows.size + mrows.size
        return (packed[:a], packed[a:b].view(-1, K.RLE_PART_INTS), packed[b:c].view(-1, K.RLE_MASK_INTS),
                None if rows is None else packed[c:].view(-1, K.VIEW_INTS))

    def _affine_masks(self, planned, hw, dev, ahw):
        """_masks for a batch in which some sample carries affine entries.  Per group of samples of equal source size,
        resized size, assigner size and flip: the unflipped resized bitmaps (radet_mask_max + radet_mask_transform, or
        radet_rle_masks for run lists), one warp launch per entry rank on the stack (one channel, fill 0; the masks of a
        sample with fewer entries are copied), then flip and pad for the assigner in one radet_mask_transform pass where
        the group needs either.  The first list (the merge's masks) is the warped, unflipped stack."""
        masks, flipped = [None] * len(planned), [None] * len(planned)
        keys = [(hw[i], ahw[i], bool(s.get("flip"))) for i, s in enumerate(planned)]
        for kind, src_hw, (dst_hw, out_hw, flip), idx, counts in self._mask_groups(planned, keys):
            G = sum(counts)
            if not G:
                for i in idx:
                    masks[i] = torch.zeros(0, *dst_hw, dtype=torch.uint8, device=dev)
                    flipped[i] = torch.zeros(0, *out_hw, dtype=torch.uint8, device=dev)
                continue
            if kind == "bitmap":
                src = torch.from_numpy(np.concatenate([planned[i]["gt_masks"] for i in idx])).to(dev)
                res = K.mask_transform(src, resized_hw=dst_hw, normalize=True)
            else:
                res = K.rle_masks(*self._upload_runs(planned, idx, src_hw, np.zeros(G, bool), dev)[:3], dst_hw)
            px = dst_hw[0] * dst_hw[1]
            entries = [[(m, (0, 0, 0)) for m, _ in planned[i].get("affine", ())] for i, c in zip(idx, counts) for _ in range(c)]
            res = self._warp_packed(res.view(-1), entries, [g * px for g in range(G)], [dst_hw] * G, dev, channels=1).view(G, *dst_hw)
            fl = K.mask_transform(res, out_hw=out_hw, flip="horizontal" if flip else None) if flip or out_hw != dst_hw else res
            o = 0
            for i, c in zip(idx, counts):
                masks[i], flipped[i] = res[o:o + c], fl[o:o + c]
                o += c
        return masks, flipped

    def run(self, planned, collate=False):
        """device part of a batch of planned samples; returns per-sample dicts, or one collated batch dict"""
        if self.frames:
            return self._run_frames(planned, collate)[0]
        dev = self._dev()
        B = len(planned)
        # each sample's view: RandomCrop planned the output window of the virtual resized image, Expand / MinIoURandomCrop the
        # window of the source (it may overhang the image) that is resized; hw is the size of what is computed
        views = [sample_view(s) for s in planned]
        hw = [v[8:10] for v in views]
        crop, zoom = any("crop_window" in s for s in planned), any("src_window" in s for s in planned)
        if crop and zoom:
            raise ValueError("a batch with source windows (Expand / MinIoURandomCrop) and crop windows (RandomCrop)")
        for Hr, Wr, wy0, wx0, wh, ww, oy, ox, h, w, _, _ in views:
            if crop and not (0 <= oy <= Hr - h and 0 <= ox <= Wr - w and h > 0 and w > 0):
                raise ValueError(f"crop window {h} x {w} at ({oy}, {ox}) of a resized image of {Hr} x {Wr}")
            if zoom and (wh <= 0 or ww <= 0 or not all(-2 ** 30 < v < 2 ** 30 for v in (wy0, wx0, wh, ww))):
                raise ValueError(f"source window {wh} x {ww} at ({wy0}, {wx0})")
        windowed = crop or zoom                                   # (a batch without windows: the resize launch takes no rows)
        for h, w in hw:
            if h > K.AUG_MAX_W or w > K.AUG_MAX_W:
                raise ValueError(f"image of {h} x {w}: the augmentation kernels take sides up to {K.AUG_MAX_W}")
        # (mix pipelines: images start at multiples of 4 pixels, so the mix kernels' dword accesses are aligned)
        with_bg = [i for i, s in enumerate(planned) if "background" in s]
        sources = [s["img"] for s in planned] + [planned[i]["background"] for i in with_bg]
        if self.sample_cache is None and self.device_decode and not any(isinstance(a, jpeg.DeviceJpeg) for a in sources):
            self.decode_stats["fallback"] += len(sources)          # (every file of the batch went to the host decoder)
        if self.sample_cache is not None or any(isinstance(a, jpeg.DeviceJpeg) for a in sources):
            # decode='device': frames and backgrounds are decoded by the same three launches into one packed source buffer;
            # sample_cache='device': cached files are gathered into that buffer, new ones leave it for the arena
            src, soffs = (self._cached_packed(planned, with_bg, sources, dev, align=4 if self.mix else 1)
                          if self.sample_cache is not None else self._decode_packed(sources, dev, align=4 if self.mix else 1))
            img, offs = self._resize_packed(sources[:B], hw, dev, align=4 if self.mix else 1, src=(src, soffs[:B]),
                                            views=views if windowed else None)
            bg, bg_offs = (self._resize_packed(sources[B:], [hw[i] for i in with_bg], dev, src=(src, soffs[B:]))
                           if with_bg else (torch.zeros(1, dtype=torch.uint8, device=dev), []))
        else:
            img, offs = self._resize_packed(sources[:B], hw, dev, align=4 if self.mix else 1, views=views if windowed else None)
            bg, bg_offs = (self._resize_packed(sources[B:], [hw[i] for i in with_bg], dev)
                           if with_bg else (torch.zeros(1, dtype=torch.uint8, device=dev), []))
        bg_off = dict(zip(with_bg, bg_offs))
        affine = any(s.get("affine") for s in planned)
        if affine and windowed:
            raise ValueError("a batch with affine entries and windows (RandomCrop / Expand / MinIoURandomCrop)")
        entries = [_block_list(s) for s in planned]
        if any(entries):
            # (warps and holes in the order each sample's block ran them)
            img = self._warp_packed(img, entries, offs, hw, dev)
        # Pad(size=): the assigner sees the padded sample -- its masks / maps zero-padded to the fixed size, its points those
        # of that size, which are the head's for every sample of the batch whatever scale was drawn (with Pad(size_divisor=)
        # the points follow img_shape as in the reference)
        ahw = [tuple(s["pad_shape"][:2]) if s.get("pad_fixed_size") is not None else hw[i] for i, s in enumerate(planned)]
        masks, flipped_masks = self._affine_masks(planned, hw, dev, ahw) if affine else self._masks(planned, hw, dev, ahw)

        P = np.zeros((B, K.AUG_PARAM_INTS), np.int32)
        for i, s in enumerate(planned):
            fl = 0
            cfg = s["img_norm_cfg"]
            if cfg["to_rgb"]:
                fl |= F_TO_RGB
            if s.get("flip"):
                fl |= F_FLIP
            P[i, 0], (P[i, 1], P[i, 2]) = offs[i], hw[i]
            if i in bg_off:
                fl |= F_MERGE
                P[i, 4] = bg_off[i]
                m = masks[i]
                P[i, 5] = 0 if m is None else m.shape[0]
                if m is not None and m.shape[0]:
                    addr = m.data_ptr()
                    P[i, 6], P[i, 7] = np.array([addr & 0xFFFFFFFF, addr >> 32], np.uint32).view(np.int32)
                    if tuple(m.shape[1:]) != hw[i]:        # (the assigner's padded masks: the mask pitch word)
                        P[i, 15] = m.shape[1] << 16 | m.shape[2]
            if "aug_blur" in s:
                fl |= F_BLUR
                r, ww, fw = blur_params(s["aug_blur"])
                P[i, 8], P[i, 9], P[i, 10] = r, ww, fw
            for key, flag, col in (("aug_sharpness", F_SHARP, 11), ("aug_contrast", F_CONTRAST, 12),
                                   ("aug_brightness", F_BRIGHT, 13), ("aug_color", F_COLOR, 14)):
                if key in s:
                    fl |= flag
                    P[i, col] = _f32_bits(s[key])
            P[i, 3] = fl
        cfg0 = planned[0]["img_norm_cfg"]
        for s in planned[1:]:
            c = s["img_norm_cfg"]
            if not (np.array_equal(c["mean"], cfg0["mean"]) and np.array_equal(c["std"], cfg0["std"])):
                raise ValueError("one batch, one Normalize")
        params = torch.from_numpy(P).to(dev)
        Hp = max(s["pad_shape"][0] for s in planned)
        Wp = max(s["pad_shape"][1] for s in planned)
        max_h, max_w = max(h for h, _ in hw), max(w for _, w in hw)
        if any(s["pad_shape"][0] < h or s["pad_shape"][1] < w for s, (h, w) in zip(planned, hw)):
            raise ValueError("pad_shape smaller than the image")
        t1, t2 = torch.empty_like(img), torch.empty_like(img)
        lsum = torch.empty(B, dtype=torch.int64, device=dev)
        out = torch.empty(B, 3, Hp, Wp, dtype=torch.float32, device=dev)
        mean = cfg0["mean"].astype(np.float64).astype(np.float32)
        stdinv = (1.0 / cfg0["std"].astype(np.float64)).astype(np.float32)
        if self.mix:
            # merge (no Pillow stages in a mix pipeline) -> HSV + noise -> box -> flip / BGR->RGB / Normalize / pad
            params2 = torch.from_numpy(self._params2(planned, offs, hw)).to(dev)
            K.augment_merge_hblur(img, bg, params, t1, B, max_h, max_w)
            K.augment_hsv_noise(t1, params2, t2, B, max(h * w for h, w in hw))
            K.augment_box(t2, params2, t1, B, max_h, max_w)
            K.augment_finish(t1, lsum, params, out, B, Hp, Wp, mean, stdinv)
        else:
            K.augment_merge_hblur(img, bg, params, t1, B, max_h, max_w)
            K.augment_vblur(t1, params, t2, B, max_h, max_w)
            K.augment_sharp(t2, params, t1, lsum, B, max_h * max_w)
            K.augment_finish(t1, lsum, params, out, B, Hp, Wp, mean, stdinv)
        if any("cutout_late" in s for s in planned):
            self._cutout_late(out, planned, hw, dev, mean, stdinv)

        p2g = pw = None
        if self.assigner is not None:
            p2g, pw = [None] * B, [None] * B
            # (t1 / lsum / params: what augment_finish has just read -- the augmented u8 image exists nowhere else)
            maps = flipped_masks if self.mask_free is None else self._distance_maps(planned, ahw, t1, lsum, params, dev)
            for shape in sorted(set(ahw)):
                idx = [i for i in range(B) if ahw[i] == shape]
                a, b = self.assigner.assign_batch([planned[i]["gt_bboxes"] for i in idx], [maps[i] for i in idx], shape,
                                                  rngs=[planned[i]["_nprnd"] for i in idx], device=dev)
                for j, i in enumerate(idx):
                    p2g[i], pw[i] = a[j], b[j]
        return self._collect(planned, out, p2g, pw, collate)

    def run_frames(self, planned):
        """a frame pipeline's collated batch together with what its frames are read from, for a caller that reads them again
        (the RoI crops of the batch's detections): -> (batch, (descriptor table i32 [B, PREP_DESC_INTS], frames)).  The table
        is a view of the upload buffer and keeps it alive; the crops are cut later, possibly on another stream, so the caller
        holds both until then."""
        if not self.frames:
            raise ValueError("run_frames: not a pipeline that starts from frames in memory")
        return self._run_frames(planned, True)

    def run_tile_rows(self, frames, spec):
        """Tiled inference (ops/tiles.py; spec: ops.tiles.TileSpec or apis.set_tiling's dict): the rows of a batch of frames --
        image-major, per frame its full-frame row (spec.full_frame), then its tiles in plan order -- each planned by this
        pipeline as if its source rectangle were a frame of its own (Resize to the single img_scale, Normalize, Pad: its own
        img_shape, scale_factor and pad_shape), all written into ONE tensor [R, 3, Hp, Wp] at the largest pad_shape among
        them by ONE upload (upload_tile_rows: every host frame once) and ONE radet_preprocess_frames launch.  Row r's slice
        holds the bits the single-view pipeline writes for a copy of frame[y0:y0 + th, x0:x0 + tw].  Nothing waits for the
        device.  -> dict(img f32 [R, 3, Hp, Wp], img_metas [R], rects i32 [R, 4], edges i32 [R], row_start i32 [B + 1],
        table i32 [B + R, PREP_DESC_INTS] (its first B rows: the source frames, what crops= reads), frames, and the spec's
        edge_margin, batch, nms_pre) -- the plan DetectorRuntime.detect_tiles takes."""
        import random
        from ..ops.tiles import tile_rows, tiling_spec
        spec = tiling_spec(spec)
        if not self.frames or self.views != 1:
            raise NotImplementedError("tiled inference runs a single-view pipeline that starts from frames in memory "
                                      "(LoadImageFromWebcam, one img_scale, flip=False); drop the extra views or the tiling")
        dev = self._dev()
        frames = [f.numpy() if isinstance(f, torch.Tensor) and not f.is_cuda and f.dtype == torch.uint8 else f
                  for f in frames]                                  # (a host tensor is a host frame)
        for f in frames:
            if not isinstance(f, (np.ndarray, torch.Tensor)) or len(f.shape) != 3 or f.shape[2] != 3 or 0 in f.shape:
                raise ValueError("tiled inference takes loaded frames: ndarrays or device tensors HxWx3 uint8 (BGR)")
            if isinstance(f, torch.Tensor) and f.device != dev:
                raise ValueError(f"a frame on {f.device} in a batch prepared on {dev}")
        rects, edges, row_start = tile_rows([f.shape[:2] for f in frames], spec)
        R = len(rects)
        if R > 65535:
            raise NotImplementedError(f"a tiled batch of {R} rows: one radet_preprocess_frames launch takes at most 65535; pass "
                                      "fewer frames per batch")
        planned = []
        for b, f in enumerate(frames):
            for r in range(int(row_start[b]), int(row_start[b + 1])):
                x0, y0, tw, th = (int(v) for v in rects[r])
                planned.append(self.plan(dict(img=f[y0:y0 + th, x0:x0 + tw], bbox_fields=[], mask_fields=[], seg_fields=[]),
                                         random, np.random))      # (a view: planning reads its shape, never its pixels)
        if not planned:
            raise ValueError("tiled inference on an empty batch of frames")
        hw = [tuple(int(v) for v in s.get("resize_hw", s["img"].shape[:2])) for s in planned]
        cfg0 = planned[0]["img_norm_cfg"]
        if any(s.get("flip") for s in planned):
            raise ValueError("a single-view pipeline that starts with LoadImageFromWebcam does not flip")
        if any(s["pad_shape"][0] < h or s["pad_shape"][1] < w for s, (h, w) in zip(planned, hw)):
            raise ValueError("pad_shape smaller than the image")
        B = len(frames)
        table = upload_tile_rows(frames, rects, row_start, hw, cfg0["to_rgb"], dev)
        mean = cfg0["mean"].astype(np.float64).astype(np.float32)
        stdinv = (1.0 / cfg0["std"].astype(np.float64)).astype(np.float32)
        Hp = max(s["pad_shape"][0] for s in planned)
        Wp = max(s["pad_shape"][1] for s in planned)
        out = torch.empty(R, 3, Hp, Wp, dtype=torch.float32, device=dev)
        K.preprocess_frames(table[B:], R, Hp, Wp, mean, stdinv, out)
        metas = [{k: s[k] for k in s["_collect"].meta_keys if k in s} for s in planned]
        return dict(img=out, img_metas=metas, rects=rects, edges=edges, row_start=row_start, table=table, frames=frames,
                    edge_margin=spec.edge_margin, batch=spec.batch, nms_pre=spec.nms_pre)

    def _run_frames(self, planned, collate):
        """device part of a batch of planned frames (LoadImageFromWebcam): the descriptor table and the host frames go up
        in ONE pinned, non-blocking copy -- frames that are device tensors are not copied at all, the table holds their
        addresses -- and ONE radet_preprocess_frames launch writes the batch; no packed temporaries.  Device frames must be
        ready on the current stream; nothing here waits for the device.  Returns (what run() returns, (descriptor table,
        frames)) -- see run_frames.
        Several views (MultiScaleFlipAug with flips / scales): still ONE upload -- the table of all V * B rows, view-major,
        and every host frame once: the rows of a frame's views name the same address -- and one launch per distinct scale,
        which writes that scale's unflipped and flipped views together, [F * B, 3, Hp, Wp] with the views as slices.
        Collated: dict(img=[V tensors], img_metas=[V lists]), as the reference collates a test-time-augmentation batch.
        The table's first B rows describe the source frames (view 0's rows)."""
        dev = self._dev()
        B = len(planned)
        frames = [s["img"] for s in planned]
        for f in frames:
            if isinstance(f, torch.Tensor) and f.device != dev:
                raise ValueError(f"a frame on {f.device} in a batch prepared on {dev}")
        V = self.views
        views = [[s["_views"][v] for s in planned] for v in range(V)] if V > 1 else [planned]
        every = [s for view in views for s in view]               # view-major: row v * B + b
        hw = [tuple(int(v) for v in s.get("resize_hw", s["img"].shape[:2])) for s in every]
        cfg0 = planned[0]["img_norm_cfg"]
        for s in every[1:]:
            c = s["img_norm_cfg"]
            if not (np.array_equal(c["mean"], cfg0["mean"]) and np.array_equal(c["std"], cfg0["std"]) and c["to_rgb"] == cfg0["to_rgb"]):
                raise ValueError("one batch, one Normalize")
        if V == 1 and any(s.get("flip") for s in planned):
            raise ValueError("a single-view pipeline that starts with LoadImageFromWebcam does not flip")
        if any(s["pad_shape"][0] < h or s["pad_shape"][1] < w for s, (h, w) in zip(every, hw)):
            raise ValueError("pad_shape smaller than the image")
        flips = [K.PREP_FLIP[s["flip_direction"]] if s.get("flip") else 0 for s in every]
        table = upload_frames(frames, hw, cfg0["to_rgb"], dev, views=V, flips=flips)
        mean = cfg0["mean"].astype(np.float64).astype(np.float32)
        stdinv = (1.0 / cfg0["std"].astype(np.float64)).astype(np.float32)
        if V == 1:
            Hp = max(s["pad_shape"][0] for s in planned)
            Wp = max(s["pad_shape"][1] for s in planned)
            out = torch.empty(B, 3, Hp, Wp, dtype=torch.float32, device=dev)
            K.preprocess_frames(table, B, Hp, Wp, mean, stdinv, out)
            return self._collect(planned, out, None, None, collate), (table, frames)
        # one launch per scale: the views of a scale are consecutive (MultiScaleFlipAug's order), hence consecutive rows
        outs, v0 = [], 0
        while v0 < V:
            v1 = v0 + 1
            while v1 < V and planned[0]["_views"][v1]["scale"] == planned[0]["_views"][v0]["scale"]:
                v1 += 1
            group = [s for view in views[v0:v1] for s in view]
            Hp = max(s["pad_shape"][0] for s in group)
            Wp = max(s["pad_shape"][1] for s in group)
            out = torch.empty(len(group), 3, Hp, Wp, dtype=torch.float32, device=dev)
            K.preprocess_frames(table[v0 * B * K.PREP_DESC_INTS:], len(group), Hp, Wp, mean, stdinv, out)
            outs += [out[(v - v0) * B:(v - v0 + 1) * B] for v in range(v0, v1)]
            v0 = v1
        if not collate:
            per_view = [self._collect(view, out, None, None, False) for view, out in zip(views, outs)]
            samples = [{k: [d[b][k][0] for d in per_view] for k in per_view[0][b]} for b in range(B)]
            return samples, (table, frames)
        metas = [[{k: s[k] for k in s["_collect"].meta_keys if k in s} for s in view] for view in views]
        return dict(img=outs, img_metas=metas), (table, frames)

    def _distance_maps(self, planned, hw, img, lsum, params, dev):
        """The mask-free sampler's maps of a batch, f32 [G_i, h, w] per sample: every box's padded crop cut from the
        augmented image (one launch), the GDT / MBD chain over all crops (ops.*_box2distance.packed_maps), one paste launch
        per image size.  All descriptors come from the planned box geometry; nothing is read back from the device.
        hw: the size the maps are pasted into (the image's, or the fixed pad size: zeros outside the image)"""
        from ..ops import _Packed, _upload
        boxes = [(i, k) for i, s in enumerate(planned) for k in range(len(s["_crop_plan"][0].corners))]
        maps = [torch.zeros(0, *hw[i], dtype=torch.float32, device=dev) for i in range(len(planned))]
        if not boxes:
            return maps
        # canvases only for the boxes that are transformed (a box below small_object_size pastes ones)
        large = [n for n, (i, k) in enumerate(boxes) if planned[i]["_crop_plan"][0].large[k]]
        D = np.zeros((len(large), K.CROP_DESC_INTS), np.int32)
        sizes, o = [], 0
        for row, n in zip(D, large):
            i, k = boxes[n]
            g, fill = planned[i]["_crop_plan"]
            (cw, ch), b = g.canvas_wh[k], fill[k].astype(np.int64)
            if cw < 2 or ch < 2:
                raise ValueError(f"a gt box of sample {i} truncates to a canvas of {ch} x {cw} pixels (the transforms need 2 x 2)")
            row[:] = [i, *g.win_lo[k], cw, ch, *g.src_lo[k], *g.src_hi[k], b[0] | b[1] << 8 | b[2] << 16, o, 0]
            sizes.append((int(ch), int(cw)))
            o += int(cw) * int(ch)
        where = {}
        if large:
            canvases = torch.empty(o * 3, dtype=torch.uint8, device=dev)
            K.crop_canvases(img, lsum, params, len(planned), _upload(D, dev), len(large), max(h * w for h, w in sizes), canvases)
            dmaps, _ = self.mask_free.distance_transform.packed_maps(_Packed(canvases, sizes, 3), [True] * len(large))
            where = dict(zip(large, zip(dmaps.offs, dmaps.hw)))
        for shape in sorted(set(hw)):
            rows = [n for n, (i, k) in enumerate(boxes) if hw[i] == shape]
            if not rows:
                continue
            P = np.zeros((len(rows), K.PASTE_DESC_INTS), np.int32)
            for prow, n in zip(P, rows):
                i, k = boxes[n]
                g = planned[i]["_crop_plan"][0]
                off, (mh, mw) = where.get(n, (0, (0, 0)))
                prow[:] = [off, mh, mw, g.regions[k, 0], g.regions[k, 1], *g.corners[k], n in where]
            pasted = torch.empty(len(rows), *shape, dtype=torch.float32, device=dev)
            K.paste_maps(dmaps.data if large else pasted, _upload(P, dev), len(rows), shape[0], shape[1], pasted)
            o = 0
            for i in range(len(planned)):
                if hw[i] == shape:
                    c = len(planned[i]["_crop_plan"][0].corners)
                    maps[i] = pasted[o:o + c]
                    o += c
        return maps

    @staticmethod
    def _params2(planned, offs, hw):
        """the params2 rows of the mix stages (include/radet_hip.h, AUG2_PARAM_INTS)"""
        P = np.zeros((len(planned), K.AUG2_PARAM_INTS), np.int32)
        for i, s in enumerate(planned):
            fl = 0
            P[i, 0], (P[i, 1], P[i, 2]) = offs[i], hw[i]
            if "aug_hsv" in s:
                fl |= F2_HSV
                a, b, c = s["aug_hsv"]
                P[i, 4:7] = [_f32_bits(a), _f32_bits(b), _f32_bits(c)]
                P[i, 7] = int(a < 1) | int(b < 1) << 1 | int(c < 1) << 2        # (the double factor, as the reference tests it)
            if "aug_noise" in s:
                fl |= F2_NOISE
                sigma, key = s["aug_noise"]
                P[i, 8:10] = np.array([sigma], np.float64).view(np.int32)
                P[i, 10:14] = np.asarray(key, np.uint64).reshape(2).view(np.int32)
            if "aug_smooth" in s:
                fl |= F2_BOX
                P[i, 14] = s["aug_smooth"]
            P[i, 3] = fl
        return P

    def _masks(self, planned, hw, dev, ahw=None):
        """Normalised (mask / max), nearest-resized instance masks per sample.  The second list (the assigner's masks: flipped
        with the sample, zero-padded to ahw, which is hw without Pad(size=)) comes straight from the source masks, per group
        of equal source and assigner sizes, with one view row per mask (sample_view over the mask's own size) -- one launch
        whatever scales and windows the samples drew: radet_mask_max + radet_mask_transform for bitmaps, radet_rle_masks
        for run lists.  The first list (the merge's masks: unflipped; read for samples with a background) is the same
        output for an unflipped sample; when a merged sample is flipped, bitmaps take a second pass over the stack, and the
        run-list launch writes both orientations of every flipped mask anyway.  A flipped sample whose group took no second
        pass has no entry there.  These masks have the assigner's size: for a sample smaller than the pad the merge reads
        their top-left corner (the mask pitch word of its params row).  Nothing waits for the device."""
        masks, flipped = [None] * len(planned), [None] * len(planned)
        for kind, src_hw, out_hw, idx, counts in self._mask_groups(planned, hw if ahw is None else ahw):
            G = sum(counts)
            flips = np.repeat([bool(planned[i].get("flip")) for i in idx], counts)
            rows = np.repeat(np.array([sample_view(planned[i], src_hw) for i in idx], np.int32).reshape(-1, K.VIEW_INTS), counts, axis=0)
            if not G:
                out = plain = torch.zeros(0, *out_hw, dtype=torch.uint8, device=dev)
            elif kind == "bitmap":
                both = any(planned[i].get("flip") and "background" in planned[i] for i in idx)
                src = torch.from_numpy(np.concatenate([planned[i]["gt_masks"] for i in idx])).to(dev)
                flipped_rows = rows.copy()
                flipped_rows[:, 10] = flips
                rows = torch.from_numpy(np.concatenate([flipped_rows] + ([rows] if both else []))).to(dev)
                mx = K.mask_max(src)
                out = K.mask_transform(src, out_hw, views=rows[:G], norm_max=mx)
                plain = K.mask_transform(src, out_hw, views=rows[G:], norm_max=mx) if both else None
            else:
                *runs, rows = self._upload_runs(planned, idx, src_hw, flips, dev, rows)
                res = K.rle_masks(*runs, out_hw, with_plain=bool(flips.any()), views=rows)
                out, plain = res if flips.any() else (res, None)
            o = 0
            for i, c in zip(idx, counts):
                flipped[i] = out[o:o + c]
                if not (planned[i].get("flip") and c):
                    masks[i] = flipped[i]
                elif plain is not None:
                    masks[i] = plain[o:o + c]
                o += c
        return masks, flipped

    def _collect(self, planned, out, p2g, pw, collate):
        samples = []
        for i, s in enumerate(planned):
            col = s["_collect"]
            h, w = s["pad_shape"][:2]
            d = {}
            for key in col.keys:
                if key == "img":
                    d["img"] = out[i, :, :h, :w]
                elif key == "points_to_gt_index":
                    d[key] = p2g[i]
                elif key == "points_weight":
                    d[key] = pw[i]
                else:
                    d[key] = torch.from_numpy(np.asarray(s[key]))
            d["img_metas"] = {k: s[k] for k in col.meta_keys if k in s}
            if s.get("_tta"):
                d = {k: [v] for k, v in d.items()}
            samples.append(d)
        if not collate:
            return samples
        keys = planned[0]["_collect"].keys
        if self.tta:
            return dict(img=[out], img_metas=[[d["img_metas"][0] for d in samples]])
        batch = {k: [d[k] for d in samples] for k in keys if k != "img"}
        batch["img"] = out
        batch["img_metas"] = [d["img_metas"] for d in samples]
        return batch
