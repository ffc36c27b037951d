"""Detections drawn on frames on the device (radet_amd/csrc/draw.hip, one launch): box outlines and "name|score" labels.
`draw_detections` is the stand-alone entry point; `apis.draw_frames` runs the same launch behind `detect_frames`, and
`core.visualization.imshow_det_bboxes` / `RADet.show_result` carry the reference's names.

The pixel rules are this project's own (include/radet_hip.h, radet_draw_detections; the reference draws with matplotlib),
pinned bit for bit to the NumPy restatement tests/_draw_ref.py.  The glyphs come from an atlas that Pillow renders once per
(class names, font size, font) on the host; the kernel only ever sees coverage bytes."""
import numbers
from collections import namedtuple

import numpy as np
import torch

from .. import kernels as K
from .crops import check_frames, frame_table

# mmcv.color_val's eight names, BGR
COLORS = dict(red=(0, 0, 255), green=(0, 255, 0), blue=(255, 0, 0), cyan=(255, 255, 0), yellow=(0, 255, 255),
              magenta=(255, 0, 255), white=(255, 255, 255), black=(0, 0, 0))

Atlas = namedtuple("Atlas", "coverage widths")
Atlas.__doc__ = """coverage u8 [S, Hc, Wa]: strip s is coverage[s, :, :widths[s]]; widths i32 [S].  Strips 0-9: the digits, 10 '.',
11 '|', 12 'class ', 13 + c: the name of class c -- all on one baseline at one height Hc."""

DrawSpec = namedtuple("DrawSpec", "thickness colour text_colour a_bg score_thr max_dets pad n_names")
DrawSpec.__doc__ = """the checked style of a draw request: colour = b | g << 8 | r << 16, or None for the per-class palette"""

_GLYPHS = [str(d) for d in range(10)] + [".", "|", "class "]


def color_val(color):
    """a colour as (b, g, r) ints: one of mmcv's eight names or three ints in [0, 255]; everything else is refused"""
    if isinstance(color, str):
        if color not in COLORS:
            raise ValueError(f"colour {color!r}: expected one of {sorted(COLORS)} or three ints in [0, 255] (BGR)")
        return COLORS[color]
    c = tuple(color) if isinstance(color, (tuple, list, np.ndarray)) else None
    if c is None or len(c) != 3 or not all(isinstance(v, numbers.Integral) and not isinstance(v, bool) and 0 <= v <= 255 for v in c):
        raise ValueError(f"colour {color!r}: expected one of {sorted(COLORS)} or three ints in [0, 255] (BGR)")
    return tuple(int(v) for v in c)


def _word(bgr):
    return bgr[0] | bgr[1] << 8 | bgr[2] << 16


def class_palette(n):
    """u8 [n, 3]: the reference's per-class colours (radet/core/visualization/image.py:97-101: seed 42, one randint(0, 256,
    (1, 3), dtype=uint8) per class) from a local RandomState, so the global generator is untouched"""
    rs = np.random.RandomState(42)
    return np.concatenate([rs.randint(0, 256, (1, 3), dtype=np.uint8) for _ in range(int(n))] or [np.zeros((0, 3), np.uint8)])


_ATLASES = {}


def _load_font(font, font_size):
    from PIL import ImageFont
    if font is None:
        try:
            return ImageFont.load_default(size=font_size)          # (the scalable default: needs FreeType)
        except (TypeError, OSError, ImportError):
            return ImageFont.load_default()                          # (the bitmap default)
    if isinstance(font, (str, bytes)) or hasattr(font, "__fspath__"):
        return ImageFont.truetype(font, font_size)
    return font


def build_atlas(class_names, font_size, font=None):
    """The glyph atlas of a label style, rendered once per (names, size, font) with Pillow on the host and cached: the strips
    '0'-'9', '.', '|', 'class ', then one per class name, all drawn on one baseline into one height Hc.  font: a Pillow font
    or a path; default ImageFont.load_default(size=font_size) where FreeType is there, else the bitmap default."""
    names = tuple(str(c) for c in (class_names or ()))
    if not isinstance(font_size, numbers.Integral) or isinstance(font_size, bool) or font_size < 1:
        raise ValueError(f"font_size={font_size!r}")
    hashable = font is None or isinstance(font, (str, bytes))
    key = (names, int(font_size), font if hashable else id(font))
    if key in _ATLASES:
        return _ATLASES[key]
    from PIL import Image, ImageDraw
    f = _load_font(font, int(font_size))
    strips = _GLYPHS + list(names)
    boxes = [f.getbbox(s) if s else (0, 0, 0, 0) for s in strips]    # (left, top, right, bottom) from the drawing origin
    top = min([b[1] for b in boxes] + [0])
    Hc = max(max(b[3] for b in boxes) - top, 1)
    adv = [max(int(np.ceil(f.getlength(s))) if s else 0, b[2]) for s, b in zip(strips, boxes)]
    Wa = max(adv + [1])
    cov = np.zeros((len(strips), Hc, Wa), np.uint8)
    for i, s in enumerate(strips):
        if adv[i] > 0:
            im = Image.new("L", (Wa, Hc), 0)
            ImageDraw.Draw(im).text((0, -top), s, fill=255, font=f)
            cov[i] = np.asarray(im)
            cov[i, :, adv[i]:] = 0
    atlas = Atlas(cov, np.asarray(adv, np.int32))
    while len(_ATLASES) >= 16:
        _ATLASES.pop(next(iter(_ATLASES)))
    _ATLASES[key] = atlas
    return atlas


def text_width_bound(widths, n_names):
    """the widest text the kernel can compose from these strips"""
    w = [int(v) for v in widths]
    digit = max(w[:10])
    head = max(w[K.DRAW_STRIP_NAME0:K.DRAW_STRIP_NAME0 + n_names]) if n_names else w[K.DRAW_STRIP_CLASS] + 5 * digit
    return head + w[K.DRAW_STRIP_BAR] + 3 * digit + w[K.DRAW_STRIP_DOT]


def check_atlas(atlas, n_names):
    """-> Atlas of contiguous host arrays; refuses what the kernel would have to approximate"""
    cov, widths = np.ascontiguousarray(atlas[0]), np.ascontiguousarray(atlas[1], dtype=np.int32).reshape(-1)
    if cov.dtype != np.uint8 or cov.ndim != 3 or cov.shape[0] != widths.size or cov.shape[0] < K.DRAW_STRIP_NAME0 + n_names:
        raise ValueError(f"draw: an atlas of {cov.shape} {cov.dtype} with {widths.size} widths for {n_names} class names")
    S, Hc, Wa = cov.shape
    if not 1 <= Hc <= K.DRAW_MAX_GLYPH_H or Wa < 1 or (widths < 0).any() or (widths > Wa).any():
        raise ValueError(f"draw: glyphs {Hc} rows high (at most {K.DRAW_MAX_GLYPH_H}), widths outside [0, {Wa}]")
    if max(Wa, text_width_bound(widths, n_names)) > K.DRAW_MAX_TEXT_W:
        raise ValueError(f"draw: a text of {text_width_bound(widths, n_names)} pixels is wider than the kernel's limit "
                         f"({K.DRAW_MAX_TEXT_W})")
    return Atlas(cov, widths)


def draw_spec(class_names=None, score_thr=0.3, bbox_color="green", text_color="green", thickness=2, font_size=13,
              label_alpha=0.8, max_dets=None):
    """the checked style (nothing is approximated: what the kernel does not do is refused)"""
    def _int(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool)
    if not _int(thickness) or thickness < 1 or thickness > K.DRAW_MAX_THICKNESS:
        raise ValueError(f"draw: thickness={thickness!r} is not an int in [1, {K.DRAW_MAX_THICKNESS}]")
    if max_dets is not None and (not _int(max_dets) or max_dets < 0):
        raise ValueError(f"draw: max_dets={max_dets!r}")
    if max_dets is not None and max_dets > K.DRAW_MAX_DETS:
        raise ValueError(f"draw: max_dets={max_dets} exceeds the kernel's {K.DRAW_MAX_DETS} detections per frame")
    if not isinstance(score_thr, numbers.Real) or np.isnan(score_thr):
        raise ValueError(f"draw: score_thr={score_thr!r}")
    if not isinstance(label_alpha, numbers.Real) or not 0 <= label_alpha <= 1:
        raise ValueError(f"draw: label_alpha={label_alpha!r} is not in [0, 1]")
    if not _int(font_size) or font_size < 0:
        raise ValueError(f"draw: font_size={font_size!r}")
    pad = 1 + int(font_size) // 8
    if pad > K.DRAW_MAX_PAD:
        raise ValueError(f"draw: font_size={font_size} is beyond the kernel's label padding ({K.DRAW_MAX_PAD})")
    colour = None if isinstance(bbox_color, str) and bbox_color == "class" else _word(color_val(bbox_color))
    n_names = 0 if class_names is None else len(class_names)
    if class_names is not None and not 1 <= n_names <= 65535 - K.DRAW_STRIP_NAME0:
        raise ValueError(f"draw: {n_names} class names")
    return DrawSpec(int(thickness), colour, _word(color_val(text_color)), int(np.floor(float(label_alpha) * 255 + 0.5)),
                    float(score_thr), K.DRAW_MAX_DETS if max_dets is None else int(max_dets), pad, n_names)


def pad_detections(dets, dev):
    """per frame (dets [k,5], labels [k]) or the padded (boxes [B,K,4], scores [B,K], labels [B,K], counts [B]) -> the padded
    four on dev: f32, f32, i64, i32"""
    if isinstance(dets, (tuple, list)) and len(dets) == 4 and torch.is_tensor(dets[0]) and dets[0].dim() == 3:
        boxes, scores, labels, counts = dets
        boxes, scores = boxes.to(dev, torch.float32).contiguous(), scores.to(dev, torch.float32).contiguous()
        labels = labels.to(dev, torch.int64).contiguous()
        counts = torch.as_tensor(counts).to(dev, torch.int32).contiguous()
        if boxes.shape[2] != 4 or tuple(scores.shape) != tuple(boxes.shape[:2]) or tuple(labels.shape) != tuple(scores.shape) or \
                counts.numel() != boxes.shape[0]:
            raise ValueError(f"draw: boxes {tuple(boxes.shape)}, scores {tuple(scores.shape)}, labels {tuple(labels.shape)}, "
                             f"counts {tuple(counts.shape)}")
        return boxes, scores, labels, counts
    per = []
    for d in dets:
        if not isinstance(d, (tuple, list)) or len(d) != 2:
            raise ValueError("draw: detections are per frame (dets [k,5], labels [k]), or the padded (boxes, scores, labels, counts)")
        b, l = torch.as_tensor(d[0]).to(dev, torch.float32).reshape(-1, 5), torch.as_tensor(d[1]).to(dev, torch.int64).reshape(-1)
        if b.shape[0] != l.shape[0]:
            raise ValueError(f"draw: {b.shape[0]} boxes with {l.shape[0]} labels")
        per.append((b, l))
    Kd = max([int(b.shape[0]) for b, _ in per] + [1])
    boxes = torch.zeros(len(per), Kd, 4, device=dev)
    scores = torch.zeros(len(per), Kd, device=dev)
    labels = torch.zeros(len(per), Kd, dtype=torch.int64, device=dev)
    for i, (b, l) in enumerate(per):
        boxes[i, :b.shape[0]], scores[i, :b.shape[0]], labels[i, :b.shape[0]] = b[:, :4], b[:, 4], l
    counts = torch.tensor([int(b.shape[0]) for b, _ in per], dtype=torch.int32).to(dev)
    return boxes, scores, labels, counts


class Painter:
    """A style on a device: the atlas and the palette are uploaded once and every call is one launch on the current stream.
    What apis.draw_frames holds across batches and draw_detections builds per call."""

    def __init__(self, dev, class_names=None, score_thr=0.3, bbox_color="green", text_color="green", thickness=2, font_size=13,
                 label_alpha=0.8, max_dets=None, atlas=None):
        self.spec = draw_spec(class_names, score_thr, bbox_color, text_color, thickness, font_size, label_alpha, max_dets)
        self.dev = dev
        self.atlas = self.widths = self.palette = None
        self.host_atlas = None
        if font_size > 0:
            names = None if class_names is None else [str(c) for c in class_names]
            self.host_atlas = check_atlas(build_atlas(names, font_size) if atlas is None else atlas, self.spec.n_names)
            self.atlas = torch.from_numpy(self.host_atlas.coverage).to(dev)
            self.widths = torch.from_numpy(self.host_atlas.widths).to(dev)
        elif atlas is not None:
            raise ValueError("draw: font_size=0 draws no labels, yet an atlas was given")
        self.host_palette = None
        if self.spec.colour is None and self.spec.n_names:
            self._palette(self.spec.n_names)

    def _palette(self, n):
        self.host_palette = class_palette(n)
        self.palette = torch.from_numpy(self.host_palette).to(self.dev)

    def launch(self, src_desc, dst_desc, B, max_h, max_w, boxes, scores, labels, counts, inplace):
        s = self.spec
        if s.colour is None and not s.n_names:
            # 'class' colours without names: the reference draws max(labels) + 1 colours; the labels are on the device
            n = min(int(labels.max().item()) + 1 if labels.numel() else 1, 100000)
            if self.palette is None or self.palette.shape[0] < n:
                self._palette(max(n, 1))
        K.draw_detections(src_desc, dst_desc, B, max_h, max_w, boxes, scores, labels, counts, s.thickness, s.colour, self.palette
                          if s.colour is None else None, s.text_colour, s.a_bg, s.score_thr, s.max_dets, s.n_names, s.pad, inplace,
                          self.atlas, self.widths)


def check_device_frames(frames, what):
    for f in frames:
        if isinstance(f, np.ndarray):
            raise ValueError(f"draw: {what} needs frames that are device tensors: a host array cannot be drawn on in place")


def draw_detections(frames, dets, class_names=None, score_thr=0.3, bbox_color="green", text_color="green", thickness=2,
                    font_size=13, label_alpha=0.8, max_dets=None, inplace=False, atlas=None):
    """Box outlines and "name|score" labels of the detections drawn on their frames, one HIP launch for the whole batch.

    frames: list of HxWx3 uint8 BGR frames, ndarrays or device tensors (views into larger tensors are read, and with inplace
    written, where they are), sizes may differ.  dets: per frame (dets f32 [k,5], labels [k]) as detect_frames(on_device=True)
    yields them, or the padded (boxes [B,K,4], scores [B,K], labels [B,K], counts [B]).
    Returns the annotated frames as device u8 [H,W,3] tensors: views of one allocation, or with inplace=True the frames
    themselves (device tensors only).
    A detection is drawn when its numbers are finite, score > score_thr (strict), its label names a class (without
    class_names: 0 <= label < 100000, shown as 'class N') and its integer box is not inverted; the first max_dets of them
    (default and limit: 256 per frame) in rank order.  bbox_color / text_color: one of mmcv's eight names or three ints (BGR);
    bbox_color='class' takes the reference's per-class palette.  The score is shown as d.dd with ties rounded UP (0.125 ->
    0.13; Python's ':.02f' rounds half to even).  font_size=0 draws no labels; atlas: an Atlas to use instead of
    build_atlas(class_names, font_size).  Every pixel rule: include/radet_hip.h, radet_draw_detections (parity with the
    reference's matplotlib rendering is unpinned)."""
    check_frames(frames)
    from . import _dev
    dev = _dev()
    if inplace:
        check_device_frames(frames, "inplace=True")
    painter = Painter(dev, class_names, score_thr, bbox_color, text_color, thickness, font_size, label_alpha, max_dets, atlas)
    boxes, scores, labels, counts = pad_detections(dets, dev)
    if boxes.shape[0] != len(frames):
        raise ValueError(f"draw: {len(frames)} frames, detections of {boxes.shape[0]}")
    return draw_batch(painter, frames, boxes, scores, labels, counts, inplace)


def draw_batch(painter, frames, boxes, scores, labels, counts, inplace):
    """one launch on the current stream -> the annotated frames (device views of one allocation, or with inplace the frames)"""
    dev = painter.dev
    B = len(frames)
    max_h, max_w = max(int(f.shape[0]) for f in frames), max(int(f.shape[1]) for f in frames)
    if inplace:
        table, keep = frame_table(frames, dev)
        painter.launch(table, table, B, max_h, max_w, boxes, scores, labels, counts, True)
        return list(frames)
    sizes = [int(f.shape[0]) * int(f.shape[1]) * 3 for f in frames]
    buf = torch.empty(max(sum(sizes), 1), dtype=torch.uint8, device=dev)
    views, o = [], 0
    for f, n in zip(frames, sizes):
        views.append(buf[o:o + n].view(int(f.shape[0]), int(f.shape[1]), 3))
        o += n
    # sources and destinations in ONE table: host frames ride up behind it in the same pinned copy
    table, keep = frame_table(list(frames) + views, dev)
    n = B * K.PREP_DESC_INTS
    painter.launch(table[:n], table[n:], B, max_h, max_w, boxes, scores, labels, counts, False)
    del keep                                                         # (uploaded sources: freed in stream order, behind the launch)
    return views
