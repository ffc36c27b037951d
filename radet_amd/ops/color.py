"""mmcv's photometric image functions on the device (radet_amd/csrc/color.hip): `adjust_brightness`, `adjust_contrast`,
`adjust_color` and `imequalize` on u8 BGR images, out of place, through the two launches the image pipeline's colour stages
use (radet_color_stats_u8 for the histograms Contrast and Equalize need, radet_color_apply_u8).  An image is an H x W x 3 u8
ndarray or device tensor; a list of them (of any, mixed sizes) is one packed batch: one launch pair for the whole list.  The
result has the input's kind: ndarray, device tensor, or a list of them.

The pixel rules are this project's restatement of mmcv 1.3.18 on OpenCV 4 (include/radet_hip.h, "AutoAugment's colour
stages"): parity with mmcv's pixels is unpinned, the rules are pinned bit for bit to tests/_color_ref.py."""
import numbers

import numpy as np
import torch

from .. import kernels as K


def _packed(images):
    """a list of H x W x 3 u8 images -> (packed device buffer (a copy), pixel offsets, sizes)"""
    from . import _dev
    dev = _dev()
    ts = []
    for im in images:
        t = torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"an image is an H x W x 3 uint8 ndarray or device tensor, got {type(im).__name__} "
                             f"{getattr(im, 'dtype', '')} {tuple(getattr(im, 'shape', ()))}")
        if max(t.shape[:2]) > K.AUG_MAX_W:
            raise ValueError(f"image of {t.shape[0]} x {t.shape[1]}: the colour kernels take sides up to {K.AUG_MAX_W}")
        ts.append(t.to(dev))
    hw = [(int(t.shape[0]), int(t.shape[1])) for t in ts]
    offs = [int(v) for v in np.cumsum([0] + [h * w for h, w in hw])[:-1]]
    if sum(h * w for h, w in hw) >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 pixels in one call")
    buf = torch.cat([t.reshape(-1) for t in ts]) if len(ts) > 1 else ts[0].reshape(-1).clone()
    return buf, offs, hw


def _apply(img, kind, factor=1.0):
    single = not isinstance(img, (list, tuple))
    images = [img] if single else list(img)
    if not images:
        return []
    buf, offs, hw = _packed(images)
    n, max_px = len(images), max(h * w for h, w in hw)
    if max_px:
        D = np.zeros((n, K.COLOR_DESC_INTS), np.int32)
        for d, o, (h, w) in zip(D, offs, hw):
            K.color_desc_row(d, o, h, w, kind, factor)
        desc = torch.from_numpy(D).to(buf.device)
        hist = None
        if kind in K.COLOR_STATS_KINDS:
            hist = torch.empty((n, 4, 256), dtype=torch.int32, device=buf.device)
            K.fill_zero(hist)
            K.color_stats_u8(buf, desc, hist, n, max_px)
        K.color_apply_u8(buf, desc, hist, n, max_px)
    out = [buf[3 * o:3 * (o + h * w)].view(h, w, 3) for o, (h, w) in zip(offs, hw)]
    out = [t.cpu().numpy() if isinstance(im, np.ndarray) else t for t, im in zip(out, images)]
    return out[0] if single else out


def _factor(name, factor):
    if isinstance(factor, bool) or not isinstance(factor, numbers.Real) or not np.isfinite(factor):
        raise ValueError(f"{name}: the factor is a finite number, got {factor!r}")
    return float(factor)


def adjust_brightness(img, factor=1.0):
    """mmcv.adjust_brightness: img * factor + black * (1 - factor) in fp32, clipped, truncated"""
    return _apply(img, "brightness", _factor("adjust_brightness", factor))


def adjust_contrast(img, factor=1.0):
    """mmcv.adjust_contrast: img * factor + round(mean of the gray image) * (1 - factor) in fp32, clipped, truncated"""
    return _apply(img, "contrast", _factor("adjust_contrast", factor))


def adjust_color(img, alpha=1.0):
    """mmcv.adjust_color(img, alpha) with its defaults beta = 1 - alpha, gamma = 0 (beta / gamma are not offered): every pixel
    blended with its gray value, rounded half to even, saturated"""
    return _apply(img, "color", _factor("adjust_color", alpha))


def imequalize(img):
    """mmcv.imequalize: every channel mapped through the lookup table of its own histogram"""
    return _apply(img, "equalize")
