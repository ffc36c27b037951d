"""NumPy restatement of the image side of the BOP training pipeline: the five CosyPose Pillow stages (pinned bit for bit
to live Pillow by tests/test_augment_cpu.py), the RandomBackground merge and mmcv's imnormalize.  Images are u8 HWC; the
Pillow ops take RGB like Pillow, the merge and Normalize take BGR like the reference's cv2 side."""
import math

import numpy as np

f32 = np.float32


def blur_params(k):
    """ImagingGaussianBlur's box radius for GaussianBlur(k), 3 passes (float32 C arithmetic; the sqrt / floor in double),
    and ImagingHorizontalBoxBlur's fixed-point weights: (int radius, ww, fw)"""
    sigma2 = f32(f32(k) * f32(k)) / f32(3)
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(l * f32(l + f32(1)) - f32(3) * sigma2))
    a = f32(a / f32(f32(6) * f32(sigma2 - f32(l + f32(1)) * f32(l + f32(1)))))
    fr = f32(l + a)
    r = int(fr)
    ww = int(f32(1 << 24) / f32(fr * f32(2) + f32(1)))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def _box_pass(x, r, ww, fw, axis):
    """one box pass along `axis`: clamped window sum * ww + both far neighbours * fw, rounded, >> 24"""
    n = x.shape[axis]
    idx = np.arange(n)
    xi = x.astype(np.uint64)
    s = sum(np.take(xi, np.clip(idx + k, 0, n - 1), axis=axis) for k in range(-r, r + 1))
    far = np.take(xi, np.clip(idx - r - 1, 0, n - 1), axis=axis) + np.take(xi, np.clip(idx + r + 1, 0, n - 1), axis=axis)
    return (((s * ww + far * fw + (1 << 23)) & 0xFFFFFFFF) >> 24).astype(np.uint8)


def hblur(img, k):
    r, ww, fw = blur_params(k)
    for _ in range(3):
        img = _box_pass(img, r, ww, fw, 1)
    return img


def vblur(img, k):
    r, ww, fw = blur_params(k)
    for _ in range(3):
        img = _box_pass(img, r, ww, fw, 0)
    return img


def gaussian_blur(img, k):
    """ImageFilter.GaussianBlur(k): all rows first, then all columns"""
    return vblur(hblur(img, k), k)


def blend(in1, in2, alpha):
    """Image.blend(in1, in2, alpha): in1 + alpha * (in2 - in1) in float32, truncated; clipped when alpha is outside [0, 1]"""
    a = f32(alpha)
    t = np.asarray(in1).astype(f32) + a * (np.asarray(in2).astype(np.int32) - np.asarray(in1).astype(np.int32)).astype(f32)
    if 0 <= a <= 1:
        return t.astype(np.uint8)
    return np.clip(t, 0, 255).astype(np.uint8)          # (truncation of the clipped float)


def luma(rgb):
    """convert("L") of RGB bytes"""
    c = rgb.astype(np.int64)
    return ((c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def smooth(img):
    """ImageFilter.SMOOTH (3x3, 1 1 1 / 1 5 1 / 1 1 1, /13): float32 sums in Filter.c's order, border pixels copied"""
    h, w = img.shape[:2]
    if h < 3 or w < 3:
        return img.copy()
    k1, k5 = f32(1.0 / 13.0), f32(5.0 / 13.0)
    x = img.astype(f32)

    def row(rr, kc):
        return (rr[:, :-2] * k1 + rr[:, 1:-1] * kc) + rr[:, 2:] * k1

    ss = f32(0) + row(x[2:], k1)                         # Pillow's in1 (row y + 1) first
    ss = ss + row(x[1:-1], k5)
    ss = ss + row(x[:-2], k1)
    c = np.where(ss <= 0, 0, np.where(ss >= 255, 255, np.floor(ss.astype(np.float64) + 0.5))).astype(np.uint8)
    out = img.copy()
    out[1:-1, 1:-1] = c
    return out


def sharpness(img, f):
    return blend(smooth(img), img, f)


def contrast(img, f):
    l = luma(img).astype(np.int64)
    mean = int(float(l.sum()) / l.size + 0.5)
    return blend(np.full_like(img, mean), img, f)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def color(img, f):
    return blend(np.repeat(luma(img)[..., None], 3, axis=2), img, f)


def merge_background(img, bg_resized, masks):
    """RandomBackground.merge_background_by_mask: the background where no instance mask equals 1 (BGR in, BGR out)"""
    fg = (np.asarray(masks).reshape(-1, *img.shape[:2]) == 1).any(axis=0)
    return np.where(fg[..., None], img, bg_resized)


def normalize(img_bgr, mean, std, to_rgb=True):
    """mmcv.imnormalize: float32 (x - mean) * (1 / std) after BGR -> RGB, -> CHW"""
    x = img_bgr[..., ::-1] if to_rgb else img_bgr
    m = np.asarray(mean, np.float32).astype(np.float64).astype(f32)
    s = (1.0 / np.asarray(std, np.float32).astype(np.float64)).astype(f32)
    return ((x.astype(f32) - m) * s).transpose(2, 0, 1).copy()


def cosypose(img_rgb, blur_k=None, sharp=None, contr=None, bright=None, col=None):
    """the CosyPoseAug chain on an RGB image; None = stage skipped"""
    x = img_rgb
    if blur_k is not None:
        x = gaussian_blur(x, blur_k)
    if sharp is not None:
        x = sharpness(x, sharp)
    if contr is not None:
        x = contrast(x, contr)
    if bright is not None:
        x = brightness(x, bright)
    if col is not None:
        x = color(x, col)
    return x


def resize_linear_u8(img, w, h):
    """cv2.resize(img, (w, h)) INTER_LINEAR for u8 HWC: the restatement the project's resize kernel is pinned to"""
    from oracle import imgproc
    return imgproc.resize_linear_u8(img, (w, h))
