"""What the colour-stage tests share, in NumPy and Python integers only: this project's restatement of mmcv 1.3.18's
adjust_brightness / adjust_contrast / adjust_color / imequalize on OpenCV 4 (the rules of include/radet_hip.h,
"AutoAugment's colour stages"), written in mmcv's own expression forms where those are pure NumPy (np.histogram, np.cumsum,
the LUT shift and clamp, round(sum / count)), and the packed batch the kernels are tested on.

Every fp32 product and fused multiply-add is evaluated EXACTLY, in integers, and rounded once to fp32 (nearest even): a
float64 evaluation rounds twice and can disagree with a real fma at a tie when beta is tiny."""
import functools
from fractions import Fraction

import numpy as np

KINDS = ("brightness", "contrast", "color", "equalize")


def factors(factor):
    """(alpha, beta) as np.float32: fl32(factor), fl32(1 - factor) with 1 - factor formed in double"""
    return np.float32(float(factor)), np.float32(1.0 - float(factor))


def enhance_level_to_value(level, a=1.8, b=0.1):
    return (level / 10) * a + b


def bgr2gray(img):
    """OpenCV 4's u8 BGR2GRAY: (3735 b + 19235 g + 9798 r + 16384) >> 15"""
    x = img.astype(np.int64)
    return ((3735 * x[..., 0] + 19235 * x[..., 1] + 9798 * x[..., 2] + 16384) >> 15).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- exact fp32 arithmetic
def _dyadic(v):
    """a finite float -> (n, s) with v == n / 2**s exactly"""
    fr = Fraction(float(v))
    return fr.numerator, fr.denominator.bit_length() - 1


def _round_f32(num, s):
    """fl32(num / 2**s), one rounding to nearest even -> (n, u): the fp32 value n * 2**u (u may be negative)"""
    if num == 0:
        return 0, 0
    sign, a = (-1 if num < 0 else 1), abs(num)
    e = max(a.bit_length() - 1 - s, -126)               # floor(log2 |value|), held at the smallest normal exponent
    u = e - 23                                           # the exponent of one unit in the last place
    shift = s + u                                        # value / 2**u = a / 2**shift
    if shift <= 0:
        n = a << -shift
    else:
        n, rem = a >> shift, a & ((1 << shift) - 1)
        half = 1 << (shift - 1)
        n += rem > half or (rem == half and n & 1)
    return sign * n, u


def fma_f32(x, a, m=0.0):
    """fl32(x * a + m) for an integer x and fp32 values a, m, rounded once -> (n, u) as _round_f32"""
    (an, as_), (mn, ms) = _dyadic(a), _dyadic(m)
    s = max(as_, ms)
    return _round_f32(int(x) * an * (1 << (s - as_)) + mn * (1 << (s - ms)), s)


def mul_f32(x, a):
    """fl32(x * a) as np.float32"""
    n, u = fma_f32(x, a)
    return np.float32(n * 2.0 ** u)                      # (n has at most 24 bits: exact)


def _clip_trunc(n, u):
    """np.clip(t, 0, 255).astype(np.uint8) of t = n * 2**u"""
    if n <= 0:
        return 0
    return min(255, n << u if u >= 0 else n >> -u)


def _rint_saturate(n, u):
    """t = n * 2**u rounded half to even, saturated to [0, 255]"""
    if n <= 0:
        return 0                                         # (everything <= 0 and everything that rounds to 0 or below)
    if u >= 0:
        return min(255, n << u)
    q, rem, half = n >> -u, n & ((1 << -u) - 1), 1 << (-u - 1)
    return min(255, q + (rem > half or (rem == half and q & 1)))


@functools.lru_cache(maxsize=None)
def _linear_map(alpha, m):
    """u8 [256]: x -> fma(x, alpha, m), clipped, truncated (Brightness: m = 0; Contrast: m = fl32(mean * beta))"""
    return np.array([_clip_trunc(*fma_f32(x, alpha, m)) for x in range(256)], np.uint8)


@functools.lru_cache(maxsize=None)
def _color_table(alpha, beta):
    """u8 [256 (gray), 256 (x)]: fma(x, alpha, fl32(g * beta)), rounded half to even, saturated"""
    out = np.zeros((256, 256), np.uint8)
    for g in range(256):
        m = mul_f32(g, beta)
        out[g] = [_rint_saturate(*fma_f32(x, alpha, m)) for x in range(256)]
    return out


# ---------------------------------------------------------------------------------------------- the four functions
def gray_mean(img):
    """mmcv.adjust_contrast's mean: round(np.sum(gray) / np.sum(hist)) -- Python's round, half to even"""
    gray = bgr2gray(img)
    hist = np.histogram(gray, 256, (0, 255))[0]
    return round(np.sum(gray) / np.sum(hist))


def gray_mean_int(img):
    """the kernel's integer form of gray_mean: S / N rounded half to even"""
    ghist = np.bincount(bgr2gray(img).reshape(-1), minlength=256)
    S, N = int((np.arange(256) * ghist).sum()), int(ghist.sum())
    q, r = divmod(S, N)
    return q + (2 * r > N or (2 * r == N and q % 2 == 1))


def adjust_brightness(img, factor):
    alpha, _ = factors(factor)
    return _linear_map(alpha, np.float32(0))[img]


def adjust_contrast(img, factor):
    alpha, beta = factors(factor)
    return _linear_map(alpha, mul_f32(gray_mean(img), beta))[img]


def adjust_color(img, factor):
    alpha, beta = factors(factor)
    return _color_table(alpha, beta)[bgr2gray(img)[..., None], img]


def equalize_lut(channel):
    """mmcv.imequalize's _scale_channel up to the lookup: (lut int64 [256] before use, step)"""
    histo = np.histogram(channel, 256, (0, 255))[0]
    nonzero_histo = histo[histo > 0]
    step = (np.sum(nonzero_histo) - nonzero_histo[-1]) // 255
    if not step:
        return np.array(range(256)), step, np.array(range(256))
    raw = (np.cumsum(histo) + (step // 2)) // step
    raw = np.concatenate([[0], raw[:-1]], 0)
    lut = raw.copy()
    lut[lut > 255] = 255
    return lut, step, raw


def imequalize(img):
    out = np.empty_like(img)
    for c in range(3):
        lut, step, _ = equalize_lut(img[:, :, c])
        out[:, :, c] = np.where(np.equal(step, 0), img[:, :, c], lut[img[:, :, c]])
    return out


def apply(img, kind, factor=1.0):
    """the u8 image under one colour stage"""
    return dict(brightness=adjust_brightness, contrast=adjust_contrast, color=adjust_color)[kind](img, factor) if kind != "equalize" \
        else imequalize(img)


def histograms(img):
    """int64 [4, 256]: unit-bin counts of B, G, R and gray"""
    planes = [img[..., 0], img[..., 1], img[..., 2], bgr2gray(img)]
    return np.stack([np.bincount(p.reshape(-1), minlength=256) for p in planes])


# ---------------------------------------------------------------------------------------------- the kernels' batch
GUARD = 0xAB
SKIP_ROW = 8


def kernel_frames(chunk_px):
    """the images the kernels are tested on: 1 x 1; 3 x 5; 15 x 17 (255 pixels: Equalize's step is 0); 20 x 26 (Equalize's
    lut passes 255 and is clamped); the 60 x 80 golden sample; 48 x 64 constant; 48 x 64 two-valued; about 2.5 chunks with an
    odd width (several workgroups add into one histogram, rows start misaligned); and one more for the skip row"""
    rs = np.random.RandomState(5)
    rnd = lambda h, w, r=rs: r.randint(0, 256, (h, w, 3)).astype(np.uint8)   # noqa: E731
    two = np.where(rs.rand(48, 64, 1) < 0.4, np.array([[[30, 200, 7]]]), np.array([[[90, 201, 255]]])).astype(np.uint8)
    wide = 2 * 63 + 1
    big = rnd((5 * chunk_px // 2) // wide, wide)
    big[: big.shape[0] // 2, :, :] //= 4                                     # (a skewed histogram: Equalize changes it visibly)
    return [rnd(1, 1), rnd(3, 5), rnd(15, 17), np.random.RandomState(0).randint(0, 256, (20, 26, 3)).astype(np.uint8),
            np.random.RandomState(1).randint(0, 256, (60, 80, 3)).astype(np.uint8),
            np.full((48, 64, 3), (17, 130, 250), np.uint8), two, big, rnd(9, 11)]


def pack(frames):
    """(pixel offsets, packed buffer): guard bytes between the images, byte offsets of every residue mod 4 and mod 16"""
    offs, o = [], 3
    for k, f in enumerate(frames):
        offs.append(o)
        o += f.shape[0] * f.shape[1] + 5 + k % 3
    packed = np.full(o * 3 + 7, GUARD, np.uint8)
    for f, off in zip(frames, offs):
        packed[off * 3:off * 3 + f.size] = f.reshape(-1)
    return offs, packed


def expected(frames, offs, packed, kinds, factor_of):
    """the packed buffer after one apply launch: image i under kinds[i] (None: a skip row, left alone)"""
    want = packed.copy()
    for f, off, kind in zip(frames, offs, kinds):
        if kind is not None:
            want[off * 3:off * 3 + f.size] = apply(f, kind, factor_of[kind]).reshape(-1)
    return want
