"""NumPy restatement of the three cv2-based stages of the RADet mixpbr train pipeline (RandomHSV, RandomNoise,
RandomSmooth) that csrc/augment.hip's aug_hsv_noise / aug_box are pinned to bit for bit.  Images are u8 HWC BGR.

- RandomHSV: cv2.cvtColor BGR2HSV on u8 (OpenCV's RGB2HSV_b: 12-bit fixed point, hue range 180), the float32 scale of
  each channel with the reference's clip / truncate, then HSV2BGR on u8 (HSV2RGB_b: the float path, rounded half to even).
- RandomNoise: img + N(0, sigma) * 255 in float64, clipped, truncated.  The normals come from Box-Muller on a
  Philox-4x64-10 stream (numpy.random.Philox(key=key).random_raw() word for word) -- the reference's distribution, not its
  np.random.normal stream.
- RandomSmooth: cv2.blur(img, (k, k)): normalised k x k box, BORDER_REFLECT_101, rounded half up.
Parity with cv2 itself is unpinned (cv2 is not a dependency); tests/test_mixaug_cpu.py checks each piece against
colorsys / scipy.ndimage / numpy.random.Philox."""
import numpy as np

f32 = np.float32
HSV_SHIFT = 12
_i = np.arange(1, 256, dtype=np.float64)
# cvRound((255 << 12) / i) and cvRound((180 << 12) / (6 i)); no quotient lies on a half, so the rounding mode is moot
SDIV = np.concatenate([[0], np.rint((255 << HSV_SHIFT) / _i)]).astype(np.int64)
HDIV = np.concatenate([[0], np.rint((180 << HSV_SHIFT) / (6.0 * _i))]).astype(np.int64)


def bgr2hsv(img):
    """cv2.cvtColor(img, COLOR_BGR2HSV) for u8: H in 0..179"""
    x = img.astype(np.int64)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    s = (diff * SDIV[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV[diff] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


_SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])   # (b, g, r) -> tab index


def hsv2bgr(hsv):
    """cv2.cvtColor(hsv, COLOR_HSV2BGR) for u8 (hue range 180): float32 arithmetic, saturate_cast<uchar>(x * 255.f)"""
    h = hsv[..., 0].astype(f32) * f32(f32(6.0) / f32(180.0))
    s = hsv[..., 1].astype(f32) * f32(f32(1.0) / f32(255.0))
    v = hsv[..., 2].astype(f32) * f32(f32(1.0) / f32(255.0))
    h = np.fmod(h, f32(6.0))
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(f32)
    one = f32(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1)
    idx = _SECTOR[np.clip(sector, 0, 5)]
    bgr = np.take_along_axis(tab, idx, axis=-1)
    bgr = np.where((s == 0)[..., None], v[..., None], bgr)
    return np.clip(np.rint(bgr * f32(255.0)), 0, 255).astype(np.uint8)


def hsv_scale(hsv, a, b, c):
    """the reference's aug_hsv middle part: float32(channel) * float32(factor), clipped at 179 / 255 when the (double)
    factor is >= 1, truncated back to u8"""
    out = np.empty_like(hsv)
    for ch, (fac, top) in enumerate(((a, 179), (b, 255), (c, 255))):
        y = hsv[..., ch].astype(f32) * f32(fac)
        if not fac < 1:
            y = np.minimum(y, f32(top))
        out[..., ch] = y.astype(np.uint8)
    return out


def random_hsv(img, a, b, c):
    return hsv2bgr(hsv_scale(bgr2hsv(img), a, b, c))


# ------------------------------------------------------------------------------------------------ Philox-4x64-10
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2E7470EE14C6C93), np.uint64(0xCA5A826395121157)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBB67AE8584CAA73B)
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mulhilo(a, b):
    a0, a1, b0, b1 = a & _M32, a >> _S32, b & _M32, b >> _S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> _S32) + (p01 & _M32) + (p10 & _M32)
    return p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32), a * b


def philox_words(key, n):
    """the first n words of numpy.random.Philox(key=key).random_raw(): block b (4 words) = Philox-4x64-10 of the 256-bit
    counter b + 1 under `key` (two uint64)"""
    nb = (int(n) + 3) // 4
    with np.errstate(over="ignore"):
        c0 = np.arange(1, nb + 1, dtype=np.uint64)
        c1 = c2 = c3 = np.zeros(nb, np.uint64)
        k0, k1 = np.uint64(key[0]), np.uint64(key[1])
        for r in range(10):
            if r:
                k0, k1 = k0 + PHILOX_W0, k1 + PHILOX_W1
            hi0, lo0 = _mulhilo(PHILOX_M0, c0)
            hi1, lo1 = _mulhilo(PHILOX_M1, c2)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return np.stack([c0, c1, c2, c3], axis=1).reshape(-1)[:n]


TWO_PI = 6.283185307179586
_EPS53 = 2.0 ** -53


def normals(key, n):
    """n standard normals: Box-Muller in float64 on pairs of Philox words; pair p uses words 2p, 2p + 1:
    u1 = ((w0 >> 11) + 1) 2^-53 in (0, 1], u2 = (w1 >> 11) 2^-53, z_2p = r cos(2 pi u2), z_2p+1 = r sin(2 pi u2)"""
    npair = (int(n) + 1) // 2
    w = philox_words(key, 2 * npair).reshape(npair, 2)
    u1 = ((w[:, 0] >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * _EPS53
    u2 = (w[:, 1] >> np.uint64(11)).astype(np.float64) * _EPS53
    r = np.sqrt(-2.0 * np.log(u1))
    t = TWO_PI * u2
    return np.stack([r * np.cos(t), r * np.sin(t)], axis=1).reshape(-1)[:n]


def noise_sum(img, sigma, key):
    """img + (sigma z) 255 in float64 before the clip (element e = (y W + x) 3 + c)"""
    z = normals(key, img.size).reshape(img.shape)
    return img.astype(np.float64) + (float(sigma) * z) * 255.0


def random_noise(img, sigma, key):
    return np.clip(noise_sum(img, sigma, key), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ box filter
def reflect101(p, n):
    """cv2.borderInterpolate(p, n, BORDER_REFLECT_101) for an int array p"""
    p = np.asarray(p, np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * (n - 1) - p, p))


def box_sums(img, k):
    """k x k window sums with reflect-101 borders (int64)"""
    h, w = img.shape[:2]
    r = k // 2
    x = img.astype(np.int64)
    cols = reflect101(np.arange(-r, w + r), w)
    rows = reflect101(np.arange(-r, h + r), h)
    xp = x[rows][:, cols]
    hs = sum(xp[:, d:d + w] for d in range(k))
    return sum(hs[d:d + h] for d in range(k))


def box_filter(img, k):
    """cv2.blur(img, (k, k)) for u8: (window sum + (k^2 - 1) / 2) // k^2"""
    kk = k * k
    return ((box_sums(img, k) + (kk - 1) // 2) // kk).astype(np.uint8)


def mix_chain(img_bgr, hsv=None, noise=None, k=None):
    """RandomHSV -> RandomNoise -> RandomSmooth on a BGR image; hsv = (a, b, c), noise = (sigma, key); None = skipped"""
    x = img_bgr
    if hsv is not None:
        x = random_hsv(x, *hsv)
    if noise is not None:
        x = random_noise(x, *noise)
    if k is not None:
        x = box_filter(x, k)
    return x
