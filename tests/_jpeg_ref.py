"""A slow NumPy / Python restatement of the baseline JPEG decoder that radet_amd/csrc/jpeg.hip implements, and of the scan
walker radet_jpeg_index: it pins the arithmetic (slow-integer IDCT, fancy chroma upsampling, 16-bit fixed-point colour
conversion) to what Pillow decodes on the host, and the index rows to an independent bit-by-bit reader.  Only the header
parse is shared with the package (radet_amd.core.jpeg.parse_jpeg)."""
import io

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class Corrupt(ValueError):
    pass


class Bits:
    """one bit at a time; the position is (raw offset of the data byte that holds the next bit, bit in it)"""

    def __init__(self, data, pos, end):
        self.d, self.pos, self.end, self.bit = data, pos, end, 0

    def at_marker(self):
        d, p = self.d, self.pos
        return p >= self.end or (d[p] == 0xFF and (p + 1 >= self.end or d[p + 1] != 0))

    def get(self):
        if self.at_marker():
            raise Corrupt("the stream ends early")
        v = (self.d[self.pos] >> (7 - self.bit)) & 1
        self.bit += 1
        if self.bit == 8:
            self.bit = 0
            self.pos += 2 if self.d[self.pos] == 0xFF else 1
        return v

    def take(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.get()
        return v

    def position(self):
        return self.pos * 8 + self.bit

    def align(self):
        if self.bit:
            self.bit = 0
            self.pos += 2 if self.d[self.pos] == 0xFF else 1


def code_table(bits, vals):
    """(length, code) -> symbol"""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[(l, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


def symbol(b, table, stats=None):
    code = 0
    for l in range(1, 17):
        code = (code << 1) | b.get()
        if (l, code) in table:
            if stats is not None:
                stats["max_len"] = max(stats["max_len"], l)
            return table[(l, code)]
    raise Corrupt("an undefined Huffman code")


def extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def walk(data, h, seg_mcus, decode=False):
    """the scan of `data` (header h): (index rows [S, 8] like radet_jpeg_index, stats dict(ac = histogram of the AC symbols,
    max_len = longest code used), coefficient blocks per component [c] -> int [blocks_y, blocks_x, 64] natural order if
    `decode`)"""
    seg = h.mcux if seg_mcus == "row" else seg_mcus
    tabs = [code_table(*t) for t in h.huff]
    b = Bits(data, h.scan_lo, h.scan_hi)
    stats = dict(ac=np.zeros(256, np.int64), max_len=0)
    rows, pred, in_int, rst = [], [0, 0, 0], 0, 0
    coefs = [np.zeros((h.mcuy * (h.vs if c == 0 else 1), h.mcux * (h.hs if c == 0 else 1), 64), np.int64) for c in range(h.ncomp)]
    for m in range(h.n_mcus):
        if h.restart_interval and m and in_int == h.restart_interval:
            b.align()
            p = b.pos
            while p + 1 < h.scan_hi and data[p] == 0xFF and data[p + 1] == 0xFF:
                p += 1
            if p + 1 >= h.scan_hi:
                raise Corrupt("the stream ends early")
            if data[p] != 0xFF or data[p + 1] != 0xD0 + (rst & 7):
                raise Corrupt("a restart marker out of sequence")
            rst += 1
            b = Bits(data, p + 2, h.scan_hi)
            pred, in_int = [0, 0, 0], 0
        if in_int % seg == 0:
            pos = b.position()
            rows.append([pos >> 3, pos & 7, m, 0, *pred, 0])
        mx, my = m % h.mcux, m // h.mcux
        for c in range(h.ncomp):
            hh, vv = (h.hs, h.vs) if c == 0 else (1, 1)
            for k in range(hh * vv):
                blk = coefs[c][my * vv + k // hh, mx * hh + k % hh]
                s = symbol(b, tabs[2 * c], stats)
                if s > 15:
                    raise Corrupt("an undefined Huffman code")
                pred[c] += extend(b.take(s), s)
                blk[0] = pred[c]
                i = 1
                while i < 64:
                    rs = symbol(b, tabs[2 * c + 1], stats)
                    stats["ac"][rs] += 1
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        i += 16
                        if i > 64:
                            raise Corrupt("a coefficient index past 63")
                        continue
                    i += r
                    if i > 63:
                        raise Corrupt("a coefficient index past 63")
                    blk[ZIGZAG[i]] = extend(b.take(s), s)
                    i += 1
        rows[-1][3] += 1
        rows[-1][7] = b.position()
        in_int += 1
    b.align()
    p = b.pos
    if p + 1 < h.scan_hi and data[p] == 0xFF and 0xD0 <= data[p + 1] <= 0xD7:
        raise Corrupt("an MCU count that does not match the frame")
    return np.array(rows, np.int32), stats, (coefs if decode else None)


C = dict(F0298=2446, F0390=3196, F0541=4433, F0765=6270, F0899=7373, F1175=9633, F1501=12299, F1847=15137, F1961=16069,
         F2053=16819, F2562=20995, F3072=25172)


def idct_1d(v, shift):
    """jidctint.c's pass over the first axis of v (int64 [8, ...])"""
    z1 = (v[2] + v[6]) * C["F0541"]
    tmp2 = z1 - v[6] * C["F1847"]
    tmp3 = z1 + v[2] * C["F0765"]
    tmp0, tmp1 = (v[0] + v[4]) << 13, (v[0] - v[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * C["F1175"]
    tmp0, tmp1, tmp2, tmp3 = tmp0 * C["F0298"], tmp1 * C["F2053"], tmp2 * C["F3072"], tmp3 * C["F1501"]
    z1, z2, z3, z4 = -z1 * C["F0899"], -z2 * C["F2562"], -z3 * C["F1961"] + z5, -z4 * C["F0390"] + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + (1 << (shift - 1))) >> shift for o in out])


def range_limit(v):
    v = v & 1023
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896))).astype(np.uint8)


def plane(coefs, quant):
    """[by, bx, 64] coefficients -> u8 [by * 8, bx * 8]"""
    by, bx, _ = coefs.shape
    v = (coefs * quant.astype(np.int64)).reshape(by, bx, 8, 8)            # [.., row, col]
    v = idct_1d(np.moveaxis(v, 2, 0), 11)                                 # columns: along the row index
    v = idct_1d(np.moveaxis(v, 3, 0), 18)                                 # [col, row, by, bx] -> rows: along the column index
    px = range_limit(v)                                                   # [col, row, by, bx]
    return px.transpose(2, 1, 3, 0).reshape(by * 8, bx * 8)


def up_h2v1(p):
    p = p.astype(np.int64)
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], p.shape[1] * 2), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def up_h2v2(p):
    p = p.astype(np.int64)
    up, down = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    out = np.empty((p.shape[0] * 2, p.shape[1] * 2), np.int64)
    for par, far in ((0, up), (1, down)):
        s = 3 * p + far
        left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        out[par::2, 0::2] = (3 * s + left + 8) >> 4
        out[par::2, 1::2] = (3 * s + right + 7) >> 4
        out[par::2, 0], out[par::2, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
    return out


def FIX(v):
    return int(v * 65536 + 0.5)


def decode_bgr(data):
    """u8 [H, W, 3] BGR of a supported file's bytes"""
    from radet_amd.core.jpeg import parse_jpeg
    h = parse_jpeg(data)
    assert h is not None
    _, _, coefs = walk(data, h, 8, decode=True)
    H, W = h.height, h.width
    planes = [plane(coefs[c], h.quant[c]) for c in range(h.ncomp)]
    y = planes[0][:H, :W].astype(np.int64)
    if h.ncomp == 1:
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, 2)
    ch, cw = -(-H // h.vs), -(-W // h.hs)
    cc = []
    for p in planes[1:]:
        p = p[:ch, :cw]                                    # the component's real size: the MCU padding takes no part
        p = up_h2v2(p) if h.vs == 2 else up_h2v1(p) if h.hs == 2 else p.astype(np.int64)
        cc.append(p[:H, :W] - 128)
    cb, cr = cc
    r = y + ((FIX(1.402) * cr + 32768) >> 16)
    g = y + ((-FIX(0.34414) * cb + 32768 - FIX(0.71414) * cr) >> 16)
    b = y + ((FIX(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], 2), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ fixtures
def content(kind, h, w, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    ramp = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(h + w - 2, 1)], 2)
    if kind == "ramp":
        return ramp.astype(np.uint8)
    assert kind == "checker"
    return np.clip(ramp // 2 + 100 * ((xx + yy) & 1)[:, :, None], 0, 255).astype(np.uint8)


SIZES = [(8, 8), (16, 16), (17, 9), (37, 51), (48, 64)]                     # (width, height)
SAMPLINGS = ["444", "422", "420", "grey"]
QUALITIES = [10, 75, 95, 100]
CONTENTS = ["noise", "ramp", "checker"]


def encode(kind, w, h, sampling, quality, optimize=False, restart=0, progressive=False, seed=0):
    from PIL import Image
    a = content(kind, h, w, seed)
    im = Image.fromarray(a).convert("L") if sampling == "grey" else Image.fromarray(a)
    kw = dict(quality=quality, optimize=optimize, progressive=progressive)
    if sampling != "grey":
        kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[sampling]
    if restart:
        kw["restart_marker_blocks"] = restart
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def matrix():
    """the case matrix: name -> file bytes.  Every size x sampling x quality x content once, the flags cycled over them so
    that optimize and a restart interval each occur on and off with every size and every sampling"""
    out, n = {}, 0
    for w, h in SIZES:
        for sampling in SAMPLINGS:
            for q in QUALITIES:
                for kind in CONTENTS:
                    optimize, restart = bool(n & 1), (0, 1, 0, 3)[(n >> 1) & 3]
                    n += 1
                    out[f"{w}x{h}-{sampling}-q{q}-{kind}-o{int(optimize)}-r{restart}"] = encode(kind, w, h, sampling, q, optimize, restart,
                                                                                               seed=n)
    return out


def pillow_bgr(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])
