"""Two independent NumPy restatements of radet_draw_detections (include/radet_hip.h, radet_amd/csrc/draw.hip):

    gather(...)   per pixel: every pixel of the frame asks, in paint order, which primitive covers it (masks over the pixel
                  grid, the text through per-column lookup tables into the atlas)
    painter(...)  per primitive: outlines as four filled bands, labels as a rectangle and one pasted glyph block per strip,
                  scattered onto a copy of the frame in paint order with slices

They share no code but `Style`; tests/test_draw_cpu.py holds them to each other bit for bit, tests/test_gpu_draw.py holds
the kernel to them.  Arguments: frames = list of HxWx3 uint8 arrays; boxes f32 [B,K,4], scores f32 [B,K], labels int [B,K],
counts int [B]; atlas = (coverage u8 [S,Hc,Wa], widths int [S]) or None (no labels)."""
from collections import namedtuple
from decimal import ROUND_FLOOR, Decimal

import numpy as np

Style = namedtuple("Style", "thickness colour palette text_colour a_bg score_thr max_dets n_names pad")
Style.__doc__ = """colour: (b, g, r) or None with palette u8 [n,3]; a_bg in [0, 255]; n_names: 0 = the 'class N' text form"""

DOT, BAR, CLASS, NAME0 = 10, 11, 12, 13
FULL = 65025


# --------------------------------------------------------------------------------------------------- the per-pixel gather
def _cents(score):
    c = int(np.floor(np.float64(np.float32(score)) * 100.0 + 0.5))
    return min(max(c, 0), 100)


def score_text(score):
    c = _cents(score)
    return f"{c // 100}.{c // 10 % 10}{c % 10}"


def _strips(label, score, n_names):
    c = _cents(score)
    head = [NAME0 + label] if n_names > 0 else [CLASS] + [int(ch) for ch in str(label)]
    return head + [BAR, c // 100, DOT, c // 10 % 10, c % 10]


def _drawn_gather(boxes, scores, labels, count, st):
    out = []
    K = boxes.shape[0]
    limit = st.n_names if st.n_names > 0 else 100000
    for j in range(min(max(int(count), 0), K)):
        if len(out) >= st.max_dets:
            break
        v = np.append(boxes[j], scores[j]).astype(np.float32)
        if not np.isfinite(v).all() or not v[4] > np.float32(st.score_thr):
            continue
        lab = int(labels[j])
        if lab < 0 or lab >= limit or (st.colour is None and lab >= len(st.palette)):
            continue
        x1, y1, x2, y2 = (int(t) for t in np.clip(v[:4], -2.0 ** 20, 2.0 ** 20).astype(np.int32))
        if x2 < x1 or y2 < y1:
            continue
        out.append((x1, y1, x2, y2, lab, v[4]))
    return out


def _blend_arr(px, colour, a):
    """px int64 [..., 3], colour (3,), a int array broadcastable to px[..., 0]"""
    a = np.asarray(a, np.int64)[..., None]
    return (np.asarray(colour, np.int64) * a + px * (FULL - a) + 32512) // FULL


def gather_frame(frame, boxes, scores, labels, count, st, atlas):
    h, w = frame.shape[:2]
    out = frame.astype(np.int64)
    if h <= 0 or w <= 0:
        return frame.copy()
    Y, X = np.mgrid[0:h, 0:w]
    t = st.thickness
    lo, hi = t // 2, (t - 1) // 2
    dets = _drawn_gather(boxes, scores, labels, count, st)
    taken = np.zeros((h, w), bool)
    for x1, y1, x2, y2, lab, _ in dets:                                   # the lowest rank that covers a pixel gives its colour
        outer = (X >= x1 - lo) & (X <= x2 + hi) & (Y >= y1 - lo) & (Y <= y2 + hi)
        hole = (X > x1 + hi) & (X < x2 - lo) & (Y > y1 + hi) & (Y < y2 - lo)
        m = outer & ~hole & ~taken
        out[m] = np.asarray(st.colour if st.colour is not None else st.palette[lab], np.int64)
        taken |= m
    if atlas is not None and atlas[0].shape[1] > 0:
        cov, widths = atlas
        Hc, Wa = cov.shape[1:]
        p = st.pad
        for x1, y1, x2, y2, lab, score in reversed(dets):
            ids = _strips(lab, score, st.n_names)
            ws = [min(max(int(widths[i]), 0), Wa) for i in ids]
            Wt = sum(ws)
            col_id = np.repeat(ids, ws)                                   # text column -> strip, column inside the strip
            col_off = np.concatenate([np.arange(v) for v in ws]) if Wt else np.zeros(0, np.int64)
            lw, lh = Wt + 2 * p, Hc + 2 * p
            lx, ly = max(0, min(x1, w - lw)), max(0, min(y1, h - lh))
            U, V = X - lx, Y - ly
            rect = (U >= 0) & (U < lw) & (V >= 0) & (V < lh)
            out[rect] = _blend_arr(out[rect], (0, 0, 0), st.a_bg * 255)
            tm = rect & (U - p >= 0) & (U - p < Wt) & (V - p >= 0) & (V - p < Hc)
            tu, tv = (U - p)[tm], (V - p)[tm]
            c = cov[col_id[tu], tv, col_off[tu]].astype(np.int64)
            out[tm] = _blend_arr(out[tm], st.text_colour, 255 * c)
    return out.astype(np.uint8)


def gather(frames, boxes, scores, labels, counts, st, atlas):
    return [gather_frame(f, boxes[b], scores[b], labels[b], counts[b], st, atlas) for b, f in enumerate(frames)]


# --------------------------------------------------------------------------------------------------- the painter
def _half_up_cents(score):
    """round half up of the exact value of 100 * (the float32 score), clamped to [0, 100] (24 + 7 bits: the kernel's double
    product and sum are exact, so this is the same number)"""
    d = (Decimal(float(np.float32(score))) * 100 + Decimal("0.5")).to_integral_value(rounding=ROUND_FLOOR)
    return int(min(max(d, 0), 100))


def _text_image(label, score, n_names, cov, widths):
    cents = "%03d" % _half_up_cents(score)
    digits = lambda s: [int(ch) for ch in s]                              # noqa: E731
    seq = ([NAME0 + label] if n_names else [CLASS] + digits("%d" % label)) + [BAR] + digits(cents[0]) + [DOT] + digits(cents[1:])
    Wa = cov.shape[2]
    return np.concatenate([cov[s][:, :int(np.clip(widths[s], 0, Wa))] for s in seq], axis=1).astype(np.int64)


def _fill(img, x_lo, x_hi, y_lo, y_hi, colour):
    """inclusive rectangle, clipped to the image"""
    h, w = img.shape[:2]
    x_lo, y_lo, x_hi, y_hi = max(x_lo, 0), max(y_lo, 0), min(x_hi, w - 1), min(y_hi, h - 1)
    if x_lo <= x_hi and y_lo <= y_hi:
        img[y_lo:y_hi + 1, x_lo:x_hi + 1] = colour


def _mix(img, x_lo, y_lo, colour, alpha):
    """alpha int64 [hh, ww] in [0, 65025] composited at (x_lo, y_lo), clipped to the image"""
    h, w = img.shape[:2]
    hh, ww = alpha.shape
    ax, ay = max(0, -x_lo), max(0, -y_lo)
    bx, by = min(ww, w - x_lo), min(hh, h - y_lo)
    if ax >= bx or ay >= by:
        return
    a = alpha[ay:by, ax:bx, None]
    reg = img[y_lo + ay:y_lo + by, x_lo + ax:x_lo + bx]
    reg[...] = (np.array(colour, np.int64)[None, None] * a + reg * (FULL - a) + 32512) // FULL


def painter_frame(frame, boxes, scores, labels, count, st, atlas):
    h, w = frame.shape[:2]
    img = frame.astype(np.int64)
    if h <= 0 or w <= 0:
        return frame.copy()
    n = min(max(int(count), 0), boxes.shape[0])
    b32, s32 = np.asarray(boxes[:n], np.float32), np.asarray(scores[:n], np.float32)
    lab = np.asarray(labels[:n], np.int64)
    ok = np.isfinite(b32).all(axis=1) & np.isfinite(s32) & (s32 > np.float32(st.score_thr)) & (lab >= 0)
    ok &= lab < (st.n_names if st.n_names else 100000)
    if st.colour is None:
        ok &= lab < len(st.palette)
    ib = np.trunc(np.clip(np.where(np.isfinite(b32), b32, 0), -1048576, 1048576)).astype(np.int64)
    ok &= (ib[:, 2] >= ib[:, 0]) & (ib[:, 3] >= ib[:, 1])
    order = np.flatnonzero(ok)[:st.max_dets]
    t = st.thickness
    lo, hi = t // 2, (t - 1) // 2
    for j in order[::-1]:                                                 # painted last = on top: rank 0 goes last
        x1, y1, x2, y2 = (int(v) for v in ib[j])
        colour = st.colour if st.colour is not None else tuple(int(v) for v in st.palette[lab[j]])
        ox1, oy1, ox2, oy2 = x1 - lo, y1 - lo, x2 + hi, y2 + hi
        hx1, hy1, hx2, hy2 = x1 + hi + 1, y1 + hi + 1, x2 - lo - 1, y2 - lo - 1    # the hole, inclusive
        if hx1 > hx2 or hy1 > hy2:
            _fill(img, ox1, ox2, oy1, oy2, colour)
            continue
        _fill(img, ox1, ox2, oy1, hy1 - 1, colour)
        _fill(img, ox1, ox2, hy2 + 1, oy2, colour)
        _fill(img, ox1, hx1 - 1, hy1, hy2, colour)
        _fill(img, hx2 + 1, ox2, hy1, hy2, colour)
    if atlas is not None and atlas[0].shape[1] > 0:
        cov, widths = atlas
        p = st.pad
        for j in order[::-1]:
            text = _text_image(int(lab[j]), s32[j], st.n_names, cov, widths)
            lw, lh = text.shape[1] + 2 * p, text.shape[0] + 2 * p
            lx, ly = max(0, min(int(ib[j, 0]), w - lw)), max(0, min(int(ib[j, 1]), h - lh))
            _mix(img, lx, ly, (0, 0, 0), np.full((lh, lw), st.a_bg * 255, np.int64))
            _mix(img, lx + p, ly + p, st.text_colour, 255 * text)
    return img.astype(np.uint8)


def painter(frames, boxes, scores, labels, counts, st, atlas):
    return [painter_frame(f, boxes[b], scores[b], labels[b], counts[b], st, atlas) for b, f in enumerate(frames)]


# --------------------------------------------------------------------------------------------------- shared test material
def synthetic_atlas(n_names, Hc=7, Wa=19, seed=11):
    """random coverage, random strip widths in [1, Wa] (a strip of width 0 among the names when there are several): no
    test depends on a font's pixels"""
    rng = np.random.RandomState(seed)
    S = NAME0 + n_names
    cov = rng.randint(0, 256, (S, Hc, Wa)).astype(np.uint8)
    cov[rng.rand(S, Hc, Wa) < 0.3] = 0
    cov[rng.rand(S, Hc, Wa) < 0.1] = 255
    widths = rng.randint(1, Wa + 1, S).astype(np.int32)
    widths[:10] = rng.randint(3, 6, 10)                                   # (narrow digits keep the labels inside small frames)
    widths[DOT], widths[BAR] = 2, 1
    return cov, widths
