"""Run-length instance masks on the host (NumPy, no device): the COCO layouts that annotation files carry.

A run list (`counts`) walks a mask of h x w pixels column by column (position p = x * h + y); the first run counts zeros,
runs alternate, and the counts sum to h * w.  The compressed string form packs every count into 5-bit groups (+ 48,
continuation bit 0x20, sign bit 0x10) and stores, from the fourth count on, the difference to the count two places
earlier.  A polygon is rasterised the way pycocotools' rleFrPoly does it.  A mask is a list of parts (one run list per
polygon, or the single run list of an RLE record) that are united.

pycocotools is absent here: the uncompressed list form is exact by definition; the string form and the polygon
rasteriser restate maskApi.c (rleToString / rleFrString / rleFrPoly) and are not pinned against it.
The training path decodes nothing on the host: `pack_runs` lays the run lists of a batch out for radet_rle_masks."""
import numpy as np


# ---------------------------------------------------------------------------------------------------- list form
def rle_from_mask(mask):
    """u8 / bool [H, W] (non-zero = set) -> counts (int64 array)"""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError(f"rle_from_mask takes one [H, W] mask, got shape {m.shape}")
    v = (m != 0).T.reshape(-1)                                   # column-major
    if v.size == 0:
        return np.zeros(1, np.int64)
    edges = np.flatnonzero(v[1:] != v[:-1]) + 1
    counts = np.diff(np.concatenate([[0], edges, [v.size]]))
    return np.concatenate([[0], counts]).astype(np.int64) if v[0] else counts.astype(np.int64)


def check_counts(counts, h, w, what="run list"):
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if c.size == 0 or (c < 0).any() or int(c.sum()) != int(h) * int(w):
        raise ValueError(f"{what}: {c.size} counts that sum to {int(c.sum())}, not to {h} x {w} = {int(h) * int(w)}")
    return c


def mask_from_rle(counts, h, w):
    """counts -> u8 [H, W] of 0 / 1 (the host decoder: converter and tests only)"""
    c = check_counts(counts, h, w)
    v = np.repeat(np.arange(c.size, dtype=np.uint8) & 1, c)
    return np.ascontiguousarray(v.reshape(w, h).T)


# ---------------------------------------------------------------------------------------------------- string form
def string_from_counts(counts):
    """rleToString: counts -> bytes"""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    out = bytearray()
    for i, x in enumerate(c):
        if i > 2:
            x -= c[i - 2]
        more = True
        while more:
            g = x & 0x1f
            x >>= 5
            more = (x != -1) if (g & 0x10) else (x != 0)
            out.append((g | 0x20 if more else g) + 48)
    return bytes(out)


def counts_from_string(s):
    """rleFrString, vectorised: group boundaries from the continuation flags, a segmented shift-and-add with sign
    extension, then the two interleaved cumulative sums that undo the differences"""
    if isinstance(s, str):
        s = s.encode("ascii")
    c = np.frombuffer(bytes(s), dtype=np.uint8).astype(np.int64) - 48
    if c.size == 0:
        return np.zeros(0, np.int64)
    if (c < 0).any() or (c > 63).any():
        raise ValueError("compressed run list with a character outside '0' .. 'o'")
    last = (c & 0x20) == 0                                       # last group of its count
    if not last[-1]:
        raise ValueError("compressed run list ends inside a count")
    ends = np.flatnonzero(last)
    starts = np.concatenate([[0], ends[:-1] + 1])
    k = np.arange(c.size) - np.repeat(starts, ends - starts + 1)  # group number inside its count
    if k.max() > 11:
        raise ValueError("compressed run list with a count of more than 12 groups")
    x = np.add.reduceat((c & 0x1f) << (5 * k), starts)
    neg = (c[ends] & 0x10) != 0
    x = np.where(neg, x | (np.int64(-1) << (5 * (k[ends] + 1))), x)
    out = x.copy()
    out[1::2] = np.cumsum(x[1::2])
    out[2::2] = np.cumsum(x[2::2])
    return out


# ---------------------------------------------------------------------------------------------------- polygons
def _rle_from_polygon(xy, h, w):
    """rleFrPoly for one polygon (x0, y0, x1, y1, ...): the boundary upsampled by 5 and traced edge by edge in integers, the
    crossings of pixel-column centres kept, their column-major positions sorted and differenced"""
    scale = 5.0
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    px = (scale * xy[:, 0] + .5).astype(np.int64)                 # (int) truncates toward zero, and so does astype
    py = (scale * xy[:, 1] + .5).astype(np.int64)
    px, py = np.append(px, px[0]), np.append(py, py[0])
    us, vs = [], []
    for j in range(len(xy)):
        xs, xe, ys, ye = int(px[j]), int(px[j + 1]), int(py[j]), int(py[j + 1])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = (ye - ys) / dx if dx else 0.0                     # (a repeated vertex: one point; C divides 0 by 0 there)
            t = np.arange(dx + 1)
            t = dx - t if flip else t
            us.append(t + xs)
            vs.append((ys + s * t + .5).astype(np.int64))
        else:
            s = (xe - xs) / dy
            t = np.arange(dy + 1)
            t = dy - t if flip else t
            vs.append(t + ys)
            us.append((xs + s * t + .5).astype(np.int64))
    u, v = np.concatenate(us), np.concatenate(vs)
    j = np.flatnonzero(u[1:] != u[:-1]) + 1
    xd = np.where(u[j] < u[j - 1], u[j], u[j] - 1).astype(np.float64)
    xd = (xd + .5) / scale - .5
    keep = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    j, xd = j[keep], xd[keep]
    yd = np.minimum(v[j], v[j - 1]).astype(np.float64)
    yd = np.ceil(np.clip((yd + .5) / scale - .5, 0, h))
    a = np.sort(np.append(xd.astype(np.int64) * h + yd.astype(np.int64), h * w))
    a = np.diff(np.concatenate([[0], a]))
    # zero-length runs merge their neighbours (the first count stays, even when zero)
    b = [int(a[0])]
    i = 1
    while i < len(a):
        if a[i] > 0:
            b.append(int(a[i]))
            i += 1
        else:
            i += 1
            if i < len(a):
                b[-1] += int(a[i])
                i += 1
    return np.asarray(b, np.int64)


def rle_from_polygons(parts, h, w):
    """a COCO polygon segmentation (list of flat coordinate lists) -> one run list per valid polygon; parts with an odd
    number of values or fewer than 6 are dropped"""
    out = []
    for p in parts:
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.size % 2 == 0 and p.size >= 6:
            out.append(_rle_from_polygon(p, h, w))
    return out


# ---------------------------------------------------------------------------------------------------- records
def parts_from_segmentation(seg, h, w, what="segmentation"):
    """a COCO `segmentation` object -> list of run lists (int64 arrays) whose union is the mask: a polygon list gives one
    part per valid polygon, an RLE dict (counts as a list, or as the compressed string) is a single part.  ValueError
    (naming `what`) for counts that do not sum to h * w or a `size` that is not [h, w]."""
    if isinstance(seg, dict):
        size = seg.get("size")
        if size is None or [int(v) for v in size] != [int(h), int(w)]:
            raise ValueError(f"{what}: RLE of size {size} for an image of {h} x {w}")
        counts = seg["counts"]
        try:
            counts = counts_from_string(counts) if isinstance(counts, (str, bytes)) else np.asarray(counts, np.int64)
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None
        return [check_counts(counts, h, w, what)]
    if isinstance(seg, (list, tuple)):
        return rle_from_polygons(seg, h, w)
    raise ValueError(f"{what}: a segmentation is a polygon list or an RLE dict, got {type(seg).__name__}")


def mask_from_parts(parts, h, w):
    """the union of a mask's parts, u8 [H, W] of 0 / 1 (host decoder: tests and tools)"""
    m = np.zeros((h, w), np.uint8)
    for c in parts:
        m |= mask_from_rle(c, h, w)
    return m


# ---------------------------------------------------------------------------------------------------- device layout
RLE_MASK_INTS, RLE_PART_INTS = 5, 2            # include/radet_hip.h


def pack_runs(parts_per_mask, h, w, flips=None):
    """The arrays radet_rle_masks reads, for masks of one source size: (run_ends u32 [R] = the inclusive prefix sums of
    every part's counts, concatenated; part rows i32 [P, 2] = (offset into run_ends, runs); mask rows i32 [G, 5] = (first
    part, parts, h, w, flip)).  `flips`: one bool per mask."""
    h, w = int(h), int(w)
    if h <= 0 or w <= 0 or h * w >= 2 ** 32:
        raise ValueError(f"run-length masks of {h} x {w}: positions are 32-bit")
    G = len(parts_per_mask)
    parts = [np.asarray(c, np.int64).reshape(-1) for m in parts_per_mask for c in m]
    sizes = np.array([c.size for c in parts], np.int64)
    mrows = np.zeros((G, RLE_MASK_INTS), np.int32)
    mrows[:, 1] = [len(m) for m in parts_per_mask]
    mrows[:, 0] = np.cumsum(mrows[:, 1]) - mrows[:, 1]
    mrows[:, 2], mrows[:, 3] = h, w
    if flips is not None:
        mrows[:, 4] = np.asarray(flips, bool).reshape(G)
    prows = np.zeros((len(parts), RLE_PART_INTS), np.int32)
    prows[:, 1] = sizes
    prows[:, 0] = np.cumsum(sizes) - sizes
    if not parts:
        return np.zeros(0, np.uint32), prows, mrows
    ends = np.cumsum(np.concatenate(parts))
    last = ends[np.cumsum(sizes) - 1]                                        # every part sums to h * w
    if (sizes == 0).any() or not np.array_equal(last, h * w * np.arange(1, len(parts) + 1)) or min(c.min() for c in parts) < 0:
        raise ValueError(f"a run list does not sum to {h} x {w}")
    ends -= np.repeat(last - h * w, sizes)
    return ends.astype(np.uint32), prows, mrows
