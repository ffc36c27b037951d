"""Tiled inference: the tile plan of a frame, the checked request of apis.set_tiling, the rows of a tiled batch (host
arithmetic, no device), and, stand-alone, the rows' candidate lists filtered at the tile borders, mapped back to the frames
and packed per image (radet_merge_tiles, csrc/tiles.hip) -- the step DetectorRuntime.detect_tiles runs between the rows'
decode launches and the one NMS over their union.  The plan, the edge rule and the order of the union are this project's
own rules: the reference has no tiled inference."""
import numbers
from collections import namedtuple

import numpy as np
import torch

from .. import kernels as K

TILING_KEYS = ("tile", "overlap", "full_frame", "edge_margin", "batch", "nms_pre")
TileSpec = namedtuple("TileSpec", TILING_KEYS)


def _int(v):
    return isinstance(v, (numbers.Integral, np.integer)) and not isinstance(v, bool)


def _pair(v):
    return tuple(int(x) for x in v) if isinstance(v, (tuple, list)) and len(v) == 2 and all(_int(x) for x in v) else None


def _overlap(tile, overlap):
    """overlap in pixels (ow, oh): a pair of ints as given, one float ratio r -> (floor(r * tw), floor(r * th))"""
    if isinstance(overlap, (tuple, list)):
        o = _pair(overlap)
    elif isinstance(overlap, (float, np.floating)) or overlap == 0:
        r = float(overlap)
        o = (int(np.floor(r * tile[0])), int(np.floor(r * tile[1]))) if np.isfinite(r) else None
    else:
        o = None
    if o is None or not all(0 <= ov < t for ov, t in zip(o, tile)):
        raise ValueError(f"overlap={overlap!r}: (ow, oh) in pixels or one float ratio, with 0 <= overlap < tile={tile}")
    return o


def _tile(tile):
    t = _pair(tile)
    if t is None or min(t) < 1:
        raise ValueError(f"tile={tile!r}: (tw, th) in frame pixels, two positive ints, width first (like img_scale)")
    return t


def _axis(L, t, o):
    if L <= t:
        return [0], L
    n = -(-(L - o) // (t - o))                                  # ceil((L - o) / (t - o)) >= 2
    return [(i * (L - t)) // (n - 1) for i in range(n)], t


def plan_tiles(h, w, tile, overlap):
    """The tiles of an h x w frame: int32 [T, 4] rows (x0, y0, tw, th), row-major (y outer, x inner).  tile = (tw, th) in frame
    pixels, width first like img_scale; overlap = (ow, oh) in pixels or one float ratio r -> (floor(r * tw), floor(r * th)),
    0 <= overlap < tile.  Per axis of length L with tile t and overlap o: L <= t gives the one tile [0, L); otherwise
    n = ceil((L - o) / (t - o)) tiles of full length t at s_i = (i * (L - t)) // (n - 1) -- the first starts at 0, the last
    ends at L, consecutive tiles overlap by at least o, and every tile lies inside the frame (no overhang, no fill colour)."""
    if not (_int(h) and _int(w) and h > 0 and w > 0):
        raise ValueError(f"plan_tiles: a frame of {h} x {w}")
    tile = _tile(tile)
    ow, oh = _overlap(tile, overlap)
    xs, tw = _axis(int(w), tile[0], ow)
    ys, th = _axis(int(h), tile[1], oh)
    return np.array([(x, y, tw, th) for y in ys for x in xs], np.int32).reshape(-1, 4)


def edge_masks(rects, h, w):
    """TILE_EDGE_* bits per rectangle (x0, y0, tw, th) of an h x w frame: a bit is set where that side of the rectangle is not
    a side of the frame (a cut through the image)"""
    r = np.asarray(rects, np.int64).reshape(-1, 4)
    return ((r[:, 0] > 0) * K.TILE_EDGE_L + (r[:, 1] > 0) * K.TILE_EDGE_T + (r[:, 0] + r[:, 2] < w) * K.TILE_EDGE_R
            + (r[:, 1] + r[:, 3] < h) * K.TILE_EDGE_B).astype(np.int32)


def tiling_spec(tiling):
    """apis.set_tiling's dict -> TileSpec, checked: dict(tile=(tw, th), overlap=0.25, full_frame=True, edge_margin=0.0,
    batch=16, nms_pre=None).  ValueError for unknown keys, a missing tile, an overlap outside [0, tile)."""
    if isinstance(tiling, TileSpec):
        return tiling
    if not isinstance(tiling, dict) or "tile" not in tiling or set(tiling) - set(TILING_KEYS):
        raise ValueError(f"tiling={tiling!r}: expected dict(tile=(tw, th), [{', '.join(TILING_KEYS[1:])}])")
    tile = _tile(tiling["tile"])
    overlap = _overlap(tile, tiling.get("overlap", 0.25))
    margin = tiling.get("edge_margin", 0.0)
    if not isinstance(margin, numbers.Real) or isinstance(margin, bool) or not np.isfinite(margin) or margin < 0:
        raise ValueError(f"tiling: edge_margin={margin!r} must be a finite number >= 0")
    batch = tiling.get("batch", 16)
    if not _int(batch) or batch < 1:
        raise ValueError(f"tiling: batch={batch!r} (rows per forward batch, >= 1)")
    nms_pre = tiling.get("nms_pre")
    if nms_pre is not None and (not _int(nms_pre) or nms_pre < 1):
        raise ValueError(f"tiling: nms_pre={nms_pre!r} (a positive int, or None for test_cfg's)")
    return TileSpec(tile, overlap, bool(tiling.get("full_frame", True)), float(margin), int(batch),
                    None if nms_pre is None else int(nms_pre))


def tile_rows(shapes, spec):
    """The rows of a tiled batch, image-major; per frame (h, w) of shapes its full-frame row first (spec.full_frame), then its
    tiles in plan order.  -> (rects i32 [R, 4] (x0, y0, tw, th), edges i32 [R], row_start i32 [B + 1]).  More than
    TILE_MAX_ROWS rows for a frame are refused."""
    spec = tiling_spec(spec)
    rects, edges, row_start = [], [], [0]
    for h, w in shapes:
        h, w = int(h), int(w)
        tiles = plan_tiles(h, w, spec.tile, spec.overlap)
        n = len(tiles) + int(spec.full_frame)
        if n > K.TILE_MAX_ROWS:
            raise NotImplementedError(f"tiling a {w} x {h} frame with tile={spec.tile}, overlap={spec.overlap} gives {n} rows, more "
                                      f"than {K.TILE_MAX_ROWS} for one frame: enlarge the tile")
        if spec.full_frame:
            rects.append(np.array([[0, 0, w, h]], np.int32))
            edges.append(np.zeros(1, np.int32))
        rects.append(tiles)
        edges.append(edge_masks(tiles, h, w))
        row_start.append(row_start[-1] + n)
    if not rects:
        return np.zeros((0, 4), np.int32), np.zeros(0, np.int32), np.asarray(row_start, np.int32)
    return np.concatenate(rects), np.concatenate(edges), np.asarray(row_start, np.int32)


def merge_tile_candidates(boxes, scores, ctr, labels, counts, rows_per_image, img_shapes, scale_factors, offsets, edge_masks,
                          edge_margin=0.0):
    """Lists over the R rows of a tiled batch, image-major, as radet_decode_candidates writes them in row coordinates:
    boxes[r] f32 [cap_r, 4], scores[r] / ctr[r] f32 [cap_r], labels[r] i64 [cap_r]; counts [R] ints (below 0 counts as 0,
    above cap_r as cap_r); rows_per_image [B] (1..TILE_MAX_ROWS each, summing to R); img_shapes[r] = (h, w, ...),
    scale_factors[r] = 4 floats, offsets[r] = (x0, y0) of the row in its frame, edge_masks[r] = TILE_EDGE_* bits.
    -> (boxes f32 [B, cap_out, 4], scores, ctr f32 [B, cap_out], labels i64 [B, cap_out], counts i32 [B], dropped i32 [B]) on
    the device, cap_out = the largest sum of an image's capacities: per image the candidates that no cut tile border touches
    (include/radet_hip.h, radet_merge_tiles: the edge rule with margin edge_margin), in row order and inside a row in
    candidate order, boxes mapped back as x / sx + x0 (fp32, each operation rounded once).  Slots at and beyond counts[b] are
    unspecified.  One launch, no host synchronisation."""
    from . import _dev, _t, _upload
    R = len(boxes)
    if not (R == len(scores) == len(ctr) == len(labels) == len(counts) == len(img_shapes) == len(scale_factors) == len(offsets)
            == len(edge_masks)):
        raise ValueError("merge_tile_candidates: every argument but rows_per_image is a list over the rows")
    rows_per_image = [int(n) for n in rows_per_image]
    B = len(rows_per_image)
    if sum(rows_per_image) != R or any(not 1 <= n <= K.TILE_MAX_ROWS for n in rows_per_image):
        raise ValueError(f"merge_tile_candidates: rows_per_image={rows_per_image} (1..{K.TILE_MAX_ROWS} each) for {R} rows")
    dev = _dev()
    row_start = np.concatenate([[0], np.cumsum(rows_per_image)]).astype(np.int32)
    bx = [_t(b, torch.float32).reshape(-1, 4) for b in boxes]
    caps = np.array([int(b.shape[0]) for b in bx], np.int64)
    starts = np.concatenate([[0], np.cumsum(caps)])[:R] if R else np.zeros(0, np.int64)
    cap_out = max([int(caps[row_start[b]:row_start[b + 1]].sum()) for b in range(B)] + [1])
    hw = np.array([[s[0], s[1]] for s in img_shapes], np.float32).reshape(R, 2)
    sf = np.array([np.asarray(f, np.float32).reshape(4) for f in scale_factors], np.float32).reshape(R, 4)
    desc = K.tile_desc_rows(hw, sf, np.asarray(offsets, np.float32).reshape(R, 2), np.asarray(edge_masks, np.int32), starts, caps)

    def pool(ts, dtype):
        return torch.cat([_t(t, dtype).reshape(-1) for t in ts]) if R else torch.empty(0, dtype=dtype, device=dev)
    ob = torch.empty(B, cap_out, 4, device=dev)
    osc, oct_ = torch.empty(B, cap_out, device=dev), torch.empty(B, cap_out, device=dev)
    ol = torch.empty(B, cap_out, dtype=torch.long, device=dev)
    oc, od = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    K.merge_tiles(desc, _upload(desc, dev), row_start, _upload(row_start, dev), B,
                  torch.cat(bx) if R else torch.empty(0, 4, device=dev), pool(scores, torch.float32), pool(ctr, torch.float32),
                  pool(labels, torch.long), _upload(np.asarray([int(c) for c in counts], np.int32), dev), float(edge_margin),
                  cap_out, ob, osc, oct_, ol, oc, od)
    return ob, osc, oct_, ol, oc, od
