"""NumPy restatements for tiled inference: the tile plan (ops.plan_tiles) written again from its rule, and the merge of the
rows' candidates (radet_merge_tiles): the keep rule at cut tile borders, the map-back x / sx + x0 in float32 with every
operation rounded once, and the stable per-image order."""
import numpy as np

L_, T_, R_, B_ = 1, 2, 4, 8


def axis_tiles(L, t, o):
    """[(start, length)] of one axis of length L with tile t and overlap o (0 <= o < t)"""
    if L <= t:
        return [(0, L)]
    n = int(np.ceil((L - o) / (t - o)))
    assert n == -(-(L - o) // (t - o)) and n >= 2
    return [((i * (L - t)) // (n - 1), t) for i in range(n)]


def plan(h, w, tile, overlap):
    """int32 [T, 4] (x0, y0, tw, th), y outer and x inner; overlap: (ow, oh) pixels or a float ratio"""
    if isinstance(overlap, float):
        overlap = (int(np.floor(overlap * tile[0])), int(np.floor(overlap * tile[1])))
    xs, ys = axis_tiles(w, tile[0], overlap[0]), axis_tiles(h, tile[1], overlap[1])
    return np.array([(x, y, tw, th) for y, th in ys for x, tw in xs], np.int32).reshape(-1, 4)


def edge_mask(rect, h, w):
    x0, y0, tw, th = (int(v) for v in rect)
    return (L_ if x0 > 0 else 0) | (T_ if y0 > 0 else 0) | (R_ if x0 + tw < w else 0) | (B_ if y0 + th < h else 0)


def keep_mask(boxes, img_shape, edge, margin):
    """the candidates (row coordinates) that no cut side of their row touches within margin"""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    m = np.float32(margin)
    h, w = np.float32(img_shape[0]), np.float32(img_shape[1])
    drop = np.zeros(len(b), bool)
    if edge & L_:
        drop |= b[:, 0] <= m
    if edge & T_:
        drop |= b[:, 1] <= m
    if edge & R_:
        drop |= b[:, 2] >= np.float32(w - m)
    if edge & B_:
        drop |= b[:, 3] >= np.float32(h - m)
    return ~drop


def map_back(boxes, scale_factor, offset):
    """x / sx (one rounding), + x0 (one rounding), float32"""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    q = (b / np.asarray(scale_factor, np.float32).reshape(1, 4)).astype(np.float32)
    off = np.asarray([offset[0], offset[1], offset[0], offset[1]], np.float32).reshape(1, 4)
    return (q + off).astype(np.float32)


def merge(boxes, scores, ctr, labels, counts, rows_per_image, img_shapes, scale_factors, offsets, edge_masks, edge_margin=0.0):
    """lists over rows ([cap_r, ...] arrays) -> per image (boxes [n, 4], scores [n], ctr [n], labels [n], dropped): the kept
    candidates of the image's rows in row order, inside a row in candidate order"""
    out, r = [], 0
    for nr in rows_per_image:
        parts, dropped = [[], [], [], []], 0
        for r in range(r, r + nr):
            cap = len(np.asarray(scores[r]).reshape(-1))
            n = min(max(int(counts[r]), 0), cap)
            bx = np.asarray(boxes[r], np.float32).reshape(-1, 4)[:n]
            k = keep_mask(bx, img_shapes[r], int(edge_masks[r]), edge_margin)
            dropped += int(n - k.sum())
            parts[0].append(map_back(bx[k], scale_factors[r], offsets[r]))
            for j, src in enumerate((scores, ctr, labels), 1):
                parts[j].append(np.asarray(src[r]).reshape(-1)[:n][k])
        r += 1
        out.append(tuple(np.concatenate(p) for p in parts) + (dropped,))
    return out
