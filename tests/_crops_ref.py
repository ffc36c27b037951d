"""NumPy restatement of the RoI crops (radet_amd/csrc/crops.hip): the window rule of radet_crop_plan in float32, one rounding
per operation (NumPy's float32 scalars round after every operation, as the kernel does with its _rn intrinsics), and the
pixels as "paste the frame on a filled canvas, slice the window, resize" with the project's 8-bit INTER_LINEAR restatement
(tests/_augment_ref.resize_linear_u8), then Normalize as the frame pipeline computes it."""
import numpy as np

from _augment_ref import resize_linear_u8

ROW_INTS = 6
MAX_SIDE = 16384
F = np.float32


def _side(s):
    if not s < F(MAX_SIDE):
        return MAX_SIDE
    return max(int(np.ceil(s)), 1)


def window(box, score, size, scale, score_thr):
    """-> (wx0, wy0, ww, wh) of a valid detection, else None"""
    Ho, Wo = size
    x1, y1, x2, y2 = (F(v) for v in box)
    if not np.isfinite([x1, y1, x2, y2]).all():
        return None
    with np.errstate(over="ignore", under="ignore"):
        w, h = x2 - x1, y2 - y1
        cx, cy = (x1 + x2) * F(0.5), (y1 + y2) * F(0.5)
        if not (w > 0 and h > 0 and abs(cx) < F(2 ** 20) and abs(cy) < F(2 ** 20) and F(score) >= F(score_thr)):
            return None
        a = F(Wo) / F(Ho)
        hs = max(h, w / a) * F(scale)
        ws = hs * a
    wh, ww = _side(hs), _side(ws)
    return (int(np.floor(cx - F(0.5) * F(ww))), int(np.floor(cy - F(0.5) * F(wh))), ww, wh)


def plan(boxes, scores, counts, size, scale, score_thr, cap):
    """boxes [B,K,4], scores [B,K], counts [B] -> (rows i32 [n_out, 6] = {b, j, wx0, wy0, ww, wh}, n_out, n_total)"""
    rows = []
    for b in range(boxes.shape[0]):
        for j in range(min(int(counts[b]), boxes.shape[1])):
            win = window(boxes[b, j], scores[b, j], size, scale, score_thr)
            if win is not None:
                rows.append((b, j) + win)
    n_total = len(rows)
    n_out = min(n_total, cap)
    return np.array(rows[:n_out], np.int32).reshape(-1, ROW_INTS), n_out, n_total


def crop_u8(frame, win, size, fill):
    """the window (wx0, wy0, ww, wh) of frame u8 [h,w,3] on a canvas of `fill` (BGR), resized to size = (Ho, Wo)"""
    wx0, wy0, ww, wh = win
    canvas = np.empty((wh, ww, 3), np.uint8)
    canvas[:] = np.asarray(fill, np.uint8)
    h, w = frame.shape[:2]
    y0, y1, x0, x1 = max(wy0, 0), min(wy0 + wh, h), max(wx0, 0), min(wx0 + ww, w)
    if y1 > y0 and x1 > x0:
        canvas[y0 - wy0:y1 - wy0, x0 - wx0:x1 - wx0] = frame[y0:y1, x0:x1]
    return resize_linear_u8(canvas, size[1], size[0])


def norm_consts(mean, std):
    mean = np.asarray(mean, np.float32)
    return mean, (1.0 / np.asarray(std, np.float32).astype(np.float64)).astype(np.float32)


def crops(frames, rows, size, fill, normalize=None):
    """-> u8 [n,Ho,Wo,3] (normalize None) or f32 [n,3,Ho,Wo] = ((RGB or BGR) - mean) * f32(1 / f64(std)) in float32"""
    q = np.stack([crop_u8(frames[r[0]], tuple(r[2:6]), size, fill) for r in rows]) if len(rows) else np.zeros((0, *size, 3), np.uint8)
    if normalize is None:
        return q
    mean, stdinv = norm_consts(normalize["mean"], normalize["std"])
    q = q[..., ::-1] if normalize.get("to_rgb", True) else q
    return ((q.astype(np.float32) - mean) * stdinv).transpose(0, 3, 1, 2)
