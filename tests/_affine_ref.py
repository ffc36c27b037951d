"""What the affine-augmentation tests share, in NumPy only: cv2.warpAffine (INTER_LINEAR, BORDER_CONSTANT, output size =
input size) restated in the integer arithmetic of OpenCV's classic fixed-point path (imgwarp.cpp), the three matrices mmcv
hands to it, and the staged host restatement of a pipeline sample (resize, warp, background, flip, Normalize, assigner)."""
import math

import numpy as np

AB = 1024


def rotation_matrix(center, angle, scale):
    """cv2.getRotationMatrix2D"""
    a = math.radians(angle)
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = float(center[0]), float(center[1])
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], np.float64)


def shear_matrix(magnitude, direction="horizontal"):
    """mmcv.imshear's float32 matrix, widened"""
    m = np.float32([[1, magnitude, 0], [0, 1, 0]]) if direction == "horizontal" else np.float32([[1, 0, 0], [magnitude, 1, 0]])
    return m.astype(np.float64)


def translate_matrix(offset, direction="horizontal"):
    """mmcv.imtranslate's float32 matrix, widened"""
    m = np.float32([[1, 0, offset], [0, 1, 0]]) if direction == "horizontal" else np.float32([[1, 0, 0], [0, 1, offset]])
    return m.astype(np.float64)


def invert(M):
    """the inverse as cv2.warpAffine forms it (without WARP_INVERSE_MAP): float64, its operation order"""
    m = np.array(M, np.float64).reshape(6)
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def tables(M_forward, h, w):
    """(X, Y) int64 [h, w]: the source coordinates in 1/32 pixel (sx = X >> 5, fx = X & 31)"""
    m = invert(M_forward)
    y, x = np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64)
    X0 = np.rint((m[1] * y + m[2]) * AB).astype(np.int64) + 16             # (np.rint: half to even, like cvRound)
    Y0 = np.rint((m[4] * y + m[5]) * AB).astype(np.int64) + 16
    adelta, bdelta = np.rint(m[0] * x * AB).astype(np.int64), np.rint(m[3] * x * AB).astype(np.int64)
    return (X0[:, None] + adelta[None, :]) >> 5, (Y0[:, None] + bdelta[None, :]) >> 5


def warp_affine_u8(img, M_forward, fill):
    """img u8 [h, w] or [h, w, c]; fill: one byte per channel (a number for one channel)"""
    a = img.reshape(*img.shape[:2], -1)
    h, w, c = a.shape
    fill = np.broadcast_to(np.asarray(fill, np.int64).reshape(-1), (c,))
    X, Y = tables(M_forward, h, w)
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    acc = np.zeros((h, w, c), np.int64)
    for dy, dx, wgt in ((0, 0, (32 - fx) * (32 - fy)), (0, 1, fx * (32 - fy)), (1, 0, (32 - fx) * fy), (1, 1, fx * fy)):
        yy, xx = sy + dy, sx + dx
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        tap = np.where(inside[..., None], a[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64), fill[None, None, :])
        acc += wgt[..., None] * tap
    return ((acc + 512) >> 10).astype(np.uint8).reshape(img.shape)


def warp_masks(masks, M_forward):
    """u8 [G, h, w] -> the same, each mask warped as one channel with fill 0"""
    return np.stack([warp_affine_u8(m, M_forward, 0) for m in masks]) if len(masks) else masks.copy()


# ------------------------------------------------------------------------------------------------ boxes
def _extent(xs, ys, h, w):
    x0, y0 = np.clip(xs.min(axis=-1), 0, w), np.clip(ys.min(axis=-1), 0, h)
    x1, y1 = np.clip(xs.max(axis=-1), x0, w), np.clip(ys.max(axis=-1), y0, h)
    return np.stack([x0, y0, x1, y1], axis=-1)


def move_boxes(boxes, kind, value, h, w, M=None, direction="horizontal"):
    """float32 [n, 4] boxes under one fired stage, in the reference's dtypes: Rotate -- the float64 matrix M times the
    homogeneous corners; Shear -- a float32 2 x 2 matrix times the corners; both: the extent of the moved corners clipped
    to the image; Translate -- a shift along one axis cut at the border"""
    x0, y0, x1, y1 = (boxes[:, k:k + 1] for k in range(4))
    if kind == "Translate":
        if direction == "horizontal":
            x0, x1 = np.maximum(0, x0 + value), np.minimum(w, x1 + value)
        else:
            y0, y1 = np.maximum(0, y0 + value), np.minimum(h, y1 + value)
        return np.concatenate([x0, y0, x1, y1], axis=-1)
    corners = np.stack([[x0, y0], [x1, y0], [x0, y1], [x1, y1]])                      # [4, 2, n, 1]
    if kind == "Rotate":
        c = np.concatenate((corners, np.ones((4, 1, len(boxes), 1), corners.dtype)), axis=1).transpose((2, 0, 1, 3))
        moved = np.matmul(M, c)[..., 0]
        return _extent(moved[:, :, 0], moved[:, :, 1], h, w).astype(boxes.dtype)
    m22 = np.stack([[1, value], [0, 1]] if direction == "horizontal" else [[1, 0], [value, 1]]).astype(np.float32)
    moved = np.matmul(m22[None], corners[..., 0].transpose((2, 1, 0)).astype(np.float32))
    return _extent(moved[:, 0, :], moved[:, 1, :], h, w).astype(boxes.dtype)


def valid_boxes(boxes, min_size=0):
    return np.nonzero((boxes[:, 2] - boxes[:, 0] > min_size) & (boxes[:, 3] - boxes[:, 1] > min_size))[0]


# ------------------------------------------------------------------------------------------------ a pipeline sample, staged
def host_chain(img_bgr, masks, boxes, labels, s, out_hw, stages, norm, assigner_rng, pad_divisor=16):
    """The reference's order for one sample, every stage materialised on the host from the draws its plan `s` recorded:
    Resize (oracle.imgproc.resize_linear_u8 / nearest masks), the fired affine stages (warp of the frame with the stage's
    fill and of the masks with 0, boxes moved and filtered), RandomBackground, CosyPoseAug, RandomFlip, the assigner on the
    flipped masks, Normalize, Pad.  stages: kind -> the stage's config (direction, min_size).  Returns the expected outputs
    and what happened (`kinds`)."""
    import _augment_ref as R
    from oracle import assigner as oa, imgproc, masks as om
    h, w = out_hw
    h0, w0 = img_bgr.shape[:2]
    sf = np.array([w / w0, h / h0, w / w0, h / h0], np.float32)
    boxes = boxes.astype(np.float32) * sf
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, w)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, h)
    x = imgproc.resize_linear_u8(np.ascontiguousarray(img_bgr), (w, h))
    m = om.resize_nearest(om.normalize(masks), (h, w))
    kinds = set()
    for (M, fill), (kind, value) in zip(s.get("affine", ()), s.get("affine_draws", ())):
        cfg = stages[kind]
        x = warp_affine_u8(x, M, fill)
        m = warp_masks(m, M)
        boxes = move_boxes(boxes, kind, value, h, w, M, cfg.get("direction", "horizontal"))
        keep = valid_boxes(boxes, cfg.get("min_size", 0) if kind == "Translate" else 0)
        kinds |= {"fired", kind} | ({"dropped"} if len(keep) < len(boxes) else set())
        boxes, labels, m = boxes[keep], labels[keep], m[keep]
        if (x == np.array(fill, np.uint8)).all(axis=-1).any():
            kinds.add("fill")
    if "affine" in s and len(m) and m.any():
        kinds.add("mask")
    if "background" in s:
        x = R.merge_background(x, imgproc.resize_linear_u8(np.ascontiguousarray(s["background"]), (w, h)), m)
        kinds.add("bg")
    x = np.ascontiguousarray(R.cosypose(x[..., ::-1], s.get("aug_blur"), s.get("aug_sharpness"), s.get("aug_contrast"),
                                        s.get("aug_brightness"), s.get("aug_color"))[..., ::-1])
    if s["flip"]:
        boxes = np.stack([w - boxes[:, 2], boxes[:, 1], w - boxes[:, 0], boxes[:, 3]], axis=1)
        x, m = np.ascontiguousarray(x[:, ::-1]), om.flip(m)
        kinds.add("flip")
    p2g, pw = oa.assign_points(boxes, labels, np.ascontiguousarray(m), (h, w, 3), rng=assigner_rng)
    Hp, Wp = -(-h // pad_divisor) * pad_divisor, -(-w // pad_divisor) * pad_divisor
    out = np.zeros((3, Hp, Wp), np.float32)
    out[:, :h, :w] = R.normalize(x, norm["mean"], norm["std"])
    return dict(img=out, gt_bboxes=boxes, gt_labels=labels, p2g=p2g, pw=pw, kinds=kinds)
