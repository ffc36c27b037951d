"""What the CutOut tests share, in NumPy only: the reference's CutOut (transforms.py:1734-1804) restated -- the holes from
the recorded randint draws, the slice assignment -- and the staged host restatement of a pipeline sample with CutOut
entries in the block after Resize and behind the photometric stages."""
import numpy as np


def holes_from_draws(draws, candidates, with_ratio, h, w):
    """draws: what the stage's randint calls returned, in order: the hole count n, then per hole x1, y1 and the candidate's
    index -> int64 [n, 4] rows {x1, y1, x2, y2}"""
    draws = [int(v) for v in draws]
    n = draws[0]
    assert len(draws) == 1 + 3 * n
    rects = np.zeros((n, 4), np.int64)
    for k in range(n):
        x1, y1, idx = draws[1 + 3 * k:4 + 3 * k]
        cw, ch = candidates[idx]
        if with_ratio:
            cw, ch = int(cw * w), int(ch * h)
        rects[k] = [x1, y1, min(max(x1 + cw, 0), w), min(max(y1 + ch, 0), h)]
    return rects


def apply_holes(img, rects, fill):
    """a copy of img (u8 or f32 [h, w, c]) with img[y1:y2, x1:x2] = fill per row of rects (clipped to the image; Python's
    slices of a rectangle without area store nothing)"""
    out = img.copy()
    h, w = img.shape[:2]
    for x1, y1, x2, y2 in np.asarray(rects, np.int64).reshape(-1, 4):
        x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, w), min(y2, h)
        if x2 > x1 and y2 > y1:
            out[y1:y2, x1:x2] = fill
    return out


def hole_mask(rects, h, w, flip=False):
    """bool [h, w]: the pixels some hole covers (mirrored columns for a flipped sample)"""
    m = apply_holes(np.zeros((h, w, 1), np.uint8), rects, 1)[..., 0].astype(bool)
    return m[:, ::-1] if flip else m


U8_GUARD = 0xAB
U8_MAX_HOLES = 64
U8_SIZES = [(1, 1), (1, 257), (255, 1), (3, 5), (48, 64), (300, 200)]


def u8_kernel_cases():
    """The batch radet_cutout_u8 is tested on: the images of U8_SIZES, per image (holes or None, fill, skip), pixel offsets
    with 3 * offset never a multiple of 4, the packed buffer with canary bytes between the images, and the expected buffer"""
    rs = np.random.RandomState(0)
    frames = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in U8_SIZES]
    many = np.stack([rs.randint(-20, 200, U8_MAX_HOLES - 2), rs.randint(-20, 300, U8_MAX_HOLES - 2)], 1)
    many = np.concatenate([many, many + rs.randint(1, 60, (U8_MAX_HOLES - 2, 2))], 1)
    many = np.concatenate([many, [[150, 250, 260, 400], [-10, -10, 30, 20]]])                 # + clipped at both borders, both ways
    rows = [
        (np.array([[0, 0, 1, 1]]), (1, 2, 3), False),                                          # 1 x 1: the hole covers the image
        (np.array([[200, 0, 400, 9], [-7, -3, 4, 1]]), (0, 37, 255), False),                   # 1 x 257: clipped at both borders
        (np.array([[0, 5, 0, 9], [0, 7, 1, 7], [1, 9, 0, 3], [0, 250, 1, 300]]), (255, 255, 255), False),     # 255 x 1: no area; the bottom
        (None, (9, 9, 9), False),                                                              # 3 x 5: no holes
        (np.array([[3, 3, 40, 30]]), (7, 7, 7), True),                                         # 48 x 64: a skip row
        (many, (200, 100, 50), False),                                                         # 300 x 200: 64 overlapping holes
    ]
    offs, o = [], 3
    for f in frames:
        offs.append(o)
        o += f.shape[0] * f.shape[1] + 5
        o += o % 4 == 0
    assert all(3 * v % 4 for v in offs)
    packed = np.full(o * 3, U8_GUARD, np.uint8)
    want = packed.copy()
    for f, off, (holes, fill, skip) in zip(frames, offs, rows):
        packed[off * 3:off * 3 + f.size] = f.reshape(-1)
        out = f if holes is None or skip else apply_holes(f, holes, np.array(fill, np.uint8))
        want[off * 3:off * 3 + f.size] = out.reshape(-1)
    return frames, rows, offs, packed, want


def host_chain(img_bgr, masks, boxes, labels, s, out_hw, stages, norm, assigner_rng, pad_hw=None, pad_divisor=16, window=None):
    """The reference's order for one sample, every stage materialised on the host from the draws its plan `s` recorded: Resize,
    the RandomCrop window (window: (y0, x0, h, w) of the resized image), the block's entries in the order they ran -- a warp
    moves frame, masks and boxes (_affine_ref), a CutOut fills its holes in the frame only --, RandomBackground,
    CosyPoseAug, the late CutOut (on the blended u8 frame, where the reference's stage order puts it), RandomFlip, the
    assigner on the flipped masks (padded to pad_hw with Pad(size=)), Normalize, Pad.  stages: kind -> the warp stage's
    config.  Returns the expected outputs, what happened (`kinds`), and the u8 BGR frame (`u8`) and the masks as they are
    behind the flip: what GenerateDistanceMap and the assigner read."""
    import _affine_ref as A
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
    if window is not None:
        y0, x0, h, w = window
        x, m = np.ascontiguousarray(x[y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(m[:, y0:y0 + h, x0:x0 + w])
        b = boxes - np.array([x0, y0, x0, y0], np.float32)
        b[:, 0::2] = np.clip(b[:, 0::2], 0, w)
        b[:, 1::2] = np.clip(b[:, 1::2], 0, h)
        keep = np.nonzero((b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1]))[0]
        boxes, labels, m = b[keep], labels[keep], m[keep]
        kinds.add("window")
    ops = s.get("block_ops", [("warp", k) for k in range(len(s.get("affine", ())))])
    for kind, k in ops:
        if kind == "cutout":
            rects, fill = s["cutout"][k]
            before = x
            x = apply_holes(x, rects, np.array(fill, np.uint8))
            kinds |= {"cutout"} | ({"after-warp"} if "fired" in kinds else set()) | ({"holes"} if not np.array_equal(x, before) else set())
            continue
        (M, fill), (name, value) = s["affine"][k], s["affine_draws"][k]
        cfg = stages[name]
        x = A.warp_affine_u8(x, M, fill)
        m = A.warp_masks(m, M)
        boxes = A.move_boxes(boxes, name, value, h, w, M, cfg.get("direction", "horizontal"))
        keep = A.valid_boxes(boxes, cfg.get("min_size", 0) if name == "Translate" else 0)
        kinds |= {"fired", name} | ({"warp-after-cutout"} if "cutout" in kinds else set())
        boxes, labels, m = boxes[keep], labels[keep], m[keep]
    if "background" in s:
        x = R.merge_background(x, imgproc.resize_linear_u8(np.ascontiguousarray(s["background"]), (w, h)), m)
        kinds.add("bg")
    x = np.ascontiguousarray(R.cosypose(x[..., ::-1], s.get("aug_blur"), s.get("aug_sharpness"), s.get("aug_contrast"),
                                        s.get("aug_brightness"), s.get("aug_color"))[..., ::-1])
    if any(key in s for key in ("aug_blur", "aug_sharpness", "aug_contrast", "aug_brightness", "aug_color")):
        kinds.add("cosy")
    if "cutout_late" in s:
        rects, fill = s["cutout_late"]
        before = x
        x = apply_holes(x, rects, np.array(fill, np.uint8))
        kinds |= {"late"} | ({"late-holes"} if not np.array_equal(x, before) else set())
    if s["flip"]:
        boxes = np.stack([w - boxes[:, 2], boxes[:, 1], w - boxes[:, 0], boxes[:, 3]], axis=1)
        x, m = np.ascontiguousarray(x[:, ::-1]), om.flip(m)
        kinds.add("flip")
    Hp, Wp = pad_hw if pad_hw is not None else (-(-h // pad_divisor) * pad_divisor, -(-w // pad_divisor) * pad_divisor)
    ah, aw = (Hp, Wp) if pad_hw is not None else (h, w)
    p2g, pw = oa.assign_points(boxes, labels, np.ascontiguousarray(om.pad(m, (ah, aw), 0)), (ah, aw, 3), rng=assigner_rng)
    out = np.zeros((3, Hp, Wp), np.float32)
    out[:, :h, :w] = R.normalize(x, norm["mean"], norm["std"], norm.get("to_rgb", True))
    return dict(img=out, gt_bboxes=boxes, gt_labels=labels, p2g=p2g, pw=pw, kinds=kinds, u8=np.ascontiguousarray(x), masks=m)
