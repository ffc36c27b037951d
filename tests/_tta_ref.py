"""NumPy restatement of the test-time-augmentation merge (radet_merge_views): the reference's bbox_mapping_back in float32,
every operation rounded once, and the per-image concatenation in view order."""
import numpy as np

CODES = {None: 0, "horizontal": 1, "vertical": 2, "diagonal": 3}


def map_back(boxes, img_shape, scale_factor, flip):
    """boxes f32 [n, 4] in view coordinates -> the frame's: bbox_flip inside img_shape (h, w), then / scale_factor [4];
    flip: a code 0..3 or None / a direction"""
    code = flip if isinstance(flip, (int, np.integer)) else CODES[flip]
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    h, w = np.float32(img_shape[0]), np.float32(img_shape[1])
    out = b.copy()
    if code & 1:
        out[:, 0], out[:, 2] = w - b[:, 2], w - b[:, 0]
    if code & 2:
        out[:, 1], out[:, 3] = h - b[:, 3], h - b[:, 1]
    return (out / np.asarray(scale_factor, np.float32).reshape(1, 4)).astype(np.float32)


def merge(boxes, scores, ctr, labels, counts, img_shapes, scale_factors, flips):
    """lists over views ([B, cap_v, ...] arrays, counts [B]) -> per image (boxes [n, 4], scores [n], ctr [n], labels [n]):
    view 0's valid candidates, then view 1's, ..."""
    V, B = len(boxes), len(counts[0])
    out = []
    for b in range(B):
        parts = [[], [], [], []]
        for v in range(V):
            n = int(counts[v][b])
            parts[0].append(map_back(boxes[v][b][:n], img_shapes[v][b], scale_factors[v][b], flips[v]))
            for k, src in enumerate((scores, ctr, labels), 1):
                parts[k].append(np.asarray(src[v][b][:n]))
        out.append(tuple(np.concatenate(p) for p in parts))
    return out
