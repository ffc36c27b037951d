"""Test-time augmentation, stand-alone: the candidate lists of several views of one batch mapped back to the frames and packed
per image (radet_merge_views, csrc/tta.hip) -- the step DetectorRuntime.detect_aug runs between the views' decode launches and
the one NMS over their union."""
import numpy as np
import torch

from .. import kernels as K
from . import _dev, _t, _upload


def merge_view_candidates(boxes, scores, ctr, labels, counts, img_shapes, scale_factors, flips):
    """Lists over V views of one batch of B images, as radet_decode_candidates writes them in view coordinates:
    boxes[v] f32 [B, cap_v, 4], scores[v] / ctr[v] f32 [B, cap_v], labels[v] i64 [B, cap_v], counts[v] i32 [B] -- the
    capacities may differ from view to view; img_shapes[v][b] = (h, w, ...) and scale_factors[v][b] = 4 floats of the view's
    image b; flips[v] = None | 'horizontal' | 'vertical' | 'diagonal' (or the codes 0..3).
    -> (boxes f32 [B, cap_out, 4], scores, ctr f32 [B, cap_out], labels i64 [B, cap_out], counts i32 [B]) on the device,
    cap_out = sum of the capacities: per image view 0's valid candidates, then view 1's, ... in their order, nothing
    dropped; boxes are the reference's bbox_mapping_back (flip inside the view's img_shape, then the division by the scale
    factor, fp32, each operation rounded once).  Slots at and beyond counts[b] are unspecified.  One launch, no host
    synchronisation."""
    V = len(boxes)
    if not (V == len(scores) == len(ctr) == len(labels) == len(counts) == len(img_shapes) == len(scale_factors) == len(flips)):
        raise ValueError("merge_view_candidates: every argument is a list over the views")
    if not 1 <= V <= K.TTA_MAX_VIEWS:
        raise ValueError(f"merge_view_candidates: {V} views (1..{K.TTA_MAX_VIEWS})")
    dev = _dev()
    bx = [_t(b, torch.float32) for b in boxes]
    B = int(bx[0].shape[0])
    caps = [int(b.shape[1]) for b in bx]
    for v in range(V):
        if tuple(bx[v].shape) != (B, caps[v], 4) or len(img_shapes[v]) != B or len(scale_factors[v]) != B:
            raise ValueError(f"merge_view_candidates: view {v} does not hold {B} images")
    cap_out = sum(caps)
    hw = np.array([[s[0], s[1]] for view in img_shapes for s in view], np.float32).reshape(V * B, 2)
    sf = np.array([np.asarray(f, np.float32).reshape(4) for view in scale_factors for f in view], np.float32).reshape(V * B, 4)
    codes = [f if isinstance(f, (int, np.integer)) else K.FLIP_CODES[f] for f in flips]
    offs = np.concatenate([[0], np.cumsum([B * c for c in caps])]).astype(np.int64)
    starts = np.concatenate([offs[v] + np.arange(B) * caps[v] for v in range(V)])
    desc = K.merge_desc_rows(hw, sf, np.repeat(np.asarray(codes, np.int32), B), starts, np.repeat(np.asarray(caps, np.int32), B))

    def pool(ts, dtype, width=()):
        return torch.cat([_t(t, dtype).reshape(-1, *width) for t in ts])
    ob = torch.empty(B, cap_out, 4, device=dev)
    osc, oct_ = torch.empty(B, cap_out, device=dev), torch.empty(B, cap_out, device=dev)
    ol = torch.empty(B, cap_out, dtype=torch.long, device=dev)
    oc = torch.zeros(B, dtype=torch.int32, device=dev)
    K.merge_views(desc, _upload(desc, dev), V, B, torch.cat([b.reshape(-1, 4) for b in bx]), pool(scores, torch.float32),
                  pool(ctr, torch.float32), pool(labels, torch.long), pool(counts, torch.int32), cap_out, ob, osc, oct_, ol, oc)
    return ob, osc, oct_, ol, oc
