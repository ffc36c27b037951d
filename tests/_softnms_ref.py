"""NumPy restatements of Soft-NMS as mmcv 1.3.18's softnms_cpu computes it behind batched_nms (include/radet_hip.h,
"Soft-NMS").  All arithmetic is fp32 and unfused; the gaussian weight is exp in double of the fp32 argument, rounded once.
mmcv itself is not available to the tests, so these functions ARE the pinned behaviour."""
import numpy as np

METHODS = dict(naive=0, linear=1, gaussian=2)
f32 = np.float32


def _weight(ovr, method, thr, sigma):
    """fp32 weight(s) of fp32 ovr (scalar or array); NaN ovr -> 1"""
    ovr = np.asarray(ovr, f32)
    one = f32(1.0)
    with np.errstate(invalid="ignore"):
        if method == 2:
            arg = (-(ovr * ovr) / f32(sigma)).astype(f32)
            w = np.exp(arg.astype(np.float64)).astype(f32)
            return np.where(np.isnan(ovr), one, w).astype(f32)
        hit = ovr >= f32(thr)
        if method == 1:
            return np.where(hit, one - ovr, one).astype(f32)
        return np.where(hit, f32(0.0), one).astype(f32)


def soft_nms_literal(boxes, scores, method, thr, sigma, min_score):
    """mmcv's loops with its swaps, scalar fp32 (softnms_cpu, offset 0): the maximum is searched with a strict >, the
    picked box is swapped to position i, a pruned box is swapped with the last one.  The NaN rule is this project's.
    -> (keep i64 [k], decayed scores f32 [k])"""
    b = np.array(boxes, f32).reshape(-1, 4).copy()
    x1, y1, x2, y2 = b[:, 0].copy(), b[:, 1].copy(), b[:, 2].copy(), b[:, 3].copy()
    sc = np.array(scores, f32).reshape(-1).copy()
    areas = ((x2 - x1) * (y2 - y1)).astype(f32)
    inds = np.arange(len(sc), dtype=np.int64)
    nboxes = len(sc)
    i = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        while i < nboxes:
            max_pos = i
            for pos in range(i + 1, nboxes):
                if sc[pos] > sc[max_pos]:
                    max_pos = pos
            for a in (x1, y1, x2, y2, sc, areas, inds):
                a[i], a[max_pos] = a[max_pos], a[i]
            pos = i + 1
            while pos < nboxes:
                xx1, yy1 = max(x1[i], x1[pos]), max(y1[i], y1[pos])
                xx2, yy2 = min(x2[i], x2[pos]), min(y2[i], y2[pos])
                w, h = max(f32(0.0), f32(xx2 - xx1)), max(f32(0.0), f32(yy2 - yy1))
                inter = f32(w * h)
                ovr = f32(inter / f32(f32(areas[i] + areas[pos]) - inter))
                sc[pos] = f32(sc[pos] * _weight(ovr, method, thr, sigma))
                if sc[pos] < f32(min_score):
                    for a in (x1, y1, x2, y2, sc, areas, inds):
                        a[pos] = a[nboxes - 1]
                    nboxes -= 1
                    pos -= 1
                pos += 1
            i += 1
    return inds[:nboxes].copy(), sc[:nboxes].copy()


def soft_nms_fast(boxes, scores, method, thr, sigma, min_score, max_out=None):
    """One vectorised fp32 step per pick: highest current score among the boxes neither picked nor pruned, ties to the
    lowest input index.  -> (keep i64 [k], decayed scores f32 [k]), the first max_out of the sequence"""
    b = np.array(boxes, f32).reshape(-1, 4)
    sc = np.array(scores, f32).reshape(-1).copy()
    n = len(sc)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    areas = ((x2 - x1) * (y2 - y1)).astype(f32)
    alive = np.ones(n, bool)
    keep, out = [], []
    lim = n if max_out is None else min(n, max_out)
    with np.errstate(invalid="ignore", divide="ignore"):
        while len(keep) < lim and alive.any():
            cand = np.where(alive, sc, -np.inf)
            i = int(np.argmax(cand))                       # first maximum = lowest index
            if not alive[i]:                               # only -inf scores left: lowest alive index
                i = int(np.flatnonzero(alive)[0])
            keep.append(i)
            out.append(sc[i])
            alive[i] = False
            w = np.maximum(f32(0.0), np.minimum(x2[i], x2) - np.maximum(x1[i], x1)).astype(f32)
            h = np.maximum(f32(0.0), np.minimum(y2[i], y2) - np.maximum(y1[i], y1)).astype(f32)
            inter = (w * h).astype(f32)
            ovr = (inter / ((areas[i] + areas).astype(f32) - inter)).astype(f32)
            new = (sc * _weight(ovr, method, thr, sigma)).astype(f32)
            sc = np.where(alive, new, sc)
            alive &= ~(sc < f32(min_score))
    return np.array(keep, np.int64), np.array(out, f32)


def offset_boxes(boxes, labels, class_agnostic=False):
    """batched_nms' fp32 class offset: box + float(label) * (largest coordinate + 1)"""
    b = np.array(boxes, f32).reshape(-1, 4)
    if class_agnostic or not len(b):
        return b
    unit = f32(b.max() + f32(1.0))
    return (b + (np.asarray(labels).astype(f32) * unit).astype(f32)[:, None]).astype(f32)


def batched_soft_nms(boxes, scores, labels, method, thr, sigma, min_score, class_agnostic=False, max_out=None,
                     loop=soft_nms_fast):
    """the global loop over the class-offset boxes -> (keep, decayed scores); boxes[keep] are the original ones"""
    ob = offset_boxes(boxes, labels, class_agnostic)
    if loop is soft_nms_fast:
        return loop(ob, scores, method, thr, sigma, min_score, max_out)
    keep, sc = loop(ob, scores, method, thr, sigma, min_score)
    return (keep, sc) if max_out is None else (keep[:max_out], sc[:max_out])


def per_class_soft_nms(boxes, scores, labels, method, thr, sigma, min_score):
    """The per-class decomposition: the loop per label segment, the outputs merged by (score descending, input index
    ascending), everything after the first element cut below min_score (a segment on its own keeps its first pick even
    below min_score; the global loop would have pruned it)."""
    ob = offset_boxes(boxes, labels)
    labels = np.asarray(labels)
    scores = np.asarray(scores, f32)
    ks, ss = [], []
    for c in np.unique(labels):
        idx = np.flatnonzero(labels == c)
        k, s = soft_nms_fast(ob[idx], scores[idx], method, thr, sigma, min_score)
        ks.append(idx[k])
        ss.append(s)
    if not ks:
        return np.zeros(0, np.int64), np.zeros(0, f32)
    k, s = np.concatenate(ks), np.concatenate(ss)
    order = np.lexsort((k, -s.astype(np.float64)))
    k, s = k[order], s[order]
    ok = np.ones(len(k), bool)
    ok[1:] = ~(s[1:] < f32(min_score))
    return k[ok], s[ok]
