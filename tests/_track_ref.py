"""The tracking rules of include/radet_hip.h (radet_track_update) as plain NumPy loops on np.float32, one operation per line:
what csrc/track.hip is pinned to bit for bit (tests/test_gpu_track.py) and what tests/test_track_cpu.py checks against
hand-worked expectations.  One state is one sequence; nothing here is fast."""
import numpy as np

MAX_TRACKS = 256
F = np.float32
DEFAULTS = dict(iou_thr=0.3, track_thr=0.3, new_thr=0.5, max_age=5, max_tracks=256, motion="constant", class_aware=True)


def new_state():
    """the empty tracker: everything zero"""
    return dict(box=np.zeros((MAX_TRACKS, 4), F), vel=np.zeros((MAX_TRACKS, 4), F), label=np.zeros(MAX_TRACKS, np.int32),
                id=np.zeros(MAX_TRACKS, np.int32), misses=np.zeros(MAX_TRACKS, np.int32), hits=np.zeros(MAX_TRACKS, np.int32),
                score=np.zeros(MAX_TRACKS, F), next_id=0, frames=0, refused=0)


def _min(a, b):
    return a if a < b else b


def _max(a, b):
    return a if a > b else b


def _area(b):
    w = F(b[2] - b[0])
    h = F(b[3] - b[1])
    return F(w * h)


def _iou(a, b):
    iw = F(_min(a[2], b[2]) - _max(a[0], b[0]))
    iw = _max(iw, F(0))
    ih = F(_min(a[3], b[3]) - _max(a[1], b[1]))
    ih = _max(ih, F(0))
    inter = F(iw * ih)
    total = F(_area(a) + _area(b))
    union = F(total - inter)
    return F(inter / union)


def update_frame(st, boxes, scores, labels, iou_thr=0.3, track_thr=0.3, new_thr=0.5, max_age=5, max_tracks=256,
                 motion="constant", class_aware=True):
    """one frame: boxes [k,4], scores [k], labels [k] in rank order -> (ids i32 [k], hits i32 [k]); st is updated in place"""
    assert motion in ("constant", "none") and 1 <= max_tracks <= MAX_TRACKS
    boxes, scores = np.asarray(boxes, F).reshape(-1, 4), np.asarray(scores, F).reshape(-1)
    labels = np.asarray(labels, np.int64).reshape(-1)
    iou_thr, track_thr, new_thr = F(iou_thr), F(track_thr), F(new_thr)
    k = len(scores)
    ids, hits = np.zeros(k, np.int32), np.zeros(k, np.int32)
    with np.errstate(all="ignore"):
        # 1. predict
        pred = st["box"].copy()
        if motion == "constant":
            for s in range(MAX_TRACKS):
                for c in range(4):
                    pred[s, c] = F(st["box"][s, c] + st["vel"][s, c])
        matched = np.zeros(MAX_TRACKS, bool)
        for d in range(k):
            # 2. eligible?
            det, sc, lab = boxes[d], scores[d], int(labels[d])
            if not (np.isfinite(det).all() and np.isfinite(sc) and sc >= track_thr and 0 <= lab < 2 ** 31):
                continue
            # 3. match
            best, at = None, -1
            for s in range(max_tracks):
                if st["id"][s] == 0 or matched[s] or (class_aware and int(st["label"][s]) != lab):
                    continue
                iou = _iou(pred[s], det)
                if iou >= iou_thr and (best is None or iou > best):          # (a NaN compares false; ties stay with the lower slot)
                    best, at = iou, s
            if at >= 0:
                if motion == "constant":
                    for c in range(4):
                        st["vel"][at, c] = F(det[c] - st["box"][at, c])
                st["box"][at] = det
                st["score"][at] = sc
                st["misses"][at] = 0
                st["hits"][at] += 1
                matched[at] = True
                ids[d], hits[d] = st["id"][at], st["hits"][at]
                continue
            # 4. start a track
            if not sc >= new_thr:
                continue
            free = [s for s in range(max_tracks) if st["id"][s] == 0]
            if not free:
                st["refused"] += 1
                continue
            s = free[0]
            st["next_id"] += 1
            st["id"][s] = st["next_id"]
            st["box"][s] = det
            st["vel"][s] = 0
            st["label"][s] = lab
            st["score"][s] = sc
            st["hits"][s] = 1
            st["misses"][s] = 0
            matched[s] = True
            ids[d], hits[d] = st["id"][s], 1
        # 5. age
        for s in range(MAX_TRACKS):
            if st["id"][s] != 0 and not matched[s]:
                st["misses"][s] += 1
                if st["misses"][s] > max_age:
                    st["id"][s] = 0
                else:
                    st["box"][s] = pred[s]
    st["frames"] += 1                                                            # 6.
    return ids, hits


def update(st, frames, **params):
    """frames: list of (dets [k,5], labels [k]) -> list of (ids, hits)"""
    out = []
    for dets, labels in frames:
        dets = np.asarray(dets, F).reshape(-1, 5)
        out.append(update_frame(st, dets[:, :4], dets[:, 4], labels, **params))
    return out


def live(st):
    """the live tracks, by slot"""
    at = np.nonzero(st["id"])[0]
    return dict(slots=at, ids=st["id"][at], boxes=st["box"][at], labels=st["label"][at], misses=st["misses"][at],
                hits=st["hits"][at], scores=st["score"][at])
