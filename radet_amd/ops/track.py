"""Detections tracked across frames on the device (radet_amd/csrc/track.hip): which detection of frame t is the object of which
detection of frame t - 1.  `Tracker` holds the state of one or several sequences (cameras) on the device and takes one batch
of consecutive frames per `update`, ONE launch that reads nothing back; `track_detections` is the stand-alone form for a
recorded sequence; `apis.track_frames` runs the same launch behind `detect_frames`.

The rules are this project's own (include/radet_hip.h, radet_track_update; the reference has no tracker, parity is
unpinned), pinned bit for bit to the NumPy restatement tests/_track_ref.py: greedy IoU association in rank order against a
constant-velocity prediction, tracks born above new_thr, coasting through up to max_age missed frames.  The defaults are a
starting point; nobody has evaluated them on video data."""
import math
import numbers
from collections import namedtuple

import numpy as np
import torch

from .. import kernels as K
from .draw import pad_detections

TrackSpec = namedtuple("TrackSpec", "iou_thr track_thr new_thr max_age max_tracks motion class_aware")
TrackSpec.__doc__ = """the checked parameters of a tracker (motion: the kernel's code)"""

_WORDS = K.TRACK_STATE_BYTES // 4
_T = K.TRACK_MAX_TRACKS


def track_params(iou_thr=0.3, track_thr=0.3, new_thr=0.5, max_age=5, max_tracks=K.TRACK_MAX_TRACKS, motion="constant",
                 class_aware=True):
    """the checked parameters (needs no device): a detection of score >= track_thr may continue a track whose predicted box
    it overlaps with IoU >= iou_thr, one of score >= new_thr may start one; a track is dropped after more than max_age
    consecutive frames without a detection; motion 'constant' predicts box + last displacement, 'none' the last box;
    class_aware: only equal labels match.  At most max_tracks (<= 256) tracks live at a time."""
    def _int(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool)

    def _real(v):
        return isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v)
    if not _real(iou_thr) or not 0 < np.float32(iou_thr) <= 1:
        raise ValueError(f"track: iou_thr={iou_thr!r} is not in (0, 1]")
    if not _real(track_thr) or not np.isfinite(np.float32(track_thr)):
        raise ValueError(f"track: track_thr={track_thr!r} is not a finite number")
    if not _real(new_thr) or not np.isfinite(np.float32(new_thr)):
        raise ValueError(f"track: new_thr={new_thr!r} is not a finite number")
    if not _int(max_age) or not 0 <= max_age < 2 ** 31:
        raise ValueError(f"track: max_age={max_age!r} is not an int >= 0")
    if not _int(max_tracks) or not 1 <= max_tracks <= _T:
        raise ValueError(f"track: max_tracks={max_tracks!r} is not an int in [1, {_T}]")
    if not isinstance(motion, str) or motion not in K.TRACK_MOTIONS:
        raise ValueError(f"track: motion={motion!r}: expected one of {sorted(K.TRACK_MOTIONS)}")
    if not isinstance(class_aware, (bool, np.bool_)):
        raise ValueError(f"track: class_aware={class_aware!r} is not a bool")
    return TrackSpec(float(iou_thr), float(track_thr), float(new_thr), int(max_age), int(max_tracks), K.TRACK_MOTIONS[motion],
                     bool(class_aware))


def unpack_state(words):
    """one sequence's state, i32 [TRACK_STATE_BYTES / 4] on the host -> dict(box f32 [256,4], vel f32 [256,4], label, id,
    misses, hits i32 [256], score f32 [256], next_id, frames, refused): the layout of include/radet_hip.h"""
    w = np.ascontiguousarray(words, dtype=np.int32).reshape(_WORDS)
    n = 4 * _T
    return dict(box=w[:n].view(np.float32).reshape(_T, 4).copy(), vel=w[n:2 * n].view(np.float32).reshape(_T, 4).copy(),
                label=w[2 * n:2 * n + _T].copy(), id=w[2 * n + _T:2 * n + 2 * _T].copy(),
                misses=w[2 * n + 2 * _T:2 * n + 3 * _T].copy(), hits=w[2 * n + 3 * _T:2 * n + 4 * _T].copy(),
                score=w[2 * n + 4 * _T:2 * n + 5 * _T].view(np.float32).copy(), next_id=int(w[2 * n + 5 * _T]),
                frames=int(w[2 * n + 5 * _T + 1]), refused=int(w[2 * n + 5 * _T + 2]))


class Tracker:
    """The tracks of `sequences` independent frame sequences (cameras) on a device.  update() is one launch on the current
    stream and reads nothing back; tracks() is the deliberate host read.  **params: track_params' arguments."""

    def __init__(self, sequences=1, device=None, **params):
        self.spec = track_params(**params)
        if not isinstance(sequences, numbers.Integral) or isinstance(sequences, bool) or sequences < 1:
            raise ValueError(f"track: sequences={sequences!r} is not an int >= 1")
        self.sequences = int(sequences)
        if device is None:
            from . import _dev
            device = _dev()
        self.dev = torch.device(device)
        self.state = torch.zeros(self.sequences, _WORDS, dtype=torch.int32, device=self.dev)

    def reset(self):
        """back to the empty tracker: the next id is 1 again"""
        self.state.zero_()

    def _padded(self, dets):
        if self.sequences == 1:
            return [t[None] for t in pad_detections(dets, self.dev)]
        if not isinstance(dets, (tuple, list)) or len(dets) != self.sequences:
            raise ValueError(f"track: a tracker of {self.sequences} sequences takes a list of {self.sequences} batches, one per "
                             "sequence")
        per = [pad_detections(d, self.dev) for d in dets]
        B = int(per[0][0].shape[0])
        if any(int(p[0].shape[0]) != B for p in per):
            raise ValueError(f"track: the sequences' batches hold {[int(p[0].shape[0]) for p in per]} frames; they must be equal")
        cap = max(int(p[0].shape[1]) for p in per)
        boxes = torch.zeros(self.sequences, B, cap, 4, device=self.dev)
        scores = torch.zeros(self.sequences, B, cap, device=self.dev)
        labels = torch.zeros(self.sequences, B, cap, dtype=torch.int64, device=self.dev)
        for s, (b, sc, l, _) in enumerate(per):
            boxes[s, :, :b.shape[1]], scores[s, :, :b.shape[1]], labels[s, :, :b.shape[1]] = b, sc, l
        return boxes, scores, labels, torch.stack([p[3] for p in per])

    def update(self, dets):
        """One batch of consecutive frames through the tracker: dets is per frame (dets [k,5], labels [k]) as
        detect_frames(on_device=True) yields them, or the padded (boxes [B,cap,4], scores [B,cap], labels [B,cap], counts
        [B]); with sequences > 1 a list of one such batch per sequence, all of equal length.
        -> (ids i32 [B, cap], hits i32 [B, cap]) device tensors ([sequences, B, cap] with several sequences): the track of
        every detection slot (0: none -- ineligible, below new_thr, refused, or padding) and that track's hits so far."""
        boxes, scores, labels, counts = self._padded(dets)
        nseq, B, cap = (int(v) for v in boxes.shape[:3])
        if B < 1:
            raise ValueError("track: a batch of no frames")
        if cap > K.TRACK_MAX_DETS:
            raise ValueError(f"track: {cap} detection slots per frame exceed the kernel's {K.TRACK_MAX_DETS}")
        ids = torch.empty(nseq, B, cap, dtype=torch.int32, device=self.dev)
        hits = torch.empty(nseq, B, cap, dtype=torch.int32, device=self.dev)
        K.track_update(boxes, scores, labels, counts, nseq, B, cap, self.state, *self.spec, ids, hits)
        return (ids[0], hits[0]) if self.sequences == 1 else (ids, hits)

    def host_state(self, sequence=0):
        """the whole state of one sequence on the host (unpack_state); waits for the device"""
        return unpack_state(self.state[sequence].cpu().numpy())

    def tracks(self, sequence=0):
        """A deliberate host read: the live tracks of one sequence, in slot order, as dict(ids, boxes [n,4], labels, misses,
        hits, scores, slots -- ndarrays -- and next_id, frames, refused).  Coasting tracks (misses > 0) are included with their
        predicted box, so a caller can carry an object through a missed detection."""
        st = self.host_state(sequence)
        at = np.nonzero(st["id"])[0]
        return dict(ids=st["id"][at], boxes=st["box"][at], labels=st["label"][at], misses=st["misses"][at], hits=st["hits"][at],
                    scores=st["score"][at], slots=at, next_id=st["next_id"], frames=st["frames"], refused=st["refused"])


def track_detections(per_frame_dets, **params):
    """The detections of a recorded sequence -- a list of per frame (dets [k,5], labels [k]), tensors or ndarrays, in time
    order -- tracked in ONE launch from an empty tracker.  -> the list of per-frame id arrays, i32 ndarray [k] (0: no
    track).  **params: track_params' arguments."""
    per_frame_dets = list(per_frame_dets)
    tracker = Tracker(**params)
    if not per_frame_dets:
        return []
    ids, _ = tracker.update(per_frame_dets)
    ids = ids.cpu().numpy()
    return [ids[i, :int(torch.as_tensor(d[0]).reshape(-1, 5).shape[0])].copy() for i, d in enumerate(per_frame_dets)]
