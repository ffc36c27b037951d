"""Tracking, the host side (no GPU): the NumPy restatement of radet_track_update (tests/_track_ref.py) against hand-worked
expectations written as literals, the constants of the three declarations, and the parameter refusals of ops.track."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _track_ref as R  # noqa: E402
from radet_amd import kernels as K  # noqa: E402
from radet_amd.ops import track as T  # noqa: E402


def _frame(*dets):
    """(x1, y1, x2, y2, score, label) ... -> (dets [k,5], labels [k])"""
    a = np.array(dets, np.float64).reshape(-1, 6)
    return a[:, :5].astype(np.float32), a[:, 5].astype(np.int64)


def _ids(out):
    return [o[0].tolist() for o in out]


def test_constants_and_declarations():
    hdr = open(os.path.join(REPO, "include", "radet_hip.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert define("TRACK_MAX_TRACKS") == K.TRACK_MAX_TRACKS == R.MAX_TRACKS == 256
    assert define("TRACK_MAX_DETS") == K.TRACK_MAX_DETS >= 1024
    assert define("TRACK_STATE_BYTES") == K.TRACK_STATE_BYTES == 256 * (16 + 16 + 5 * 4) + 16
    assert K.TRACK_STATE_BYTES % 16 == 0
    assert K.TRACK_MOTIONS == dict(none=define("TRACK_MOTION_NONE"), constant=define("TRACK_MOTION_CONSTANT"))
    spec = T.track_params()
    assert spec == T.TrackSpec(0.3, 0.3, 0.5, 5, 256, 1, True)
    assert {k: (K.TRACK_MOTIONS[v] if k == "motion" else v) for k, v in R.DEFAULTS.items()} == spec._asdict()
    # the host's view of the state is the restatement's dict
    st = T.unpack_state(np.arange(K.TRACK_STATE_BYTES // 4, dtype=np.int32))
    assert set(st) == set(R.new_state())
    assert st["label"][0] == 2048 and st["id"][0] == 2304 and st["misses"][0] == 2560 and st["hits"][255] == 3071
    assert (st["next_id"], st["frames"], st["refused"]) == (3328, 3329, 3330)
    assert st["box"].view(np.int32)[1, 0] == 4 and st["vel"].view(np.int32)[0, 0] == 1024 and st["score"].view(np.int32)[0] == 3072


def test_missed_frames_coast_and_return():
    """two objects over five frames; A moves by +2 in x per frame and is missing in frames 2 and 3"""
    st = R.new_state()
    b = (100, 100, 140, 140, 0.9, 1)
    out = R.update(st, [_frame((10, 10, 30, 30, 0.9, 0), b), _frame((12, 10, 32, 30, 0.9, 0), b)])
    assert _ids(out) == [[1, 2], [1, 2]] and [o[1].tolist() for o in out] == [[1, 1], [2, 2]]
    assert st["vel"][0].tolist() == [2, 0, 2, 0] and st["vel"][1].tolist() == [0, 0, 0, 0]
    out = R.update(st, [_frame(b)])
    assert _ids(out) == [[2]] and st["box"][0].tolist() == [14, 10, 34, 30] and st["misses"][0] == 1
    out = R.update(st, [_frame(b)])
    assert _ids(out) == [[2]] and st["box"][0].tolist() == [16, 10, 36, 30] and st["misses"][0] == 2     # box + vel, twice
    assert st["vel"][0].tolist() == [2, 0, 2, 0] and st["hits"][0] == 2
    ids, hits = R.update(st, [_frame((18, 10, 38, 30, 0.9, 0), b)])[0]
    assert ids.tolist() == [1, 2] and hits.tolist() == [3, 5]
    assert st["misses"][0] == 0 and st["vel"][0].tolist() == [2, 0, 2, 0] and st["box"][0].tolist() == [18, 10, 38, 30]
    assert (st["next_id"], st["frames"], st["refused"]) == (2, 5, 0)
    live = R.live(st)
    assert live["slots"].tolist() == [0, 1] and live["ids"].tolist() == [1, 2] and live["labels"].tolist() == [0, 1]


def test_expiry_is_at_max_age_plus_one():
    a, none = _frame((10, 10, 30, 30, 0.9, 0)), _frame()
    st = R.new_state()
    assert _ids(R.update(st, [a, none, none], max_age=2)) == [[1], [], []]
    assert st["id"][0] == 1 and st["misses"][0] == 2                       # misses == max_age: still alive
    assert _ids(R.update(st, [a], max_age=2)) == [[1]] and st["hits"][0] == 2
    st = R.new_state()
    R.update(st, [a, none, none, none], max_age=2)
    assert st["id"][0] == 0 and st["misses"][0] == 3                       # freed at misses == max_age + 1
    assert _ids(R.update(st, [a], max_age=2)) == [[2]]
    assert st["id"][0] == 2 and st["hits"][0] == 1 and st["next_id"] == 2
    # max_age=0: one missed frame ends the track
    st = R.new_state()
    assert _ids(R.update(st, [a, none, a], max_age=0)) == [[1], [], [2]]


def test_two_detections_compete_for_one_track():
    first = _frame((0, 0, 10, 10, 0.9, 0))
    # the earlier rank takes the track although the later one overlaps it more (IoU 9/11 against 1)
    st = R.new_state()
    out = R.update(st, [first, _frame((1, 0, 11, 10, 0.9, 0), (0, 0, 10, 10, 0.6, 0))])
    assert _ids(out) == [[1], [1, 2]] and out[1][1].tolist() == [2, 1]
    assert st["box"][0].tolist() == [1, 0, 11, 10] and st["box"][1].tolist() == [0, 0, 10, 10]
    # below new_thr (and above track_thr) the loser gets no track
    st = R.new_state()
    out = R.update(st, [first, _frame((1, 0, 11, 10, 0.9, 0), (0, 0, 10, 10, 0.4, 0))])
    assert _ids(out) == [[1], [1, 0]] and out[1][1].tolist() == [2, 0] and st["next_id"] == 1 and st["id"][1] == 0
    # a detection below track_thr does not even continue a track; one between the thresholds does
    st = R.new_state()
    out = R.update(st, [first, _frame((0, 0, 10, 10, 0.2, 0)), _frame((0, 0, 10, 10, 0.4, 0))])
    assert _ids(out) == [[1], [0], [1]] and st["hits"][0] == 2 and st["score"][0] == np.float32(0.4)


def test_equal_iou_goes_to_the_lower_slot():
    two = _frame((0, 0, 10, 10, 0.9, 0), (20, 0, 30, 10, 0.9, 0))
    st = R.new_state()
    # IoU 50 / 250 with both tracks, bit for bit
    out = R.update(st, [two, _frame((5, 0, 25, 10, 0.9, 0))], iou_thr=0.1)
    assert _ids(out) == [[1, 2], [1]] and st["misses"].tolist()[:2] == [0, 1]
    # not simply the first slot: 40 / 260 against 60 / 240
    st = R.new_state()
    out = R.update(st, [two, _frame((6, 0, 26, 10, 0.9, 0))], iou_thr=0.1)
    assert _ids(out) == [[1, 2], [2]]
    # and the threshold is inclusive: 50 / 250 == 0.2 in fp32
    st = R.new_state()
    assert _ids(R.update(st, [two, _frame((5, 0, 25, 10, 0.9, 0))], iou_thr=0.2)) == [[1, 2], [1]]
    st = R.new_state()
    assert _ids(R.update(st, [two, _frame((5, 0, 25, 10, 0.9, 0))], iou_thr=0.21)) == [[1, 2], [3]]


def test_class_aware():
    frames = [_frame((0, 0, 10, 10, 0.9, 0)), _frame((0, 0, 10, 10, 0.9, 1))]
    st = R.new_state()
    assert _ids(R.update(st, frames, class_aware=True)) == [[1], [2]] and st["label"].tolist()[:2] == [0, 1]
    st = R.new_state()
    assert _ids(R.update(st, frames, class_aware=False)) == [[1], [1]] and st["label"][0] == 0 and st["hits"][0] == 2


def test_motion_none_and_degenerate():
    st = R.new_state()
    out = R.update(st, [_frame((0, 0, 10, 10, 0.9, 0)), _frame((4, 0, 14, 10, 0.9, 0)), _frame()], motion="none")
    assert _ids(out) == [[1], [1], []] and st["vel"][0].tolist() == [0, 0, 0, 0] and st["box"][0].tolist() == [4, 0, 14, 10]
    # NaN IoU of two zero-area boxes: no match, a new track
    st = R.new_state()
    out = R.update(st, [_frame((5, 5, 5, 5, 0.9, 0)), _frame((5, 5, 5, 5, 0.9, 0))])
    assert _ids(out) == [[1], [2]]
    # ineligible detections touch nothing
    st = R.new_state()
    out = R.update(st, [_frame((0, 0, 10, 10, 0.9, 0)),
                        _frame((np.nan, 0, 10, 10, 0.9, 0), (0, 0, 10, 10, np.inf, 0), (0, 0, 10, 10, 0.9, -1))])
    assert _ids(out) == [[1], [0, 0, 0]] and st["misses"][0] == 1 and st["next_id"] == 1
    # capacity: the third track of max_tracks=2 is refused
    st = R.new_state()
    out = R.update(st, [_frame((0, 0, 10, 10, 0.9, 0), (20, 0, 30, 10, 0.9, 0), (40, 0, 50, 10, 0.9, 0))], max_tracks=2)
    assert _ids(out) == [[1, 2, 0]] and st["refused"] == 1


@pytest.mark.parametrize("bad, word", [
    (dict(iou_thr=0), "iou_thr"), (dict(iou_thr=1.5), "iou_thr"), (dict(iou_thr=float("nan")), "iou_thr"),
    (dict(iou_thr="0.3"), "iou_thr"), (dict(track_thr=float("inf")), "track_thr"), (dict(new_thr=float("nan")), "new_thr"),
    (dict(new_thr=None), "new_thr"), (dict(max_age=-1), "max_age"), (dict(max_age=2.5), "max_age"),
    (dict(max_tracks=0), "max_tracks"), (dict(max_tracks=257), "max_tracks"), (dict(max_tracks=True), "max_tracks"),
    (dict(motion="kalman"), "motion"), (dict(motion=1), "motion"), (dict(class_aware=1), "class_aware")])
def test_parameter_refusals(bad, word):
    with pytest.raises(ValueError, match=word):
        T.track_params(**bad)
    with pytest.raises(ValueError, match=word):
        T.Tracker(**bad)                                       # (refused before a device is asked for)


def test_parameter_forms():
    assert T.track_params(iou_thr=1, max_age=0, max_tracks=1, motion="none", class_aware=False) == \
        T.TrackSpec(1.0, 0.3, 0.5, 0, 1, 0, False)
    with pytest.raises(TypeError):
        T.track_params(kalman=True)
    with pytest.raises(ValueError, match="sequences"):
        T.Tracker(sequences=0)
