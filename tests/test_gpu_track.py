"""Tracking on the device: radet_track_update against the NumPy restatement tests/_track_ref.py bit for bit -- ids, hits and the
whole state after every batch -- on seeded sequences, across batch splits, at the lane and sub-slot boundaries of the
one-wave-per-sequence mapping, at capacity, on degenerate input, with several sequences, its argument refusals, and
apis.track_frames against detect_frames + Tracker.update."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _track_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

N_FRAMES = 40


def make_sequence(seed, n_frames=N_FRAMES, n_obj=12):
    """a recorded sequence: up to n_obj objects in 3 classes on jittered straight paths, appearing within the first frames,
    dropping out for 1 to 8 frames, false positives, scores drawn around track_thr (0.3) and new_thr (0.5); per frame
    (dets f32 [k,5], labels i64 [k]) in descending score order"""
    rng = np.random.RandomState(seed)
    pos, size = rng.uniform(60, 540, (n_obj, 2)), rng.uniform(24, 90, (n_obj, 2))
    v, lab = rng.uniform(-5, 5, (n_obj, 2)), rng.randint(0, 3, n_obj)
    start, out_until = rng.randint(0, 8, n_obj), np.zeros(n_obj, int)
    frames = []
    for t in range(n_frames):
        rows = []
        pos += v
        for o in range(n_obj):
            if t < start[o] or t < out_until[o]:
                continue
            if rng.rand() < 0.1:
                out_until[o] = t + rng.randint(1, 9)
                continue
            c, s = pos[o] + rng.normal(0, 1.5, 2), size[o] * (1 + rng.normal(0, 0.03, 2))
            score = rng.choice([0.27, 0.33, 0.47, 0.53, 0.7, 0.9]) + rng.uniform(-0.04, 0.04)
            rows.append((c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2, score, lab[o]))
        for _ in range(rng.randint(0, 3)):
            c, s = rng.uniform(0, 600, 2), rng.uniform(10, 120, 2)
            rows.append((c[0], c[1], c[0] + s[0], c[1] + s[1], rng.uniform(0.2, 0.7), rng.randint(0, 3)))
        rows.sort(key=lambda r: -r[4])
        a = np.array(rows, np.float64).reshape(-1, 6)
        frames.append((a[:, :5].astype(np.float32), a[:, 5].astype(np.int64)))
    return frames


_REF = {}


def reference(seed, **params):
    """the restatement's (per-frame (ids, hits), state after every frame) of make_sequence(seed): computed once, never changed"""
    key = (seed, tuple(sorted(params.items())))
    if key not in _REF:
        st, outs, states = R.new_state(), [], []
        for f in make_sequence(seed):
            outs += R.update(st, [f], **params)
            states.append({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()})
        _REF[key] = (outs, states)
    return _REF[key]


def same_state(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        if isinstance(w, np.ndarray):
            g = got[k]
            assert g.dtype == w.dtype and g.shape == w.shape, k
            assert np.array_equal(g.view(np.int32), w.view(np.int32)), (k, np.nonzero(g.view(np.int32) != w.view(np.int32)))
        else:
            assert got[k] == w, (k, got[k], w)


def same_outputs(ids, hits, frames, want):
    """ids / hits [B, cap] of the device against the restatement's per-frame arrays; padded slots are 0"""
    ids, hits = ids.cpu().numpy(), hits.cpu().numpy()
    assert ids.dtype == np.int32 and hits.dtype == np.int32 and ids.shape == hits.shape and ids.shape[0] == len(frames)
    for i, ((d, _), (wi, wh)) in enumerate(zip(frames, want)):
        k = len(d)
        assert np.array_equal(ids[i, :k], wi) and np.array_equal(hits[i, :k], wh), (i, ids[i, :k], wi)
        assert not ids[i, k:].any() and not hits[i, k:].any()


def frame(*dets):
    a = np.array(dets, np.float64).reshape(-1, 6)
    return a[:, :5].astype(np.float32), a[:, 5].astype(np.int64)


def grid_boxes(n, score=0.9, label=0, first=0):
    """n disjoint 10 x 10 boxes on a 20-pixel grid, numbered from `first`"""
    return [(20 * (i % 32), 20 * (i // 32), 20 * (i % 32) + 10, 20 * (i // 32) + 10, score, label) for i in range(first, first + n)]


def run_both(batches, **params):
    """batches through a Tracker and through the restatement, compared after every batch -> (tracker, restatement's state)"""
    from radet_amd.ops import Tracker
    trk, st = Tracker(**params), R.new_state()
    for frames in batches:
        ids, hits = trk.update(frames)
        same_outputs(ids, hits, frames, R.update(st, frames, **params))
        same_state(trk.host_state(), st)
    return trk, st


# ------------------------------------------------------------------------------------------- 1. parity on seeded sequences
@pytest.mark.parametrize("motion", ["constant", "none"])
@pytest.mark.parametrize("class_aware", [True, False])
def test_parity_with_the_restatement(motion, class_aware):
    from radet_amd.ops import Tracker
    params = dict(motion=motion, class_aware=class_aware)
    frames = make_sequence(5)
    outs, states = reference(5, **params)
    n_ids = max(int(o[0].max()) if len(o[0]) else 0 for o in outs)
    n_miss = sum(int((o[0] == 0).sum()) for o in outs)
    print("tracks started:", n_ids, "detections without a track:", n_miss, "live at the end:", int((states[-1]["id"] != 0).sum()))
    assert n_ids > 12 and n_miss > 0 and any(s["misses"].max() > 2 for s in states)        # (returns, drops and coasting occur)
    trk = Tracker(**params)
    for lo in range(0, N_FRAMES, 8):
        ids, hits = trk.update(frames[lo:lo + 8])
        same_outputs(ids, hits, frames[lo:lo + 8], outs[lo:lo + 8])
        same_state(trk.host_state(), states[lo + 7])
    live, want = trk.tracks(), R.live(states[-1])
    for k in ("ids", "boxes", "labels", "misses", "hits", "scores", "slots"):
        assert np.array_equal(live[k], want[k]), k
    assert (live["next_id"], live["frames"], live["refused"]) == (states[-1]["next_id"], N_FRAMES, 0)
    trk.reset()
    same_state(trk.host_state(), R.new_state())


def test_split_invariance():
    from radet_amd.ops import Tracker, track_detections
    frames = make_sequence(7)
    outs, states = reference(7)
    for step in (1, 3, 8, 40):
        trk = Tracker()
        for lo in range(0, N_FRAMES, step):
            ids, hits = trk.update(frames[lo:lo + step])
            same_outputs(ids, hits, frames[lo:lo + step], outs[lo:lo + step])
        same_state(trk.host_state(), states[-1])
    # the stand-alone form: one launch over the recorded sequence, tensors or arrays
    got = track_detections(frames)
    assert len(got) == N_FRAMES and all(g.dtype == np.int32 and np.array_equal(g, o[0]) for g, o in zip(got, outs))
    got = track_detections([(torch.from_numpy(d).cuda(), torch.from_numpy(l)) for d, l in frames[:5]])
    assert all(np.array_equal(g, o[0]) for g, o in zip(got, outs))
    assert track_detections([]) == []


# ------------------------------------------------------------------------------------------- 2. the mapping's boundaries
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256])
def test_last_slot_of_n_tracks_matches(n):
    boxes = grid_boxes(n)
    trk, st = run_both([[frame(*boxes), frame(boxes[-1])]])
    ids, _ = trk.update([frame(boxes[-1])])
    assert ids.cpu().numpy()[0, 0] == n
    live = trk.tracks()
    assert live["slots"].tolist() == list(range(n)) and live["ids"].tolist() == list(range(1, n + 1))
    assert live["hits"].tolist() == [1] * (n - 1) + [3] and live["misses"].tolist() == [2] * (n - 1) + [0]


def test_lowest_free_slot_across_lanes():
    """slots 0 and 64 (lane 0 and lane 16) expire; the next track lands in slot 0"""
    boxes = grid_boxes(66)
    kept = [b for i, b in enumerate(boxes) if i not in (0, 64)]
    trk, st = run_both([[frame(*boxes), frame(*kept)], [frame(*(kept + grid_boxes(1, first=100)))]], max_age=0)
    live = trk.tracks()
    assert live["slots"].tolist() == [s for s in range(66) if s != 64]
    assert live["ids"].tolist() == [67] + list(range(2, 65)) + [66] and live["next_id"] == 67
    # and the one after it in slot 64
    ids, _ = trk.update([frame(*(kept + grid_boxes(2, first=100)))])
    assert ids.cpu().numpy()[0, 64:66].tolist() == [67, 68]
    live = trk.tracks()
    assert live["slots"].tolist() == list(range(66)) and live["ids"][64] == 68


# ------------------------------------------------------------------------------------------- 3. capacity
def test_capacity():
    boxes = grid_boxes(259)
    trk, st = run_both([[frame(*boxes)]])
    ids, hits = trk.update([frame(*boxes)])
    assert ids.shape == (1, 259)
    assert ids.cpu().numpy()[0].tolist() == list(range(1, 257)) + [0, 0, 0] and hits.cpu().numpy()[0].tolist() == [2] * 256 + [0] * 3
    assert trk.tracks()["refused"] == 6 and st["refused"] == 3
    trk, st = run_both([[frame(*grid_boxes(5))]], max_tracks=4)
    assert st["id"][:5].tolist() == [1, 2, 3, 4, 0] and st["refused"] == 1 and trk.tracks()["refused"] == 1


# ------------------------------------------------------------------------------------------- 4. degenerate input
def test_degenerate_detections():
    from radet_amd.ops import Tracker
    first = frame((0, 0, 10, 10, 0.9, 0), (30, 0, 40, 10, 0.9, 1))
    calm = Tracker()
    calm.update([first, frame()])
    want = calm.host_state()
    for bad in [(np.nan, 0, 10, 10, 0.9, 0), (0, 0, 10, np.inf, 0.9, 0), (0, 0, 10, 10, np.inf, 0), (0, 0, 10, 10, np.nan, 0),
                (0, 0, 10, 10, 0.9, -1), (0, 0, 10, 10, 0.9, 2 ** 31), (0, 0, 10, 10, 0.29, 0)]:
        trk, st = run_both([[first, frame(bad)]])
        same_state(trk.host_state(), want)                       # (what an empty frame leaves, bit for bit)
    # zero area over zero area: a NaN IoU, no match, a new track
    trk, st = run_both([[frame((5, 5, 5, 5, 0.9, 0)), frame((5, 5, 5, 5, 0.9, 0))]])
    assert st["id"][:2].tolist() == [1, 2] and st["misses"][:2].tolist() == [1, 0]


def test_empty_frames():
    seq = make_sequence(9)[:12]
    none = frame()
    # empty frames in the middle of a batch, then a whole batch of them: everything coasts, then expires
    trk, st = run_both([seq[:3] + [none, none] + seq[5:8], [none] * 3, [none] * 3])
    assert len(trk.tracks()["ids"]) == 0 and trk.tracks()["frames"] == 14 and st["next_id"] > 0
    trk, st = run_both([seq[:4], [none] * 5])
    live = trk.tracks()
    assert len(live["ids"]) > 0 and (live["misses"] >= 5).all()          # (max_age = 5: alive after five misses)
    trk.update([none])
    assert len(trk.tracks()["ids"]) == 0


def test_padded_slots_are_written_as_zero():
    from radet_amd import kernels as K
    from radet_amd.ops.track import track_params, unpack_state
    rng = np.random.RandomState(3)
    B, cap = 3, 70                                               # (two chunks of 64 slots per frame)
    counts = [5, 0, 66]
    boxes = np.zeros((B, cap, 4), np.float32)
    for b in range(B):
        boxes[b] = np.array([r[:4] for r in grid_boxes(cap)], np.float32)          # (valid-looking boxes beyond the counts too)
    scores = rng.uniform(0.5, 1, (B, cap)).astype(np.float32)
    labels = np.zeros((B, cap), np.int64)
    dev = torch.device("cuda")
    state = torch.zeros(1, K.TRACK_STATE_BYTES // 4, dtype=torch.int32, device=dev)
    ids = torch.full((1, B, cap), -7, dtype=torch.int32, device=dev)
    hits = torch.full((1, B, cap), -7, dtype=torch.int32, device=dev)
    K.track_update(torch.from_numpy(boxes)[None].to(dev), torch.from_numpy(scores)[None].to(dev),
                   torch.from_numpy(labels)[None].to(dev), torch.tensor([counts], dtype=torch.int32, device=dev), 1, B, cap, state,
                   *track_params(), ids, hits)
    st = R.new_state()
    want = R.update(st, [(np.concatenate([boxes[b, :c], scores[b, :c, None]], 1), labels[b, :c]) for b, c in enumerate(counts)])
    ids, hits = ids.cpu().numpy()[0], hits.cpu().numpy()[0]
    for b, c in enumerate(counts):
        assert np.array_equal(ids[b, :c], want[b][0]) and np.array_equal(hits[b, :c], want[b][1])
        assert not ids[b, c:].any() and not hits[b, c:].any()
    same_state(unpack_state(state[0].cpu().numpy()), st)
    assert st["next_id"] == 66


# ------------------------------------------------------------------------------------------- 5. several sequences
def test_three_sequences_in_one_launch():
    from radet_amd.ops import Tracker
    seqs = [make_sequence(s)[:16] for s in (21, 22, 23)]
    many, single = Tracker(sequences=3), [Tracker() for _ in seqs]
    for lo in (0, 8):
        ids, hits = many.update([s[lo:lo + 8] for s in seqs])
        assert ids.shape[:2] == (3, 8)
        for q, (s, one) in enumerate(zip(seqs, single)):
            wi, wh = one.update(s[lo:lo + 8])
            cap = wi.shape[1]
            assert torch.equal(ids[q, :, :cap], wi) and torch.equal(hits[q, :, :cap], wh)
            assert not ids[q, :, cap:].any() and not hits[q, :, cap:].any()
            same_state(many.host_state(q), one.host_state())
    assert len({int(many.host_state(q)["next_id"]) for q in range(3)}) > 1           # (the sequences really differ)
    with pytest.raises(ValueError):
        many.update(seqs[0][:8])
    with pytest.raises(ValueError):
        many.update([seqs[0][:8], seqs[1][:8], seqs[2][:7]])


# ------------------------------------------------------------------------------------------- 6. refusals
GOOD = dict(nseq=1, B=2, cap=8, iou_thr=0.3, track_thr=0.3, new_thr=0.5, max_age=5, max_tracks=256, motion=1, class_aware=1)
BAD = [dict(nseq=0), dict(B=0), dict(cap=0), dict(cap=4097), dict(nseq=-1), dict(max_tracks=0), dict(max_tracks=257),
       dict(iou_thr=0.0), dict(iou_thr=1.5), dict(iou_thr=-0.1), dict(iou_thr=float("nan")), dict(max_age=-1),
       dict(track_thr=float("inf")), dict(new_thr=float("nan")), dict(motion=2), dict(motion=-1), dict(class_aware=2)]


def test_bad_arguments_launch_nothing():
    from radet_amd import _lib, kernels as K
    from radet_amd.ops import Tracker
    fn = _lib.load().radet_track_update
    dev = torch.device("cuda")
    trk = Tracker()
    trk.update(make_sequence(5)[:4])
    before = trk.state.clone()
    assert before.any()
    boxes = torch.tensor([r[:4] for r in grid_boxes(8)], dtype=torch.float32, device=dev).repeat(2, 1, 1).contiguous()
    scores = torch.full((2, 8), 0.9, device=dev)
    labels = torch.zeros(2, 8, dtype=torch.int64, device=dev)
    counts = torch.full((2,), 8, dtype=torch.int32, device=dev)
    ids = torch.full((2, 8), -7, dtype=torch.int32, device=dev)
    hits = torch.full((2, 8), -7, dtype=torch.int32, device=dev)

    def call(state=trk.state, boxes_ptr=None, **kw):
        a = dict(GOOD, **kw)
        return fn(boxes.data_ptr() if boxes_ptr is None else boxes_ptr, scores.data_ptr(), labels.data_ptr(), counts.data_ptr(),
                  a["nseq"], a["B"], a["cap"], None if state is None else state.data_ptr(), a["iou_thr"], a["track_thr"],
                  a["new_thr"], a["max_age"], a["max_tracks"], a["motion"], a["class_aware"], ids.data_ptr(), hits.data_ptr(),
                  K._stream())
    assert K.TRACK_MAX_DETS == 4096
    for bad in BAD:
        assert call(**bad) != 0, bad
    assert call(state=None) != 0 and call(boxes_ptr=boxes.data_ptr() + 4) != 0
    torch.cuda.synchronize()
    assert (ids == -7).all() and (hits == -7).all() and torch.equal(trk.state, before)
    assert call() == 0                                           # (the same call with nothing wrong runs)
    torch.cuda.synchronize()
    assert (ids != -7).all() and (hits != -7).all() and not torch.equal(trk.state, before)
    assert _lib.load().radet_track_state_bytes(3) == 3 * K.TRACK_STATE_BYTES and _lib.load().radet_track_state_bytes(0) == 0
    with pytest.raises(ValueError):
        trk.update((torch.zeros(1, 4097, 4), torch.zeros(1, 4097), torch.zeros(1, 4097, dtype=torch.int64), torch.zeros(1)))


# ------------------------------------------------------------------------------------------- 7. track_frames
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])


def _pipe(loader, scale):
    return [dict(type=loader),
            dict(type="MultiScaleFlipAug", img_scale=scale, flip=False, transforms=[
                dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", to_rgb=True, **NORM),
                dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])])]


@pytest.fixture(scope="module")
def det():
    """the detector of tests/test_gpu_frames.py: img_scale (640, 480) on small landscape frames"""
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    d = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().eval()
    synth_fill(d, seed=0)
    with torch.no_grad():
        d.bbox_head.atss_cls.bias += 2.0                       # (scores above the thresholds: the comparisons are not vacuous)
    d.cfg = Config(dict(data=dict(test=dict(pipeline=_pipe("LoadImageFromFile", (640, 480))))))
    return d


@pytest.fixture(scope="module")
def frames():
    """a dozen frames of two sizes: a textured scene that drifts by a few pixels per frame, so detections recur"""
    rng = np.random.RandomState(11)
    scene = rng.randint(0, 256, (96, 128, 3)).astype(np.uint8)
    out = []
    for t in range(12):
        h, w = (48, 64) if t % 2 == 0 else (60, 80)
        out.append(np.ascontiguousarray(scene[t:t + h, 2 * t:2 * t + w]))
    return out


@pytest.fixture(scope="module")
def plain(det, frames):
    """detect_frames on the same frames, on the device and on the host: computed once"""
    from radet_amd.apis import detect_frames
    return (list(detect_frames(det, frames, batch_size=2, on_device=True)), list(detect_frames(det, frames, batch_size=2)))


def test_track_frames(det, frames, plain):
    from radet_amd.apis import track_frames
    from radet_amd.core.bbox import bbox2result
    from radet_amd.ops import Tracker
    raw, host = plain
    assert sum(int(b.shape[0]) for b, _ in raw) > 0
    # the ids of Tracker.update fed with detect_frames' outputs, batch by batch
    trk, want = Tracker(), []
    for lo in range(0, 12, 2):
        ids, _ = trk.update(raw[lo:lo + 2])
        want += [ids[i, :int(raw[lo + i][0].shape[0])].cpu().numpy() for i in range(2)]
    print("detections:", [len(w) for w in want], "tracks:", trk.tracks()["next_id"])
    assert any(w.any() for w in want)
    got = list(track_frames(det, iter(frames), batch_size=2, on_device=True))
    assert len(got) == 12
    for ((b, l), ids), (wb, wl), wi in zip(got, raw, want):
        assert torch.equal(b, wb) and torch.equal(l, wl)
        assert ids.is_cuda and ids.dtype == torch.int32 and np.array_equal(ids.cpu().numpy(), wi)
    # on the host: the results of detect_frames, the ids regrouped as bbox2result regroups the boxes
    got_host = list(track_frames(det, frames, batch_size=2))
    nc = det.bbox_head.num_classes
    for (res, ids), wres, (wb, wl), wi in zip(got_host, host, raw, want):
        assert len(res) == len(wres) == len(ids) == nc
        assert all(a.dtype == w.dtype and np.array_equal(a, w) for a, w in zip(res, wres))
        wl = wl.cpu().numpy()
        for c in range(nc):
            assert ids[c].dtype == np.int32 and np.array_equal(ids[c], wi[wl == c]) and len(ids[c]) == len(res[c])
        regrouped = bbox2result(np.concatenate([wb.cpu().numpy()[:, :4], wi[:, None].astype(np.float32)], 1), wl, nc)
        assert all(np.array_equal(r[:, 4].astype(np.int32), i) for r, i in zip(regrouped, ids))
    # another batch size: the same ids
    got3 = list(track_frames(det, frames, batch_size=3, on_device=True))
    assert [i.cpu().numpy().tolist() for _, i in got3] == [w.tolist() for w in want]


def test_track_frames_crops_and_continuation(det, frames, plain):
    from radet_amd.apis import detect_frames, track_frames
    from radet_amd.ops import Tracker
    raw, _ = plain
    req = dict(size=16, max_crops=64)
    both = list(track_frames(det, frames[:4], batch_size=2, on_device=True, crops=req))
    ref = list(detect_frames(det, frames[:4], batch_size=2, on_device=True, crops=req))
    n = 0
    for ((b, l), ids, crops), ((wb, wl), wcrops) in zip(both, ref):
        assert torch.equal(b, wb) and torch.equal(l, wl) and ids.shape[0] == b.shape[0]
        assert torch.equal(crops.index, wcrops.index) and torch.equal(crops.images, wcrops.images)
        rank = crops.index[:, 1].cpu().numpy()
        assert ((0 <= rank) & (rank < ids.shape[0])).all()       # (every crop names a detection of its frame)
        of_crop = ids[crops.index[:, 1].long()]
        assert np.array_equal(of_crop.cpu().numpy(), ids.cpu().numpy()[rank])
        n += len(rank)
    assert n > 0
    # a tracker passed in continues its numbering across two calls; the whole equals one call
    whole = [i.cpu().numpy() for _, i in track_frames(det, frames, batch_size=2, on_device=True)]
    trk = Tracker()
    halves = [i.cpu().numpy() for _, i in track_frames(det, frames[:6], batch_size=2, on_device=True, tracker=trk)]
    mid = trk.tracks()
    assert mid["frames"] == 6
    halves += [i.cpu().numpy() for _, i in track_frames(det, frames[6:], batch_size=2, on_device=True, tracker=trk)]
    assert all(np.array_equal(a, b) for a, b in zip(halves, whole)) and trk.tracks()["frames"] == 12
    assert trk.tracks()["next_id"] >= mid["next_id"] > 0
    # refusals
    with pytest.raises(TypeError):
        next(track_frames(det, frames, colour="red"))
    with pytest.raises(TypeError):
        next(track_frames(det, frames, tracker=trk, max_age=2))
    with pytest.raises(ValueError):
        next(track_frames(det, frames, tracker=Tracker(sequences=2)))
    with pytest.raises(ValueError):
        next(track_frames(det, frames, iou_thr=0))
