"""Times the tracker's update launch (radet_track_update) and writes profiles/bench_track.json.

  * A: one launch over 8 consecutive frames x 100 detections with about 100 live tracks -- 100 objects of 3 classes on small
    periodic paths (period 8 frames, so every launch sees the same batch and the tracks stay alive), all of which match --
    beside the same launch over 8 EMPTY frames of the same shape (the launch's floor: state load, ageing, state store), in the
    same process.  Rounds alternate; device events around --iters back-to-back launches; medians with 10th-90th percentiles.
  * api (default on): track_frames against detect_frames alone on the same host frames of 480 x 640 (a synth-initialised r50
    detector, host wall clock per batch of 8, alternating rounds), as added milliseconds per batch, host results and
    on_device=True.
No figure here is a pass condition: no threshold was set in advance.

    python tools/bench_track.py [--iters 20] [--reps 15] [--no-api] [--out profiles/bench_track.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def event_ms(fn, iters):
    """device milliseconds per call of `iters` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, int(round(q * (len(xs) - 1)))))]


def kernel_case(B, Kd, iters, reps, dev):
    from radet_amd import kernels as K
    from radet_amd.ops.track import Tracker
    rng = np.random.RandomState(0)
    cx, cy = rng.uniform(60, 580, Kd), rng.uniform(60, 420, Kd)
    w, h = rng.uniform(40, 100, Kd), rng.uniform(40, 100, Kd)
    phase = rng.uniform(0, 2 * np.pi, Kd)
    boxes = np.zeros((B, Kd, 4), np.float32)
    for f in range(B):
        dx, dy = 3 * np.sin(2 * np.pi * f / B + phase), 3 * np.cos(2 * np.pi * f / B + phase)
        boxes[f] = np.stack([cx + dx - w / 2, cy + dy - h / 2, cx + dx + w / 2, cy + dy + h / 2], -1)
    boxes = torch.from_numpy(boxes)[None].to(dev)
    scores = torch.from_numpy(np.sort(rng.uniform(0.5, 1.0, (1, B, Kd)).astype(np.float32))[..., ::-1].copy()).to(dev)
    labels = torch.from_numpy(rng.randint(0, 3, (1, 1, Kd)).astype(np.int64)).expand(1, B, Kd).contiguous().to(dev)
    full, none = torch.full((1, B), Kd, dtype=torch.int32, device=dev), torch.zeros(1, B, dtype=torch.int32, device=dev)
    busy, idle = Tracker(device=dev), Tracker(device=dev)
    ids, hits, ids0, hits0 = (torch.empty(1, B, Kd, dtype=torch.int32, device=dev) for _ in range(4))
    fns = dict(update=lambda: K.track_update(boxes, scores, labels, full, 1, B, Kd, busy.state, *busy.spec, ids, hits),
               empty=lambda: K.track_update(boxes, scores, labels, none, 1, B, Kd, idle.state, *idle.spec, ids0, hits0))
    for fn in fns.values():
        event_ms(fn, 3)
    rounds = {k: [] for k in fns}
    live = []
    for _ in range(reps):
        for k, fn in fns.items():
            rounds[k].append(event_ms(fn, iters))
        t = busy.tracks()
        live.append(len(t["ids"]))
    t = busy.tracks()
    med = {k: statistics.median(v) for k, v in rounds.items()}
    return dict(frames=B, detections_per_frame=Kd, live_tracks_min_max=[min(live), max(live)], tracks_started=t["next_id"],
                refused=t["refused"], matched_last_launch=int((ids != 0).sum()),
                update_ms=med["update"], update_p10_p90_ms=[pct(rounds["update"], 0.1), pct(rounds["update"], 0.9)],
                empty_frames_ms=med["empty"], empty_p10_p90_ms=[pct(rounds["empty"], 0.1), pct(rounds["empty"], 0.9)],
                us_per_detection=(med["update"] - med["empty"]) * 1e3 / (B * Kd), rounds_ms=rounds)


def api_case(reps, dev):
    from radet_amd.apis import detect_frames, track_frames
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().eval()
    synth_fill(det, seed=0)
    with torch.no_grad():
        det.bbox_head.atss_cls.bias += 2.0
    pipe = [dict(type="LoadImageFromFile"),
            dict(type="MultiScaleFlipAug", img_scale=(640, 480), flip=False, transforms=[
                dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", **NORM),
                dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])])]
    det.cfg = Config(dict(data=dict(test=dict(pipeline=pipe))))
    rng = np.random.RandomState(1)
    batches = 4
    frames = [rng.randint(0, 256, (480, 640, 3)).astype(np.uint8) for _ in range(8 * batches)]

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        n = sum(1 for _ in fn())
        torch.cuda.synchronize()
        assert n == len(frames)
        return (time.perf_counter() - t) * 1e3 / batches
    fns = dict(detect=lambda: detect_frames(det, frames, batch_size=8), track=lambda: track_frames(det, frames, batch_size=8),
               detect_on_device=lambda: detect_frames(det, frames, batch_size=8, on_device=True),
               track_on_device=lambda: track_frames(det, frames, batch_size=8, on_device=True))
    for fn in fns.values():
        wall(fn)
    first = list(track_frames(det, frames[:8], batch_size=8, on_device=True))
    rounds = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            rounds[k].append(wall(fn))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    return dict(frames_per_batch=8, frame_hw=[480, 640], batches_per_round=batches,
                detections_first_batch=sum(int(i.shape[0]) for _, i in first),
                tracked_first_batch=sum(int((i != 0).sum()) for _, i in first),
                detect_frames_ms_per_batch=med["detect"], track_frames_ms_per_batch=med["track"],
                added_ms_per_batch=med["track"] - med["detect"],
                detect_frames_p10_p90_ms=[pct(rounds["detect"], 0.1), pct(rounds["detect"], 0.9)],
                on_device_detect_ms_per_batch=med["detect_on_device"], on_device_track_ms_per_batch=med["track_on_device"],
                on_device_added_ms_per_batch=med["track_on_device"] - med["detect_on_device"],
                on_device_detect_p10_p90_ms=[pct(rounds["detect_on_device"], 0.1), pct(rounds["detect_on_device"], 0.9)],
                rounds_ms=rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-api", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_track.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_track.py measures on the GPU: no device found")
    if args.reps < 15:
        raise SystemExit("at least 15 alternating rounds")
    dev = torch.device("cuda", torch.cuda.current_device())
    out = dict(device=torch.cuda.get_device_name(0), clocks="default governor, not pinned; medians of alternating rounds",
               iters=args.iters, reps=args.reps, parameters="the defaults of ops.track.track_params",
               A=kernel_case(8, 100, args.iters, args.reps, dev))
    if not args.no_api:
        out["api"] = api_case(args.reps, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "rounds_ms"} if isinstance(v, dict) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
