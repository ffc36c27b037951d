"""Times the detection overlay (radet_draw_detections) and writes profiles/bench_draw.json.

  * A: 8 frames of 480 x 640 on the device, 100 detections each;   * B: one frame of 1080 x 1920, 100 detections.
Class names of YCB-V, the default font at size 13, thickness 2, every detection above the threshold.  The draw launch, out of
place and in place, is timed beside radet_copy_segments copying the SAME frames into the same destinations in the same
process -- a sibling that moves the same bytes (3 read + 3 stored per pixel) and draws nothing.  Rounds alternate (out of
place, in place, sibling, round by round; device events around --iters back-to-back launches); medians are reported with the
sibling's 10th-90th percentile band and the ratio.  With --api (default) the streaming interface is timed too:
draw_frames against detect_frames alone on the same host frames of workload A (a synth-initialised r50 detector, host wall
clock per batch of 8, alternating rounds), as added milliseconds per batch.  No figure here is a pass condition.

    python tools/bench_draw.py [--iters 20] [--reps 15] [--no-api] [--out profiles/bench_draw.json]
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


def kernel_case(B, H, W, Kd, names, iters, reps, dev):
    from radet_amd import kernels as K
    from radet_amd.ops.crops import frame_table
    from radet_amd.ops.draw import Painter
    rng = np.random.RandomState(0)
    frames = [torch.from_numpy(rng.randint(0, 256, (H, W, 3)).astype(np.uint8)).to(dev) for _ in range(B)]
    dsts = [torch.empty_like(f) for f in frames]
    cx, cy = rng.uniform(0.1 * W, 0.9 * W, (B, Kd)), rng.uniform(0.1 * H, 0.9 * H, (B, Kd))
    w, h = rng.uniform(0.06 * W, 0.3 * W, (B, Kd)), rng.uniform(0.08 * H, 0.4 * H, (B, Kd))
    boxes = torch.from_numpy(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32)).to(dev)
    scores = torch.from_numpy(np.sort(rng.uniform(0.31, 1.0, (B, Kd)).astype(np.float32))[:, ::-1].copy()).to(dev)
    labels = torch.from_numpy(rng.randint(0, len(names), (B, Kd)).astype(np.int64)).to(dev)
    counts = torch.full((B,), Kd, dtype=torch.int32, device=dev)
    painter = Painter(dev, class_names=names, score_thr=0.3, bbox_color="class", thickness=2, font_size=13)
    table, keep = frame_table(frames + dsts, dev)
    n = B * K.PREP_DESC_INTS
    src_t, dst_t = table[:n], table[n:]
    ctab, tiles = K.copy_segments_table([(f.data_ptr(), d.data_ptr(), f.numel()) for f, d in zip(frames, dsts)])
    cdesc = torch.from_numpy(ctab).to(dev)
    fns = dict(draw_out=lambda: painter.launch(src_t, dst_t, B, H, W, boxes, scores, labels, counts, False),
               draw_in=lambda: painter.launch(src_t, src_t, B, H, W, boxes, scores, labels, counts, True),
               sibling=lambda: K.copy_segments(cdesc, B, tiles))
    for fn in fns.values():
        event_ms(fn, 3)
    rounds = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            rounds[k].append(event_ms(fn, iters))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    moved = 2 * B * H * W * 3
    del keep
    return dict(frames=B, frame_hw=[H, W], detections_per_frame=Kd, bytes_read_plus_stored=moved,
                draw_out_of_place_ms=med["draw_out"], draw_in_place_ms=med["draw_in"], sibling_copy_segments_ms=med["sibling"],
                sibling_p10_p90_ms=[pct(rounds["sibling"], 0.1), pct(rounds["sibling"], 0.9)],
                draw_out_p10_p90_ms=[pct(rounds["draw_out"], 0.1), pct(rounds["draw_out"], 0.9)],
                draw_in_p10_p90_ms=[pct(rounds["draw_in"], 0.1), pct(rounds["draw_in"], 0.9)],
                out_of_place_over_sibling=med["draw_out"] / med["sibling"], in_place_over_sibling=med["draw_in"] / med["sibling"],
                draw_out_tb_per_s=moved / med["draw_out"] / 1e9, sibling_tb_per_s=moved / med["sibling"] / 1e9, rounds_ms=rounds)


def api_case(names, reps, dev):
    from radet_amd.apis import detect_frames, draw_frames
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
    style = dict(class_names=names, score_thr=0.3, bbox_color="class")

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        n = sum(1 for _ in fn())
        torch.cuda.synchronize()
        assert n == len(frames)
        return (time.perf_counter() - t) * 1e3 / batches
    fns = dict(detect=lambda: detect_frames(det, frames, batch_size=8), draw=lambda: draw_frames(det, frames, batch_size=8, **style),
               detect_on_device=lambda: detect_frames(det, frames, batch_size=8, on_device=True),
               draw_on_device=lambda: draw_frames(det, frames, batch_size=8, on_device=True, **style))
    for fn in fns.values():
        wall(fn)
    drawn = sum(int((np.vstack(r)[:, 4] > 0.3).sum()) for r, _ in draw_frames(det, frames[:8], batch_size=8, **style))
    rounds = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            rounds[k].append(wall(fn))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    return dict(frames_per_batch=8, frame_hw=[480, 640], batches_per_round=batches, detections_drawn_first_batch=drawn,
                detect_frames_ms_per_batch=med["detect"], draw_frames_ms_per_batch=med["draw"],
                added_ms_per_batch=med["draw"] - med["detect"],
                detect_frames_p10_p90_ms=[pct(rounds["detect"], 0.1), pct(rounds["detect"], 0.9)],
                on_device_detect_ms_per_batch=med["detect_on_device"], on_device_draw_ms_per_batch=med["draw_on_device"],
                on_device_added_ms_per_batch=med["draw_on_device"] - med["detect_on_device"], rounds_ms=rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-api", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_draw.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_draw.py measures on the GPU: no device found")
    if args.reps < 15:
        raise SystemExit("at least 15 alternating rounds")
    from radet_amd.datasets.bop import YCBV_CLASSES
    dev = torch.device("cuda", torch.cuda.current_device())
    names = list(YCBV_CLASSES)
    out = dict(device=torch.cuda.get_device_name(0), clocks="default governor, not pinned; medians of alternating rounds",
               iters=args.iters, reps=args.reps, style="YCB-V names, default font size 13, thickness 2, class colours",
               A=kernel_case(8, 480, 640, 100, names, args.iters, args.reps, dev),
               B=kernel_case(1, 1080, 1920, 100, names, args.iters, args.reps, dev))
    if not args.no_api:
        out["api"] = api_case(names, args.reps, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "rounds_ms"} if isinstance(v, dict) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
