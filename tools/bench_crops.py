"""Times the RoI crops of detections (radet_crop_plan, radet_crop_frames) and writes profiles/bench_crops.json.

Two cases at B = 8 frames of 480 x 640 on the device, 256 x 256 f32 crops:
  * full:    K = 100 detections per frame, every slot valid -> 800 crops, 629 MB stored;
  * typical: 6 detections per frame -> 48 crops (the launch still has 800 slots: 752 of them exit at once).

The plan kernel and the pixel kernel are timed separately (device events around --iters back-to-back launches).  The
yardstick is radet_preprocess_frames writing the SAME number of output bytes in the same process: a sibling that reads four
source pixels and stores 12 bytes per output pixel, too (one descriptor row per crop, all rows pointing at the 8 frames,
resized to 256 x 256).  Rounds are interleaved (plan, pixels, sibling, round by round); medians are reported, with the
sibling's 10th-90th percentile band.  The byte floor is the stored bytes over the measured HBM copy rate (6.29 TB/s); the
source reads (8 frames, 7.4 MB) stay in cache.  No figure here is a pass condition.

    python tools/bench_crops.py [--iters 20] [--reps 9] [--out profiles/bench_crops.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
HBM_COPY_TBS = 6.29                  # measured float4 copy rate of the MI355X (8.0 TB/s spec)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_crops.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_crops.py measures on the GPU: no device found")
    from radet_amd import kernels as K
    from radet_amd.datasets.loading import frame_desc_rows
    from radet_amd.ops.crops import crop_spec, frame_table
    dev = torch.device("cuda", torch.cuda.current_device())
    B, Kd, Ho, Wo = 8, 100, 256, 256
    cap = B * Kd
    rng = np.random.RandomState(0)
    frames = [torch.from_numpy(rng.randint(0, 256, (480, 640, 3)).astype(np.uint8)).to(dev) for _ in range(B)]
    desc, keep = frame_table(frames, dev)
    cx, cy = rng.uniform(60, 580, (B, Kd)), rng.uniform(60, 420, (B, Kd))
    w, h = rng.uniform(40, 200, (B, Kd)), rng.uniform(40, 200, (B, Kd))
    boxes = torch.from_numpy(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32)).to(dev)
    scores = torch.from_numpy(rng.uniform(0.1, 1.0, (B, Kd)).astype(np.float32)).to(dev)
    spec = crop_spec((Ho, Wo), normalize=NORM)
    rows = torch.empty(cap, K.CROP_ROW_INTS, dtype=torch.int32, device=dev)
    counters = torch.zeros(2 + B, dtype=torch.int32, device=dev)
    images = torch.empty(cap, 3, Ho, Wo, dtype=torch.float32, device=dev)
    sib_out = torch.empty(cap, 3, Ho, Wo, dtype=torch.float32, device=dev)
    out = dict(case=dict(frames=B, frame_hw=[480, 640], slots=cap, crop_hw=[Ho, Wo], mode="f32 NCHW", scale=spec.scale,
                         iters=args.iters, reps=args.reps),
               device=torch.cuda.get_device_name(0), clocks="default governor, not pinned; medians of interleaved rounds",
               hbm_copy_tb_per_s=HBM_COPY_TBS)
    for name, per_frame in (("full", Kd), ("typical", 6)):
        counts = torch.full((B,), per_frame, dtype=torch.int32, device=dev)
        n = B * per_frame
        # the sibling: n descriptor rows over the same 8 frames, each resized to Ho x Wo -> n * 3 * Ho * Wo floats
        srows, _, _ = frame_desc_rows([frames[i % B] for i in range(n)], [(Ho, Wo)] * n, True, 0)
        sdesc = torch.from_numpy(srows).to(dev)
        fns = dict(plan=lambda: K.crop_plan(boxes, scores, counts, spec.size, spec.scale, spec.score_thr, cap, rows, counters),
                   pixels=lambda: K.crop_frames(rows, counters, desc, B, cap, spec.size, images, spec.fill, spec.mean, spec.stdinv,
                                                spec.to_rgb),
                   sibling=lambda: K.preprocess_frames(sdesc, n, Ho, Wo, spec.mean, spec.stdinv, sib_out))
        for fn in fns.values():                                      # warm-up (the plan first: the pixels read its rows)
            event_ms(fn, 3)
        assert counters.cpu().tolist() == [n, n] + [per_frame * (b + 1) for b in range(B)]
        rounds = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                rounds[k].append(event_ms(fn, args.iters))
        stored = n * 3 * Ho * Wo * 4
        floor_ms = stored / (HBM_COPY_TBS * 1e12) * 1e3
        med = {k: statistics.median(v) for k, v in rounds.items()}
        out[name] = dict(crops=n, stored_bytes=stored, byte_floor_ms=floor_ms, plan_ms=med["plan"], pixels_ms=med["pixels"],
                         sibling_preprocess_frames_ms=med["sibling"],
                         sibling_p10_p90_ms=[pct(rounds["sibling"], 0.1), pct(rounds["sibling"], 0.9)],
                         pixels_p10_p90_ms=[pct(rounds["pixels"], 0.1), pct(rounds["pixels"], 0.9)],
                         pixels_over_sibling=med["pixels"] / med["sibling"], pixels_stored_tb_per_s=stored / med["pixels"] / 1e9,
                         sibling_stored_tb_per_s=stored / med["sibling"] / 1e9, rounds_ms=rounds)
    del keep
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "rounds_ms"} if isinstance(v, dict) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
