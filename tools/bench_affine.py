"""Affine augmentation against the fixed-scale pipeline: the device part (ImagePipeline.run) of one planned bs-16 batch each,
in one process on one GPU, default clocks.

    python tools/bench_affine.py [--iters 20] [--rounds 5] [--out profiles/bench_affine.json]

`fixed`   = the r50_ycbv_pbr train pipeline: 640 x 480 frames, Resize((640, 480)), output 480 x 640.
`fixed_b` = the same pipeline, the same planned batch, measured as a variant of its own: the difference between the two
            medians, and the spread of the per-round medians, are what run-to-run noise looks like in this process.
`rotate`  = the same with Rotate(level=10, max_rotate_angle=30, prob=0.5, img_fill_val=128) directly after the Resize
            (configs/base/datasets/bop_detection_rotate.py), on the same files.
The variants alternate within each round; per call a device event pair around run() and a host clock around the call and
a synchronise.  The yardstick is `fixed`: the affine stages do not change its code path.  No threshold is set: the added
time (rotate - fixed) is reported next to the traffic floor of the warp launches -- the bytes they read plus write, frames
2 * B * H * W * 3 and masks 2 * sum(G) * H * W over the mask groups in which a sample fired, over 6.3 TB/s (the HBM rate a streaming copy reaches on an MI355X; the
8 TB/s peak gives a floor 21 % lower).  Prints one JSON line (and writes it to --out): per variant the medians and scatter,
the per-round medians, the spread of the fixed pipeline (max - min over the per-round medians of fixed and fixed_b), and
the entry points each variant calls."""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.synth_bop import pipelines, write_tree  # noqa: E402

ROTATE = dict(type="Rotate", level=10, max_rotate_angle=30, prob=0.5, img_fill_val=128)
HBM_BYTES_PER_S = 6.3e12


def _fresh(planned):
    """the planned samples with copies of their RandomStates (the assigner advances them)"""
    return [dict(s, _nprnd=copy.deepcopy(s["_nprnd"])) for s in planned]


def _scatter(times):
    t = np.asarray(times)
    return dict(median=float(np.median(t)), min=float(t.min()), p90=float(np.percentile(t, 90)), max=float(t.max()), n=int(t.size))


def measure(args, root):
    import torch
    from radet_amd import _lib
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_affine.py measures on a GPU; none is visible")
    tree = write_tree(root, n_frames=16, objects=(6, 6), seed=0)
    train, _ = pipelines(tree["background_dir"])
    sub = dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"], seg_prefix=tree["seg_prefix"])
    fixed = build_dataset(dict(sub, pipeline=train))
    ds = dict(fixed=fixed, rotate=build_dataset(dict(sub, pipeline=train[:3] + [ROTATE] + train[3:])), fixed_b=fixed)
    planned = {k: [d.plan_sample(i, *sample_generators(0, 0, i)) for i in range(16)] for k, d in ds.items()}
    res = dict(tool="bench_affine", batch=16, iters=args.iters, rounds=args.rounds, warmup=args.warmup,
               device=torch.cuda.get_device_name(0), clocks="default governor, not pinned; medians over alternating rounds")

    res["samples"] = {k: dict(fired=sum("affine" in s for s in v), output_px=int(sum(s["img_shape"][0] * s["img_shape"][1] for s in v)),
                              boxes=int(sum(len(s["gt_bboxes"]) for s in v)), masks=int(sum(len(s["gt_masks"]) for s in v)),
                              flips=sum(bool(s["flip"]) for s in v), backgrounds=sum("background" in s for s in v))
                      for k, v in planned.items()}
    # what the warp launches of the rotate batch read plus write: every frame and every kept mask once each way
    H, W = 480, 640
    # (masks are warped per group of equal flip; a group in which no sample fired issues no warp launch)
    warped_masks = sum(len(s["gt_masks"]) for s in planned["rotate"]
                       if any("affine" in t and bool(t["flip"]) == bool(s["flip"]) for t in planned["rotate"]))
    res["samples"]["rotate"]["warped_masks"] = int(warped_masks)
    warp_bytes = 2 * 16 * H * W * 3 + 2 * warped_masks * H * W
    res["warp_traffic"] = dict(bytes=warp_bytes, hbm_bytes_per_s=HBM_BYTES_PER_S, floor_ms=warp_bytes / HBM_BYTES_PER_S * 1e3)
    calls = {}
    for k, d in ds.items():
        seen, call = [], _lib.call
        _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
        try:
            out = d.pipeline.run(_fresh(planned[k]), collate=True)
        finally:
            _lib.call = call
        assert tuple(out["img"].shape) == (16, 3, 480, 640)
        calls[k] = seen
    res["entry_points"] = calls
    for k, d in ds.items():                                    # warm-up of every variant's shapes
        for _ in range(args.warmup):
            d.pipeline.run(_fresh(planned[k]), collate=True)
    wall, evt = {k: [] for k in ds}, {k: [] for k in ds}
    rounds = {k: [] for k in ds}
    for _ in range(args.rounds):
        for k, d in ds.items():
            for _ in range(args.iters):
                batch = _fresh(planned[k])
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                d.pipeline.run(batch, collate=True)
                e1.record()
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
                evt[k].append(e0.elapsed_time(e1))
            rounds[k].append(float(np.median(evt[k][-args.iters:])))
    res["run_ms"] = {k: dict(wall=_scatter(wall[k]), event=_scatter(evt[k])) for k in ds}
    res["median_event_ms"] = {k: float(np.median(evt[k])) for k in ds}
    res["round_median_event_ms"] = rounds
    both = rounds["fixed"] + rounds["fixed_b"]
    res["fixed_spread_ms"] = float(max(both) - min(both))
    lo, hi = min(both), max(both)
    res["rotate_within_fixed_spread"] = bool(lo <= res["median_event_ms"]["rotate"] <= hi)
    res["added_ms"] = res["median_event_ms"]["rotate"] - res["median_event_ms"]["fixed"]
    res["added_over_floor"] = res["added_ms"] / res["warp_traffic"]["floor_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_affine.json"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as root:
        res = measure(args, root)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
