"""Zoom augmentation against the fixed-scale pipeline: the device part (ImagePipeline.run) of one planned bs-16 batch each, in
one process on one GPU, default clocks.

    python tools/bench_zoom.py [--iters 20] [--rounds 3] [--out profiles/bench_zoom.json]

`fixed`   = the r50_ycbv_pbr train pipeline with Resize((640, 480), keep_ratio=False): 640 x 480 frames, output 480 x 640.
`fixed_b` = the same pipeline, the same planned batch, measured as a variant of its own: the difference between the two
            medians, and the spread of the per-round medians, are what run-to-run noise looks like in this process.
`zoom`    = the same with Expand(ratio_range=(1, 2), prob=0.5) + MinIoURandomCrop(min_crop_size=0.3) in front of the Resize
            (configs/base/datasets/bop_detection_zoom.py): the same output pixels, at most the same source pixels read.
The variants alternate within each round; per call a device event pair around run() and a host clock around the call and
a synchronise.  The yardstick is `fixed`: the zoom stages do not change its code path.  Prints one
JSON line (and writes it to --out): per variant the medians and scatter, the per-round medians, the spread of the fixed
pipeline (max - min over the per-round medians of fixed and fixed_b), and the entry points each variant calls."""
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

ZOOM = [dict(type="Expand", mean=[123.675, 116.28, 103.53], to_rgb=True, ratio_range=(1, 2), prob=0.5),
        dict(type="MinIoURandomCrop", min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3)]


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
        raise RuntimeError("tools/bench_zoom.py measures on a GPU; none is visible")
    tree = write_tree(root, n_frames=16, objects=(6, 6), seed=0)
    train, _ = pipelines(tree["background_dir"])
    train[2] = dict(type="Resize", img_scale=(640, 480), keep_ratio=False)
    sub = dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"], seg_prefix=tree["seg_prefix"])
    fixed = build_dataset(dict(sub, pipeline=train))
    ds = dict(fixed=fixed, zoom=build_dataset(dict(sub, pipeline=train[:2] + ZOOM + train[2:])), fixed_b=fixed)
    planned = {k: [d.plan_sample(i, *sample_generators(0, 0, i)) for i in range(16)] for k, d in ds.items()}
    res = dict(tool="bench_zoom", batch=16, iters=args.iters, rounds=args.rounds, warmup=args.warmup,
               device=torch.cuda.get_device_name(0), clocks="default governor, not pinned; medians over alternating rounds")

    def src_px(s):
        """the pixels of the image that the sample's source window covers"""
        h, w = s["img"].shape[:2]
        y0, x0, wh, ww = s["src_window"][:4] if "src_window" in s else (0, 0, h, w)
        return max(0, min(y0 + wh, h) - max(y0, 0)) * max(0, min(x0 + ww, w) - max(x0, 0))
    res["samples"] = {k: dict(windowed=sum("src_window" in s for s in v), expanded=sum("expand" in s for s in v),
                              cropped=sum(s.get("crop_mode", 1) != 1 for s in v), source_px_read=int(sum(src_px(s) for s in v)),
                              output_px=int(sum(s["img_shape"][0] * s["img_shape"][1] for s in v)), boxes=int(sum(len(s["gt_bboxes"]) for s in v)),
                              flips=sum(bool(s["flip"]) for s in v), backgrounds=sum("background" in s for s in v))
                      for k, v in planned.items()}
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
    res["zoom_within_fixed_spread"] = bool(lo <= res["median_event_ms"]["zoom"] <= hi)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_zoom.json"))
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
