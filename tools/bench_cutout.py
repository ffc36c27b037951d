"""CutOut against the fixed-scale pipeline: the device part (ImagePipeline.run) of one planned bs-16 batch each, in one
process on one GPU, default clocks.

    python tools/bench_cutout.py [--iters 20] [--rounds 5] [--out profiles/bench_cutout.json]

`fixed`   = the r50_ycbv_pbr train pipeline: 640 x 480 frames, Resize((640, 480)), output 480 x 640.
`fixed_b` = the same pipeline, the same planned batch, measured as a variant of its own: the difference between the two
            medians, and the spread of the per-round medians, are what run-to-run noise looks like in this process.
`cutout`  = the same with the AutoAugment of configs/base/datasets/bop_detection_cutout.py directly after the Resize
            (policies [Rotate, CutOut], [CutOut], [Translate]), on the same files: warp launches and hole launches.
`holes`   = the same with that config's CutOut stage alone, once directly after the Resize (radet_cutout_u8) and once in
            front of RandomFlip (radet_cutout_f32): hole launches only.
The variants alternate within each round; per call a device event pair around run() and a host clock around the call and
a synchronise.  The yardstick is `fixed`: the stage does not change its code path.  No threshold is set: the added time
(variant - fixed) is reported next to the bytes the hole launches store -- 3 per hole pixel of the u8 launches, 12 per hole
pixel of the f32 launch, a pixel under two holes counted twice, as it is stored twice -- and to the number of launches
added.  Prints one JSON line (and writes it to --out): per variant the medians and scatter, the per-round medians, the
spread of the fixed pipeline (max - min over the per-round medians of fixed and fixed_b), and the entry points each variant
calls."""
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

VARIANTS = ("cutout", "holes")


def _hole_px(rects, h, w):
    r = np.asarray(rects, np.int64).reshape(-1, 4)
    return int((np.clip(np.clip(r[:, 2], 0, w) - np.clip(r[:, 0], 0, w), 0, None) * np.clip(np.clip(r[:, 3], 0, h) - np.clip(r[:, 1], 0, h), 0, None)).sum())


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
    from radet_amd.utils import Config
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_cutout.py measures on a GPU; none is visible")
    tree = write_tree(root, n_frames=16, objects=(6, 6), seed=0)
    train, _ = pipelines(tree["background_dir"])
    sub = dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"], seg_prefix=tree["seg_prefix"])
    fixed = build_dataset(dict(sub, pipeline=train))
    stages = Config.fromfile(os.path.join(ROOT, "configs", "base", "datasets", "bop_detection_cutout.py")).train_pipeline
    auto = next(t for t in stages if t["type"] == "AutoAugment")
    cut = auto["policies"][1][0]
    k = [t["type"] for t in train].index("RandomFlip")
    assert train[2]["type"] == "Resize"
    ds = dict(fixed=fixed, cutout=build_dataset(dict(sub, pipeline=train[:3] + [auto] + train[3:])),
              holes=build_dataset(dict(sub, pipeline=train[:3] + [cut] + train[3:k] + [cut] + train[k:])), fixed_b=fixed)
    planned = {k: [d.plan_sample(i, *sample_generators(0, 0, i)) for i in range(16)] for k, d in ds.items()}
    res = dict(tool="bench_cutout", batch=16, iters=args.iters, rounds=args.rounds, warmup=args.warmup,
               device=torch.cuda.get_device_name(0), clocks="default governor, not pinned; medians over alternating rounds")

    H, W = 480, 640
    res["samples"] = {k: dict(warps=sum(len(s.get("affine", ())) for s in v), hole_entries=sum(len(s.get("cutout", ())) for s in v),
                              late_entries=sum("cutout_late" in s for s in v),
                              holes=int(sum(len(r) for s in v for r, _ in list(s.get("cutout", ())) + ([s["cutout_late"]] if "cutout_late" in s else []))),
                              boxes=int(sum(len(s["gt_bboxes"]) for s in v)), masks=int(sum(len(s["gt_masks"]) for s in v)),
                              flips=sum(bool(s["flip"]) for s in v), backgrounds=sum("background" in s for s in v))
                      for k, v in planned.items()}
    # what the hole launches store
    res["hole_stores"] = {}
    for k in VARIANTS:
        u8 = sum(_hole_px(r, H, W) for s in planned[k] for r, _ in s.get("cutout", ()))
        f32 = sum(_hole_px(s["cutout_late"][0], H, W) for s in planned[k] if "cutout_late" in s)
        res["hole_stores"][k] = dict(u8_px=u8, f32_px=f32, bytes=3 * u8 + 12 * f32, image_bytes=16 * H * W * 3)
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
    res["within_fixed_spread"] = {k: bool(lo <= res["median_event_ms"][k] <= hi) for k in VARIANTS}
    res["added_ms"] = {k: res["median_event_ms"][k] - res["median_event_ms"]["fixed"] for k in VARIANTS}
    res["added_launches"] = {k: {n: calls[k].count(n) - calls["fixed"].count(n) for n in sorted(set(calls[k]))
                                 if calls[k].count(n) != calls["fixed"].count(n)} for k in VARIANTS}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_cutout.json"))
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
