"""AutoAugment's colour stages against the fixed-scale pipeline, and their two kernels alone: one process, one GPU,
default clocks.

    python tools/bench_color.py [--iters 20] [--rounds 5] [--out profiles/bench_color.json]

Pipeline part (the device part, ImagePipeline.run, of one planned bs-16 batch each):
`fixed`   = the r50_ycbv_pbr train pipeline: 640 x 480 frames, Resize((640, 480)), output 480 x 640.
`fixed_b` = the same pipeline, the same planned batch, measured as a variant of its own: the difference between the two
            medians, and the spread of the per-round medians, are what run-to-run noise looks like in this process.
`color`   = the same with the AutoAugment of configs/base/datasets/bop_detection_color.py directly after the Resize
            (policies [Rotate, ColorTransform], [EqualizeTransform], [BrightnessTransform, ContrastTransform], [CutOut]), on
            the same files: warp, hole, histogram (with its zero fill) and apply launches.
The variants alternate within each round; per call a device event pair around run() and a host clock around the call and a
synchronise.  No threshold is set: the added time (color - fixed) is reported next to the launches added.

Kernel part (8 frames of 480 x 640 packed back to back, the launches alone, `reps` launches between one event pair):
`stats` / `stats_constant` = radet_color_stats_u8 on decoded synthetic frames / on constant frames (every pixel of a wave
            hits the same four LDS addresses: the worst case of the per-wave histograms), all rows 'equalize';
`apply_<kind>` = radet_color_apply_u8 with all rows of that kind (in place, on the frames as the launches before left them);
`copy`    = radet_copy_segments moving the same bytes (read once, written once), the yardstick of a memory-bound pass;
`fill`    = the radet_fill_zero of the 8 x 4 KB histogram.
The byte floor is the bytes each launch must move (stats: the image once; apply and copy: the image twice) over --hbm-gbs.
Prints one JSON line (and writes it to --out)."""
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


def _fresh(planned):
    """the planned samples with copies of their RandomStates (the assigner advances them)"""
    return [dict(s, _nprnd=copy.deepcopy(s["_nprnd"])) for s in planned]


def _scatter(times):
    t = np.asarray(times)
    return dict(median=float(np.median(t)), min=float(t.min()), p90=float(np.percentile(t, 90)), max=float(t.max()), n=int(t.size))


def measure_pipeline(args, tree, res):
    import torch
    from radet_amd import _lib
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.utils import Config
    train, _ = pipelines(tree["background_dir"])
    sub = dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"], seg_prefix=tree["seg_prefix"])
    fixed = build_dataset(dict(sub, pipeline=train))
    stages = Config.fromfile(os.path.join(ROOT, "configs", "base", "datasets", "bop_detection_color.py")).train_pipeline
    auto = next(t for t in stages if t["type"] == "AutoAugment")
    assert train[2]["type"] == "Resize"
    ds = dict(fixed=fixed, color=build_dataset(dict(sub, pipeline=train[:3] + [auto] + train[3:])), fixed_b=fixed)
    planned = {k: [d.plan_sample(i, *sample_generators(0, 0, i)) for i in range(16)] for k, d in ds.items()}
    res["samples"] = {k: dict(warps=sum(len(s.get("affine", ())) for s in v), hole_entries=sum(len(s.get("cutout", ())) for s in v),
                              colour_entries={kind: sum(op.kind == kind for s in v for op in s.get("color", ()))
                                              for kind in ("color", "equalize", "brightness", "contrast")},
                              ranks=max(len(s.get("block_ops", s.get("affine", ()))) for s in v),
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
    wall, evt, rounds = {k: [] for k in ds}, {k: [] for k in ds}, {k: [] for k in ds}
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
    res["within_fixed_spread"] = bool(min(both) <= res["median_event_ms"]["color"] <= max(both))
    res["added_ms"] = res["median_event_ms"]["color"] - res["median_event_ms"]["fixed"]
    res["added_launches"] = {n: calls["color"].count(n) - calls["fixed"].count(n) for n in sorted(set(calls["color"]))
                             if calls["color"].count(n) != calls["fixed"].count(n)}


def measure_kernels(args, tree, res):
    import torch
    from radet_amd import kernels as K
    from radet_amd.datasets.loading import decode_bgr
    dev = torch.device("cuda", torch.cuda.current_device())
    H, W, N = 480, 640, 8
    files = sorted(os.path.join(dp, f) for dp, _, fs in os.walk(tree["img_prefix"]) for f in fs if f.endswith(".jpg"))[:N]
    frames = [decode_bgr(p) for p in files]
    assert len(frames) == N and all(f.shape == (H, W, 3) for f in frames), [f.shape for f in frames]
    natural = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(dev)
    constant = torch.full_like(natural, 117)
    offs = [i * H * W for i in range(N)]
    nbytes = N * H * W * 3

    def table(kind):
        D = np.zeros((N, K.COLOR_DESC_INTS), np.int32)
        for d, o in zip(D, offs):
            K.color_desc_row(d, o, H, W, kind, 1.18)
        return torch.from_numpy(D).to(dev)

    desc = {kind: table(kind) for kind in K.COLOR_KINDS}
    hist = torch.zeros((N, 4, 256), dtype=torch.int32, device=dev)
    work, dst = natural.clone(), torch.empty_like(natural)
    rows, tiles = K.copy_segments_table([(work.data_ptr(), dst.data_ptr(), nbytes)])
    ctab = torch.from_numpy(rows).to(dev)
    # the statistics the apply launches read: of the natural frames, counted once
    K.color_stats_u8(natural, desc["equalize"], hist, N, H * W)
    stats_hist = hist.clone()
    runs = dict(stats=lambda: K.color_stats_u8(natural, desc["equalize"], hist, N, H * W),
                stats_constant=lambda: K.color_stats_u8(constant, desc["equalize"], hist, N, H * W),
                copy=lambda: K.copy_segments(ctab, 1, tiles), fill=lambda: K.fill_zero(hist),
                **{f"apply_{kind}": (lambda kind=kind: K.color_apply_u8(work, desc[kind], stats_hist, N, H * W)) for kind in K.COLOR_KINDS})
    for fn in runs.values():
        for _ in range(args.warmup):
            fn()
    per = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            per[k].append(e0.elapsed_time(e1) * 1e3 / args.reps)
    moved = {k: nbytes * (1 if k.startswith("stats") else 2) for k in runs if k != "fill"}
    res["kernels"] = dict(frames=N, h=H, w=W, image_bytes=nbytes, reps=args.reps, hbm_gbs=args.hbm_gbs,
                          note="back-to-back launches between one event pair: launch gaps are inside the figure; 7.4 MB fit the L2s "
                               "and the Infinity Cache, so the floor at the HBM rate is a lower bound the passes can beat",
                          us={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in per.items()},
                          floor_us={k: b / (args.hbm_gbs * 1e3) for k, b in moved.items()},
                          gbs={k: moved[k] / (float(np.median(per[k])) * 1e3) for k in moved})
    u = res["kernels"]["us"]
    res["kernels"]["stats_constant_over_natural"] = u["stats_constant"]["median"] / u["stats"]["median"]
    res["kernels"]["over_copy"] = {k: u[k]["median"] / u["copy"]["median"] for k in u if k not in ("copy", "fill")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate the byte floor is computed at (GB/s)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_color.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_color.py measures on a GPU; none is visible")
    res = dict(tool="bench_color", batch=16, iters=args.iters, rounds=args.rounds, warmup=args.warmup,
               device=torch.cuda.get_device_name(0), clocks="default governor, not pinned; medians over alternating rounds")
    with tempfile.TemporaryDirectory() as root:
        tree = write_tree(root, n_frames=16, objects=(6, 6), seed=0)
        measure_pipeline(args, tree, res)
        measure_kernels(args, tree, res)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
