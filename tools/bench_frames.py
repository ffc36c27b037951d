"""Times the preparation of in-memory frames and writes profiles/bench_frames.json:

  * the frame path (ImagePipeline on LoadImageFromWebcam: one pinned upload, one radet_preprocess_frames launch) against
    the file pipeline's device chain (upload, radet_resize_linear_u8, the four augmentation launches) fed the SAME pixels
    from host arrays, per batch of --batch frames of 640 x 480 -> img_scale (640, 480), upload included, planning excluded;
    the two are timed in alternation, round by round, and their outputs are compared bit for bit first;
  * the same frame path on frames that already are device tensors (no pixel upload);
  * `detect_frames` end to end (host frames in, per-class arrays out) in images / s.

Host clock around work that ends in a device synchronise; medians over --reps rounds of --iters batches after a warm-up of
every shape.  No figure here is a pass condition.

    python tools/bench_frames.py [--batch 8] [--iters 50] [--reps 7] [--frames 400]

--tta times test-time augmentation instead and writes profiles/bench_tta.json: `inference_detector(frames)` with a set_tta override of
V = 2 views (img_scale (640, 480), unflipped + horizontal flip: one forward batch of 2 * --batch) against the yardstick,
V single-view `inference_detector` calls on the same frames in the same process, in alternating rounds; and, between HIP
events, the radet_merge_views launch on the call's own candidate pool and a radet_preprocess_frames launch with flipped rows
beside the same launch without flips.  The single-view call's launch sequence is recorded (names and count) so that it can be
compared with the commit before.

    python tools/bench_frames.py --tta [--batch 4] [--iters 20] [--reps 7]

--tiles times tiled inference instead and writes profiles/bench_tiles.json: `inference_detector(frame)` on one 1080 x 1920
frame with set_tiling(tile=(640, 480), overlap=0.25): 12 tiles + the full frame, one forward batch of 13, one merge, one NMS,
against `inference_detector` on the 13 copied slices as one batch (what the code could do without tiling: 13 separate
results in tile coordinates), in alternating rounds; and, between HIP events, radet_merge_tiles on synthetic pools of 8 images
x 13 and x 64 rows x cap 1000 at 30 % and full fill, beside radet_merge_views on the same candidate volume where it can take it.

    python tools/bench_frames.py --tiles [--iters 5] [--reps 5]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def pipeline_cfg(loader):
    return [dict(type=loader),
            dict(type="MultiScaleFlipAug", img_scale=(640, 480), flip=False, transforms=[
                dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", **NORM),
                dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])])]


def wall_ms(fn, iters):
    """host milliseconds per call of `iters` back-to-back calls, the last one followed by a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def event_ms(fn, iters):
    """device milliseconds per launch of `iters` back-to-back launches between two HIP events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def log_calls(fn):
    from radet_amd import _lib
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        fn()
    finally:
        _lib.call = call
    return seen


def band(xs):
    xs = sorted(xs)
    return [xs[int(0.1 * (len(xs) - 1))], xs[int(round(0.9 * (len(xs) - 1)))]]


def tta_main(args):
    from radet_amd import kernels as K
    from radet_amd.apis import inference_detector, set_tta
    from radet_amd.apis.inference import _frame_pipeline, _prepare_frames
    from radet_amd.datasets.loading import frame_desc_rows
    from radet_amd.models import build_detector
    from radet_amd.runtime import _aug_plan
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill
    dev = torch.device("cuda")
    B = args.batch
    rng = np.random.RandomState(0)
    frames = [rng.randint(0, 256, (480, 640, 3)).astype(np.uint8) for _ in range(B)]
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(dev).eval()
    synth_fill(model, seed=0)
    with torch.no_grad():
        model.bbox_head.atss_cls.bias += 2.0                        # (candidates above the threshold: full lists)
    model.cfg = Config(dict(data=dict(test=dict(pipeline=pipeline_cfg("LoadImageFromFile")))))
    tta = dict(img_scale=[(640, 480)], flip=True, flip_direction="horizontal")
    V = 2
    def tta_call():
        set_tta(model, tta)
        try:
            return inference_detector(model, frames)
        finally:
            set_tta(model, None)
    paths = dict(tta=tta_call,
                 single_x_v=lambda: [inference_detector(model, frames) for _ in range(V)])
    for fn in paths.values():
        wall_ms(fn, 3)
    single_log = log_calls(lambda: inference_detector(model, frames))
    tta_log = log_calls(paths["tta"])
    rounds = {k: [] for k in paths}
    for _ in range(args.reps):
        for k, fn in paths.items():                                 # alternating: drift hits both alike
            rounds[k].append(wall_ms(fn, args.iters))
    # the merge launch alone, on the pool the call above left behind
    rt = model.runtime()
    data = _prepare_frames(_frame_pipeline(model, tta), frames)
    plan = _aug_plan(rt, data["img"], data["img_metas"], model.test_cfg)
    p = next(v for k, v in rt._posts.items() if k[0] == "aug")
    host_desc = plan["tables"]["desc"]
    desc = torch.from_numpy(host_desc).to(dev)

    def merge():
        K.merge_views(host_desc, desc, V, B, p["pool_boxes"], p["pool_scores"], p["pool_ctr"], p["pool_labels"], p["row_count"],
                      plan["cap_out"], p["boxes"], p["scores"], p["ctr"], p["labels"], p["count"])
    # the preparation launch: V * B rows with the second half flipped, beside the same rows unflipped
    buf = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(dev)
    mean = np.array(NORM["mean"], np.float32)
    stdinv = (1.0 / np.array(NORM["std"], np.float64)).astype(np.float32)
    out = torch.empty(V * B, 3, 480, 640, device=dev)
    tables = {}
    for name, flips in (("flipped", [0] * B + [K.PREP_FLIP_H] * B), ("unflipped", [0] * (V * B))):
        rows, _, _ = frame_desc_rows(frames, [(480, 640)] * (V * B), True, buf.data_ptr(), views=V, flips=flips)
        tables[name] = torch.from_numpy(rows).to(dev)
    launches = dict(merge_views_ms=merge,
                    preprocess_flipped_ms=lambda: K.preprocess_frames(tables["flipped"], V * B, 480, 640, mean, stdinv, out),
                    preprocess_unflipped_ms=lambda: K.preprocess_frames(tables["unflipped"], V * B, 480, 640, mean, stdinv, out))
    for fn in launches.values():
        event_ms(fn, 10)
    lrounds = {k: [] for k in launches}
    for _ in range(args.reps):
        for k, fn in launches.items():
            lrounds[k].append(event_ms(fn, 50))
    counts = p["row_count"].cpu().tolist()
    med = statistics.median
    out = dict(case=dict(batch=B, views=V, frame_hw=[480, 640], tta=dict(img_scale=[[640, 480]], flip=True, flip_direction="horizontal"),
                         forward_batch=V * B, nms_pre=int(model.test_cfg["nms_pre"]), merged_capacity=plan["cap_out"],
                         candidates_per_view_row=[min(counts), max(counts)], iters=args.iters, reps=args.reps),
               device=torch.cuda.get_device_name(0), clocks="default governor, not pinned; medians of alternating rounds",
               yardstick="V single-view inference_detector calls on the same frames, same process (the single-view path issues "
                         "the launches of the commit before: single_view_launches)",
               tta_call_ms=med(rounds["tta"]), single_view_x_v_ms=med(rounds["single_x_v"]),
               tta_over_yardstick=med(rounds["tta"]) / med(rounds["single_x_v"]),
               tta_call_ms_band=band(rounds["tta"]), single_view_x_v_ms_band=band(rounds["single_x_v"]),
               tta_call_ms_all=rounds["tta"], single_view_x_v_ms_all=rounds["single_x_v"],
               **{k: med(v) for k, v in lrounds.items()}, **{k + "_all": v for k, v in lrounds.items()},
               single_view_launches=len(single_log), tta_launches=len(tta_log),
               single_view_launch_tail=single_log[-3:], single_view_first_launch=single_log[0],
               tta_launch_counts={n: tta_log.count(n) for n in ("radet_preprocess_frames", "radet_decode_candidates",
                                                                "radet_merge_views", "radet_nms")})
    path = args.out or os.path.join(ROOT, "profiles", "bench_tta.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def tiles_main(args):
    from radet_amd import kernels as K
    from radet_amd.apis import inference_detector, set_tiling
    from radet_amd.models import build_detector
    from radet_amd.ops.tiles import tile_rows
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill
    dev = torch.device("cuda")
    rng = np.random.RandomState(0)
    frame = rng.randint(0, 256, (1080, 1920, 3)).astype(np.uint8)
    tiling = dict(tile=(640, 480), overlap=0.25, full_frame=True, batch=16)
    rects, _, row_start = tile_rows([frame.shape[:2]], tiling)
    slices = [np.ascontiguousarray(frame[y0:y0 + th, x0:x0 + tw]) for x0, y0, tw, th in rects.tolist()]
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(dev).eval()
    synth_fill(model, seed=0)
    with torch.no_grad():
        model.bbox_head.atss_cls.bias += 2.0                        # (candidates above the threshold: full lists)
    model.cfg = Config(dict(data=dict(test=dict(pipeline=pipeline_cfg("LoadImageFromFile")))))

    def tiled_call():
        set_tiling(model, tiling)
        try:
            return inference_detector(model, frame)
        finally:
            set_tiling(model, None)
    paths = dict(tiled=tiled_call, slices_one_batch=lambda: inference_detector(model, slices))
    for fn in paths.values():
        wall_ms(fn, 3)
    tiled_log = log_calls(paths["tiled"])
    rounds = {k: [] for k in paths}
    for _ in range(args.reps):
        for k, fn in paths.items():                                 # alternating: drift hits both alike
            rounds[k].append(wall_ms(fn, args.iters))
    row_counts = next(v for k, v in model.runtime()._posts.items() if k[0] == "tiles")["row_count"].cpu().tolist()

    # the merge launch alone on synthetic pools: B images x rows x cap, every row filled to `fill` of its cap, a quarter of
    # the candidates on a cut edge; radet_merge_views beside it on the same candidate volume (it takes at most 16 views)
    def pool_case(B, rows, cap, fill):
        Rn, n = B * rows, B * rows * cap
        g = torch.Generator(device="cpu").manual_seed(1)
        lo = torch.rand(n, 2, generator=g) * 200 + 1
        boxes = torch.cat([lo, lo + 50 + torch.rand(n, 2, generator=g) * 100], 1)
        boxes[::4, 2] = 640.0
        p = dict(boxes=boxes.to(dev), scores=torch.rand(n, generator=g).to(dev), ctr=torch.rand(n, generator=g).to(dev),
                 labels=torch.zeros(n, dtype=torch.long, device=dev),
                 counts=torch.full((Rn,), int(fill * cap), dtype=torch.int32, device=dev))
        cap_out = rows * cap
        outs = (torch.empty(B, cap_out, 4, device=dev), torch.empty(B, cap_out, device=dev), torch.empty(B, cap_out, device=dev),
                torch.empty(B, cap_out, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
        dropped = torch.zeros(B, dtype=torch.int32, device=dev)
        hw, sf = np.tile(np.array([[480.0, 640.0]], np.float32), (Rn, 1)), np.full((Rn, 4), 1.5, np.float32)
        tdesc = K.tile_desc_rows(hw, sf, np.full((Rn, 2), 426.0), np.full(Rn, 15, np.int32), np.arange(Rn) * cap, np.full(Rn, cap))
        rs = (np.arange(B + 1) * rows).astype(np.int32)
        tdev, rdev = torch.from_numpy(tdesc).to(dev), torch.from_numpy(rs).to(dev)
        fns = dict(merge_tiles=lambda: K.merge_tiles(tdesc, tdev, rs, rdev, B, p["boxes"], p["scores"], p["ctr"], p["labels"],
                                                     p["counts"], 0.0, cap_out, *outs, dropped))
        if rows <= K.TTA_MAX_VIEWS:
            vdesc = K.merge_desc_rows(hw, sf, np.zeros(Rn, np.int32), np.arange(Rn) * cap, np.full(Rn, cap))
            vdev = torch.from_numpy(vdesc).to(dev)
            fns["merge_views"] = lambda: K.merge_views(vdesc, vdev, rows, B, p["boxes"], p["scores"], p["ctr"], p["labels"],
                                                       p["counts"], cap_out, *outs)
        for fn in fns.values():
            event_ms(fn, 10)
        r = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():                               # interleaved launches, medians
                r[k].append(event_ms(fn, 50))
        return dict(images=B, rows_per_image=rows, cap=cap, fill=fill, candidates=int(fill * cap) * Rn,
                    **{k + "_us": statistics.median(v) * 1e3 for k, v in r.items()},
                    **{k + "_us_band": [x * 1e3 for x in band(v)] for k, v in r.items()},
                    **{k + "_us_all": [x * 1e3 for x in v] for k, v in r.items()})
    cases = [pool_case(8, 13, 1000, 0.3), pool_case(8, 13, 1000, 1.0), pool_case(8, 64, 1000, 0.3), pool_case(8, 64, 1000, 1.0)]
    med = statistics.median
    out = dict(case=dict(frame_hw=[1080, 1920], tiling=dict(tile=[640, 480], overlap=0.25, full_frame=True, batch=16),
                         rows=int(row_start[-1]), nms_pre=int(model.test_cfg["nms_pre"]), candidates_per_row=[min(row_counts), max(row_counts)],
                         iters=args.iters, reps=args.reps),
               device=torch.cuda.get_device_name(0), clocks="default governor, not pinned; medians of alternating rounds",
               yardstick="inference_detector on the 13 copied slices as ONE batch, same process: what the commit before can do for "
                         "the same rows (13 separate results in tile coordinates, no merge)",
               tiled_call_ms=med(rounds["tiled"]), slices_one_batch_ms=med(rounds["slices_one_batch"]),
               tiled_over_yardstick=med(rounds["tiled"]) / med(rounds["slices_one_batch"]),
               tiled_call_ms_band=band(rounds["tiled"]), slices_one_batch_ms_band=band(rounds["slices_one_batch"]),
               tiled_call_ms_all=rounds["tiled"], slices_one_batch_ms_all=rounds["slices_one_batch"],
               tiled_launches=len(tiled_log),
               tiled_launch_counts={n: tiled_log.count(n) for n in ("radet_preprocess_frames", "radet_decode_candidates",
                                                                    "radet_merge_tiles", "radet_nms")},
               merge_launch=cases)
    path = args.out or os.path.join(ROOT, "profiles", "bench_tiles.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=400, help="frames of the end-to-end pass")
    ap.add_argument("--tta", action="store_true", help="time test-time augmentation instead -> profiles/bench_tta.json")
    ap.add_argument("--tiles", action="store_true", help="time tiled inference instead -> profiles/bench_tiles.json")
    ap.add_argument("--out", default=None, help="default: profiles/bench_frames.json (profiles/bench_tta.json with --tta, "
                                                "profiles/bench_tiles.json with --tiles)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames.py measures on the GPU: no device found")
    if args.tta:
        return tta_main(args)
    if args.tiles:
        return tiles_main(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "bench_frames.json")
    from radet_amd.apis import detect_frames
    from radet_amd.datasets.loading import ImagePipeline
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill
    dev = torch.device("cuda")
    B = args.batch
    rng = np.random.RandomState(0)
    frames = [rng.randint(0, 256, (480, 640, 3)).astype(np.uint8) for _ in range(B)]
    on_dev = [torch.from_numpy(f).to(dev) for f in frames]
    new, old = ImagePipeline(pipeline_cfg("LoadImageFromWebcam")), ImagePipeline(pipeline_cfg("LoadImageFromFile"))

    def plan(imgs):
        return [new.plan(dict(img=f, bbox_fields=[], mask_fields=[], seg_fields=[]), random, np.random) for f in imgs]
    planned, planned_dev = plan(frames), plan(on_dev)
    # (a planned frame is what the file pipeline plans for a decoded file, but for the file names: its device chain takes it)
    a = new.run(planned, collate=True)["img"][0]
    b = old.run(planned, collate=True)["img"][0]
    c = new.run(planned_dev, collate=True)["img"][0]
    torch.cuda.synchronize()
    equal = bool(torch.equal(a, b) and torch.equal(a, c))
    paths = dict(frames_ms=lambda: new.run(planned, collate=True), file_chain_ms=lambda: old.run(planned, collate=True),
                 device_frames_ms=lambda: new.run(planned_dev, collate=True))
    for fn in paths.values():                                       # warm-up: code objects, pinned and device allocator
        wall_ms(fn, 10)
    rounds = {k: [] for k in paths}
    for _ in range(args.reps):
        for k, fn in paths.items():                                 # alternating: drift hits every path alike
            rounds[k].append(wall_ms(fn, args.iters))
    plan_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        plan(frames)
        plan_ms.append((time.perf_counter() - t0) * 1e3)

    cfg = Config.fromfile(os.path.join(ROOT, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(dev).eval()
    synth_fill(model, seed=0)
    model.cfg = Config(dict(data=dict(test=dict(pipeline=pipeline_cfg("LoadImageFromFile")))))
    n = -(-args.frames // B) * B

    def end_to_end():
        return sum(1 for _ in detect_frames(model, (frames[i % B] for i in range(n)), batch_size=B))
    end_to_end()
    e2e = []
    for _ in range(max(3, args.reps // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert end_to_end() == n
        torch.cuda.synchronize()
        e2e.append(n / (time.perf_counter() - t0))

    med = statistics.median
    out = dict(case=dict(batch=B, frame_hw=[480, 640], img_scale=[640, 480], pad_divisor=32, iters=args.iters, reps=args.reps),
               device=torch.cuda.get_device_name(0), clocks="default governor, not pinned; medians of alternating rounds",
               outputs_bit_identical=equal,
               prepare_frames_ms=med(rounds["frames_ms"]), prepare_file_chain_ms=med(rounds["file_chain_ms"]),
               prepare_device_frames_ms=med(rounds["device_frames_ms"]),
               prepare_frames_ms_all=rounds["frames_ms"], prepare_file_chain_ms_all=rounds["file_chain_ms"],
               prepare_device_frames_ms_all=rounds["device_frames_ms"],
               file_chain_over_frames=med(rounds["file_chain_ms"]) / med(rounds["frames_ms"]),
               plan_ms_per_batch=med(plan_ms), detect_frames_images=n, detect_frames_img_per_s=med(e2e),
               detect_frames_img_per_s_all=e2e)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
