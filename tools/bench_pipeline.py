"""Measures the BOP image pipeline (radet_amd.datasets.loading / loader) on a synthetic 640x480 BOP tree written from a seed.

    python tools/bench_pipeline.py --part kernels [--iters 20]     # the device part of bs-16 batches, every stage on
                                                                   # (run it under `rocprofv3 --kernel-trace --stats`)
    python tools/bench_pipeline.py --part decode                   # host planning (decode + draws) per thread count
    python tools/bench_pipeline.py --part train [--steps 60]       # r50_ycbv_pbr fp32 bs 16: loader-fed vs one prebuilt batch
    python tools/bench_pipeline.py --part maskfree [--iters 7]     # GenerateDistanceMap(with_gt_mask=False), gdt-sobel and mbd:
                                                                   # the batched device chain vs per-sample host calls vs masks
                                                                   # (one GPU step: run it under its own time limit,
                                                                   #  timeout -k 10 400 python tools/bench_pipeline.py --part
                                                                   #  maskfree --out profiles/bench_pipeline_maskfree.json)
    python tools/bench_pipeline.py --part rle [--iters 20]          # the same frames under PNG-path and RLE annotations:
                                                                   # host plan, device mask stage, loader-fed training
                                                                   # (timeout -k 10 500 python tools/bench_pipeline.py --part rle
                                                                   #  --out profiles/bench_pipeline_rle.json)
    python tools/bench_pipeline.py --part jpeg [--iters 20] [--steps 30]   # the same frames with decode='host' and 'device':
                                                                   # host plan (cold / cached index), the decode stage per
                                                                   # launch for seg_mcus 8 / 16 / row, loader-fed training
                                                                   # (timeout -k 10 700 python tools/bench_pipeline.py --part jpeg
                                                                   #  --steps 30 --out profiles/bench_pipeline_jpeg.json)
    python tools/bench_pipeline.py --part cache [--iters 20] [--steps 30]  # the same frames without and with sample_cache='device',
                                                                   # PNG masks + host decoding and run lists + device decoding
                                                                   # (timeout -k 10 900 python tools/bench_pipeline.py --part cache
                                                                   #  --steps 30 --out profiles/bench_pipeline_cache.json)
    python tools/bench_pipeline.py --part jitter [--iters 20]       # Resize(ratio_range) + RandomCrop + Pad(size) against the
                                                                   # fixed-scale pipeline on the same files, output 480 x 640
                                                                   # both: the device part of one bs-16 batch, alternating rounds
                                                                   # (timeout -k 10 400 python tools/bench_pipeline.py --part
                                                                   #  jitter --out profiles/bench_jitter.json)
`--pipeline mix` runs the mixpbr train pipeline instead (RandomHSV / RandomNoise / RandomSmooth in place of CosyPoseAug,
the training set a MixDataset of the tree twice, ratios 2 and 1).
Each part prints one JSON line (and writes it to --out if given)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.synth_bop import pipelines, write_tree  # noqa: E402


MIX_STAGES = [dict(type="RandomHSV", h_ratio=0.2, s_ratio=0.5, v_ratio=0.5, prob=1.0),
              dict(type="RandomNoise", noise_ratio=0.1, prob=1.0),
              dict(type="RandomSmooth", max_kernel_size=7, prob=1.0)]


def dataset(root, n_frames, all_on=False, mix=False):
    from radet_amd.datasets import build_dataset
    tree = write_tree(root, n_frames=n_frames, seed=0)
    train, _ = pipelines(tree["background_dir"], bg_prob=1.0 if all_on else 0.3, cosy_p=1.0 if all_on else 0.8)
    if all_on:
        for st in train[4]["pipelines"]:
            st["p"] = 1.0
    sub = dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"], seg_prefix=tree["seg_prefix"])
    if not mix:
        return build_dataset(dict(sub, pipeline=train))
    train = train[:4] + MIX_STAGES + train[5:]
    return build_dataset(dict(type="MixDataset", dataset_0=dict(sub, pipeline=train, ratio=2),
                              dataset_1=dict(sub, pipeline=train, ratio=1)))


def part_kernels(args, root):
    import torch
    from radet_amd.datasets.loader import sample_generators
    ds = dataset(root, 16, all_on=True, mix=args.pipeline == "mix")
    planned = [ds.plan_sample(i, *sample_generators(0, 0, i)) for i in range(16)]
    key = "aug_smooth" if args.pipeline == "mix" else "aug_color"
    assert all("background" in s and key in s for s in planned)
    for s in planned:          # every stage on, blur / box at its widest
        s["aug_smooth" if args.pipeline == "mix" else "aug_blur"] = 7 if args.pipeline == "mix" else 3
    pipe = ds.pipeline
    pipe.run(planned, collate=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        pipe.run(planned, collate=True)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.iters
    px = 16 * 480 * 640
    # bytes of the four augmentation launches: merge+hblur reads image + background + masks, writes image; vblur, sharp
    # read + write the image; finish reads the image, writes f32 x 3
    masks = sum(int(s["gt_masks"].shape[0]) for s in planned) * 480 * 640
    aug_bytes = (3 * px * 2 + masks + 3 * px) + 3 * px * 2 + 3 * px * 2 + (3 * px + 12 * px)
    # (mix: hsv_noise and box each read + write the image in place of vblur and sharp: the same count; the two mix
    # launches alone move 4 x 3 px bytes)
    return dict(part="kernels", pipeline=args.pipeline, batch=16, iters=args.iters, host_ms_per_batch=dt * 1e3,
                aug_kernel_bytes=aug_bytes, mix_kernel_bytes=4 * 3 * px if args.pipeline == "mix" else None)


def part_decode(args, root):
    from concurrent.futures import ThreadPoolExecutor
    from radet_amd.datasets.loader import sample_generators
    ds = dataset(root, 32, mix=args.pipeline == "mix")
    out = {}
    for threads in (1, 2, 4, 8, 12, 16):
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(lambda i: ds.plan_sample(i, *sample_generators(0, 0, i)), range(4)))
            t0 = time.perf_counter()
            n = 0
            for rep in range(2):
                list(pool.map(lambda i: ds.plan_sample(i, *sample_generators(0, rep, i)), range(len(ds))))
                n += len(ds)
            out[threads] = n / (time.perf_counter() - t0)
    return dict(part="decode", pipeline=args.pipeline, images_per_s_by_threads=out)


def part_train(args, root):
    import torch
    from oracle import synth
    from radet_amd.datasets import build_dataloader
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    ds = dataset(root, 64, mix=args.pipeline == "mix")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    synth.fill_state_dict(det.state_dict(), seed=0)
    det = det.cuda().train()
    rt = det.runtime()
    rt.init_optimizer(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, max_norm=35.0)
    rt.set_loss_from_head(det.bbox_head)
    loader = build_dataloader(ds, samples_per_gpu=16, workers=args.workers, seed=0)

    def stream():
        epoch = 0
        while True:
            loader.set_epoch(epoch)
            yield from loader
            epoch += 1
    it = stream()
    fixed = next(it)

    def step(b):
        tg = rt.pack_targets(b["gt_bboxes"], b["gt_labels"], b["points_to_gt_index"], b["points_weight"])
        rt.train_step(b["img"], tg, lr=1e-4)

    for _ in range(args.warmup):
        step(fixed)
        step(next(it))
    torch.cuda.synchronize()
    res = dict(prebuilt=[], loader=[])
    for rnd in range(args.rounds):
        for name in ("prebuilt", "loader"):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(fixed if name == "prebuilt" else next(it))
            torch.cuda.synchronize()
            res[name].append(16 * args.steps / (time.perf_counter() - t0))
    loader.close()
    med = {k: float(np.median(v)) for k, v in res.items()}
    return dict(part="train", pipeline=args.pipeline, batch=16, steps=args.steps, rounds=args.rounds, workers=loader.workers,
                images_per_s=res, median=med, loader_over_prebuilt=med["loader"] / med["prebuilt"],
                replays=(rt.tape_stats() or {}).get("replays"))


MASK_FREE = dict(gdt=dict(type="GenerateDistanceMap", with_gt_mask=False, distance_transform="gdt", edge_mode="sobel"),
                 mbd=dict(type="GenerateDistanceMap", with_gt_mask=False, distance_transform="mbd"))


def _median_ms(fn, iters):
    import torch
    fn()                                                    # warm-up (allocator, pinned staging, code objects)
    fn()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), times


def part_maskfree(args, root):
    """bs 16, 640 x 480, 6 boxes per image.  Per transform: (a) the batched chain crop -> pasted maps
    (ImagePipeline._distance_maps), (b) GenerateDistanceMap.__call__ per sample on host copies of the same augmented
    images (the only way to these maps before the chain existed), (c) the mask pipeline's whole batch; and the chain's
    time per entry point, each launch timed between two device synchronisations."""
    import torch
    from radet_amd import _lib, kernels as K
    from radet_amd.datasets import PIPELINES, build_dataset
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.utils import build_from_cfg
    tree = write_tree(root, n_frames=16, objects=(6, 6), seed=0)
    train, _ = pipelines(tree["background_dir"])
    at = [t["type"] for t in train].index("GenerateDistanceMap")
    if args.pipeline == "mix":
        train = train[:4] + MIX_STAGES + train[5:]
        at = [t["type"] for t in train].index("GenerateDistanceMap")

    def build(dm):
        return build_dataset(dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"],
                                  seg_prefix=tree["seg_prefix"], pipeline=train[:at] + [dm] + train[at + 1:]))

    def plan(ds):
        return [ds.plan_sample(i, *sample_generators(0, 0, i)) for i in range(16)]
    mask_ds = build(dict(type="GenerateDistanceMap"))
    mask_plan = plan(mask_ds)
    mask_ms, _ = _median_ms(lambda: mask_ds.pipeline.run(_fresh(mask_plan), collate=True), args.iters)
    res = dict(part="maskfree", pipeline=args.pipeline, batch=16, iters=args.iters, mask_pipeline_ms=mask_ms)
    for name, dm in MASK_FREE.items():
        ds = build(dm)
        pipe, planned = ds.pipeline, plan(ds)
        nbox = sum(len(s["gt_bboxes"]) for s in planned)
        grabbed, inner = [], pipe._distance_maps
        pipe._distance_maps = lambda *a: grabbed.append(a) or inner(*a)
        pipe.run(_fresh(planned), collate=True)
        del pipe._distance_maps
        chain_args = grabbed[0]
        chain_ms, _ = _median_ms(lambda: pipe._distance_maps(*chain_args), args.iters)
        run_ms, _ = _median_ms(lambda: pipe.run(_fresh(planned), collate=True), args.iters)
        # host copies of the augmented images: one canvas per image that covers it
        _, hw, img, lsum, params, dev = chain_args
        D = np.zeros((16, K.CROP_DESC_INTS), np.int32)
        o = 0
        for i, (h, w) in enumerate(hw):
            D[i] = [i, 0, 0, w, h, 0, 0, w, h, 0, o, 0]
            o += h * w
        full = torch.empty(o * 3, dtype=torch.uint8, device=dev)
        K.crop_canvases(img, lsum, params, 16, torch.from_numpy(D).to(dev), 16, max(h * w for h, w in hw), full)
        host, o = [], 0
        for h, w in hw:
            host.append(full[o * 3:(o + h * w) * 3].view(h, w, 3).cpu().numpy())
            o += h * w
        gdm = build_from_cfg(dm, PIPELINES)

        def per_sample():
            return [gdm(dict(img=im, img_shape=im.shape, gt_bboxes=s["gt_bboxes"]))["distance_maps"] for im, s in zip(host, planned)]
        host_ms, _ = _median_ms(per_sample, args.iters)
        # the chain's entry points one by one (synchronised: the sum exceeds the chain's own time by the lost overlap)
        by_name, call = {}, _lib.call

        def timed(fn_name, *a):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = call(fn_name, *a)
            torch.cuda.synchronize()
            by_name.setdefault(fn_name, []).append((time.perf_counter() - t0) * 1e3)
            return out
        pipe._distance_maps(*chain_args)
        _lib.call = timed
        try:
            for _ in range(args.iters):
                pipe._distance_maps(*chain_args)
        finally:
            _lib.call = call
        launches = {k: dict(calls_per_batch=len(v) // args.iters, ms_per_batch=float(np.sum(v) / args.iters)) for k, v in by_name.items()}
        res[name] = dict(boxes=nbox, transformed=int(sum(s["_crop_plan"][0].large.sum() for s in planned)),
                         chain_ms=chain_ms, per_sample_host_ms=host_ms, chain_over_per_sample=chain_ms / host_ms,
                         chain_share_of_mask_pipeline=chain_ms / mask_ms, maskfree_pipeline_ms=run_ms, entry_points=launches)
    return res


def _scatter(times):
    t = np.asarray(times, np.float64)
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), p25=float(np.percentile(t, 25)),
                p75=float(np.percentile(t, 75)), n=int(t.size))


def part_rle(args, root):
    """bs 16, 640 x 480, 6 objects per image; one tree annotated twice (visible-mask PNG paths / run lists in the json).
    (a) host plan per sample and images/s at 1 / 12 / 16 threads; (b) the device mask stage of one batch
    (ImagePipeline._masks: upload + mask_max + mask_transform + flip, against upload + rle_masks), each call between two
    device synchronisations, and the same with a device event pair; (c) loader-fed training images/s, as in --part train."""
    import copy
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from radet_amd.datasets import build_dataloader, build_dataset
    from radet_amd.datasets.bop_convert import add_segmentation
    from radet_amd.datasets.loader import sample_generators
    tree = write_tree(root, n_frames=64, objects=(6, 6), seed=0)
    ann = os.path.join(root, "train_pbr_rle.json")
    with open(tree["ann_file"]) as f:
        coco = add_segmentation(json.load(f), tree["seg_prefix"], "rle")
    with open(ann, "w") as f:
        json.dump(coco, f)
    train, _ = pipelines(tree["background_dir"])
    rle_train = copy.deepcopy(train)
    rle_train[1] = dict(type="LoadAnnotations", with_bbox=True, with_mask=True)
    ds = dict(png=build_dataset(dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"],
                                     seg_prefix=tree["seg_prefix"], pipeline=train)),
              rle=build_dataset(dict(type="BOPDataset", ann_file=ann, img_prefix=tree["img_prefix"], mask_source="annotation",
                                     pipeline=rle_train)))
    res = dict(part="rle", batch=16, iters=args.iters, frames=len(ds["png"]), masks_per_batch=96,
               ann_file_bytes=dict(png=os.path.getsize(tree["ann_file"]), rle=os.path.getsize(ann)))
    # (a) host planning
    host = {}
    for name, d in ds.items():
        d.plan_sample(0, *sample_generators(0, 0, 0))
        per = []
        for i in range(len(d)):
            t0 = time.perf_counter()
            d.plan_sample(i, *sample_generators(0, 0, i))
            per.append((time.perf_counter() - t0) * 1e3)
        # the mask share alone: LoadAnnotations.plan on a sample whose image is already decoded
        stage, only = d.pipeline.transforms[1], []
        for i in range(len(d)):
            s = d._results(i, True)
            t0 = time.perf_counter()
            stage.plan(s, None, None)
            only.append((time.perf_counter() - t0) * 1e3)
        rate = {}
        for threads in (1, 12, 16):
            with ThreadPoolExecutor(threads) as pool:
                list(pool.map(lambda i: d.plan_sample(i, *sample_generators(0, 0, i)), range(threads)))
                runs = []
                for rep in range(3):
                    t0 = time.perf_counter()
                    list(pool.map(lambda i: d.plan_sample(i, *sample_generators(0, rep, i)), range(len(d))))
                    runs.append(len(d) / (time.perf_counter() - t0))
                rate[threads] = dict(median=float(np.median(runs)), runs=runs)
        host[name] = dict(plan_ms_per_sample=_scatter(per), load_annotations_ms_per_sample=_scatter(only), images_per_s_by_threads=rate)
    res["host"] = host
    # (b) the device mask stage of one batch
    dev_res = {}
    for name, d in ds.items():
        planned = [d.plan_sample(i, *sample_generators(0, 0, i)) for i in range(16)]
        assert sum(len(s["gt_bboxes"]) for s in planned) == 96 and any(s["flip"] for s in planned)
        hw = [tuple(s["resize_hw"]) for s in planned]
        dev = d.pipeline._dev()
        wall, evt = [], []
        for it in range(args.iters + 3):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            d.pipeline._masks(planned, hw, dev)
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                wall.append((time.perf_counter() - t0) * 1e3)
                evt.append(e0.elapsed_time(e1))
        up = (sum(s["gt_masks"].nbytes for s in planned) if name == "png" else
              4 * sum(c.size for s in planned for m in s["gt_masks_rle"][0] for c in m))
        dev_res[name] = dict(wall_ms=_scatter(wall), event_ms=_scatter(evt), upload_bytes=int(up))
    res["device_mask_stage"] = dev_res
    # (c) loader-fed training
    if args.steps > 0:
        from oracle import synth
        from radet_amd.models import build_detector
        from radet_amd.utils import Config
        cfg = Config.fromfile(os.path.join(ROOT, "configs", "bop", "r50_ycbv_pbr.py"))
        cfg.model["pretrained"] = None
        torch.manual_seed(0)
        det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
        synth.fill_state_dict(det.state_dict(), seed=0)
        det = det.cuda().train()
        rt = det.runtime()
        rt.init_optimizer(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, max_norm=35.0)
        rt.set_loss_from_head(det.bbox_head)

        def step(b):
            tg = rt.pack_targets(b["gt_bboxes"], b["gt_labels"], b["points_to_gt_index"], b["points_weight"])
            rt.train_step(b["img"], tg, lr=1e-4)
        loaders = {k: build_dataloader(d, samples_per_gpu=16, workers=args.workers, seed=0) for k, d in ds.items()}

        def stream(loader):
            epoch = 0
            while True:
                loader.set_epoch(epoch)
                yield from loader
                epoch += 1
        its = {k: stream(v) for k, v in loaders.items()}
        fixed = next(its["png"])
        for _ in range(args.warmup):
            step(fixed)
            step(next(its["png"]))
            step(next(its["rle"]))
        torch.cuda.synchronize()
        rates = dict(prebuilt=[], png=[], rle=[])
        for rnd in range(args.rounds):
            for name in rates:
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(fixed if name == "prebuilt" else next(its[name]))
                torch.cuda.synchronize()
                rates[name].append(16 * args.steps / (time.perf_counter() - t0))
        for v in loaders.values():
            v.close()
        med = {k: float(np.median(v)) for k, v in rates.items()}
        res["train"] = dict(steps=args.steps, rounds=args.rounds, workers=args.workers, images_per_s=rates, median=med,
                            png_over_prebuilt=med["png"] / med["prebuilt"], rle_over_prebuilt=med["rle"] / med["prebuilt"])
    return res


def part_jpeg(args, root):
    """bs 16, 640 x 480, the frames of --part rle under run-list annotations; the same call runs decode='host' (the
    baseline) and decode='device'.  (a) host plan per sample: host decoding, device decoding with a cold index (the walk is
    paid) and with a cached one; images/s at 1 / 2 / 12 / 16 loader threads; (b) the device decode stage of one batch
    (frames + backgrounds) for seg_mcus 8 / 16 / one MCU row: upload + three launches between a device event pair, and
    each launch alone; (c) loader-fed training against one prebuilt batch, host and device decoding alternated."""
    import copy
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from radet_amd import kernels as K
    from radet_amd.core import jpeg
    from radet_amd.datasets import build_dataloader, build_dataset
    from radet_amd.datasets.bop_convert import add_segmentation
    from radet_amd.datasets.loader import sample_generators
    tree = write_tree(root, n_frames=64, objects=(6, 6), seed=0)
    ann = os.path.join(root, "train_pbr_rle.json")
    with open(tree["ann_file"]) as f:
        coco = add_segmentation(json.load(f), tree["seg_prefix"], "rle")
    with open(ann, "w") as f:
        json.dump(coco, f)
    train, _ = pipelines(tree["background_dir"])
    train = copy.deepcopy(train)
    train[1] = dict(type="LoadAnnotations", with_bbox=True, with_mask=True)

    def build(decode, **kw):
        return build_dataset(dict(type="BOPDataset", ann_file=ann, img_prefix=tree["img_prefix"], mask_source="annotation",
                                  pipeline=train, image_decode=decode, **kw))

    def plan_all(d, epoch=0):
        per = []
        for i in range(len(d)):
            t0 = time.perf_counter()
            d.plan_sample(i, *sample_generators(0, epoch, i))
            per.append((time.perf_counter() - t0) * 1e3)
        return per
    res = dict(part="jpeg", batch=16, iters=args.iters, frames=64, default_seg_mcus=jpeg.DEFAULT_SEG_MCUS)
    # (a) host planning
    host_ds, dev_ds = build("host"), build("device")
    build("device").plan_sample(0, *sample_generators(0, 0, 0))           # (library load, Pillow import: not the walk's cost)
    host_ds.plan_sample(0, *sample_generators(0, 0, 0))
    plans = dict(host=_scatter(plan_all(host_ds)), device_cold_index=_scatter(plan_all(dev_ds)),
                 device_cached_index=_scatter(plan_all(dev_ds)))
    rates = {}
    for name, d in (("host", host_ds), ("device_cached_index", dev_ds)):
        rate = {}
        for threads in (1, 2, 12, 16):
            with ThreadPoolExecutor(threads) as pool:
                list(pool.map(lambda i: d.plan_sample(i, *sample_generators(0, 0, i)), range(threads)))
                runs = []
                for rep in range(3):
                    t0 = time.perf_counter()
                    list(pool.map(lambda i: d.plan_sample(i, *sample_generators(0, rep, i)), range(len(d))))
                    runs.append(len(d) / (time.perf_counter() - t0))
                rate[threads] = dict(median=float(np.median(runs)), runs=runs)
        rates[name] = rate
    res["host"] = dict(plan_ms_per_sample=plans, images_per_s_by_threads=rates,
                       cached_plan_over_host_plan=plans["device_cached_index"]["median"] / plans["host"]["median"],
                       images_per_s_at_2_threads_device_over_host=rates["device_cached_index"][2]["median"] / rates["host"][2]["median"])
    # (b) the decode stage of one batch, per segment length
    stage = {}
    for seg in (8, 16, "row"):
        d = build("device", seg_mcus=seg)
        planned = [d.plan_sample(i, *sample_generators(0, 0, i)) for i in range(16)]
        sources = [s["img"] for s in planned] + [s["background"] for s in planned if "background" in s]
        assert all(isinstance(a, jpeg.DeviceJpeg) for a in sources)
        pipe, dev = d.pipeline, d.pipeline._dev()
        offs = np.cumsum([0] + [a.shape[0] * a.shape[1] for a in sources])
        blob, sections, sizes = jpeg.pack_batch(sources, offs[:-1])
        dblob = torch.from_numpy(blob).to(dev)
        dst = torch.empty(int(offs[-1]) * 3, dtype=torch.uint8, device=dev)
        _, coef, planes = K.jpeg_decode(dblob, sections, sizes, len(sources), dst)
        whole, launches = [], {1: [], 2: [], 4: []}
        for it in range(args.iters + 3):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pipe._decode_packed(sources, dev)
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                whole.append(e0.elapsed_time(e1))
            for bit in (1, 2, 4):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                K.jpeg_decode(dblob, sections, sizes, len(sources), dst, stages=bit, work=(coef, planes))
                e1.record()
                torch.cuda.synchronize()
                if it >= 3:
                    launches[bit].append(e0.elapsed_time(e1))
        pipe.check_decode_errors(wait=True)
        stage[str(seg)] = dict(images=len(sources), segments=sizes["n_rows"], workgroups=sizes["n_wg"], upload_bytes=int(blob.size),
                               file_bytes=int(sections["files"][1]), upload_and_launches_event_ms=_scatter(whole),
                               entropy_event_ms=_scatter(launches[1]), idct_event_ms=_scatter(launches[2]),
                               convert_event_ms=_scatter(launches[4]))
    res["device_decode_stage"] = stage
    # (c) loader-fed training
    if args.steps > 0:
        from oracle import synth
        from radet_amd.models import build_detector
        from radet_amd.utils import Config
        cfg = Config.fromfile(os.path.join(ROOT, "configs", "bop", "r50_ycbv_pbr.py"))
        cfg.model["pretrained"] = None
        torch.manual_seed(0)
        det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
        synth.fill_state_dict(det.state_dict(), seed=0)
        det = det.cuda().train()
        rt = det.runtime()
        rt.init_optimizer(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, max_norm=35.0)
        rt.set_loss_from_head(det.bbox_head)

        def step(b):
            tg = rt.pack_targets(b["gt_bboxes"], b["gt_labels"], b["points_to_gt_index"], b["points_weight"])
            rt.train_step(b["img"], tg, lr=1e-4)
        loaders = {k: build_dataloader(d, samples_per_gpu=16, workers=args.workers, seed=0)
                   for k, d in (("host", host_ds), ("device", dev_ds))}

        def stream(loader):
            epoch = 0
            while True:
                loader.set_epoch(epoch)
                yield from loader
                epoch += 1
        its = {k: stream(v) for k, v in loaders.items()}
        fixed = next(its["host"])
        for _ in range(args.warmup):
            step(fixed)
            step(next(its["host"]))
            step(next(its["device"]))
        torch.cuda.synchronize()
        tr = dict(prebuilt=[], host=[], device=[])
        for rnd in range(args.rounds):
            for name in tr:
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(fixed if name == "prebuilt" else next(its[name]))
                torch.cuda.synchronize()
                tr[name].append(16 * args.steps / (time.perf_counter() - t0))
        for v in loaders.values():
            v.close()
        med = {k: float(np.median(v)) for k, v in tr.items()}
        res["train"] = dict(steps=args.steps, rounds=args.rounds, workers=args.workers, images_per_s=tr, median=med,
                            host_over_prebuilt=med["host"] / med["prebuilt"], device_over_prebuilt=med["device"] / med["prebuilt"],
                            decode_stats=dev_ds.pipeline.decode_stats)
    return res


def part_cache(args, root):
    """bs 16, 640 x 480, the frames of --part rle, for (png_host: PNG-mask annotations, host decoding) and (rle_device:
    run-list annotations, device decoding); the uncached pipeline of the same call is the baseline.  (a) host plan per
    sample: uncached, cached cold (every file a miss; the masks are converted) and warm; images/s at 1 / 2 / 12 / 16
    loader threads; (b) run() of one batch between a device event pair, uncached and warm, and the gather and insert
    launches alone with the bytes they move; (c) loader-fed training against one prebuilt batch, all variants alternated."""
    import copy
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from radet_amd import kernels as K
    from radet_amd.datasets import build_dataloader, build_dataset
    from radet_amd.datasets.bop_convert import add_segmentation
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.datasets.sample_cache import CachedImage
    tree = write_tree(root, n_frames=64, objects=(6, 6), seed=0)
    ann = os.path.join(root, "train_pbr_rle.json")
    with open(tree["ann_file"]) as f:
        coco = add_segmentation(json.load(f), tree["seg_prefix"], "rle")
    with open(ann, "w") as f:
        json.dump(coco, f)
    train, _ = pipelines(tree["background_dir"])
    rle_train = copy.deepcopy(train)
    rle_train[1] = dict(type="LoadAnnotations", with_bbox=True, with_mask=True)
    budget = 2 << 30

    def build(style, **kw):
        if style == "png_host":
            return build_dataset(dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"],
                                      seg_prefix=tree["seg_prefix"], pipeline=train, image_decode="host", **kw))
        return build_dataset(dict(type="BOPDataset", ann_file=ann, img_prefix=tree["img_prefix"], mask_source="annotation",
                                  pipeline=rle_train, image_decode="device", **kw))

    def plan_all(d, epoch):
        per = []
        for i in range(len(d)):
            t0 = time.perf_counter()
            d.plan_sample(i, *sample_generators(0, epoch, i))
            per.append((time.perf_counter() - t0) * 1e3)
        return per

    def rate_by_threads(d):
        rate = {}
        for threads in (1, 2, 12, 16):
            with ThreadPoolExecutor(threads) as pool:
                list(pool.map(lambda i: d.plan_sample(i, *sample_generators(0, 0, i)), range(threads)))
                runs = []
                for rep in range(3):
                    t0 = time.perf_counter()
                    list(pool.map(lambda i: d.plan_sample(i, *sample_generators(0, rep, i)), range(len(d))))
                    runs.append(len(d) / (time.perf_counter() - t0))
                rate[threads] = dict(median=float(np.median(runs)), runs=runs)
        return rate

    def timed(fn, iters):
        out = []
        for it in range(iters + 3):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                out.append(e0.elapsed_time(e1))
        return _scatter(out)
    res = dict(part="cache", batch=16, iters=args.iters, frames=64, cache_bytes=budget)
    sets = {}
    for style in ("png_host", "rle_device"):
        plain, cached = build(style), build(style, sample_cache="device", cache_bytes=budget)
        plain.plan_sample(0, *sample_generators(0, 0, 0))                   # (library load, Pillow import)
        r = dict(plan_ms_per_sample=dict(uncached=_scatter(plan_all(plain, 0)), cached_cold=_scatter(plan_all(cached, 0))))
        # the first epoch: every batch of 16 through run(), then every background a later epoch may draw
        for epoch in (0, 1, 2):
            for b in range(0, len(cached), 16):
                cached.pipeline.run([cached.plan_sample(i, *sample_generators(0, epoch, i)) for i in range(b, b + 16)])
        cached.pipeline.check_decode_errors(wait=True)
        r["plan_ms_per_sample"]["cached_warm"] = _scatter(plan_all(cached, 3))
        r["images_per_s_by_threads"] = dict(uncached=rate_by_threads(plain), cached_warm=rate_by_threads(cached))
        # (b) run() of one batch
        warm = [cached.plan_sample(i, *sample_generators(0, 3, i)) for i in range(16)]
        cold = [plain.plan_sample(i, *sample_generators(0, 3, i)) for i in range(16)]
        sources = [s["img"] for s in warm] + [s["background"] for s in warm if "background" in s]
        assert all(isinstance(a, CachedImage) for a in sources), "a file of the timed batch is not cached"
        dev = cached.pipeline._dev()
        nbytes = sum(a.nbytes for a in sources)
        buf = torch.empty(nbytes + 16 * len(sources), dtype=torch.uint8, device=dev)
        arena = torch.empty(nbytes + 256 * len(sources), dtype=torch.uint8, device=dev)
        g_rows, i_rows, o, ao = [], [], 0, 0
        for a in sources:                                                    # (packed at 3-byte granularity, like run())
            g_rows.append((a.addr, buf.data_ptr() + o, a.nbytes))
            i_rows.append((buf.data_ptr() + o, arena.data_ptr() + ao, a.nbytes))
            o += a.nbytes + 3
            ao += -(-a.nbytes // 256) * 256
        tabs = {}
        for name, rows in (("gather", g_rows), ("insert", i_rows)):
            t, tiles = K.copy_segments_table(rows)
            tabs[name] = (torch.from_numpy(t).to(dev), len(t), tiles)
        r["run_event_ms"] = dict(uncached=timed(lambda: plain.pipeline.run(_fresh(cold)), args.iters),
                                 cached_warm=timed(lambda: cached.pipeline.run(_fresh(warm)), args.iters))
        launches = {}
        for name, tab in tabs.items():
            ms = timed(lambda: K.copy_segments(*tab), args.iters)
            launches[name] = dict(event_ms=ms, bytes=int(nbytes), tiles=tab[2], rows=tab[1],
                                  gbytes_per_s_read_plus_write=2 * nbytes / (ms["median"] * 1e-3) / 1e9)
        r["launches"] = launches
        r["cache_stats"] = cached.pipeline.cache_stats
        sets[style] = (plain, cached)
        res[style] = r
    # (c) loader-fed training
    if args.steps > 0:
        from oracle import synth
        from radet_amd.models import build_detector
        from radet_amd.utils import Config
        cfg = Config.fromfile(os.path.join(ROOT, "configs", "bop", "r50_ycbv_pbr.py"))
        cfg.model["pretrained"] = None
        torch.manual_seed(0)
        det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
        synth.fill_state_dict(det.state_dict(), seed=0)
        det = det.cuda().train()
        rt = det.runtime()
        rt.init_optimizer(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, max_norm=35.0)
        rt.set_loss_from_head(det.bbox_head)

        def step(b):
            tg = rt.pack_targets(b["gt_bboxes"], b["gt_labels"], b["points_to_gt_index"], b["points_weight"])
            rt.train_step(b["img"], tg, lr=1e-4)
        loaders = {f"{style}_{kind}": build_dataloader(d, samples_per_gpu=16, workers=args.workers, seed=0)
                   for style, pair in sets.items() for kind, d in zip(("uncached", "cached"), pair)}

        def stream(loader):
            epoch = 0
            while True:
                loader.set_epoch(epoch)
                yield from loader
                epoch += 1
        its = {k: stream(v) for k, v in loaders.items()}
        fixed = next(its["png_host_uncached"])
        for _ in range(args.warmup):
            step(fixed)
            for it in its.values():
                step(next(it))
        torch.cuda.synchronize()
        tr = {k: [] for k in ["prebuilt", *its]}
        for rnd in range(args.rounds):
            for name in tr:
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(fixed if name == "prebuilt" else next(its[name]))
                torch.cuda.synchronize()
                tr[name].append(16 * args.steps / (time.perf_counter() - t0))
        for v in loaders.values():
            v.close()
        med = {k: float(np.median(v)) for k, v in tr.items()}
        res["train"] = dict(steps=args.steps, rounds=args.rounds, workers=args.workers, images_per_s=tr, median=med,
                            over_prebuilt={k: med[k] / med["prebuilt"] for k in its},
                            cache_stats={style: pair[1].pipeline.cache_stats for style, pair in sets.items()})
    return res


def part_jitter(args, root):
    """bs 16, 640 x 480 frames, 6 objects per image.  The device part (ImagePipeline.run) of one planned batch per variant:
    `fixed` = the r50_ycbv_pbr train pipeline (output 480 x 640), `jitter` = the same with Resize(ratio_range=(0.6, 1.6)) +
    RandomCrop((480, 640)) + Pad(size=(480, 640)) (configs/base/datasets/bop_detection_jitter.py: samples drawn below 1 are
    smaller than the crop), `jitter_up` = ratio_range (1.0, 1.6): every sample is a 480 x 640 window of a larger virtual
    image, the same output pixels as `fixed`.  The variants alternate within each round; per call a device event pair and a
    host clock around the call and a synchronise.  Also the entry points each variant calls."""
    import torch
    from radet_amd import _lib
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    tree = write_tree(root, n_frames=16, objects=(6, 6), seed=0)
    train, _ = pipelines(tree["background_dir"])

    def jitter(ratio_range):
        p = list(train)
        p[2] = dict(type="Resize", img_scale=(640, 480), ratio_range=ratio_range, keep_ratio=True)
        p.insert(3, dict(type="RandomCrop", crop_size=(480, 640)))
        return [dict(type="Pad", size=(480, 640)) if t["type"] == "Pad" else t for t in p]
    sub = dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"], seg_prefix=tree["seg_prefix"])
    ds = dict(fixed=build_dataset(dict(sub, pipeline=train)), jitter=build_dataset(dict(sub, pipeline=jitter((0.6, 1.6)))),
              jitter_up=build_dataset(dict(sub, pipeline=jitter((1.0, 1.6)))))
    planned = {k: [d.plan_sample(i, *sample_generators(0, 0, i)) for i in range(16)] for k, d in ds.items()}
    res = dict(part="jitter", batch=16, iters=args.iters, rounds=args.rounds, device=torch.cuda.get_device_name(0),
               clocks="default governor, not pinned; medians over alternating rounds")
    res["samples"] = {k: dict(windowed=sum(tuple(s.get("crop_window", (0, 0, *s["resize_hw"]))[2:]) != tuple(s["resize_hw"]) for s in v),
                              resized_px=int(sum(s["resize_hw"][0] * s["resize_hw"][1] for s in v)),
                              output_px=int(sum(s["img_shape"][0] * s["img_shape"][1] for s in v)),
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
    res["run_ms"] = {k: dict(wall=_scatter(wall[k]), event=_scatter(evt[k])) for k in ds}
    res["median_event_ms"] = {k: float(np.median(evt[k])) for k in ds}
    return res


def _fresh(planned):
    """the planned samples with copies of their RandomStates (the assigner advances them)"""
    import copy
    return [dict(s, _nprnd=copy.deepcopy(s["_nprnd"])) for s in planned]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "decode", "train", "maskfree", "rle", "jpeg", "cache", "jitter"), required=True)
    ap.add_argument("--pipeline", choices=("pbr", "mix"), default="pbr")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--out")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as root:
        res = dict(kernels=part_kernels, decode=part_decode, train=part_train, maskfree=part_maskfree, rle=part_rle, jpeg=part_jpeg, cache=part_cache,
                   jitter=part_jitter)[args.part](args, root)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
