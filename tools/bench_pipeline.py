"""Measures the BOP image pipeline (radet_amd.datasets.loading / loader) on a synthetic 640x480 BOP tree written from a seed.

    python tools/bench_pipeline.py --part kernels [--iters 20]     # the device part of bs-16 batches, every stage on
                                                                   # (run it under `rocprofv3 --kernel-trace --stats`)
    python tools/bench_pipeline.py --part decode                   # host planning (decode + draws) per thread count
    python tools/bench_pipeline.py --part train [--steps 60]       # r50_ycbv_pbr fp32 bs 16: loader-fed vs one prebuilt batch
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "decode", "train"), required=True)
    ap.add_argument("--pipeline", choices=("pbr", "mix"), default="pbr")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--out")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as root:
        res = dict(kernels=part_kernels, decode=part_decode, train=part_train)[args.part](args, root)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
