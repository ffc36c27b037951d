"""Times one evaluation of a test run in one process and writes profiles/bench_eval.json:

  * the host evaluator (radet_amd/datasets/cocoeval.py:COCOeval, evaluate() + accumulate()),
  * the device evaluator (DeviceCOCOeval, from device-resident detections to the three tables on the host),
  * the inference pass over the same number of synthetic 640 x 480 images with detect_stream,

on a seeded case at the detector's operating point: 1000 images, 21 categories, 6 ground truths and 100 detections per image;
detections are jittered copies of the ground truths plus random boxes, 10 % crowds, fp32 scores drawn from a coarse grid so
that ties occur.  Medians of --reps repetitions after a warm-up; HIP events for the device parts.

    python tools/bench_eval.py [--images 1000] [--reps 5] [--batch 8] [--no-host]
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


def make_case(n_img, n_cat=21, n_gt=6, n_dt=100, seed=0):
    """(annotation dict, per-image (dets f32[n_dt,5], labels i64[n_dt]) host arrays)"""
    rng = np.random.RandomState(seed)
    anns, raw = [], []
    for i in range(n_img):
        wh = rng.choice([14.0, 50.0, 160.0], size=(n_gt, 2)) * rng.uniform(0.8, 1.2, size=(n_gt, 2))
        xy = rng.uniform(0, [640 - 200, 480 - 200], size=(n_gt, 2))
        cat = rng.randint(1, n_cat + 1, size=n_gt)
        crowd = rng.rand(n_gt) < 0.1
        for j in range(n_gt):
            anns.append(dict(id=len(anns) + 1, image_id=i + 1, category_id=int(cat[j]), iscrowd=int(crowd[j]),
                             bbox=[float(xy[j, 0]), float(xy[j, 1]), float(wh[j, 0]), float(wh[j, 1])],
                             area=float(wh[j, 0] * wh[j, 1])))
        src = rng.randint(0, n_gt, size=n_dt)
        copy = rng.rand(n_dt) < 0.5
        bx = np.where(copy[:, None], xy[src] + rng.uniform(-6, 6, size=(n_dt, 2)), rng.uniform(0, [440, 280], size=(n_dt, 2)))
        bw = np.where(copy[:, None], wh[src] * rng.uniform(0.85, 1.15, size=(n_dt, 2)), rng.uniform(8, 180, size=(n_dt, 2)))
        label = np.where(copy & (rng.rand(n_dt) < 0.9), cat[src] - 1, rng.randint(0, n_cat, size=n_dt)).astype(np.int64)
        score = (np.round(rng.rand(n_dt) * 400) / 400).astype(np.float32)          # a grid of 401 values: fp32 ties
        raw.append((np.concatenate([bx, bx + bw, score[:, None]], axis=1).astype(np.float32), label))
    gt = dict(images=[dict(id=i + 1, width=640, height=480, file_name=f"000000/rgb/{i:06d}.jpg") for i in range(n_img)],
              categories=[dict(id=c + 1, name=f"c{c + 1}") for c in range(n_cat)], annotations=anns)
    return gt, raw


def host_records(raw, n_cat):
    """the records BOPDataset._det2json writes (image, then label, then row)"""
    out = []
    for i, (dets, labels) in enumerate(raw):
        for k in range(n_cat):
            for det in dets[labels == k]:
                x1, y1, x2, y2 = (float(v) for v in det[:4])
                out.append(dict(image_id=i + 1, category_id=k + 1, bbox=[x1, y1, x2 - x1, y2 - y1], score=float(det[4])))
    return out


def timed_ms(fn):
    """(wall ms by HIP events on the current stream, the call's result); the call ends host-synchronised"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-host", action="store_true", help="skip the host evaluator (about 10 s per repetition)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_eval.json"))
    args = ap.parse_args()
    from radet_amd.datasets.cocoeval import COCO, COCOeval
    from radet_amd.datasets.cocoeval_device import DeviceCOCOeval
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill
    dev = torch.device("cuda")
    n_cat = 21
    gt_dict, raw = make_case(args.images, n_cat)
    gt = COCO(gt_dict)
    img_ids, cat_ids = [i + 1 for i in range(args.images)], [c + 1 for c in range(n_cat)]
    raw_dev = [(torch.from_numpy(d).to(dev), torch.from_numpy(l).to(dev)) for d, l in raw]

    # ---- device evaluator: device-resident detections -> precision / recall / scores on the host
    def device_eval():
        ev = DeviceCOCOeval(gt, raw_dev, cat_ids, img_ids, dev, logger="silent")
        ev.params.catIds, ev.params.imgIds = cat_ids, img_ids
        t_match, _ = timed_ms(ev.evaluate)
        t_acc, _ = timed_ms(ev.accumulate)
        return ev, t_match, t_acc
    device_eval()                                                    # warm-up (ground-truth upload, allocator, code objects)
    dev_ms, match_ms, acc_ms = [], [], []
    for _ in range(args.reps):
        t, (ev, tm, ta) = timed_ms(device_eval)
        dev_ms.append(t)
        match_ms.append(tm)
        acc_ms.append(ta)
    assert ev.host is None
    ev.summarize()

    # ---- host evaluator on the same inputs
    host_ms, same = [], None
    if not args.no_host:
        det = gt.loadRes(host_records(raw, n_cat))
        for r in range(args.reps + 1):
            hv = COCOeval(gt, det, "bbox")
            hv.params.catIds, hv.params.imgIds = cat_ids, img_ids
            t0 = time.perf_counter()
            hv.evaluate()
            hv.accumulate()
            if r:                                                    # (the first repetition is the warm-up)
                host_ms.append((time.perf_counter() - t0) * 1e3)
        same = all(np.array_equal(hv.eval[k].view(np.uint64), ev.eval[k].view(np.uint64)) for k in ("precision", "recall", "scores"))

    # ---- inference pass over as many synthetic 640 x 480 images
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(dev)
    synth_fill(model, seed=0)
    model.eval()
    rt = model.runtime()
    B = args.batch
    img = torch.randn(B, 3, 480, 640, generator=torch.Generator().manual_seed(0)).to(dev)
    metas = [dict(img_shape=(480, 640, 3), pad_shape=(480, 640, 3), scale_factor=np.ones(4, np.float32), flip=False) for _ in range(B)]
    n_batches = -(-args.images // B)

    def inference():
        return sum(len(d) for d in rt.detect_stream(((img, metas) for _ in range(n_batches)), model.test_cfg, rescale=True))
    inference()
    inf_ms = [timed_ms(inference)[0] for _ in range(args.reps)]

    med = statistics.median
    out = dict(case=dict(images=args.images, categories=n_cat, gts_per_image=6, dets_per_image=100, crowds=0.1, seed=0),
               reps=args.reps, device_eval_ms=med(dev_ms), device_evaluate_ms=med(match_ms), device_accumulate_ms=med(acc_ms),
               device_eval_ms_all=dev_ms, inference_ms=med(inf_ms), inference_ms_all=inf_ms, inference_batch=B,
               inference_images=n_batches * B, device_eval_over_inference=med(dev_ms) / med(inf_ms),
               device_eval_no_longer_than_inference=bool(med(dev_ms) <= med(inf_ms)))
    if host_ms:
        out.update(host_eval_ms=med(host_ms), host_eval_ms_all=host_ms, host_over_device=med(host_ms) / med(dev_ms),
                   tables_bit_identical=bool(same))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
