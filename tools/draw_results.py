"""Paints the detections of a result file on their images: the file workflow of the reference's tools/show_bop_detbbox.py
(and of `tools/test.py --show-dir`, which this project's test loop does not have).

    python tools/draw_results.py <image_dir> <result_json> <save_dir> [--show-score-thr 0.3] [--dataset ycbv | --classes a,b,c]
                                 [--ext jpg] [--ann instances.json] [--batch 8]

result_json is what `dataset.format_results` writes: COCO result records {image_id, category_id, bbox (xywh), score}.  With a
`scene_id` in the records (bop_submission=True) an image is <image_dir>/<scene:06d>/rgb/<image:06d>.<ext> and the label is
category_id - 1, as in the reference's tool; without it --ann names the COCO annotation file that maps image_id to
file_name and category_id to the label.  Images go through radet_amd.ops.draw_detections in batches (one upload and one
overlay launch per batch, detections by descending score so the best one's label is on top) and are written under <save_dir>
with the same relative path.  At most 256 detections per image are drawn (the rest by score are left out and counted)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the class names of the reference's tool
CLASS_NAMES = dict(
    icbin=("coffee_cup", "juice_carton"),
    tudl=("dragon", "frog", "can"),
    lmo=("ape", "benchvise", "bowl", "cam", "can", "cat", "cup", "driller", "duck", "eggbox", "glue", "holepuncher", "iron", "lamp",
         "phone"),
    hb=tuple(str(i + 1) for i in range(33)),
    itodd=tuple(str(i + 1) for i in range(28)),
    tless=tuple(str(i + 1) for i in range(30)),
)


def group_records(records, image_dir, ext, ann=None):
    """-> {relative image path: (bboxes f32 [n,5] xyxy + score by descending score, labels i64 [n])}"""
    names, cat2label = {}, None
    if ann is not None:
        with open(ann) as f:
            coco = json.load(f)
        names = {im["id"]: im["file_name"] for im in coco["images"]}
        cat2label = {c["id"]: i for i, c in enumerate(sorted(coco["categories"], key=lambda c: c["id"]))}
    per = {}
    for r in records:
        if "scene_id" in r:
            rel = os.path.join(f"{int(r['scene_id']):06d}", "rgb", f"{int(r['image_id']):06d}.{ext}")
        elif r["image_id"] in names:
            rel = names[r["image_id"]]
        else:
            raise SystemExit(f"image_id {r['image_id']!r}: records without scene_id need --ann (image_id -> file_name)")
        x, y, w, h = r["bbox"]
        label = cat2label[r["category_id"]] if cat2label is not None else int(r["category_id"]) - 1
        per.setdefault(rel, []).append((x, y, x + w, y + h, r["score"], label))
    out = {}
    for rel, rows in per.items():
        a = np.array(sorted(rows, key=lambda v: -v[4]), np.float64).reshape(-1, 6)
        out[rel] = (a[:, :5].astype(np.float32), a[:, 5].astype(np.int64))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("image_dir")
    ap.add_argument("result_json")
    ap.add_argument("save_dir")
    ap.add_argument("--show-score-thr", type=float, default=0.3)
    ap.add_argument("--dataset", choices=sorted(CLASS_NAMES) + ["ycbv"])
    ap.add_argument("--classes", help="comma-separated class names (instead of --dataset)")
    ap.add_argument("--ext", default="jpg")
    ap.add_argument("--ann")
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    from radet_amd.core.visualization import imread_bgr, imwrite_bgr
    from radet_amd.datasets.bop import YCBV_CLASSES
    from radet_amd.ops import draw_detections
    names = None
    if args.classes:
        names = args.classes.split(",")
    elif args.dataset:
        names = list(YCBV_CLASSES if args.dataset == "ycbv" else CLASS_NAMES[args.dataset])
    with open(args.result_json) as f:
        per = group_records(json.load(f), args.image_dir, args.ext, args.ann)
    rels = sorted(per)
    left_out = 0
    for i in range(0, len(rels), max(args.batch, 1)):
        group = rels[i:i + max(args.batch, 1)]
        frames = [np.ascontiguousarray(imread_bgr(os.path.join(args.image_dir, rel))) for rel in group]
        dets = []
        for rel in group:
            b, l = per[rel]
            left_out += max(int((b[:, 4] > args.show_score_thr).sum()) - 256, 0)
            dets.append((b, l))
        shown = draw_detections(frames, dets, class_names=names, score_thr=args.show_score_thr, bbox_color=(72, 101, 241),
                                text_color=(72, 101, 241))
        for rel, img in zip(group, shown):
            imwrite_bgr(img.cpu().numpy(), os.path.join(args.save_dir, rel))
    print(f"{len(rels)} images written under {args.save_dir}" + (f"; {left_out} detections beyond 256 per image left out" if left_out else ""))


if __name__ == "__main__":
    main()
