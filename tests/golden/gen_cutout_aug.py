"""Generates tests/golden/cutout_aug.npz: the reference's CutOut run on the small synthetic sample of gen_scale_jitter.py
under seeded np.random -- bare, and inside AutoAugment policies next to Rotate / Translate -- for tests/test_cutout_cpu.py
to compare the planning of radet_amd and the NumPy restatement of tests/_cutout_ref.py against.

    python tests/golden/gen_cutout_aug.py

The reference is imported at generation time only (ref_import), with the mmcv / cv2 stubs of gen_scale_jitter.py and the
warp stubs of gen_affine_aug.py.  CutOut is pure NumPy, so the bare cases record the reference's own OUTPUT IMAGES; the
stage keeps neither its draws nor its holes, so np.random.randint is wrapped while a CutOut runs and what it returned is
recorded (the hole count, then x1, y1 and the candidate's index per hole).  The holes those draws give
(_cutout_ref.holes_from_draws) are checked here against the recorded image before anything is written.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_affine_aug as G  # noqa: E402  (installs the reference, the mmcv stub and the warp stubs)
import _cutout_ref as C  # noqa: E402

from radet.datasets.pipelines.auto_augment import AutoAugment  # noqa: E402
from radet.datasets.pipelines.transforms import CutOut  # noqa: E402

J = G.J
H, W = J.H, J.W
EVENTS = []                                                   # per CutOut call: (warps of the image before it, its randint draws)


class Recorded:
    """a CutOut of a policy (or a bare one) that says when it ran and what np.random.randint returned to it"""

    def __init__(self, stage):
        self.stage = stage

    def __call__(self, results):
        draws, randint = [], np.random.randint

        def logged(*a, **k):
            v = randint(*a, **k)
            draws.append(int(v))
            return v

        np.random.randint = logged
        try:
            out = self.stage(results)
        finally:
            np.random.randint = randint
        EVENTS.append((len(G.CALLS), draws))
        return out


# bare stages on the 60 x 80 sample: shape and ratio candidates, lists of them, n_holes as an int and as a range from 0, holes
# that overhang the right and the bottom border (and both), a ratio that gives holes without area
CASES = [
    dict(n_holes=2, cutout_shape=(10, 8)),
    dict(n_holes=(0, 3), cutout_shape=[(10, 8), (30, 40)], fill_in=(7, 200, 33)),
    dict(n_holes=1, cutout_ratio=(0.2, 0.25)),
    dict(n_holes=(1, 4), cutout_ratio=[(0.1, 0.1), (0.2, 0.15)], fill_in=(0, 37, 255)),
    dict(n_holes=3, cutout_ratio=(0.01, 0.5), fill_in=(255, 255, 255)),
    dict(n_holes=1, cutout_shape=(200, 200), fill_in=(128, 128, 128)),
]
SEEDS = range(4)
CUT = dict(type="CutOut", n_holes=(0, 2), cutout_ratio=[(0.1, 0.1), (0.2, 0.15)], fill_in=(9, 8, 7))
ROT = dict(type="Rotate", level=8, prob=0.7, img_fill_val=(0., 37., 255.))
# AutoAugment: a hole before a warp, a hole after a warp, holes alone, a warp alone
POLICIES = [[ROT, CUT], [CUT, ROT], [dict(CUT, n_holes=2, cutout_shape=(12, 9), cutout_ratio=None)],
            [dict(type="Translate", level=2, prob=0.8, max_translate_offset=100.)]]
AUTO_SEEDS = range(24)


def _args(case):
    """JSON turns tuples into lists: the candidates are written as {"tuple": ...} or {"list": [...]}"""
    out = dict(case)
    for key in ("cutout_shape", "cutout_ratio"):
        if out.get(key) is not None:
            out[key] = {"list": [list(c) for c in out[key]]} if isinstance(out[key], list) else {"tuple": list(out[key])}
    return out


def main():
    img, masks = J.sample()
    out = dict(boxes=G.BOXES, ignore=G.IGNORE, labels=G.LABELS, src_hw=np.array([H, W]),
               cases=np.asarray(json.dumps([_args(c) for c in CASES])),
               policies=np.asarray(json.dumps([[_args(t) for t in p] for p in POLICIES])))
    seen = dict(no_hole=0, overhang_right=0, overhang_bottom=0, overhang_both=0, zero_area=0, several=0, second_candidate=0,
                hole_then_warp=0, warp_then_hole=0, holes_only=0, warp_only=0, nothing=0)
    rows, cat, images = {}, {}, []
    for c, args in enumerate(CASES):
        for seed in SEEDS:
            np.random.seed(seed)
            del EVENTS[:], G.CALLS[:]
            r = Recorded(CutOut(**args))(dict(img=img.copy(), img_shape=img.shape, img_fields=["img"]))
            nxt = np.random.random_sample()
            (_, draws), = EVENTS
            with_ratio = "cutout_ratio" in args
            cand = args["cutout_ratio"] if with_ratio else args["cutout_shape"]
            cand = cand if isinstance(cand, list) else [cand]
            rects = C.holes_from_draws(draws, cand, with_ratio, H, W)
            assert np.array_equal(C.apply_holes(img, rects, np.array(args.get("fill_in", (0, 0, 0)), np.uint8)), r["img"])
            assert r["img"].dtype == np.uint8 and r["img"].shape == img.shape
            seen["no_hole"] += len(rects) == 0
            seen["several"] += len(rects) > 1
            seen["second_candidate"] += any(d > 0 for d in draws[3::3])
            for (x1, y1, x2, y2), k in zip(rects, range(len(rects))):
                cw, ch = cand[draws[3 + 3 * k]]
                cw, ch = (int(cw * W), int(ch * H)) if with_ratio else (cw, ch)
                right, bottom = x1 + cw > W, y1 + ch > H
                seen["overhang_right"] += right and not bottom
                seen["overhang_bottom"] += bottom and not right
                seen["overhang_both"] += right and bottom
                seen["zero_area"] += x2 == x1 or y2 == y1
            images.append(r["img"])
            for key, v in dict(case=c, seed=seed, next=nxt, n_draws=len(draws)).items():
                rows.setdefault(key, []).append(v)
            cat.setdefault("draws", []).append(np.array(draws, np.int64))
    auto, acat = {}, {}
    for seed in AUTO_SEEDS:
        np.random.seed(seed)
        r = dict(img=img.copy(), img_shape=img.shape, img_fields=["img"], bbox_fields=["gt_bboxes_ignore", "gt_bboxes"],
                 mask_fields=["gt_masks"], gt_bboxes=G.BOXES.copy(), gt_bboxes_ignore=G.IGNORE.copy(), gt_labels=G.LABELS.copy(),
                 gt_masks=G.Masks(masks))
        stage = AutoAugment(policies=[[dict(t) for t in p] for p in POLICIES])
        for policy in stage.transforms:                       # (mmdet's Compose of the policy's stages)
            policy.transforms = [Recorded(t) if isinstance(t, CutOut) else t for t in policy.transforms]
        stage.transforms = [G.Tagged(k, t) for k, t in enumerate(stage.transforms)]
        del EVENTS[:], G.CALLS[:], G.Tagged.chosen[:]
        r = stage(r)
        nxt = np.random.random_sample()
        # the entries in the order they ran: "w" a warp of the image, "c" a CutOut that drew at least one hole
        order, w = "", 0
        for before, draws in EVENTS:
            order += "w" * (before - w) + ("c" if draws[0] else "")
            w = before
        order += "w" * (len(G.CALLS) - w)
        seen["hole_then_warp"] += "cw" in order
        seen["warp_then_hole"] += "wc" in order
        seen["holes_only"] += order == "c"
        seen["warp_only"] += order == "w"
        seen["nothing"] += order == ""
        for key, v in dict(seed=seed, policy=G.Tagged.chosen[0], next=nxt, order=order, n_cutouts=len(EVENTS),
                           n_warps=len(G.CALLS), n_boxes=len(r["gt_bboxes"])).items():
            auto.setdefault("auto_" + key, []).append(v)
        for before, draws in EVENTS:
            acat.setdefault("auto_n_draws", []).append(np.array([len(draws)], np.int64))
            acat.setdefault("auto_draws", []).append(np.array(draws, np.int64))
        acat.setdefault("auto_matrices", []).append(np.array([m for _, _, m in G.CALLS], np.float64).reshape(-1, 2, 3))
        acat.setdefault("auto_gt_bboxes", []).append(r["gt_bboxes"])
    out.update({k: np.array(v) for k, v in rows.items()})
    out.update({k: np.concatenate(v) for k, v in cat.items()})
    out.update({k: np.array(v) for k, v in auto.items()})
    out.update({k: np.concatenate(v) for k, v in acat.items()})
    out["images"] = np.stack(images)
    print(seen)
    assert all(seen.values()), seen
    path = os.path.join(HERE, "cutout_aug.npz")
    np.savez_compressed(path, **out)
    print(f"cutout_aug.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
