"""Generates tests/golden/color_aug.npz: the reference's ColorTransform, EqualizeTransform, BrightnessTransform and
ContrastTransform run on the small synthetic sample of gen_scale_jitter.py under seeded np.random -- bare, and inside one
AutoAugment whose policies order colour, warp and CutOut entries every way round -- for tests/test_color_cpu.py to compare
the planning of radet_amd against.

    python tests/golden/gen_color_aug.py

The reference is imported at generation time only (ref_import), with the mmcv / cv2 stubs of gen_scale_jitter.py and the
warp stubs of gen_affine_aug.py.  mmcv.adjust_color / adjust_brightness / adjust_contrast / imequalize are supplied here:
they record (name, factor) and return the image, so what is pinned is the reference's planning -- gates, factors, the order
of the entries, the policy drawn, the boxes, the number of draws -- not mmcv's pixels.  The file holds recorded results only.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_affine_aug as G  # noqa: E402  (installs the reference, the mmcv stub and the warp stubs)

import mmcv  # noqa: E402  (the stub)

J = G.J
H, W = J.H, J.W
LOG = []                                  # per colour call ("k", name, factor, warps so far); per CutOut ("c", draws, warps so far)
NAMES = ["adjust_color", "imequalize", "adjust_brightness", "adjust_contrast"]


def _stub(name):
    def fn(img, factor=None, *args, **kwargs):
        assert not args and not kwargs and img.dtype == np.uint8
        LOG.append(("k", name, 1.0 if factor is None else factor, len(G.CALLS)))
        return img
    return fn


for _n in NAMES:
    setattr(mmcv, _n, _stub(_n))

from radet.datasets.pipelines.auto_augment import (AutoAugment, BrightnessTransform, ColorTransform, ContrastTransform,  # noqa: E402
                                                   EqualizeTransform)
from radet.datasets.pipelines.transforms import CutOut  # noqa: E402


class Recorded:
    """a CutOut of a policy that says when it ran and what np.random.randint returned to it"""

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
        LOG.append(("c", draws, None, len(G.CALLS)))
        return out


STAGES = dict(ColorTransform=ColorTransform, EqualizeTransform=EqualizeTransform, BrightnessTransform=BrightnessTransform,
              ContrastTransform=ContrastTransform)
# bare stages: prob 0, 1 and in between, levels 0, 10 and in between (an int and a float)
CASES = [(name, dict(prob=p, **({} if name == "EqualizeTransform" else dict(level=lv))))
         for name in STAGES for p in (0, 0.5, 1) for lv in ((0,) if name == "EqualizeTransform" else (0, 3, 7.5, 10))]
SEEDS = range(4)
ROT = dict(type="Rotate", level=8, prob=0.9, img_fill_val=(0., 37., 255.))
CUT = dict(type="CutOut", n_holes=(0, 3), cutout_ratio=[(0.1, 0.1), (0.2, 0.15)], fill_in=(9, 8, 7))
COL = dict(type="ColorTransform", level=6, prob=0.9)
EQ = dict(type="EqualizeTransform", prob=0.9)
BRI = dict(type="BrightnessTransform", level=3, prob=0.9)
CON = dict(type="ContrastTransform", level=7.5, prob=0.9)
# AutoAugment: warp (w), CutOut (c) and colour (k) entries in all six orders, and a policy that often fires nothing
POLICIES = [[ROT, CUT, COL], [ROT, EQ, CUT], [CUT, ROT, BRI], [CUT, CON, ROT], [COL, ROT, CUT], [EQ, CUT, ROT],
            [dict(ROT, prob=0.2), dict(BRI, prob=0.2), dict(CON, prob=0.5)]]
AUTO_SEEDS = range(120)
ORDERS = ("wck", "wkc", "cwk", "ckw", "kwc", "kcw")


def _sample(img, masks):
    return dict(img=img.copy(), img_shape=img.shape, img_fields=["img"], bbox_fields=["gt_bboxes_ignore", "gt_bboxes"],
                mask_fields=["gt_masks"], gt_bboxes=G.BOXES.copy(), gt_bboxes_ignore=G.IGNORE.copy(), gt_labels=G.LABELS.copy(),
                gt_masks=G.Masks(masks))


def main():
    img, masks = J.sample()
    out = dict(boxes=G.BOXES, ignore=G.IGNORE, labels=G.LABELS, src_hw=np.array([H, W]),
               cases=np.asarray(json.dumps([[a, b] for a, b in CASES])), policies=np.asarray(json.dumps(POLICIES)),
               names=np.asarray(json.dumps(NAMES)))
    seen = dict(fired=0, skipped=0, nothing=0, colour_only=0, two_colours=0, **dict.fromkeys(ORDERS, 0))
    rows = {}
    for c, (name, args) in enumerate(CASES):
        for seed in SEEDS:
            np.random.seed(seed)
            del LOG[:], G.CALLS[:]
            r = STAGES[name](**args)(_sample(img, masks))
            nxt = np.random.random_sample()
            assert np.array_equal(r["img"], img) and np.array_equal(r["gt_bboxes"], G.BOXES) and not G.CALLS and len(LOG) <= 1
            assert np.array_equal(r["gt_bboxes_ignore"], G.IGNORE) and np.array_equal(r["gt_labels"], G.LABELS)
            seen["fired" if LOG else "skipped"] += 1
            if LOG:
                assert LOG[0][1] == NAMES[list(STAGES).index(name)]
            for key, v in dict(case=c, seed=seed, next=nxt, fired=len(LOG), factor=LOG[0][2] if LOG else np.nan).items():
                rows.setdefault(key, []).append(v)
    auto, acat = {}, {}
    for seed in AUTO_SEEDS:
        np.random.seed(seed)
        stage = AutoAugment(policies=[[dict(t) for t in p] for p in POLICIES])
        for policy in stage.transforms:                       # (mmdet's Compose of the policy's stages)
            policy.transforms = [Recorded(t) if isinstance(t, CutOut) else t for t in policy.transforms]
        stage.transforms = [G.Tagged(k, t) for k, t in enumerate(stage.transforms)]
        del LOG[:], G.CALLS[:], G.Tagged.chosen[:]
        r = stage(_sample(img, masks))
        nxt = np.random.random_sample()
        # the entries in the order they ran: "w" a warp of the image, "c" a CutOut that drew at least one hole, "k" a colour stage
        order, w = "", 0
        for kind, a, _, before in LOG:
            order += "w" * (before - w) + ("k" if kind == "k" else "c" if a[0] else "")
            w = before
        order += "w" * (len(G.CALLS) - w)
        seen["nothing"] += order == ""
        seen["colour_only"] += order == "k"
        seen["two_colours"] += order.count("k") == 2
        if order in ORDERS:
            seen[order] += 1
        colour = [e for e in LOG if e[0] == "k"]
        cuts = [e for e in LOG if e[0] == "c"]
        for key, v in dict(seed=seed, policy=G.Tagged.chosen[0], next=nxt, order=order, n_colours=len(colour), n_cutouts=len(cuts),
                           n_warps=len(G.CALLS), n_boxes=len(r["gt_bboxes"])).items():
            auto.setdefault("auto_" + key, []).append(v)
        acat.setdefault("auto_colour_names", []).append(np.array([NAMES.index(e[1]) for e in colour], np.int64))
        acat.setdefault("auto_colour_factors", []).append(np.array([e[2] for e in colour], np.float64))
        acat.setdefault("auto_n_draws", []).append(np.array([len(e[1]) for e in cuts], np.int64))
        acat.setdefault("auto_draws", []).append(np.array([d for e in cuts for d in e[1]], np.int64))
        acat.setdefault("auto_matrices", []).append(np.array([m for _, _, m in G.CALLS], np.float64).reshape(-1, 2, 3))
        acat.setdefault("auto_gt_bboxes", []).append(r["gt_bboxes"])
    out.update({k: np.array(v) for k, v in rows.items()})
    out.update({k: np.array(v) for k, v in auto.items()})
    out.update({k: np.concatenate(v) for k, v in acat.items()})
    print(seen)
    assert all(seen.values()), seen
    assert set(out["auto_policy"]) == set(range(len(POLICIES)))
    path = os.path.join(HERE, "color_aug.npz")
    np.savez_compressed(path, **out)
    print(f"color_aug.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
