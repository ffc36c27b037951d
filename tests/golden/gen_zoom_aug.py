"""Generates tests/golden/zoom_aug.npz: the reference's Expand, MinIoURandomCrop and Resize run on small synthetic samples
under seeded np.random, for tests/test_zoomaug_cpu.py to compare the planning of radet_amd against.

    python tests/golden/gen_zoom_aug.py

The reference is imported at generation time only (ref_import), with the mmcv stub of gen_scale_jitter.py (whose sample
this uses).  Neither stage keeps its draws: Expand's are replayed from a saved generator state and checked against the
canvas it made; the crop's mode is its `mode` attribute, its patch the last one it handed to bbox_overlaps (which it
calls for every patch that is not degenerate, the accepted one last), and the modes it drew are counted by a proxy in
the place of the `random` name of the reference's module.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_scale_jitter as J  # noqa: E402  (installs the reference and the mmcv stub)
from oracle import masks as om  # noqa: E402

import radet.datasets.pipelines.transforms as T  # noqa: E402
from radet.datasets.pipelines.transforms import Expand, MinIoURandomCrop, Resize  # noqa: E402

H, W, BOXES, IGNORE, LABELS = J.H, J.W, J.BOXES, J.IGNORE, J.LABELS
MEAN = (123.675, 116.28, 103.53)


class Masks(J.Masks):
    """+ BitmapMasks.expand (core/mask/structures.py): zeros around the masks"""

    def expand(self, expanded_h, expanded_w, top, left):
        out = np.zeros((len(self.masks), expanded_h, expanded_w), np.uint8)
        out[:, top:top + self.masks.shape[1], left:left + self.masks.shape[2]] = self.masks
        return Masks(out, self.index)

    def rescale(self, scale):
        h, w = self.masks.shape[1:]
        nw, nh = om.rescale_size((w, h), scale)
        return Masks(om.resize_nearest(self.masks, (nh, nw)), self.index)

    def resize(self, out_shape):
        return Masks(om.resize_nearest(self.masks, tuple(out_shape)), self.index)

    def __getitem__(self, idx):
        return Masks(self.masks[idx].reshape(-1, *self.masks.shape[1:]), self.index[idx])

    def crop(self, bbox):
        return Masks(J.Masks.crop(self, bbox).masks, self.index)


class CountingRandom:
    """np.random where the reference's transforms look `random` up: the same stream, the choice calls counted"""

    def __init__(self):
        self.choices = 0

    def choice(self, *a, **k):
        self.choices += 1
        return np.random.choice(*a, **k)

    def __getattr__(self, name):
        return getattr(np.random, name)


PATCHES = []
_overlaps = T.bbox_overlaps


def recording_overlaps(patch, boxes, *a, **k):
    PATCHES.append(patch.reshape(-1).copy())
    return _overlaps(patch, boxes, *a, **k)


T.bbox_overlaps = recording_overlaps

# (expand arguments or None, crop arguments or None, with boxes)
CASES = [
    (dict(mean=MEAN, to_rgb=True, ratio_range=(1, 4), prob=0), None, True),
    (dict(mean=MEAN, to_rgb=True, ratio_range=(1, 4), prob=0.5), None, True),
    (dict(mean=MEAN, to_rgb=False, ratio_range=(1, 2), prob=1), None, True),
    (dict(mean=(7.9, 7.9, 7.9), to_rgb=True, ratio_range=(1, 4), prob=1), None, True),
    (None, dict(), True),
    (None, dict(min_ious=(0.9,)), True),
    (None, dict(bbox_clip_border=False), True),
    (None, dict(min_crop_size=0.9), True),
    (None, dict(min_crop_size=0.2), True),                      # (small patches: MORE_SEEDS holds one with an ignore box only)
    (dict(mean=MEAN, to_rgb=True, ratio_range=(1, 2), prob=0.5), dict(), True),
    (dict(mean=MEAN, to_rgb=True, ratio_range=(1, 4), prob=1), dict(min_ious=(0.1, 0.3), min_crop_size=0.5), True),
    (dict(mean=MEAN, to_rgb=True, ratio_range=(1, 2), prob=0.5), dict(), False),
    (None, dict(min_crop_size=0.9), False),
]
RESIZES = [dict(img_scale=(64, 48), keep_ratio=True), dict(img_scale=(64, 48), keep_ratio=False)]
SEEDS = range(8)
MORE_SEEDS = {8: (21, 367)}                                     # (case index -> further seeds)


def main():
    img, masks = J.sample()
    out = dict(boxes=BOXES, ignore=IGNORE, labels=LABELS, src_hw=np.array([H, W]),
               cases=np.asarray(json.dumps([[a, b, c] for a, b, c in CASES])), resizes=np.asarray(json.dumps(RESIZES)))
    seen = dict(skipped=0, expanded=0, mode1=0, abandoned=0, dropped=0, gt_emptied=0, fill=0, no_boxes=0)
    rows, cat = {}, {}
    for c, (ea, ca, with_boxes) in enumerate(CASES):
        for k, ra in enumerate(RESIZES):
            for seed in (*SEEDS, *MORE_SEEDS.get(c, ())):
                np.random.seed(seed)
                nb = len(BOXES) if with_boxes else 0
                r = dict(img=img.copy(), img_shape=img.shape, img_fields=["img"], bbox_fields=["gt_bboxes_ignore", "gt_bboxes"],
                         mask_fields=["gt_masks"], gt_bboxes=BOXES[:nb].copy(), gt_bboxes_ignore=IGNORE[:nb and 2].copy(),
                         gt_labels=LABELS[:nb].copy(), gt_masks=Masks(masks[:nb]))
                canvas, left, top, applied = (H, W), 0, 0, False
                if ea is not None:
                    # Expand's draws, replayed from the saved state and checked against what it made
                    state = np.random.get_state()
                    if not np.random.uniform(0, 1) > ea["prob"]:
                        applied = True
                        ratio = np.random.uniform(*ea["ratio_range"])
                        canvas = (int(H * ratio), int(W * ratio))
                        left, top = int(np.random.uniform(0, W * ratio - W)), int(np.random.uniform(0, H * ratio - H))
                    np.random.set_state(state)
                    r = Expand(**ea)(r)
                    assert r["img"].shape[:2] == canvas and np.array_equal(r["img"][top:top + H, left:left + W], img)
                    assert r["gt_masks"].masks.shape[1:] == canvas
                    if applied:
                        fill = np.asarray(ea["mean"][::-1] if ea["to_rgb"] else ea["mean"]).astype(np.uint8)
                        outside = np.ones(canvas, bool)
                        outside[top:top + H, left:left + W] = False
                        assert (r["img"][outside] == fill).all()
                    seen["expanded" if applied else "skipped"] += 1
                mode, patch, modes = -1.0, (-1, -1, -1, -1), 0              # (-1: no crop stage)
                if ca is not None:
                    crop, T.random = MinIoURandomCrop(**ca), CountingRandom()
                    del PATCHES[:]
                    before = r["img"]
                    r = crop(r)
                    mode, modes = float(crop.mode), T.random.choices
                    T.random = np.random
                    if mode != 1:
                        patch = tuple(int(v) for v in PATCHES[-1])
                        assert np.array_equal(r["img"], before[patch[1]:patch[3], patch[0]:patch[2]])
                        assert r["img_shape"] == r["img"].shape
                        assert r["img"].shape[:2] == (patch[3] - patch[1], patch[2] - patch[0])
                        seen["fill"] += applied and not (left <= patch[0] and top <= patch[1] and patch[2] <= left + W
                                                         and patch[3] <= top + H)
                    else:
                        assert r["img"] is before
                    seen["mode1"] += mode == 1
                    seen["abandoned"] += modes > 1
                zoom = dict(zoom_hw=r["img"].shape[:2], zoom_img_shape=r["img_shape"], zoom_boxes=r["gt_bboxes"].copy(),
                            zoom_ignore=r["gt_bboxes_ignore"].copy())
                assert not with_boxes or r["gt_masks"].masks.shape[1:] == r["img"].shape[:2]
                r = Resize(**ra)(r)
                nxt = np.random.random_sample()
                assert len(r["gt_masks"].index) == len(r["gt_bboxes"]) == len(r["gt_labels"])
                seen["dropped"] += with_boxes and len(r["gt_bboxes"]) < len(BOXES)
                seen["gt_emptied"] += with_boxes and len(r["gt_bboxes"]) == 0 and len(r["gt_bboxes_ignore"]) > 0
                seen["no_boxes"] += not with_boxes and mode not in (-1.0, 1.0)
                for name, v in dict(case=c, resize=k, seed=seed, applied=applied, canvas=canvas, left=left, top=top, mode=mode,
                                    modes=modes, patch=patch, zoom_hw=zoom["zoom_hw"], zoom_img_shape=zoom["zoom_img_shape"],
                                    img_shape=r["img_shape"], scale_factor=r["scale_factor"], next=nxt,
                                    n_boxes=len(r["gt_bboxes"]), n_ignore=len(r["gt_bboxes_ignore"])).items():
                    rows.setdefault(name, []).append(v)
                for name, v in (("gt_bboxes", r["gt_bboxes"]), ("gt_bboxes_ignore", r["gt_bboxes_ignore"]), ("gt_labels", r["gt_labels"]),
                                ("kept", r["gt_masks"].index), ("zoom_boxes", zoom["zoom_boxes"]), ("zoom_ignore", zoom["zoom_ignore"])):
                    cat.setdefault(name, []).append(v)
    out.update({k: np.array(v) for k, v in rows.items()})
    out.update({k: np.concatenate(v) for k, v in cat.items()})
    print(seen)
    assert all(seen.values()), seen
    path = os.path.join(HERE, "zoom_aug.npz")
    np.savez_compressed(path, **out)
    print(f"zoom_aug.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
