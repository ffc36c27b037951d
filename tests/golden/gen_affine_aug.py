"""Generates tests/golden/affine_aug.npz: the reference's Rotate, Shear, Translate and AutoAugment run on the small synthetic
sample of gen_scale_jitter.py under seeded np.random, for tests/test_affine_cpu.py to compare the planning of radet_amd
against.

    python tests/golden/gen_affine_aug.py

The reference is imported at generation time only (ref_import), with the mmcv / cv2 stubs of gen_scale_jitter.py.
mmcv.imrotate / imshear / imtranslate and cv2.getRotationMatrix2D are supplied here: they record their arguments and
return the restatement of tests/_affine_ref.py, so what is pinned is the reference's planning -- gates, signs, matrices,
box arithmetic, filters, the number of draws -- not cv2's pixels.  The policy an AutoAugment drew is recorded by tagged
wrappers put in the place of its composed policies.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_scale_jitter as J  # noqa: E402  (installs the reference and the mmcv stub)
import _affine_ref as A  # noqa: E402

import cv2  # noqa: E402  (the stub)
import mmcv  # noqa: E402  (the stub)

H, W, BOXES, IGNORE, LABELS = J.H, J.W, J.BOXES, J.IGNORE, J.LABELS
CALLS = []                                                       # (kind, signed parameter, forward matrix) per warp of the image


def _centre(img, center):
    h, w = img.shape[:2]
    return ((w - 1) * 0.5, (h - 1) * 0.5) if center is None else center


def imrotate(img, angle, center=None, scale=1.0, border_value=0, interpolation="bilinear", auto_bound=False):
    assert interpolation == "bilinear" and not auto_bound
    M = A.rotation_matrix(_centre(img, center), -angle, scale)
    if img.ndim == 3 and img.shape[2] == 3:
        CALLS.append(("Rotate", float(angle), M))
    return A.warp_affine_u8(img, M, np.rint(np.asarray(border_value, np.float64)))


def imshear(img, magnitude, direction="horizontal", border_value=0, interpolation="bilinear"):
    assert interpolation == "bilinear"
    M = A.shear_matrix(magnitude, direction)
    if img.ndim == 3 and img.shape[2] == 3:
        CALLS.append(("Shear", float(magnitude), M))
    return A.warp_affine_u8(img, M, np.rint(np.asarray(border_value, np.float64)))


def imtranslate(img, offset, direction="horizontal", border_value=0, interpolation="bilinear"):
    assert interpolation == "bilinear"
    M = A.translate_matrix(offset, direction)
    if img.ndim == 3 and img.shape[2] == 3:
        CALLS.append(("Translate", float(offset), M))
    return A.warp_affine_u8(img, M, np.rint(np.asarray(border_value, np.float64)))


ROTATION_MATRICES = []


def getRotationMatrix2D(center, angle, scale):
    M = A.rotation_matrix(center, angle, scale)
    ROTATION_MATRICES.append(M)
    return M


mmcv.imrotate, mmcv.imshear, mmcv.imtranslate, cv2.getRotationMatrix2D = imrotate, imshear, imtranslate, getRotationMatrix2D

from radet.datasets.pipelines.auto_augment import AutoAugment, Rotate, Shear, Translate  # noqa: E402


class Masks(J.Masks):
    """+ BitmapMasks.rotate / shear / translate (core/mask/structures.py): the masks warped as channels, fill 0"""

    def __getitem__(self, idx):
        return Masks(self.masks[idx].reshape(-1, *self.masks.shape[1:]), self.index[idx])

    def rotate(self, out_shape, angle, center=None, scale=1.0, fill_val=0):
        assert tuple(out_shape) == self.masks.shape[1:] and fill_val == 0
        M = A.rotation_matrix(_centre(self.masks[0] if len(self.masks) else np.zeros(out_shape), center), -angle, scale)
        return Masks(A.warp_masks(self.masks, M), self.index)

    def shear(self, out_shape, magnitude, direction="horizontal", border_value=0, interpolation="bilinear"):
        assert tuple(out_shape) == self.masks.shape[1:] and border_value == 0 and interpolation == "bilinear"
        return Masks(A.warp_masks(self.masks, A.shear_matrix(magnitude, direction)), self.index)

    def translate(self, out_shape, offset, direction="horizontal", fill_val=0, interpolation="bilinear"):
        assert tuple(out_shape) == self.masks.shape[1:] and fill_val == 0
        return Masks(A.warp_masks(self.masks, A.translate_matrix(offset, direction)), self.index)


class Tagged:
    """a composed policy of an AutoAugment that says when it was chosen"""
    chosen = []

    def __init__(self, k, transform):
        self.k, self.transform = k, transform

    def __call__(self, results):
        Tagged.chosen.append(self.k)
        return self.transform(results)


STAGES = dict(Rotate=Rotate, Shear=Shear, Translate=Translate, AutoAugment=AutoAugment)
POLICIES = [[dict(type="Shear", level=6, prob=0.7, direction="vertical"), dict(type="Rotate", level=8, prob=0.6, img_fill_val=(0., 37., 255.))],
            [dict(type="Translate", level=2, prob=0.8, max_translate_offset=100.)]]
# (stage, arguments): each stage at prob 0, 0.5 and 1, both directions, an off-centre centre, scale 0.8, level 0, offsets that
# push boxes out, min_size > 0, a two-policy AutoAugment whose first policy has two stages
CASES = [
    ("Rotate", dict(level=10, prob=0)),
    ("Rotate", dict(level=10, prob=0.5)),
    ("Rotate", dict(level=10, prob=1, max_rotate_angle=30)),
    ("Rotate", dict(level=7, prob=1, center=(5, 40), scale=0.8, img_fill_val=(0., 37., 255.))),
    ("Rotate", dict(level=10, prob=1, max_rotate_angle=90, random_negative_prob=0.)),
    ("Rotate", dict(level=0, prob=1)),
    ("Shear", dict(level=10, prob=0)),
    ("Shear", dict(level=10, prob=0.5)),
    ("Shear", dict(level=10, prob=1, direction="vertical")),
    ("Shear", dict(level=5, prob=1, max_shear_magnitude=1.0)),
    ("Shear", dict(level=0, prob=1)),
    ("Translate", dict(level=10, prob=0)),
    ("Translate", dict(level=1, prob=0.5)),
    ("Translate", dict(level=2, prob=1, direction="vertical")),
    ("Translate", dict(level=3, prob=1, max_translate_offset=150.)),                 # (45 pixels: boxes leave the image)
    ("Translate", dict(level=10, prob=1, max_translate_offset=56, direction="vertical", min_size=2, random_negative_prob=0.)),
    ("Translate", dict(level=4, prob=1, max_translate_offset=100., min_size=12)),
    ("Translate", dict(level=0, prob=1)),
    ("AutoAugment", dict(policies=POLICIES)),
]
SEEDS = range(8)
MAX_ENTRIES = 2


def main():
    img, masks = J.sample()
    out = dict(boxes=BOXES, ignore=IGNORE, labels=LABELS, src_hw=np.array([H, W]),
               cases=np.asarray(json.dumps([[a, b] for a, b in CASES])))
    seen = dict(fired=0, skipped=0, negative=0, positive=0, dropped=0, gt_emptied=0, policy0=0, policy1=0, two_entries=0)
    rows, cat = {}, {}
    for c, (name, args) in enumerate(CASES):
        for seed in SEEDS:
            np.random.seed(seed)
            r = dict(img=img.copy(), img_shape=img.shape, img_fields=["img"], bbox_fields=["gt_bboxes_ignore", "gt_bboxes"],
                     mask_fields=["gt_masks"], gt_bboxes=BOXES.copy(), gt_bboxes_ignore=IGNORE.copy(), gt_labels=LABELS.copy(),
                     gt_masks=Masks(masks))
            stage = STAGES[name](**args)
            if name == "AutoAugment":
                stage.transforms = [Tagged(k, t) for k, t in enumerate(stage.transforms)]
            del CALLS[:], ROTATION_MATRICES[:], Tagged.chosen[:]
            r = stage(r)
            nxt = np.random.random_sample()
            assert r["img"].shape == img.shape and r["gt_masks"].masks.shape[1:] == (H, W)
            assert len(r["gt_masks"].index) == len(r["gt_bboxes"]) == len(r["gt_labels"])
            assert len(CALLS) <= MAX_ENTRIES
            rot = [m for kind, _, m in CALLS if kind == "Rotate"]
            assert len(rot) == len(ROTATION_MATRICES) and all(np.array_equal(a, b) for a, b in zip(rot, ROTATION_MATRICES))
            policy = Tagged.chosen[0] if name == "AutoAugment" else -1                  # (-1: no AutoAugment)
            seen["fired" if CALLS else "skipped"] += 1
            for _, v, _ in CALLS:
                seen["negative" if np.copysign(1.0, v) < 0 else "positive"] += 1
            seen["dropped"] += 0 < len(r["gt_bboxes"]) < len(BOXES)
            seen["gt_emptied"] += len(r["gt_bboxes"]) == 0 and len(r["gt_bboxes_ignore"]) > 0
            seen["two_entries"] += len(CALLS) == 2
            if policy >= 0:
                seen[f"policy{policy}"] += 1
            for key, v in dict(case=c, seed=seed, n_entries=len(CALLS), policy=policy, next=nxt, n_boxes=len(r["gt_bboxes"]),
                               n_ignore=len(r["gt_bboxes_ignore"])).items():
                rows.setdefault(key, []).append(v)
            for key, v in (("gt_bboxes", r["gt_bboxes"]), ("gt_bboxes_ignore", r["gt_bboxes_ignore"]), ("gt_labels", r["gt_labels"]),
                           ("kept", r["gt_masks"].index), ("values", np.array([v for _, v, _ in CALLS], np.float64)),
                           ("matrices", np.array([m for _, _, m in CALLS], np.float64).reshape(-1, 2, 3))):
                cat.setdefault(key, []).append(v)
    out.update({k: np.array(v) for k, v in rows.items()})
    out.update({k: np.concatenate(v) for k, v in cat.items()})
    print(seen)
    assert all(seen.values()), seen
    path = os.path.join(HERE, "affine_aug.npz")
    np.savez_compressed(path, **out)
    print(f"affine_aug.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
