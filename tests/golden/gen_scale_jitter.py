"""Generates tests/golden/scale_jitter.npz: the reference's Resize (random scales) and RandomCrop run on small synthetic
samples under seeded np.random, for tests/test_scalejitter_cpu.py to compare the planning of radet_amd against.

    python tests/golden/gen_scale_jitter.py

The reference is imported at generation time only (ref_import).  mmcv is absent: imrescale / imresize / rescale_size are
set on its stub from oracle/imgproc.py and oracle/masks.py; the instance masks go through a small wrapper that restates
BitmapMasks.rescale / resize / __getitem__ / crop with oracle/masks.py and keeps the indices of the surviving masks.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ref_import  # noqa: E402
from oracle import imgproc, masks as om  # noqa: E402

ref_import.install()
import mmcv  # noqa: E402  (the stub)


def imrescale(img, scale, return_scale=False, interpolation="bilinear", backend=None):
    h, w = img.shape[:2]
    new_size = om.rescale_size((w, h), scale)
    out = imgproc.resize_linear_u8(img, new_size)
    return (out, min(new_size[0] / w, new_size[1] / h)) if return_scale else out


def imresize(img, size, return_scale=False, interpolation="bilinear", backend=None):
    h, w = img.shape[:2]
    out = imgproc.resize_linear_u8(img, size)
    return (out, size[0] / w, size[1] / h) if return_scale else out


mmcv.imrescale, mmcv.imresize, mmcv.rescale_size = imrescale, imresize, om.rescale_size
mmcv.is_list_of = lambda seq, t: isinstance(seq, list) and all(isinstance(v, t) for v in seq)

from radet.datasets.pipelines.transforms import RandomCrop, Resize  # noqa: E402


class Masks:
    """BitmapMasks.rescale / resize / __getitem__ / crop (core/mask/structures.py) over oracle/masks.py"""

    def __init__(self, masks, index=None):
        self.masks = masks
        self.index = np.arange(len(masks)) if index is None else index

    def rescale(self, scale):
        h, w = self.masks.shape[1:]
        nw, nh = om.rescale_size((w, h), scale)
        return Masks(om.resize_nearest(self.masks, (nh, nw)), self.index)

    def resize(self, out_shape):
        return Masks(om.resize_nearest(self.masks, tuple(out_shape)), self.index)

    def __getitem__(self, idx):
        return Masks(self.masks[idx].reshape(-1, *self.masks.shape[1:]), self.index[idx])

    def crop(self, bbox):
        h, w = self.masks.shape[1:]
        bbox = bbox.copy()
        bbox[0::2] = np.clip(bbox[0::2], 0, w)
        bbox[1::2] = np.clip(bbox[1::2], 0, h)
        x1, y1, x2, y2 = bbox
        cw, ch = np.maximum(x2 - x1, 1), np.maximum(y2 - y1, 1)
        return Masks(self.masks[:, y1:y1 + ch, x1:x1 + cw], self.index)


H, W = 60, 80
BOXES = np.array([[4.5, 6.0, 30.25, 28.0], [40.0, 10.5, 78.0, 55.0], [60.0, 2.0, 79.5, 12.0], [10.0, 40.0, 35.0, 58.5]], np.float32)
IGNORE = np.array([[0.0, 0.0, 12.0, 9.0], [50.0, 45.0, 80.0, 60.0]], np.float32)
LABELS = np.array([3, 0, 7, 11], np.int64)

# (resize arguments, crop arguments); every multiscale mode, ratio_range, the four crop types, both bbox_clip_border values
CASES = [
    (dict(img_scale=(80, 60), ratio_range=(0.6, 1.6)), dict(crop_size=(60, 80))),
    (dict(img_scale=(80, 60), ratio_range=(0.6, 1.6)), dict(crop_size=(60, 80), bbox_clip_border=False)),
    (dict(img_scale=(80, 60), ratio_range=(1.5, 2.5), bbox_clip_border=False), dict(crop_size=(30, 24))),
    (dict(img_scale=[(64, 48), (128, 96)], multiscale_mode="range"), dict(crop_size=(40, 72), crop_type="absolute_range")),
    (dict(img_scale=[(64, 48), (96, 72), (160, 120)], multiscale_mode="value"), dict(crop_size=(0.5, 0.6), crop_type="relative")),
    (dict(img_scale=[(64, 48), (96, 72), (160, 120)], multiscale_mode="value", keep_ratio=False),
     dict(crop_size=(0.3, 0.4), crop_type="relative_range", bbox_clip_border=False)),
    (dict(img_scale=(82, 62)), dict(crop_size=(60, 80))),                    # (margins of 2: windows in the corners)
    (dict(img_scale=(200, 150)), dict(crop_size=(8, 8))),                    # (small crops: some hold no box)
    (dict(img_scale=(200, 150)), dict(crop_size=(8, 8), allow_negative_crop=True)),
]
SEEDS = range(8)


def sample():
    rng = np.random.RandomState(1)
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    masks = np.zeros((len(BOXES), H, W), np.uint8)
    for m, (x0, y0, x1, y1) in zip(masks, BOXES.astype(int)):
        m[y0:y1, x0:x1] = 1
    return img, masks


def main():
    img, masks = sample()
    out = dict(boxes=BOXES, ignore=IGNORE, labels=LABELS, src_hw=np.array([H, W]),
               cases=np.asarray(json.dumps([[a, b] for a, b in CASES])))
    seen = dict(dropped=0, none=0, larger=0, below1=0, corner=0)
    rows, cat = {}, {}
    for c, (ra, ca) in enumerate(CASES):
        for seed in SEEDS:
            np.random.seed(seed)
            r = dict(img=img.copy(), img_fields=["img"], bbox_fields=["gt_bboxes_ignore", "gt_bboxes"], mask_fields=["gt_masks"],
                     gt_bboxes=BOXES.copy(), gt_bboxes_ignore=IGNORE.copy(), gt_labels=LABELS.copy(), gt_masks=Masks(masks))
            r = Resize(**ra)(r)
            Hr, Wr = r["img"].shape[:2]
            pre = dict(scale=r["scale"], scale_idx=-1 if r["scale_idx"] is None else r["scale_idx"],     # (-1: None)
                       resized_hw=[Hr, Wr], scale_factor=r["scale_factor"])
            # RandomCrop draws the window inside _crop_data and does not keep it: the same draws, replayed
            state = np.random.get_state()
            crop = RandomCrop(**ca)
            ch, cw = crop._get_crop_size((Hr, Wr))
            y0 = np.random.randint(0, max(Hr - ch, 0) + 1)
            x0 = np.random.randint(0, max(Wr - cw, 0) + 1)
            np.random.set_state(state)
            r = crop(r)
            nxt = np.random.random_sample()
            ch, cw = min(ch, Hr - y0), min(cw, Wr - x0)
            for name, v in dict(pre, window=[y0, x0, ch, cw], next=nxt, none=r is None, case=c, seed=seed).items():
                rows.setdefault(name, []).append(v)
            seen["larger"] += ca.get("crop_type", "absolute") == "absolute" and (ca["crop_size"][0] > Hr or ca["crop_size"][1] > Wr)
            seen["below1"] += "ratio_range" in ra and r is not None and pre["scale"][0] < ra["img_scale"][0]
            seen["corner"] += y0 + ch == Hr and x0 + cw == Wr and (y0 > 0 or x0 > 0)
            if r is None:
                seen["none"] += 1
                r = dict(img_shape=(0, 0, 0), gt_bboxes=BOXES[:0], gt_bboxes_ignore=BOXES[:0], gt_labels=LABELS[:0], gt_masks=Masks(masks[:0]))
            else:
                assert r["img"].shape[:2] == (ch, cw) and r["gt_masks"].masks.shape[1:] == (ch, cw)
                assert len(r["gt_masks"].index) == len(r["gt_bboxes"]) == len(r["gt_labels"])
                seen["dropped"] += len(r["gt_bboxes"]) < len(BOXES)
            # the ragged fields, concatenated over the samples: n_boxes / n_ignore rows each
            rows.setdefault("img_shape", []).append(r["img_shape"])
            rows.setdefault("n_boxes", []).append(len(r["gt_bboxes"]))
            rows.setdefault("n_ignore", []).append(len(r["gt_bboxes_ignore"]))
            for name, v in (("gt_bboxes", r["gt_bboxes"]), ("gt_bboxes_ignore", r["gt_bboxes_ignore"]), ("gt_labels", r["gt_labels"]),
                            ("kept", r["gt_masks"].index)):
                cat.setdefault(name, []).append(v)
    out.update({k: np.array(v) for k, v in rows.items()})
    out.update({k: np.concatenate(v) for k, v in cat.items()})
    print(seen)
    assert all(seen.values()), seen
    path = os.path.join(HERE, "scale_jitter.npz")
    np.savez_compressed(path, **out)
    print(f"scale_jitter.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
