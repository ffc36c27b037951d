"""Generates tests/golden/tta_views.npz by RUNNING THE REFERENCE on the CPU, for tests/test_tta_cpu.py and
tests/test_gpu_tta.py (test-time augmentation).

    python tests/golden/gen_tta.py

Only data is written.  The reference is imported at generation time through ref_import, like gen_golden.py.

(a) `bbox_mapping_back` (radet/core/bbox/transforms.py:46-55) on 200 boxes per case: `a_boxes` f32 [N, 200, 4] the inputs,
    `a_out` f32 [N, 200, 4] the reference's outputs, `a_hw` i32 [N, 2] the img_shape, `a_sf` f32 [N, 4] the scale factor,
    `a_flip` i32 [N] the code (0 none, 1 horizontal, 2 vertical, 3 diagonal).  Cases: every flip with each of four
    geometries -- odd img_shapes and the scale factors keep_ratio rounding gives them (w_scale != h_scale), a unit scale, a
    non-round downscale.  Of the 200 boxes the first 16 lie on the image border (coordinates 0, w, h, zero-size boxes in the
    corners), the others are random inside the image, as the decode kernel's clamp leaves them.
(b) the reference `MultiScaleFlipAug`'s view order for three configurations: `b<k>_scale` i32 [V, 2], `b<k>_flip` u8 [V],
    `b<k>_dir` i32 [V] (codes as above), and the configuration itself (`b<k>_img_scale` i32 [S, 2], `b<k>_cfg_flip`,
    `b<k>_cfg_dir` i32 [D]).  The reference's pipeline package does not import here without mmcv and cv2, so
    radet/datasets/pipelines/test_time_aug.py is loaded ALONE: its `..builder` and `.compose` imports resolve to small
    stand-ins (a registry holding one recording stage named RandomFlip, and a Compose that calls the stages in order).
    What runs and is recorded is the reference's own MultiScaleFlipAug.__init__ / __call__; the stand-ins only return the
    `scale`, `flip` and `flip_direction` each view was called with.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ref_import  # noqa: E402

ref_import.install()

CODES = {None: 0, "horizontal": 1, "vertical": 2, "diagonal": 3}
NBOX = 200


def geometries():
    """(img_shape, scale_factor) as Resize(keep_ratio=True) computes them for a source size and an img_scale"""
    out = []
    for (h, w), scale in (((37, 53), (64, 48)), ((480, 640), (1333, 801)), ((5, 7), (5, 7)), ((481, 641), (333, 200))):
        f = min(max(scale) / max(h, w), min(scale) / min(h, w))
        nw, nh = int(w * float(f) + 0.5), int(h * float(f) + 0.5)
        sf = np.array([nw / w, nh / h, nw / w, nh / h], np.float32)
        out.append(((nh, nw), sf))
    return out


def boxes_for(h, w, rng):
    border = np.array([[0, 0, w, h], [0, 0, 0, 0], [w, h, w, h], [0, h, 0, h], [w, 0, w, 0], [0, 0, w, 1], [0, 0, 1, h],
                       [w - 1, 0, w, h], [0, h - 1, w, h], [0, 0, 0.5, 0.5], [w - 0.25, h - 0.25, w, h], [0, 1, w, 2],
                       [1, 0, 2, h], [0.125, 0.375, w, h], [0, 0, w - 0.125, h - 0.375], [w / 2, h / 2, w / 2, h / 2]], np.float32)
    p = rng.random_sample((NBOX - len(border), 4)).astype(np.float32) * np.array([w, h, w, h], np.float32)
    lo, hi = np.minimum(p[:, :2], p[:, 2:]), np.maximum(p[:, :2], p[:, 2:])
    return np.concatenate([border, np.concatenate([lo, hi], 1)]).astype(np.float32)


def mapping_back():
    from radet.core.bbox.transforms import bbox_mapping_back
    rng = np.random.RandomState(20)
    A = dict(a_boxes=[], a_out=[], a_hw=[], a_sf=[], a_flip=[])
    for (h, w), sf in geometries():
        for direction, code in CODES.items():
            b = boxes_for(h, w, rng)
            out = bbox_mapping_back(torch.from_numpy(b), (h, w, 3), sf, direction is not None, direction or "horizontal")
            assert out.dtype == torch.float32
            A["a_boxes"].append(b)
            A["a_out"].append(out.numpy())
            A["a_hw"].append([h, w])
            A["a_sf"].append(sf)
            A["a_flip"].append(code)
    return dict(a_boxes=np.stack(A["a_boxes"]), a_out=np.stack(A["a_out"]), a_hw=np.array(A["a_hw"], np.int32),
                a_sf=np.stack(A["a_sf"]).astype(np.float32), a_flip=np.array(A["a_flip"], np.int32))


def load_reference_msfa():
    pkg = types.ModuleType("_ref_tta")
    pkg.__path__ = []
    sub = types.ModuleType("_ref_tta.pipelines")
    sub.__path__ = []
    registry = ref_import.Registry("pipeline")

    class RandomFlip:                                            # records what the view was called with
        def __call__(self, results):
            return dict(scale=results["scale"], flip=results["flip"], flip_direction=results["flip_direction"])
    registry.register_module()(RandomFlip)

    class Compose:
        def __init__(self, transforms):
            self.transforms = [ref_import.build_from_cfg(t, registry) for t in transforms]

        def __call__(self, data):
            for t in self.transforms:
                data = t(data)
            return data
    builder = types.ModuleType("_ref_tta.builder")
    builder.PIPELINES = registry
    compose = types.ModuleType("_ref_tta.pipelines.compose")
    compose.Compose = Compose
    sys.modules.update({"_ref_tta": pkg, "_ref_tta.pipelines": sub, "_ref_tta.builder": builder,
                        "_ref_tta.pipelines.compose": compose})
    import mmcv
    mmcv.is_list_of = lambda seq, t: isinstance(seq, list) and all(isinstance(v, t) for v in seq)
    path = os.path.join(ref_import.REFERENCE_ROOT, "radet", "datasets", "pipelines", "test_time_aug.py")
    spec = importlib.util.spec_from_file_location("_ref_tta.pipelines.test_time_aug", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MultiScaleFlipAug


CONFIGS = [
    dict(img_scale=[(64, 48), (96, 80)], flip=True, flip_direction="horizontal"),
    dict(img_scale=(64, 48), flip=True, flip_direction=["horizontal", "vertical", "diagonal"]),
    dict(img_scale=[(64, 48), (96, 80), (48, 32)], flip=False, flip_direction="horizontal"),
]


def view_orders():
    MSFA = load_reference_msfa()
    out = {}
    for k, cfg in enumerate(CONFIGS):
        got = MSFA(transforms=[dict(type="RandomFlip")], **cfg)(dict(img=None))
        out[f"b{k}_scale"] = np.array(got["scale"], np.int32).reshape(-1, 2)
        out[f"b{k}_flip"] = np.array(got["flip"], np.uint8)
        out[f"b{k}_dir"] = np.array([CODES[d] for d in got["flip_direction"]], np.int32)
        scales = cfg["img_scale"] if isinstance(cfg["img_scale"], list) else [cfg["img_scale"]]
        dirs = cfg["flip_direction"] if isinstance(cfg["flip_direction"], list) else [cfg["flip_direction"]]
        out[f"b{k}_img_scale"] = np.array(scales, np.int32)
        out[f"b{k}_cfg_flip"] = np.array(cfg["flip"])
        out[f"b{k}_cfg_dir"] = np.array([CODES[d] for d in dirs], np.int32)
    return out


if __name__ == "__main__":
    data = {**mapping_back(), **view_orders()}
    path = os.path.join(HERE, "tta_views.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, {k: v.shape for k, v in data.items()}, os.path.getsize(path), "bytes")
