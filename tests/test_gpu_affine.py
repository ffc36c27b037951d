"""Affine augmentation on the GPU: radet_warp_affine_u8 on frames and on masks against the integer NumPy restatement of
cv2.warpAffine (tests/_affine_ref.py), entries in sequence, the pipeline on Rotate and on AutoAugment against the staged
host restatement built from each planned sample's recorded draws, launch parity and the rotate config.  Every comparison
is array_equal / torch.equal."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _affine_ref as A  # noqa: E402
from _affine_cfg import rotate_train_cfg  # noqa: E402
from _maskfree_pipelines import ASSIGNER, COSY, NORM  # noqa: E402
from oracle import masks as om  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0xAB
SIZES = [(1, 1), (2, 9), (37, 53), (48, 64)]
FILLS = [(128, 128, 128), (0, 37, 255)]


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def matrices(h, w):
    """name -> forward matrix for an h x w image (None: the skip flag)"""
    centre = ((w - 1) * 0.5, (h - 1) * 0.5)
    out = {"identity": np.array([[1, 0, 0], [0, 1, 0]], np.float64), "skip": None}
    for angle in (30, -30, 90):
        out[f"rotate {angle}"] = A.rotation_matrix(centre, angle, 1)
    for scale in (0.8, 1.3):
        out[f"rotate 17.5 about (5, 40) x {scale}"] = A.rotation_matrix((5, 40), 17.5, scale)
    for m in (0.3, -0.3):
        for d in ("horizontal", "vertical"):
            out[f"shear {m} {d}"] = A.shear_matrix(m, d)
    for off in (7, -7, 100, -100):
        out[f"translate {off}"] = A.translate_matrix(off)
    out["translate 7 vertical"] = A.translate_matrix(7, "vertical")
    return out


@pytest.fixture(scope="module")
def frames():
    rs = np.random.RandomState(0)
    return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]


@pytest.fixture(scope="module")
def frame_rows(frames):
    """every (image, matrix, fill) as one row of one launch: (image index, name, matrix, fill, expected output)"""
    rows = []
    for k, img in enumerate(frames):
        for name, M in matrices(*img.shape[:2]).items():
            for fill in FILLS:
                rows.append((k, name, M, fill, img if M is None else A.warp_affine_u8(img, M, fill)))
    return rows


def test_reference_rows_are_not_vacuous(frames, frame_rows):
    big = [r for r in frame_rows if r[0] == 3]
    assert all((r[4] == np.array(r[3], np.uint8)).all() for r in big if r[1] in ("translate 100", "translate -100"))     # all fill
    assert all(np.array_equal(r[4], frames[3]) for r in big if r[1] in ("identity", "skip"))
    for r in big:
        if r[1].startswith(("rotate", "shear")):
            is_fill = (r[4] == np.array(r[3], np.uint8)).all(axis=-1)
            assert 0 < is_fill.sum() < is_fill.size and not np.array_equal(r[4], frames[3]), r[1]


def test_kernel_equals_the_restatement(frames, frame_rows):
    """one launch over all rows: mixed sizes, images 5 pixels apart in the destination; the whole buffer is compared, the
    bytes between the images included"""
    from radet_amd import kernels as K
    dev = _dev()
    soff = np.cumsum([0] + [f.shape[0] * f.shape[1] for f in frames])
    src = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(dev)
    D = np.zeros((len(frame_rows), K.WARP_DESC_INTS), np.int32)
    o = 5
    for row, (k, name, M, fill, want) in zip(D, frame_rows):
        h, w = frames[k].shape[:2]
        K.warp_desc_row(row, int(soff[k]), o, h, w, 3, M, fill)
        o += h * w + 5
    want = np.full(o * 3, GUARD, np.uint8)
    for row, r in zip(D, frame_rows):
        want[row[1] * 3:row[1] * 3 + r[4].size] = r[4].reshape(-1)
    dst = torch.full((o * 3,), GUARD, dtype=torch.uint8, device=dev)
    K.warp_affine_u8(src, dst, torch.from_numpy(D).to(dev), len(D), max(h * w for h, w in SIZES), 3)
    got = dst.cpu().numpy()
    for row, r in zip(D, frame_rows):
        np.testing.assert_array_equal(got[row[1] * 3:row[1] * 3 + r[4].size].reshape(r[4].shape), r[4], err_msg=f"image {r[0]}: {r[1]}, fill {r[3]}")
    assert torch.equal(dst.cpu(), torch.from_numpy(want))


def test_kernel_refuses_bad_arguments(frames):
    from radet_amd import _lib, kernels as K
    dev = _dev()
    src = torch.from_numpy(frames[2].reshape(-1)).to(dev)
    dst = torch.full_like(src, GUARD)
    D = np.zeros((2, K.WARP_DESC_INTS), np.int32)
    K.warp_desc_row(D[0], 0, 0, 37, 53, 3, A.translate_matrix(7))
    desc = torch.from_numpy(D).to(dev)
    for args in ((src, dst, desc, 1, 37 * 53, 2), (src, dst, desc, -1, 37 * 53, 3), (src, src, desc, 1, 37 * 53, 3),
                 (src, dst, desc, 1, -5, 3)):
        with pytest.raises(_lib.RadetHipError):
            K.warp_affine_u8(*args)
    # rows that leave their buffers, with another channel count or without pixels are not written
    K.warp_desc_row(D[0], 1, 0, 37, 53, 3, A.translate_matrix(7))
    K.warp_desc_row(D[1], 0, 0, 37, 53, 1, A.translate_matrix(7))
    K.warp_affine_u8(src, dst, torch.from_numpy(D).to(dev), 2, 37 * 53, 3)
    assert bool((dst == GUARD).all())
    with pytest.raises(ValueError, match="fixed point"):
        K.warp_desc_row(D[0], 0, 0, 37, 53, 3, A.translate_matrix(1e7))


# ------------------------------------------------------------------------------------------------ the mask form
MH, MW = 37, 53


@pytest.mark.parametrize("G", [0, 1, 5])
def test_mask_form_then_flip_and_pad(G):
    from radet_amd import kernels as K
    dev = _dev()
    rs = np.random.RandomState(G)
    masks = (rs.rand(G, MH, MW) < 0.5).astype(np.uint8)
    masks[:, 10:25, 20:40] = 1                                       # (a solid part: something survives every rotation)
    src = torch.from_numpy(masks).to(dev)
    for name, M in matrices(MH, MW).items():
        got = K.warp_affine_masks(src, [M] * G)
        want = masks if M is None else A.warp_masks(masks, M)
        assert set(np.unique(want)) <= {0, 1}
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=name)
        # resize, warp, then flip and pad: what the existing mask transform does to a bitmap
        out = K.mask_transform(got, out_hw=(48, 64), flip="horizontal")
        np.testing.assert_array_equal(out.cpu().numpy(), om.pad(om.flip(want), (48, 64), 0), err_msg=name)
    if G:
        assert A.warp_masks(masks, matrices(MH, MW)["rotate 30"]).any() and not A.warp_masks(masks, A.translate_matrix(100)).any()


def test_two_entries_in_sequence(frames):
    """a batch whose images carry 0, 1 and 2 entries: two launches, the shorter lists skipped"""
    from radet_amd import _lib
    from radet_amd.datasets.loading import ImagePipeline
    dev = _dev()
    imgs = [frames[2], frames[3], frames[2]]
    shear, rot = A.shear_matrix(0.3), A.rotation_matrix((26, 18), -30, 1)
    entries = [[], [(shear, FILLS[1])], [(shear, FILLS[1]), (rot, FILLS[0])]]
    offs, o = [], 0
    for f in imgs:
        offs.append(o)
        o += -(-f.shape[0] * f.shape[1] // 4) * 4                   # (the mix pipelines' packing)
    packed = np.full(o * 3, GUARD, np.uint8)
    for f, off in zip(imgs, offs):
        packed[off * 3:off * 3 + f.size] = f.reshape(-1)
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        out = ImagePipeline._warp_packed(torch.from_numpy(packed).to(dev), entries, offs, [f.shape[:2] for f in imgs], dev)
    finally:
        _lib.call = call
    assert seen == ["radet_warp_affine_u8"] * 2
    got = out.cpu().numpy()
    want = [imgs[0], A.warp_affine_u8(imgs[1], shear, FILLS[1]), A.warp_affine_u8(A.warp_affine_u8(imgs[2], shear, FILLS[1]), rot, FILLS[0])]
    for f, off, w in zip(imgs, offs, want):
        np.testing.assert_array_equal(got[off * 3:off * 3 + f.size].reshape(f.shape), w)
    assert not np.array_equal(want[2], want[1][:37, :53]) and not np.array_equal(want[1], imgs[1])


# ------------------------------------------------------------------------------------------------ the pipeline
SEED = 3
OUT = (48, 64)
ROTATE = dict(type="Rotate", level=10, max_rotate_angle=30, prob=1, img_fill_val=(0., 37., 255.))
POLICIES = [[dict(type="Shear", level=10, prob=0.8, direction="vertical"), dict(type="Rotate", level=6, prob=0.8, scale=0.9)],
            [dict(type="Translate", level=1, prob=0.9, max_translate_offset=120., min_size=3)]]
AUTO = dict(type="AutoAugment", policies=POLICIES)


def affine_pipeline(background_dir, *affine, ann="png"):
    """the pbr stages at Resize((64, 48)) with the affine stages directly after it"""
    return [
        dict(type="LoadImageFromFile"),
        dict(type="LoadAnnotations", with_bbox=True, **(dict(with_bop_mask=True) if ann == "png" else dict(with_mask=True))),
        dict(type="Resize", img_scale=(64, 48), keep_ratio=True),
        *affine,
        dict(type="RandomBackground", background_dir=background_dir, prob=0.5),
        dict(type="CosyPoseAug", p=0.8, pipelines=COSY),
        dict(type="RandomFlip", flip_ratio=0.5),
        dict(type="GenerateDistanceMap"),
        ASSIGNER,
        dict(type="Normalize", **NORM),
        dict(type="Pad", size_divisor=16),
        dict(type="DefaultFormatBundle"),
        dict(type="Collect", keys=["img", "gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight"]),
    ]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL decodes the generated JPEG / PNG files")
    import json
    from radet_amd.datasets.bop_convert import add_segmentation
    from tools.synth_bop import write_tree
    root = str(tmp_path_factory.mktemp("bop"))
    t = write_tree(root, n_frames=4, objects=(3, 5), n_backgrounds=2, seed=11)
    t["rle"] = os.path.join(root, "train_pbr_rle.json")
    json.dump(add_segmentation(json.load(open(t["ann_file"])), t["seg_prefix"], "rle"), open(t["rle"], "w"))
    return t


def _dataset(tree, *affine, ann="png", **kw):
    from radet_amd.datasets import build_dataset
    cfg = dict(type="BOPDataset", img_prefix=tree["img_prefix"], pipeline=affine_pipeline(tree["background_dir"], *affine, ann=ann), **kw)
    if ann == "png":
        return build_dataset(dict(cfg, ann_file=tree["ann_file"], seg_prefix=tree["seg_prefix"]))
    return build_dataset(dict(cfg, ann_file=tree["rle"], mask_source="annotation"))


def _plans(ds, epoch):
    from radet_amd.datasets.loader import sample_generators
    return [ds.plan_sample(i, *sample_generators(SEED, epoch, i)) for i in range(4)]


def _chain(ds, idx, s, stages):
    from PIL import Image
    info, ann = ds.data_infos[idx], ds.get_ann_info(idx)
    x = np.asarray(Image.open(os.path.join(ds.img_prefix, info["filename"])).convert("RGB"))[..., ::-1]
    m = np.stack([np.asarray(Image.open(os.path.join(ds.seg_prefix, p))) for p in ann["masks"]])
    if "policy" in s:
        stages = {t["type"]: t for t in POLICIES[s["policy"]]}
    return A.host_chain(x, m, ann["bboxes"], ann["labels"], s, OUT, stages, NORM, copy.deepcopy(s["_nprnd"]))


@pytest.fixture(scope="module")
def chains(tree):
    """the staged host restatement of one batch per pipeline (Rotate(prob=1); the two-policy AutoAugment), computed once"""
    out = {}
    for name, stage in (("rotate", ROTATE), ("auto", AUTO)):
        ds = _dataset(tree, stage)
        for idx, s in enumerate(_plans(ds, 0)):
            assert isinstance(s["img"], np.ndarray)
            out[(name, idx)] = _chain(ds, idx, s, {"Rotate": ROTATE})
    return out


def test_chains_are_not_vacuous(chains):
    for name in ("rotate", "auto"):
        kinds = [c["kinds"] for (n, _), c in chains.items() if n == name]
        assert any("fired" in k for k in kinds) and any("fill" in k for k in kinds) and any("mask" in k for k in kinds), (name, kinds)
    kinds = set().union(*(c["kinds"] for c in chains.values()))
    assert {"Rotate", "Shear", "Translate", "bg", "flip"} <= kinds, kinds
    assert any(c["kinds"] >= {"fill", "bg"} for c in chains.values())            # a background over the fill border


VARIANTS = {"host": dict(), "runs": dict(ann="rle"), "device-decode": dict(image_decode="device")}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["rotate", "auto"])
def test_pipeline_equals_the_staged_host_restatement(tree, chains, name, variant):
    ds = _dataset(tree, ROTATE if name == "rotate" else AUTO, **VARIANTS[variant])
    batch = ds.pipeline.run(_plans(ds, 0), collate=True)
    assert tuple(batch["img"].shape) == (4, 3, *OUT)
    img = batch["img"].cpu().numpy()
    for j in range(4):
        ref, what = chains[(name, j)], f"{name} sample {j}: {sorted(chains[(name, j)]['kinds'])}"
        np.testing.assert_array_equal(img[j], ref["img"], err_msg=what)
        np.testing.assert_array_equal(batch["gt_bboxes"][j].numpy(), ref["gt_bboxes"], err_msg=what)
        np.testing.assert_array_equal(batch["gt_labels"][j].numpy(), ref["gt_labels"], err_msg=what)
        np.testing.assert_array_equal(batch["points_to_gt_index"][j].cpu().numpy(), ref["p2g"], err_msg=what)
        np.testing.assert_array_equal(batch["points_weight"][j].cpu().numpy(), ref["pw"], err_msg=what)


def test_mix_fixed_pad_and_mask_free_pipelines_take_affine_entries(tree):
    """the mixpbr packing (images at multiples of 4 pixels), Pad(size=) (the assigner's masks padded after the warp) and the
    mask-free sampler on the same planned draws: the frames equal the plain pipeline's"""
    from _maskfree_pipelines import DM, MIX
    from radet_amd.datasets import build_dataset
    base = [t for t in affine_pipeline(tree["background_dir"], ROTATE) if t["type"] != "CosyPoseAug"]
    sub = dict(type="BOPDataset", img_prefix=tree["img_prefix"], ann_file=tree["ann_file"], seg_prefix=tree["seg_prefix"])
    ref = build_dataset(dict(sub, pipeline=base))
    want = ref.pipeline.run(_plans(ref, 0), collate=True)
    k = [t["type"] for t in base].index("RandomFlip")
    mix = build_dataset(dict(sub, pipeline=base[:k] + [dict(t, prob=0.0) for t in MIX] + base[k:]))
    assert mix.pipeline.mix
    got = mix.pipeline.run(_plans(mix, 0), collate=True)
    assert torch.equal(got["img"], want["img"])
    for key in ("gt_bboxes", "points_to_gt_index", "points_weight"):
        assert all(torch.equal(a, b) for a, b in zip(got[key], want[key]))
    padded = build_dataset(dict(sub, pipeline=[dict(type="Pad", size=(64, 80)) if t["type"] == "Pad" else t for t in base]))
    got = padded.pipeline.run(_plans(padded, 0), collate=True)
    assert tuple(got["img"].shape) == (4, 3, 64, 80) and torch.equal(got["img"][:, :, :48, :64], want["img"])
    assert bool((got["img"][:, :, 48:] == 0).all()) and bool((got["img"][:, :, :, 64:] == 0).all())
    assert all(torch.equal(a, b) for a, b in zip(got["gt_bboxes"], want["gt_bboxes"]))
    free = build_dataset(dict(sub, pipeline=[DM["mbd"] if t["type"] == "GenerateDistanceMap" else t for t in base]))
    assert free.pipeline.mask_free is not None
    got = free.pipeline.run(_plans(free, 0), collate=True)
    assert torch.equal(got["img"], want["img"]) and all(torch.equal(a, b) for a, b in zip(got["gt_bboxes"], want["gt_bboxes"]))


def test_launch_parity_when_no_sample_fires(tree):
    """a batch in which no sample drew an affine stage: the launches and the output of the pipeline built without the stage,
    under the same seeds (a stage with prob=0 draws once from the NumPy generator, so the flips are set equal by hand)"""
    from radet_amd import _lib
    never = _dataset(tree, dict(ROTATE, prob=0))
    without = _dataset(tree)
    a, b = _plans(never, 0), _plans(without, 0)
    assert not any("affine" in s for s in a)
    for s, t in zip(a, b):                                           # the same draws but for the gate's: hand the state over
        assert set(s) == set(t)
        for key in ("flip", "flip_direction", "gt_bboxes", "_nprnd"):
            s[key] = copy.deepcopy(t[key])
    seen, call = [], _lib.call
    _lib.call = lambda name, *args: seen.append(name) or call(name, *args)
    try:
        got = never.pipeline.run(a, collate=True)
        first = list(seen)
        del seen[:]
        want = without.pipeline.run(b, collate=True)
    finally:
        _lib.call = call
    assert first == seen and "radet_warp_affine_u8" not in first
    assert torch.equal(got["img"], want["img"])
    for key in ("gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight"):
        assert all(torch.equal(x, y) for x, y in zip(got[key], want[key]))
    # and a batch in which one fired adds exactly the warp launches: one on the frames, one per mask group
    fired = _dataset(tree, ROTATE)
    del seen[:]
    _lib.call = lambda name, *args: seen.append(name) or call(name, *args)
    try:
        fired.pipeline.run(_plans(fired, 0), collate=True)
    finally:
        _lib.call = call
    assert seen.count("radet_warp_affine_u8") >= 2 and seen.index("radet_warp_affine_u8") > seen.index("radet_resize_linear_u8")
    assert seen.index("radet_augment_merge_hblur") > len(seen) - 1 - seen[::-1].index("radet_warp_affine_u8")


def test_rotate_config_batch(tree):
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    cfg, train = rotate_train_cfg(tree)
    ds = build_dataset(train)
    for epoch in range(20):                                          # a batch in which one sample fires and one does not
        plans = [ds.plan_sample(i, *sample_generators(0, epoch, i)) for i in range(2)]
        if sum("affine" in s for s in plans) == 1:
            break
    assert sum("affine" in s for s in plans) == 1
    batch = ds.pipeline.run(plans, collate=True)
    assert tuple(batch["img"].shape) == (2, 3, 480, 640) and bool(torch.isfinite(batch["img"]).all())
    assert all(len(b) == len(l) for b, l in zip(batch["gt_bboxes"], batch["gt_labels"]))
