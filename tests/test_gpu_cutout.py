"""CutOut on the GPU: radet_cutout_u8 and radet_cutout_f32 against the NumPy restatement of the reference's stage
(tests/_cutout_ref.py, pinned to the reference's pixels by tests/test_cutout_cpu.py), the entry order of a block that mixes
holes and warps, the pipeline with the stage in both of its places against the staged host restatement built from each
planned sample's recorded draws, launch parity and the cutout config.  Every comparison is array_equal / torch.equal."""
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
import _augment_ref as R  # noqa: E402
import _cutout_ref as C  # noqa: E402
from _jitter_cfg import jitter_train_cfg  # noqa: E402
from _maskfree_pipelines import ASSIGNER, COSY, DM, MIX, NORM  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = C.U8_GUARD
MAX_HOLES, SIZES = C.U8_MAX_HOLES, C.U8_SIZES


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _log_calls(fn):
    """the entry-point names fn() called, and its result"""
    from radet_amd import _lib
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        return seen, fn()
    finally:
        _lib.call = call


# ------------------------------------------------------------------------------------------------ radet_cutout_u8
@pytest.fixture(scope="module")
def u8_batch():
    """the packed batch of tests/_cutout_ref.py (tests/test_cutout_cpu.py shows that it holds the cases), computed once"""
    return C.u8_kernel_cases()


def _u8_tables(K, frames, rows, offs):
    D = np.zeros((len(frames), K.CUTOUT_DESC_INTS), np.int32)
    table, first = [], 0
    for d, f, off, (holes, fill, skip) in zip(D, frames, offs, rows):
        n = 0 if holes is None else len(holes)
        K.cutout_desc_row(d, off, f.shape[0], f.shape[1], fill, first, n, skip=skip)
        if n:
            table.append(holes)
            first += n
    return D, np.concatenate(table).astype(np.int32)


def test_cutout_u8_equals_the_restatement(u8_batch):
    from radet_amd import kernels as K
    frames, rows, offs, packed, want = u8_batch
    dev = _dev()
    D, table = _u8_tables(K, frames, rows, offs)
    most, area = K.cutout_launch_dims([None if skip else h for h, _, skip in rows], SIZES)
    assert most == MAX_HOLES and area >= 57
    desc, holes = torch.from_numpy(D).to(dev), torch.from_numpy(table).to(dev)
    runs = []
    for _ in range(2):
        buf = torch.from_numpy(packed).to(dev)
        seen, _ = _log_calls(lambda: K.cutout_u8(buf, desc, holes, len(frames), most, area))
        assert seen == ["radet_cutout_u8"]
        runs.append(buf.cpu().numpy())
    for f, off, got in zip(frames, offs, [runs[0][o * 3:o * 3 + f.size].reshape(f.shape) for f, o in zip(frames, offs)]):
        np.testing.assert_array_equal(got, want[off * 3:off * 3 + f.size].reshape(f.shape), err_msg=f"image {f.shape}")
    assert np.array_equal(runs[0], want)                                                        # canaries and the skip row included
    assert np.array_equal(runs[0], runs[1])
    # the holes in another order: overlapping holes store identical bytes
    perm = np.random.RandomState(1).permutation(MAX_HOLES)
    first = int(D[5, 4])
    table2 = table.copy()
    table2[first:first + MAX_HOLES] = table[first:first + MAX_HOLES][perm]
    buf = torch.from_numpy(packed).to(dev)
    K.cutout_u8(buf, desc, torch.from_numpy(table2).to(dev), len(frames), most, area)
    assert np.array_equal(buf.cpu().numpy(), want)


def test_cutout_u8_bad_arguments(u8_batch):
    from radet_amd import _lib, kernels as K
    frames, rows, offs, packed, want = u8_batch
    dev = _dev()
    f = frames[4]
    src = torch.from_numpy(np.concatenate([f.reshape(-1), np.full(30, GUARD, np.uint8)])).to(dev)
    buf = src.clone()
    D = np.zeros((3, K.CUTOUT_DESC_INTS), np.int32)
    K.cutout_desc_row(D[0], 0, 48, 64, (1, 2, 3), 0, 1)
    desc = torch.from_numpy(D).to(dev)
    holes = torch.tensor([[3, 3, 40, 30], [0, 0, 64, 48]], dtype=torch.int32, device=dev)
    for args in ((buf, desc, holes, 1, 1, 64 * 48, 2), (buf, desc, holes, 1, 1, 64 * 48, 1), (buf, desc, holes, -1, 1, 64 * 48),
                 (buf, desc, holes, 1, -1, 64 * 48), (buf, desc, holes, 1, 1, -5)):
        with pytest.raises(_lib.RadetHipError):
            K.cutout_u8(*args)
    assert torch.equal(buf, src)
    # rows that leave the buffer (offset 11: the last rows would pass the end; a negative offset; h * w beyond the buffer), a
    # row whose holes leave the table, a row without pixels: nothing is written
    K.cutout_desc_row(D[0], 11, 48, 64, (1, 2, 3), 0, 2)
    K.cutout_desc_row(D[1], -1, 48, 64, (1, 2, 3), 0, 2)
    K.cutout_desc_row(D[2], 0, 480, 640, (1, 2, 3), 0, 2)
    K.cutout_u8(buf, torch.from_numpy(D).to(dev), holes, 3, 2, 64 * 48)
    assert torch.equal(buf, src)
    K.cutout_desc_row(D[0], 0, 48, 64, (1, 2, 3), 1, 2)
    K.cutout_desc_row(D[1], 0, 48, 64, (1, 2, 3), -1, 2)
    K.cutout_desc_row(D[2], 0, 0, 64, (1, 2, 3), 0, 2)
    K.cutout_u8(buf, torch.from_numpy(D).to(dev), holes, 3, 2, 64 * 48)
    assert torch.equal(buf, src)
    # and the same launch with a row that fits writes that row only, inside its image
    K.cutout_desc_row(D[2], 10, 48, 64, (1, 2, 3), 0, 2)
    K.cutout_u8(buf, torch.from_numpy(D).to(dev), holes, 3, 2, 64 * 48)
    got = buf.cpu().numpy()
    assert (got[30:30 + f.size].reshape(48, 64, 3) == np.array((1, 2, 3), np.uint8)).all()
    assert np.array_equal(got[:30], src.cpu().numpy()[:30])


# ------------------------------------------------------------------------------------------------ radet_cutout_f32
F32_HP, F32_WP = 32, 48
# (h, w, flip, to_rgb, holes or None, fill)
F32_ROWS = [
    (20, 30, False, True, [[3, 2, 12, 9], [25, 15, 40, 40]], (10, 20, 30)),
    (32, 48, True, True, [[0, 0, 5, 32], [40, 10, 48, 12]], (255, 0, 128)),
    (17, 31, True, False, [[-4, -4, 3, 3], [10, 5, 20, 6], [30, 16, 31, 17]], (0, 37, 255)),
    (5, 7, False, False, [[0, 0, 7, 5]], (128, 128, 128)),
    (24, 40, True, True, None, (1, 1, 1)),
    (24, 40, False, True, [[5, 5, 30, 20]], (7, 7, 7)),                       # a skip row
]


def _finish(K, L, frames, blends=None):
    """radet_augment_finish on packed u8 frames with the rows' flip / to_rgb flags; blends: extra flags and factor bits per row"""
    dev = _dev()
    B = len(frames)
    P = np.zeros((B, K.AUG_PARAM_INTS), np.int32)
    o = 0
    for i, (f, row) in enumerate(zip(frames, F32_ROWS)):
        P[i, 0], P[i, 1], P[i, 2] = o, f.shape[0], f.shape[1]
        P[i, 3] = (L.F_FLIP if row[2] else 0) | (L.F_TO_RGB if row[3] else 0)
        if blends is not None:
            P[i, 3] |= L.F_BRIGHT | L.F_COLOR
            P[i, 13], P[i, 14] = L._f32_bits(blends[0]), L._f32_bits(blends[1])
        o += f.shape[0] * f.shape[1]
    src = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(dev)
    lsum = torch.zeros(B, dtype=torch.int64, device=dev)
    out = torch.empty(B, 3, F32_HP, F32_WP, dtype=torch.float32, device=dev)
    mean = np.asarray(NORM["mean"], np.float32).astype(np.float64).astype(np.float32)
    stdinv = (1.0 / np.asarray(NORM["std"], np.float32).astype(np.float64)).astype(np.float32)
    K.augment_finish(src, lsum, torch.from_numpy(P).to(dev), out, B, F32_HP, F32_WP, mean, stdinv)
    return out, mean, stdinv


def _f32_tables(K):
    D = np.zeros((len(F32_ROWS), K.CUTOUT_DESC_INTS), np.int32)
    table, first = [], 0
    for i, (d, (h, w, flip, rgb, holes, fill)) in enumerate(zip(D, F32_ROWS)):
        n = 0 if holes is None else len(holes)
        K.cutout_desc_row(d, i, h, w, fill, first, n, skip=i == 5, flip=flip, to_rgb=rgb)
        table += holes or []
        first += n
    most, area = K.cutout_launch_dims([None if i == 5 else r[4] for i, r in enumerate(F32_ROWS)], [r[:2] for r in F32_ROWS])
    return torch.from_numpy(D).to(_dev()), torch.tensor(table, dtype=torch.int32, device=_dev()), most, area


@pytest.fixture(scope="module")
def f32_frames():
    rs = np.random.RandomState(2)
    frames = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w, *_ in F32_ROWS]
    filled = [f if holes is None or i == 5 else C.apply_holes(f, holes, np.array(fill, np.uint8))
              for i, (f, (_, _, _, _, holes, fill)) in enumerate(zip(frames, F32_ROWS))]
    return frames, filled


def test_cutout_f32_equals_finish_of_the_filled_image(f32_frames):
    from radet_amd import kernels as K
    from radet_amd.datasets import loading as L
    frames, filled = f32_frames
    out, mean, stdinv = _finish(K, L, frames)
    before = out.clone()
    desc, table, most, area = _f32_tables(K)
    seen, _ = _log_calls(lambda: K.cutout_f32(out, desc, table, len(frames), most, area, mean, stdinv))
    assert seen == ["radet_cutout_f32"]
    want_dev, _, _ = _finish(K, L, filled)                                                 # the device's finish of the filled frames
    assert torch.equal(out, want_dev)
    got = out.cpu().numpy()
    for i, (f, (h, w, flip, rgb, holes, fill)) in enumerate(zip(filled, F32_ROWS)):         # and tests/_augment_ref.py's
        want = np.zeros((3, F32_HP, F32_WP), np.float32)
        want[:, :h, :w] = R.normalize(f[:, ::-1] if flip else f, NORM["mean"], NORM["std"], rgb)
        np.testing.assert_array_equal(got[i], want, err_msg=f"row {i}")
        assert (got[i, :, h:] == 0).all() and (got[i, :, :, w:] == 0).all()                # Pad's zeros stay
    assert torch.equal(out[4], before[4]) and torch.equal(out[5], before[5])               # no holes; skipped
    assert not torch.equal(out[:4], before[:4])
    again = before.clone()
    K.cutout_f32(again, desc, table, len(frames), most, area, mean, stdinv)
    assert torch.equal(again, out)


def test_cutout_f32_holes_keep_the_fill_through_the_blends(f32_frames):
    from radet_amd import kernels as K
    from radet_amd.datasets import loading as L
    frames, _ = f32_frames
    blended, mean, stdinv = _finish(K, L, frames, blends=(1.7, 0.3))
    plain, _, _ = _finish(K, L, frames)
    out = blended.clone()
    desc, table, most, area = _f32_tables(K)
    K.cutout_f32(out, desc, table, len(frames), most, area, mean, stdinv)
    got, bl, pl = out.cpu().numpy(), blended.cpu().numpy(), plain.cpu().numpy()
    for i, (h, w, flip, rgb, holes, fill) in enumerate(F32_ROWS[:4]):
        inside = C.hole_mask(holes, h, w, flip)
        want = R.normalize(np.array(fill, np.uint8).reshape(1, 1, 3), NORM["mean"], NORM["std"], rgb).reshape(3)
        assert inside.any()
        for c in range(3):
            assert (got[i, c, :h, :w][inside] == want[c]).all(), f"row {i}"
            assert np.array_equal(got[i, c, :h, :w][~inside], bl[i, c, :h, :w][~inside])     # the neighbours carry the blend
        if (~inside).any():
            assert not np.array_equal(bl[i, :, :h, :w][:, ~inside], pl[i, :, :h, :w][:, ~inside])


def test_cutout_f32_bad_arguments(f32_frames):
    from radet_amd import _lib, kernels as K
    dev = _dev()
    out = torch.full((2, 3, 8, 8), 5.0, device=dev)
    want = out.clone()
    D = np.zeros((4, K.CUTOUT_DESC_INTS), np.int32)
    holes = torch.tensor([[0, 0, 8, 8]], dtype=torch.int32, device=dev)
    one = (1.0, 1.0, 1.0)
    K.cutout_desc_row(D[0], 2, 8, 8, (1, 2, 3), 0, 1)                          # an image index outside the batch
    K.cutout_desc_row(D[1], -1, 8, 8, (1, 2, 3), 0, 1)
    K.cutout_desc_row(D[2], 0, 9, 8, (1, 2, 3), 0, 1)                          # an image larger than the planes
    K.cutout_desc_row(D[3], 1, 8, 8, (1, 2, 3), 0, 2)                          # holes outside the table
    K.cutout_f32(out, torch.from_numpy(D).to(dev), holes, 4, 2, 64, one, one)
    assert torch.equal(out, want)
    for args in ((-1, 1, 64), (1, -1, 64), (1, 1, -1)):
        with pytest.raises(_lib.RadetHipError):
            K.cutout_f32(out, torch.from_numpy(D).to(dev), holes, *args, one, one)


# ------------------------------------------------------------------------------------------------ the order of a block's entries
def test_rank_order_of_holes_and_warps():
    """[CutOut, Rotate] and [Rotate, CutOut] on the same frame, and a frame with holes only, in one batch: a warp launch then a
    CutOut launch per rank; a hole cut before the Rotate is turned with the image, one cut after it is axis-aligned"""
    from radet_amd.datasets.loading import CutHoles, ImagePipeline
    dev = _dev()
    frame = np.random.RandomState(3).randint(0, 256, (48, 64, 3)).astype(np.uint8)
    rot, wfill = A.rotation_matrix((31.5, 23.5), -30, 1), (128, 128, 128)
    holes, fill = np.array([[10, 8, 40, 30], [50, 40, 70, 60]], np.int32), (0, 37, 255)
    cut_entry, warp_entry = CutHoles(holes, fill), (rot, wfill)
    ops = [[cut_entry, warp_entry], [warp_entry, cut_entry], [cut_entry], []]
    offs = [k * (48 * 64 + 4) for k in range(4)]
    packed = np.full(offs[-1] * 3 + frame.size + 12, GUARD, np.uint8)
    for o in offs:
        packed[o * 3:o * 3 + frame.size] = frame.reshape(-1)
    seen, out = _log_calls(lambda: ImagePipeline._warp_packed(torch.from_numpy(packed).to(dev), ops, offs, [(48, 64)] * 4, dev))
    assert seen == ["radet_warp_affine_u8", "radet_cutout_u8", "radet_warp_affine_u8", "radet_cutout_u8"]
    got = out.cpu().numpy()
    cut = lambda x: C.apply_holes(x, holes, np.array(fill, np.uint8))           # noqa: E731
    warp = lambda x: A.warp_affine_u8(x, rot, wfill)                            # noqa: E731
    want = [warp(cut(frame)), cut(warp(frame)), cut(frame), frame]
    for o, w in zip(offs, want):
        np.testing.assert_array_equal(got[o * 3:o * 3 + frame.size].reshape(frame.shape), w)
    assert not np.array_equal(want[0], want[1])
    assert (want[1][8:30, 10:40] == np.array(fill, np.uint8)).all() and not (want[0][8:30, 10:40] == np.array(fill, np.uint8)).all()


# ------------------------------------------------------------------------------------------------ the pipeline
SEED = 3
OUT = (48, 64)
ROTATE = dict(type="Rotate", level=10, max_rotate_angle=30, prob=1, img_fill_val=(0., 37., 255.))
TRANSLATE = dict(type="Translate", level=1, prob=0.9, max_translate_offset=120., min_size=3)
CUT = dict(type="CutOut", n_holes=(1, 4), cutout_ratio=[(0.2, 0.2), (0.4, 0.3)], fill_in=(9, 200, 77))
CUT2 = dict(type="CutOut", n_holes=2, cutout_shape=(20, 12), fill_in=(255, 0, 0))
LATE = dict(type="CutOut", n_holes=(0, 3), cutout_shape=[(16, 10), (30, 30)], fill_in=(3, 2, 1))
POLICIES = [[ROTATE, CUT], [CUT2, dict(ROTATE, prob=0.7)], [CUT], [TRANSLATE]]
STAGES = {"Rotate": ROTATE, "Translate": TRANSLATE}
PIPES = {"bare": ((CUT, ROTATE, CUT2), ()), "auto": ((dict(type="AutoAugment", policies=POLICIES),), ()),
         "late": ((), (LATE,)), "both": ((CUT2,), (LATE,))}


def cutout_pipeline(background_dir, block=(), late=(), ann="png", cosy=True, crop=None, pad=None, dm=None, mix=False):
    """the pbr stages at Resize((64, 48)) with `block` directly after it (after RandomCrop) and `late` in front of RandomFlip"""
    return [
        dict(type="LoadImageFromFile"),
        dict(type="LoadAnnotations", with_bbox=True, **(dict(with_bop_mask=True) if ann == "png" else dict(with_mask=True))),
        dict(type="Resize", img_scale=(64, 48), keep_ratio=True),
        *([dict(type="RandomCrop", crop_size=crop, allow_negative_crop=True)] if crop else []),
        *block,
        dict(type="RandomBackground", background_dir=background_dir, prob=0.5),
        *([dict(type="CosyPoseAug", p=0.8, pipelines=COSY)] if cosy and not mix else []),
        *([dict(t, prob=0.0) for t in MIX] if mix else []),
        *late,
        dict(type="RandomFlip", flip_ratio=0.5),
        dm or dict(type="GenerateDistanceMap"),
        ASSIGNER,
        dict(type="Normalize", **NORM),
        dict(type="Pad", size=pad) if pad else dict(type="Pad", size_divisor=16),
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


def _dataset(tree, block=(), late=(), ann="png", **kw):
    from radet_amd.datasets import build_dataset
    cfg = dict(type="BOPDataset", img_prefix=tree["img_prefix"], pipeline=cutout_pipeline(tree["background_dir"], block, late, ann=ann, **kw))
    if ann == "png":
        return build_dataset(dict(cfg, ann_file=tree["ann_file"], seg_prefix=tree["seg_prefix"]))
    return build_dataset(dict(cfg, ann_file=tree["rle"], mask_source="annotation"))


def _plans(ds, epoch=0):
    from radet_amd.datasets.loader import sample_generators
    return [ds.plan_sample(i, *sample_generators(SEED, epoch, i)) for i in range(4)]


def _chain(tree, ds, idx, s, **kw):
    """the staged host restatement of sample idx from the PNG tree (the run-list variants decode the same masks)"""
    from PIL import Image
    from radet_amd.datasets import build_dataset
    png = _PNG.get(id(tree))
    if png is None:
        png = _PNG[id(tree)] = build_dataset(dict(type="BOPDataset", img_prefix=tree["img_prefix"], ann_file=tree["ann_file"],
                                                  seg_prefix=tree["seg_prefix"], pipeline=cutout_pipeline(tree["background_dir"])))
    info, ann = png.data_infos[idx], png.get_ann_info(idx)
    x = np.asarray(Image.open(os.path.join(png.img_prefix, info["filename"])).convert("RGB"))[..., ::-1]
    m = np.stack([np.asarray(Image.open(os.path.join(png.seg_prefix, p))) for p in ann["masks"]])
    stages = {t["type"]: t for t in POLICIES[s["policy"]]} if "policy" in s else STAGES
    return C.host_chain(x, m, ann["bboxes"], ann["labels"], s, OUT, stages, NORM, copy.deepcopy(s["_nprnd"]), **kw)


_PNG = {}


@pytest.fixture(scope="module")
def chains(tree):
    """the staged host restatement of one batch per pipeline, computed once"""
    out = {}
    for name, (block, late) in PIPES.items():
        ds = _dataset(tree, block, late)
        for idx, s in enumerate(_plans(ds)):
            assert isinstance(s["img"], np.ndarray)
            out[(name, idx)] = _chain(tree, ds, idx, s)
    return out


def test_chains_are_not_vacuous(chains):
    per = {name: set().union(*(c["kinds"] for (n, _), c in chains.items() if n == name)) for name in PIPES}
    assert per["bare"] >= {"holes", "after-warp", "warp-after-cutout", "Rotate", "bg", "flip", "cosy"}, per["bare"]
    assert per["auto"] >= {"holes", "fired", "cutout"}, per["auto"]
    assert {frozenset(c["kinds"] & {"cutout", "fired"}) for (n, _), c in chains.items() if n == "auto"} >= {frozenset({"cutout"}), frozenset({"cutout", "fired"})}
    assert per["late"] >= {"late-holes", "cosy", "flip", "bg"} and "cutout" not in per["late"], per["late"]
    assert per["both"] >= {"late-holes", "holes"}, per["both"]
    assert any(c["kinds"] >= {"late-holes", "flip"} for c in chains.values()) and any(c["kinds"] >= {"late-holes", "cosy"} for c in chains.values())


def _assert_batch(batch, refs, what):
    img = batch["img"].cpu().numpy()
    for j, ref in enumerate(refs):
        msg = f"{what} sample {j}: {sorted(ref['kinds'])}"
        np.testing.assert_array_equal(img[j], ref["img"], err_msg=msg)
        np.testing.assert_array_equal(batch["gt_bboxes"][j].numpy(), ref["gt_bboxes"], err_msg=msg)
        np.testing.assert_array_equal(batch["gt_labels"][j].numpy(), ref["gt_labels"], err_msg=msg)
        np.testing.assert_array_equal(batch["points_to_gt_index"][j].cpu().numpy(), ref["p2g"], err_msg=msg)
        np.testing.assert_array_equal(batch["points_weight"][j].cpu().numpy(), ref["pw"], err_msg=msg)


@pytest.mark.parametrize("variant", ["host", "runs"])
@pytest.mark.parametrize("name", list(PIPES))
def test_pipeline_equals_the_staged_host_restatement(tree, chains, name, variant):
    """the whole batch: the frames, and -- through the assigner's outputs -- the masks, which follow the warps alone"""
    block, late = PIPES[name]
    ds = _dataset(tree, block, late, ann="rle" if variant == "runs" else "png")
    batch = ds.pipeline.run(_plans(ds), collate=True)
    assert tuple(batch["img"].shape) == (4, 3, *OUT)
    _assert_batch(batch, [chains[(name, j)] for j in range(4)], f"{name} / {variant}")


@pytest.mark.parametrize("variant", ["mix", "pad", "crop", "crop-runs"])
def test_mix_fixed_pad_and_crop_pipelines_take_cutout(tree, variant):
    """block and late CutOut with the mixpbr packing (images at multiples of 4 pixels), Pad(size=) and RandomCrop windows (a
    CutOut-only block is pointwise), each against the staged host restatement of its own planned draws"""
    kw, ckw = dict(mix=dict(mix=True), pad=dict(pad=(64, 80)), crop=dict(crop=(40, 56)))[variant.split("-")[0]], {}
    ds = _dataset(tree, (CUT, CUT2), (LATE,), ann="rle" if variant.endswith("runs") else "png", **kw)
    assert ds.pipeline.mix == (variant == "mix")
    plans = _plans(ds)
    refs = []
    for idx, s in enumerate(plans):
        if variant == "pad":
            ckw = dict(pad_hw=(64, 80))
        if variant.startswith("crop"):
            ckw = dict(window=s["crop_window"])
        refs.append(_chain(tree, ds, idx, s, **ckw))
    kinds = set().union(*(r["kinds"] for r in refs))
    assert kinds >= {"holes", "late-holes", "flip", "bg"} and (not variant.startswith("crop") or "window" in kinds), kinds
    seen, batch = _log_calls(lambda: ds.pipeline.run(plans, collate=True))
    assert seen.count("radet_cutout_u8") == 2 and seen.count("radet_cutout_f32") == 1 and "radet_warp_affine_u8" not in seen
    assert tuple(batch["img"].shape) == (4, 3, *dict(mix=OUT, pad=(64, 80), crop=(48, 64))[variant.split("-")[0]])
    _assert_batch(batch, refs, variant)


def test_mask_free_sampler_sees_block_cutout(tree):
    """block-position CutOut with the mask-free sampler against the host: the u8 frame of the staged restatement (resize, the
    block's holes and warp in order, background, CosyPoseAug, flip), GenerateDistanceMap.__call__ on it with `random` at the
    sample's stream position, the oracle assigner on the sample's RandomState (as tests/test_gpu_maskfree.py: host_sample).
    The crops must hold the holes: the same chain without the CutOut entries gives other maps."""
    import random
    from oracle import assigner as oa
    from radet_amd.datasets import PIPELINES
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.utils import build_from_cfg
    block = (CUT, ROTATE, CUT2)
    small = dict(DM["mbd"], small_object_size=4 ** 2)             # (at 48 x 64 no box reaches the default of 32 x 32 pixels)
    free = _dataset(tree, block, dm=small)
    masked = _dataset(tree, block)                               # (its GenerateDistanceMap draws nothing: `random` stops in front of it)
    assert free.pipeline.mask_free is not None
    plans = _plans(free)
    assert all(s["block_ops"] == [("cutout", 0), ("warp", 0), ("cutout", 1)] for s in plans)
    gdm = build_from_cfg(small, PIPELINES)
    assert sum(int(s["_crop_plan"][0].large.sum()) for s in plans) >= 8          # boxes whose crops are transformed
    refs, differ, cosy = [], 0, 0
    for idx, s in enumerate(plans):
        rnd, nprnd = sample_generators(SEED, 0, idx)
        masked.plan_sample(idx, rnd, nprnd)
        ref = _chain(tree, free, idx, s)
        maps = []
        for frame in (ref["u8"], _chain(tree, free, idx, {k: v for k, v in s.items() if k not in ("block_ops", "cutout")})["u8"]):
            random.setstate(rnd.getstate())
            res = gdm(dict(img=frame, img_shape=(*OUT, 3), gt_bboxes=ref["gt_bboxes"]))
            maps.append(res["distance_maps"].cpu().numpy())
        differ += not np.array_equal(maps[0], maps[1])
        cosy += "cosy" in ref["kinds"]
        ref["p2g"], ref["pw"] = oa.assign_points(ref["gt_bboxes"], ref["gt_labels"], maps[0], (*OUT, 3), rng=copy.deepcopy(s["_nprnd"]))
        refs.append(ref)
    assert differ >= 2 and cosy and any("flip" in r["kinds"] for r in refs) and any("bg" in r["kinds"] for r in refs)
    assert all((r["p2g"] > 0).any() and (r["pw"] > 0).any() for r in refs)      # every sample assigns points to its boxes
    _assert_batch(free.pipeline.run(plans, collate=True), refs, "mask-free")


def test_masks_follow_the_warps_alone(tree):
    """the masks of samples whose block holds holes before and after the Rotate equal the resized masks under the warp alone"""
    from oracle import masks as om
    ds = _dataset(tree, (CUT, ROTATE, CUT2))
    plans = _plans(ds)
    assert all(s["block_ops"] == [("cutout", 0), ("warp", 0), ("cutout", 1)] and len(s["affine"]) == 1 for s in plans)
    masks, flipped = ds.pipeline._affine_masks(plans, [OUT] * 4, _dev(), [OUT] * 4)
    kept = 0
    for s, m, fl in zip(plans, masks, flipped):
        want = A.warp_masks(om.resize_nearest(om.normalize(s["gt_masks"]), OUT), s["affine"][0][0])
        np.testing.assert_array_equal(m.cpu().numpy(), want)
        np.testing.assert_array_equal(fl.cpu().numpy(), om.flip(want) if s["flip"] else want)
        kept += int(want.any())
    assert kept


HANDED = ("flip", "flip_direction", "gt_bboxes", "gt_labels", "gt_masks", "affine", "affine_draws", "_nprnd")


def test_launch_parity_when_no_hole_is_drawn(tree):
    """a batch in which no CutOut drew a hole: the launches and the output of the pipeline built without the stages, under the
    same seeds (a stage with n_holes=0 draws once from the NumPy generator, so the later draws are set equal by hand)"""
    never = _dataset(tree, (dict(CUT, n_holes=0), ROTATE), (dict(LATE, n_holes=0),))
    without = _dataset(tree, (ROTATE,))
    a, b = _plans(never), _plans(without)
    assert not any(key in s for s in a for key in ("block_ops", "cutout", "cutout_late")) and all("affine" in s for s in a)
    keep = [{key: copy.deepcopy(t[key]) for key in HANDED} for t in b]         # (before a run advances the RandomStates)
    for s, t, k in zip(a, b, keep):
        assert set(s) == set(t)
        s.update(copy.deepcopy(k))
    first, got = _log_calls(lambda: never.pipeline.run(a, collate=True))
    second, want = _log_calls(lambda: without.pipeline.run(b, collate=True))
    assert first == second and not any("cutout" in n for n in first) and "radet_warp_affine_u8" in first
    assert torch.equal(got["img"], want["img"])
    for key in ("gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight"):
        assert all(torch.equal(x, y) for x, y in zip(got[key], want[key]))
    # a policy that drew no CutOut: the launches of the warp-only batch again
    auto = _dataset(tree, (dict(type="AutoAugment", policies=[[ROTATE], [ROTATE, dict(CUT, n_holes=0)]]),))
    c = _plans(auto)
    assert not any(key in s for s in c for key in ("block_ops", "cutout")) and {s["policy"] for s in c} == {0, 1}
    for s, k in zip(c, keep):
        s.update(copy.deepcopy(k))
    third, got = _log_calls(lambda: auto.pipeline.run(c, collate=True))
    assert third == second
    assert torch.equal(got["img"], want["img"])
    for key in ("gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight"):
        assert all(torch.equal(x, y) for x, y in zip(got[key], want[key]))
    # and holes add exactly their launches: one per entry rank on the frames, none on the masks, one on the finished batch
    fired = _dataset(tree, (CUT, ROTATE), (dict(LATE, n_holes=2),))
    d = _plans(fired)
    assert all(s["block_ops"] == [("cutout", 0), ("warp", 0)] and len(s["cutout_late"][0]) == 2 for s in d)
    for s, k in zip(d, keep):
        s.update(copy.deepcopy(k))
    fourth, _ = _log_calls(lambda: fired.pipeline.run(d, collate=True))
    assert [n for n in fourth if "cutout" not in n] == second
    assert fourth.count("radet_cutout_u8") == 1 and fourth.count("radet_cutout_f32") == 1
    assert fourth.index("radet_cutout_u8") < fourth.index("radet_augment_merge_hblur")
    assert fourth.index("radet_cutout_f32") == fourth.index("radet_augment_finish") + 1


def test_cutout_config_batch_feeds_a_train_step(tree):
    from oracle import synth
    from radet_amd.apis import train_detector
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.models import build_detector
    cfg, train = jitter_train_cfg(tree, name="r50_ycbv_pbr_cutout.py")
    ds = build_dataset(train)
    for epoch in range(30):                                          # a batch with a hole before a warp and a warp-free sample
        plans = [ds.plan_sample(i, *sample_generators(0, epoch, i)) for i in range(2)]
        orders = {"".join(k[0] for k, _ in s.get("block_ops", ())) for s in plans}
        if "wc" in orders and len(orders) > 1:
            break
    assert "wc" in orders and len(orders) > 1
    batch = ds.pipeline.run(plans, collate=True)
    assert tuple(batch["img"].shape) == (2, 3, 480, 640) and bool(torch.isfinite(batch["img"]).all())
    assert all(len(b) == len(l) for b, l in zip(batch["gt_bboxes"], batch["gt_labels"]))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    synth.fill_state_dict(det.state_dict(), seed=0)
    det = det.cuda()
    cfg.merge_from_dict({"lr_config.total_steps": 40, "log_config.interval": 1})
    hist = train_detector(det, iter([batch]), cfg, max_iters=1, log=lambda *_: None)
    assert len(hist) == 1 and np.isfinite(hist[0]).all()
