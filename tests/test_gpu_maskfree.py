"""The mask-free sampler inside the image pipeline on the GPU: radet_crop_canvases against GenerateDistanceMap.crop_boxes,
radet_paste_maps against the zeros + slice-copy loop, and ImagePipeline.run with GenerateDistanceMap(with_gt_mask=False)
against the host chain (tests/_augment_ref.py / _mixaug_ref.py image, GenerateDistanceMap.__call__ on it, oracle assigner)
fed the same per-sample generators.  Every comparison is array_equal.  cv2 itself stays unpinned, as everywhere in this
path: the resize / blur / Sobel arithmetic is pinned by oracle/imgproc.py (tests/test_gpu_distance.py)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _augment_ref as R  # noqa: E402
import _mixaug_ref as M  # noqa: E402
from oracle import masks as om  # noqa: E402
from _maskfree_pipelines import DM, boxes_on_borders as _boxes, train_pipeline  # noqa: E402

pytestmark = pytest.mark.gpu

F_CONTRAST, F_BRIGHT, F_COLOR, F_FLIP = 8, 16, 32, 64


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("flip", [False, True])
def test_crop_canvases_equals_crop_boxes(flip):
    """two packed images of different sizes, boxes on every border and in every corner (canvases partly outside on two
    sides); the first image with identity photometric stages, the second with contrast / brightness / color blends (its
    own luma sum in lsum, another number in the first image's slot): the kernel's canvases == crop_boxes on the blended,
    (flipped) u8 image"""
    import struct
    from radet_amd import kernels as K
    from radet_amd.datasets.pipelines import GenerateDistanceMap, crop_geometry
    rs = np.random.RandomState(3)
    shapes = [(240, 320), (131, 203)]
    images = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    gdm = GenerateDistanceMap(with_gt_mask=False, distance_transform="mbd", pad_ratio=0.1)
    P = np.zeros((2, K.AUG_PARAM_INTS), np.int32)
    rows, expected, o, off = [], [], 0, 0
    blends = dict(contr=0.6, bright=1.7, col=2.5)
    lsums = [12345, int(R.luma(images[1][..., ::-1]).astype(np.int64).sum())]
    for i, (img, (h, w)) in enumerate(zip(images, shapes)):
        P[i, :4] = [off, h, w, (F_FLIP if flip else 0) | (F_CONTRAST | F_BRIGHT | F_COLOR if i == 1 else 0)]
        if i == 1:
            P[i, 12:15] = [struct.unpack("<i", struct.pack("<f", v))[0] for v in blends.values()]
            img = R.cosypose(img[..., ::-1], **blends)[..., ::-1]
        off += h * w
        boxes = _boxes(rs, h, w, 6)
        seen = img[:, ::-1] if flip else img
        random.seed(5 + i)
        canvases, _, _ = gdm.crop_boxes(np.ascontiguousarray(seen), (h, w), boxes)
        g = crop_geometry(boxes, (h, w), gdm.pad_ratio, gdm.small_object_size)
        random.seed(5 + i)
        fill = [[random.randint(0, 255) for _ in range(3)] for _ in boxes]
        for k, c in enumerate(canvases):
            ch, cw = c.shape[:2]
            assert (cw, ch) == tuple(g.canvas_wh[k])
            if ch == 0 or cw == 0:
                continue
            b = fill[k]
            rows.append([i, *g.win_lo[k], cw, ch, *g.src_lo[k], *g.src_hi[k], b[0] | b[1] << 8 | b[2] << 16, o, 0])
            expected.append((o, c))
            o += ch * cw
    assert any(r[1] < 0 and r[2] < 0 for r in rows) and any(r[1] + r[3] > shapes[r[0]][1] for r in rows)
    dev = _dev()
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(dev)
    dst = torch.full((o * 3 + 9,), 77, dtype=torch.uint8, device=dev)
    desc = torch.tensor(rows, dtype=torch.int32, device=dev)
    assert desc.shape[1] == K.CROP_DESC_INTS
    lsum = torch.tensor(lsums, dtype=torch.int64, device=dev)
    K.crop_canvases(src, lsum, torch.from_numpy(P).to(dev), 2, desc, len(rows), max(c.shape[0] * c.shape[1] for _, c in expected),
                    dst[:o * 3])
    got = dst.cpu().numpy()
    assert (got[o * 3:] == 77).all()
    for n, (po, c) in enumerate(expected):
        np.testing.assert_array_equal(got[po * 3:po * 3 + c.size].reshape(c.shape), c, err_msg=f"canvas {n}: {rows[n]}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("H,W", [(96, 128), (61, 83)])
def test_paste_maps_equals_slice_copies(dtype, H, W):
    from radet_amd import kernels as K
    from radet_amd.datasets.pipelines import crop_geometry
    rs = np.random.RandomState(W)
    boxes = _boxes(rs, H, W, 5)
    g = crop_geometry(boxes, (H, W), 0.05, 32 ** 2)
    enabled = g.large.copy()
    enabled[0] = False                                                  # one box disabled whatever its size
    assert enabled.any() and not enabled.all()
    maps, rows, o = [], [], 0
    ref = np.zeros((len(boxes), H, W), np.float32)
    for k, (cw, ch) in enumerate(g.canvas_wh):
        x0, y0, x1, y1 = g.corners[k]
        r = g.regions[k]
        if enabled[k]:
            m = (rs.rand(ch, cw) * 3).astype(dtype)
            maps.append(m.reshape(-1))
            rows.append([o, ch, cw, r[0], r[1], x0, y0, x1, y1, 1])
            o += ch * cw
        else:
            m = np.ones((ch, cw), np.uint8)
            rows.append([0, 0, 0, r[0], r[1], x0, y0, x1, y1, 0])
        ref[k, y0:y1, x0:x1] = m[r[1]:r[3], r[0]:r[2]]                  # (loading.py:641-643, .astype(float32) for f64)
    dev = _dev()
    packed = torch.from_numpy(np.concatenate(maps)).to(dev)
    desc = torch.tensor(rows, dtype=torch.int32, device=dev)
    assert desc.shape[1] == K.PASTE_DESC_INTS
    out = torch.full((len(boxes), H, W), 7.0, dtype=torch.float32, device=dev)
    K.paste_maps(packed, desc, len(boxes), H, W, out)
    np.testing.assert_array_equal(out.cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------ end to end
SEED = 5


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL decodes the generated JPEG / PNG files")
    from tools.synth_bop import write_tree
    # six frames of two sizes; frame 3 holds small objects only, frame 4 none
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=6, objects=(3, 6), n_backgrounds=3, seed=17,
                      sizes=[(640, 480), (600, 480)], small_frames=(3,), empty_frames=(4,))


def _dataset(tree, dm, mix):
    from radet_amd.datasets import build_dataset
    return build_dataset(dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"],
                              seg_prefix=tree["seg_prefix"], filter_empty_gt=False,
                              pipeline=train_pipeline(tree["background_dir"], dm, mix=mix, bg_prob=0.5)))


def host_sample(ds, idx, mix, gdm, background_dir):
    """the reference's train pipeline for sample idx on fresh per-sample generators, restated on the host up to the u8
    BGR image GenerateDistanceMap reads; then GenerateDistanceMap.__call__ with `random` at the sample's stream position
    and the oracle assigner on the sample's RandomState.  Returns the results and both generators."""
    from PIL import Image
    from oracle import assigner as oa
    from radet_amd.datasets.loader import sample_generators
    rnd, nprnd = sample_generators(SEED, 0, idx)
    info, ann = ds.data_infos[idx], ds.get_ann_info(idx)
    img = np.asarray(Image.open(os.path.join(ds.img_prefix, info["filename"])).convert("RGB"))[..., ::-1]
    h0, w0 = img.shape[:2]
    masks = (np.stack([np.asarray(Image.open(os.path.join(ds.seg_prefix, p))) for p in ann["masks"]]) if ann["masks"]
             else np.zeros((0, h0, w0), np.uint8))
    f = min(640 / max(h0, w0), 480 / min(h0, w0))
    w, h = int(w0 * f + 0.5), int(h0 * f + 0.5)
    sf = np.array([w / w0, h / h0, w / w0, h / h0], np.float32)
    boxes = ann["bboxes"] * sf
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, w)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, h)
    x = R.resize_linear_u8(img, w, h)
    m = om.transform(masks, resized_hw=(h, w), norm=True) if len(masks) else np.zeros((0, h, w), np.uint8)
    if not rnd.random() > 0.5:
        bgs = sorted(os.path.join(background_dir, n) for n in os.listdir(background_dir))
        bg = np.asarray(Image.open(rnd.choice(bgs)).convert("RGB"))[..., ::-1]
        x = R.merge_background(x, R.resize_linear_u8(bg, w, h), m)
    if mix:
        rnd.random()
        x = M.random_hsv(x, *tuple(rnd.uniform(-1, 1) * r + 1 for r in (0.2, 0.5, 0.5)))
        rnd.random()
        sigma = rnd.uniform(0, 0.1)
        x = np.clip(M.noise_sum(x, sigma, nprnd.randint(0, 2 ** 64, size=2, dtype=np.uint64)), 0, 255).astype(np.uint8)
        rnd.random()
        x = M.box_filter(x, rnd.choice([1, 3, 5, 7]))
    else:
        aug = {}
        if not rnd.random() > 0.8:
            aug["blur_k"] = rnd.randint(1, 3)
            for key, (p, iv) in zip(("sharp", "contr", "bright", "col"),
                                    ((0.3, (0., 50.)), (0.3, (0.2, 50.)), (0.5, (0.1, 6.0)), (0.3, (0., 20.)))):
                if rnd.random() <= p:
                    aug[key] = rnd.uniform(*iv)
        x = R.cosypose(x[..., ::-1], **aug)[..., ::-1]
    flip = nprnd.choice(["horizontal", None], p=[0.5, 0.5]) is not None
    if flip:
        boxes = np.stack([w - boxes[:, 2], boxes[:, 1], w - boxes[:, 0], boxes[:, 3]], axis=1)
        x = x[:, ::-1]
    random.setstate(rnd.getstate())                       # GenerateDistanceMap draws from the global `random`
    res = gdm(dict(img=np.ascontiguousarray(x), img_shape=(h, w, 3), gt_bboxes=boxes))
    rnd.setstate(random.getstate())
    maps = res["distance_maps"].cpu().numpy()
    p2g, pw = oa.assign_points(boxes, ann["labels"], maps, (h, w, 3), rng=nprnd)
    return dict(p2g=p2g, pw=pw, boxes=boxes, flip=flip, hw=(h, w), maps=maps), rnd, nprnd


@pytest.mark.parametrize("mix", [False, True], ids=["pbr", "mix"])
@pytest.mark.parametrize("dm", ["gdt", "mbd"])
def test_mask_free_pipeline_equals_host_chain(tree, dm, mix):
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.utils import build_from_cfg
    from radet_amd.datasets import PIPELINES
    ds = _dataset(tree, dm, mix)
    pipe = ds.pipeline
    B = len(ds)
    assert B == 6
    gens = [sample_generators(SEED, 0, i) for i in range(B)]
    planned = [ds.plan_sample(i, *gens[i]) for i in range(B)]

    # the mask-free part of run() may not wait for the device: it runs with synchronising calls made an error
    inner, calls = pipe._distance_maps, []

    def no_sync(*a, **k):
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = inner(*a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        calls.append(sum(len(m) for m in out))
        return out
    pipe._distance_maps = no_sync
    try:
        out = pipe.run(planned)
    finally:
        del pipe._distance_maps
    assert len(calls) == 1 and calls[0] == sum(len(s["gt_bboxes"]) for s in planned)

    gdm = build_from_cfg(DM[dm], PIPELINES)
    flips, sizes, counts, positives, blended = set(), set(), [], [], []
    for i in range(B):
        ref, rnd, nprnd = host_sample(ds, i, mix, gdm, tree["background_dir"])
        np.testing.assert_array_equal(out[i]["gt_bboxes"].numpy(), ref["boxes"])
        np.testing.assert_array_equal(out[i]["points_to_gt_index"].cpu().numpy(), ref["p2g"], err_msg=f"sample {i}")
        np.testing.assert_array_equal(out[i]["points_weight"].cpu().numpy(), ref["pw"], err_msg=f"sample {i}")
        assert gens[i][0].getstate() == rnd.getstate(), f"sample {i}: random.Random position"
        for a, b in zip(gens[i][1].get_state(), nprnd.get_state()):
            assert np.array_equal(a, b), f"sample {i}: RandomState position"
        flips.add(ref["flip"])
        sizes.add(ref["hw"])
        counts.append((len(ref["boxes"]), int(planned[i]["_crop_plan"][0].large.sum())))
        blended.append(i > 0 and counts[-1][1] > 0 and any(k in planned[i] for k in ("aug_contrast", "aug_brightness", "aug_color")))
        positives.append(int((ref["p2g"] > 0).sum()))
    assert flips == {True, False} and len(sizes) == 2
    assert (0, 0) in counts and any(g > 0 and big == 0 for g, big in counts)        # no boxes; small boxes only
    assert max(positives) > 10
    assert mix or any(blended)          # pbr: a sample past the first whose crops go through the contrast / brightness / color blends

    # the image is what the mask pipeline makes of the same plan
    masked = _dataset(tree, "mask", mix)
    again = masked.pipeline.run([masked.plan_sample(i, *sample_generators(SEED, 0, i)) for i in range(B)])
    for i in range(B):
        assert torch.equal(out[i]["img"], again[i]["img"]), f"sample {i}"


def test_mask_pipeline_launches_nothing_new(tree):
    """with_gt_mask=True: the crop / paste entry points are never called"""
    from radet_amd import _lib
    from radet_amd.datasets.loader import sample_generators
    ds = _dataset(tree, "mask", False)
    seen, call = [], _lib.call

    def spy(name, *a):
        seen.append(name)
        return call(name, *a)
    _lib.call = spy
    try:
        ds.pipeline.run([ds.plan_sample(i, *sample_generators(SEED, 0, i)) for i in range(2)])
    finally:
        _lib.call = call
    assert "radet_augment_finish" in seen and not {"radet_crop_canvases", "radet_paste_maps", "radet_mbd", "radet_gdt"} & set(seen)
