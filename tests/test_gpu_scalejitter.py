"""Scale-jitter training on the GPU: output windows (view rows) of the resize and of both mask kernels against "full transform,
then slice" (the same kernels without rows and oracle/masks.py), the loader on Resize(ratio_range) + RandomCrop + Pad(size) against a host
restatement of the reference's order fed the same per-sample seeds, the launch log, and a training run on the jitter
config.  Every comparison is array_equal / torch.equal."""
import json
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
from oracle import masks as om  # noqa: E402
from _maskfree_pipelines import ASSIGNER, COSY, DM, NORM  # noqa: E402
from _rle_cases import edge_masks  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0xAB


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def windows(Hr, Wr):
    """(y0, x0, h, w) inside an Hr x Wr image: at the origin, odd origins, ending exactly at the last row and column,
    1 x 1, one row, one column, the full size, fewer pixels than a workgroup's 256 threads, and no multiple of 256"""
    out = [(0, 0, max(Hr // 2, 1), max(Wr // 2, 1)), (0, 0, Hr, Wr), (Hr - 1, Wr - 1, 1, 1), (0, 0, 1, 1),
           (Hr // 2, 0, 1, Wr), (0, Wr // 2, Hr, 1), (Hr - max(Hr // 3, 1), Wr - max(Wr // 3, 1), max(Hr // 3, 1), max(Wr // 3, 1))]
    if Hr > 4 and Wr > 8:
        out += [(1, 3, Hr - 2, Wr - 5), (3, 1, 3, 5), (Hr // 2 - 1 | 1, Wr // 2 - 1 | 1, Hr - (Hr // 2 - 1 | 1), Wr - (Wr // 2 - 1 | 1))]
    for y0, x0, h, w in out:
        assert 0 <= y0 and 0 <= x0 and h > 0 and w > 0 and y0 + h <= Hr and x0 + w <= Wr
    return out


# ------------------------------------------------------------------------------------------------ the resize window
@pytest.fixture(scope="module")
def sources():
    rs = np.random.RandomState(0)
    return [rs.randint(0, 256, (37, 53, 3)).astype(np.uint8), rs.randint(0, 256, (5, 7, 3)).astype(np.uint8)]


# (source, virtual resized size): an upscale by 1.7, a non-integer downscale, the identity
VIRTUAL = [(0, (63, 90)), (0, (23, 31)), (0, (37, 53)), (1, (9, 12)), (1, (3, 4))]


def _plain_resize(K, src, hw):
    dev = _dev()
    h, w = hw
    dst = torch.empty(h * w * 3, dtype=torch.uint8, device=dev)
    desc = torch.tensor([[0, src.shape[0], src.shape[1]], [0, h, w]], dtype=torch.int32, device=dev)
    K.resize_linear_u8(torch.from_numpy(src.reshape(-1)).to(dev), desc[:1], dst, desc[1:], 1, h * w, 3)
    return dst.cpu().numpy().reshape(h, w, 3)


def view_rows(src_hw, cases):
    """the view rows of (Hr, Wr, y0, x0, h, w[, flip]) cases: the whole src_hw source resized to Hr x Wr, the h x w window at
    (y0, x0) of that"""
    return np.array([(Hr, Wr, 0, 0, *src_hw, y0, x0, h, w, *(fl or [0]), 0) for Hr, Wr, y0, x0, h, w, *fl in cases], np.int32)


def _window_resize(K, srcs, rows, align, guard=64):
    """one launch: rows = (source index, Hr, Wr, y0, x0, h, w); returns the per-row outputs and checks the guard bytes"""
    dev = _dev()
    soff = np.cumsum([0] + [s.shape[0] * s.shape[1] for s in srcs])
    sdesc = [(soff[k], srcs[k].shape[0], srcs[k].shape[1]) for k, *_ in rows]
    wdesc, o = [], guard
    for k, Hr, Wr, y0, x0, h, w in rows:
        wdesc.append((o, h, w, Hr, Wr, y0, x0))
        o += -(-h * w // align) * align
    total = o + guard
    dst = torch.full((total * 3,), GUARD, dtype=torch.uint8, device=dev)
    views = np.concatenate([view_rows(srcs[k].shape[:2], [case]) for k, *case in rows])
    K.resize_linear_u8(torch.from_numpy(np.concatenate([s.reshape(-1) for s in srcs])).to(dev),
                       torch.tensor(np.array(sdesc), dtype=torch.int32, device=dev), dst,
                       torch.tensor(np.array([d[:3] for d in wdesc]), dtype=torch.int32, device=dev), len(rows),
                       max(r[5] * r[6] for r in rows), 3, views=torch.from_numpy(views).to(dev))
    host = dst.cpu().numpy()
    written = np.zeros(total * 3, bool)
    outs = []
    for (off, h, w, *_), row in zip(wdesc, rows):
        assert off % align == 0
        outs.append(host[off * 3:(off + h * w) * 3].reshape(h, w, 3))
        written[off * 3:(off + h * w) * 3] = True
    assert (host[~written] == GUARD).all(), "bytes outside the windows were written"
    return outs


def test_resize_window_equals_full_resize_sliced(sources):
    from radet_amd import kernels as K
    full = {(k, hw): _plain_resize(K, sources[k], hw) for k, hw in VIRTUAL}
    for (k, hw), img in full.items():                       # the plain kernel itself is the oracle's resize
        np.testing.assert_array_equal(img, R.resize_linear_u8(sources[k], hw[1], hw[0]))
    small = multiple = False
    for k, (Hr, Wr) in VIRTUAL:
        rows = [(k, Hr, Wr, *win) for win in windows(Hr, Wr)]
        for row, out in zip(rows, _window_resize(K, sources, rows, align=1)):
            _, _, _, y0, x0, h, w = row
            np.testing.assert_array_equal(out, full[(k, (Hr, Wr))][y0:y0 + h, x0:x0 + w], err_msg=str(row))
            small |= h * w < 256
            multiple |= h * w > 256 and h * w % 256 != 0
    assert small and multiple
    # one batch of mixed sources, scales and window sizes, every window at a multiple of 4 pixels (a mix pipeline's packing)
    rows = [(k, Hr, Wr, *win) for k, (Hr, Wr) in VIRTUAL for win in windows(Hr, Wr)[::2]]
    assert len({r[5] * r[6] % 4 for r in rows}) > 1
    for row, out in zip(rows, _window_resize(K, sources, rows, align=4)):
        k, Hr, Wr, y0, x0, h, w = row
        np.testing.assert_array_equal(out, full[(k, (Hr, Wr))][y0:y0 + h, x0:x0 + w], err_msg=str(row))
    # the full-size window is the plain kernel's output
    for k, (Hr, Wr) in VIRTUAL:
        np.testing.assert_array_equal(_window_resize(K, sources, [(k, Hr, Wr, 0, 0, Hr, Wr)], 1)[0], full[(k, (Hr, Wr))])


def test_resize_window_outside_its_image_is_not_written(sources):
    """a row whose window leaves its virtual image writes nothing (and the other rows of the launch are unaffected)"""
    from radet_amd import kernels as K
    rows = [(0, 63, 90, 0, 0, 8, 8), (0, 63, 90, 60, 0, 8, 8), (0, 63, 90, 0, 85, 8, 8), (0, 63, 90, -1, 0, 8, 8), (0, 63, 90, 2, 2, 8, 8)]
    outs = _window_resize(K, sources, rows, 1)
    full = _plain_resize(K, sources[0], (63, 90))
    np.testing.assert_array_equal(outs[0], full[:8, :8])
    np.testing.assert_array_equal(outs[4], full[2:10, 2:10])
    for out in outs[1:4]:
        assert (out == GUARD).all()


# ------------------------------------------------------------------------------------------------ the mask windows
MH, MW = 23, 31
MASK_VIRTUAL = [(39, 53), (14, 19), (23, 31)]                # x1.7, a non-integer downscale, the identity


@pytest.fixture(scope="module")
def bitmaps():
    """G = 3: all zero, maximum 255, maximum 1"""
    e = edge_masks(MH, MW)
    m = np.stack([e["zeros"], e["random"] * 255, e["span"]]).astype(np.uint8)
    m[1, 3, 4] = 7                                            # (a value below the maximum normalises to 0)
    m.setflags(write=False)
    return m


def _mask_cases():
    """(Hr, Wr, y0, x0, h, w, flip) for every virtual size, window and both orientations"""
    return [(Hr, Wr, *win, fl) for Hr, Wr in MASK_VIRTUAL for win in windows(Hr, Wr) for fl in (0, 1)]


def _want(full, case, out_hw, pad_val=0):
    """transform-then-slice: the window of the full resized stack, flipped inside the window, padded"""
    Hr, Wr, y0, x0, h, w, fl = case
    m = full[:, y0:y0 + h, x0:x0 + w]
    m = om.flip(m) if fl else m
    return om.pad(m, out_hw, pad_val)


def test_mask_transform_window_equals_transform_then_slice(bitmaps):
    from radet_amd import kernels as K
    dev = _dev()
    cases = _mask_cases()
    G = len(bitmaps)
    src = torch.from_numpy(bitmaps.copy()).to(dev)
    host = {hw: om.transform(bitmaps, resized_hw=hw, norm=True) for hw in MASK_VIRTUAL}
    for hw, m in host.items():                               # the plain kernel agrees with the oracle on the full masks
        assert np.array_equal(K.mask_transform(src, resized_hw=hw, normalize=True).cpu().numpy(), m)
    assert host[(39, 53)][0].max() == 0 and host[(39, 53)][1].max() == 1 and host[(39, 53)][2].max() == 1
    # one launch over all cases: every mask of the stack carries its own window; the output is padded to one size
    out_hw = (max(c[4] for c in cases) + 3, max(c[5] for c in cases) + 2)
    rows = torch.tensor(np.repeat(view_rows((MH, MW), cases), G, axis=0), device=dev)
    got = K.mask_transform(src.repeat(len(cases), 1, 1), out_hw, views=rows, pad_val=9, normalize=True).cpu().numpy()
    for n, case in enumerate(cases):
        np.testing.assert_array_equal(got[n * G:(n + 1) * G], _want(host[case[:2]], case, out_hw, 9), err_msg=str(case))
    # unpadded, without normalisation (the flip pass over windows that are already cut)
    case = (39, 53, 5, 7, 20, 33, 1)
    got = K.mask_transform(src, (20, 33), views=torch.from_numpy(view_rows((MH, MW), [case] * G)).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got, _want(om.transform(bitmaps, resized_hw=(39, 53)), case, (20, 33)))
    # a window that leaves its virtual mask, or the destination: pad_val only
    bad = [(39, 53, 30, 0, 20, 33, 0), (39, 53, 0, 0, 21, 33, 0), (39, 53, -1, 0, 20, 33, 0)]
    got = K.mask_transform(src, (20, 33), views=torch.from_numpy(view_rows((MH, MW), bad)).to(dev), pad_val=5)
    assert bool((got == 5).all())


def test_rle_masks_window_equals_transform_then_slice():
    from radet_amd import kernels as K
    from radet_amd.core import rle
    dev = _dev()
    e = edge_masks(MH, MW)
    # all zero (one run), a polygon segmentation of two parts, a compressed run list
    compressed = dict(size=[MH, MW], counts=rle.string_from_counts(rle.rle_from_mask(e["random"])).decode("ascii"))
    segs = [dict(size=[MH, MW], counts=[MH * MW]), [[3, 2, 10, 2, 10, 7, 3, 7], [8.5, 5, 29, 5.5, 20, 20.5]], compressed]
    parts = [rle.parts_from_segmentation(s, MH, MW) for s in segs]
    decoded = np.stack([rle.mask_from_parts(p, MH, MW) for p in parts])
    assert decoded[0].max() == 0 and decoded[1].sum() > 30 and np.array_equal(decoded[2], e["random"])
    G = len(parts)
    host = {hw: om.transform(decoded, resized_hw=hw) for hw in MASK_VIRTUAL}
    cases = _mask_cases()
    out_hw = (max(c[4] for c in cases) + 3, max(c[5] for c in cases) + 2)
    flips = np.repeat([bool(c[6]) for c in cases], G)
    ends, prows, mrows = rle.pack_runs([p for _ in cases for p in parts], MH, MW, flips)
    wrows = np.repeat(view_rows((MH, MW), cases), G, axis=0)
    wrows[:, 10] = 0                                           # (the flip is the mask row's)
    got, plain = K.rle_masks(torch.from_numpy(ends.view(np.int32)).to(dev), torch.from_numpy(prows).to(dev),
                             torch.from_numpy(mrows).to(dev), out_hw, views=torch.from_numpy(wrows).to(dev), pad_val=9, with_plain=True)
    got, plain = got.cpu().numpy(), plain.cpu().numpy()
    for n, case in enumerate(cases):
        np.testing.assert_array_equal(got[n * G:(n + 1) * G], _want(host[case[:2]], case, out_hw, 9), err_msg=str(case))
        if case[6]:                                            # both orientations from one lookup
            np.testing.assert_array_equal(plain[n * G:(n + 1) * G], _want(host[case[:2]], (*case[:6], 0), out_hw, 9), err_msg=str(case))
    # against the plain kernel, sliced
    for hw in MASK_VIRTUAL:
        e2, p2, m2 = rle.pack_runs(parts, MH, MW, np.zeros(G, bool))
        full = K.rle_masks(torch.from_numpy(e2.view(np.int32)).to(dev), torch.from_numpy(p2).to(dev), torch.from_numpy(m2).to(dev), hw)
        assert np.array_equal(full.cpu().numpy(), host[hw])


# ------------------------------------------------------------------------------------------------ the loader
SEED = 5
CROP = (480, 640)
RATIO = (0.6, 1.6)


def jitter_pipeline(background_dir, dm="mask", ann="png"):
    return [
        dict(type="LoadImageFromFile"),
        dict(type="LoadAnnotations", with_bbox=True, **(dict(with_bop_mask=True) if ann == "png" else dict(with_mask=True))),
        dict(type="Resize", img_scale=(640, 480), ratio_range=RATIO, keep_ratio=True),
        dict(type="RandomCrop", crop_size=CROP),
        dict(type="RandomBackground", background_dir=background_dir, prob=0.5),
        dict(type="CosyPoseAug", p=0.8, pipelines=COSY),
        dict(type="RandomFlip", flip_ratio=0.5),
        DM[dm],
        ASSIGNER,
        dict(type="Normalize", **NORM),
        dict(type="Pad", size=CROP),
        dict(type="DefaultFormatBundle"),
        dict(type="Collect", keys=["img", "gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight"]),
    ]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL decodes the generated JPEG / PNG files")
    from radet_amd.datasets.bop_convert import add_segmentation
    from tools.synth_bop import write_tree
    root = str(tmp_path_factory.mktemp("bop"))
    t = write_tree(root, n_frames=8, objects=(3, 6), n_backgrounds=3, seed=11)
    t["rle"] = os.path.join(root, "train_pbr_rle.json")
    json.dump(add_segmentation(json.load(open(t["ann_file"])), t["seg_prefix"], "rle"), open(t["rle"], "w"))
    return t


def _dataset(tree, dm="mask", ann="png", **kw):
    from radet_amd.datasets import build_dataset
    pipe = jitter_pipeline(tree["background_dir"], dm, ann)
    cfg = dict(type="BOPDataset", img_prefix=tree["img_prefix"], pipeline=pipe, **kw)
    if ann == "png":
        return build_dataset(dict(cfg, ann_file=tree["ann_file"], seg_prefix=tree["seg_prefix"]))
    return build_dataset(dict(cfg, ann_file=tree["rle"], mask_source="annotation"))


def restate_sample(png, idx, dm, background_dir):
    """the reference's order for sample idx on the sample's generators, restated on the host: full resize -> slice -> masks
    transform -> slice -> background / CosyPose / flip / Normalize / fixed pad -> assigner (on the padded sample).  `png`:
    the dataset with mask PNG paths (the run-list datasets decode the same masks)."""
    from PIL import Image
    from oracle import assigner as oa
    from radet_amd.datasets.loader import sample_generators
    rnd, nprnd = sample_generators(SEED, 0, idx)
    while True:
        info, ann = png.data_infos[idx], png.get_ann_info(idx)
        img = np.asarray(Image.open(os.path.join(png.img_prefix, info["filename"])).convert("RGB"))[..., ::-1]
        masks = np.stack([np.asarray(Image.open(os.path.join(png.seg_prefix, p))) for p in ann["masks"]])
        h0, w0 = img.shape[:2]
        ratio = nprnd.random_sample() * (RATIO[1] - RATIO[0]) + RATIO[0]
        w, h = om.rescale_size((w0, h0), (int(640 * ratio), int(480 * ratio)))
        sf = np.array([w / w0, h / h0, w / w0, h / h0], np.float32)
        boxes = ann["bboxes"] * sf
        boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, w)
        boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, h)
        ch, cw = min(CROP[0], h), min(CROP[1], w)
        y0 = nprnd.randint(0, max(h - ch, 0) + 1)
        x0 = nprnd.randint(0, max(w - cw, 0) + 1)
        boxes = boxes - np.array([x0, y0, x0, y0], np.float32)
        boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, cw)
        boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, ch)
        valid = (boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])
        if valid.any():
            break
        idx = nprnd.choice(np.flatnonzero(png.flag == png.flag[idx]))            # (the dataset's re-draw)
    boxes, labels = boxes[valid], ann["labels"][valid]
    x = np.ascontiguousarray(R.resize_linear_u8(img, w, h)[y0:y0 + ch, x0:x0 + cw])
    m = np.ascontiguousarray(om.transform(masks[valid], resized_hw=(h, w), norm=True)[:, y0:y0 + ch, x0:x0 + cw])
    bg = None
    if not rnd.random() > 0.5:
        bgs = sorted(os.path.join(background_dir, n) for n in os.listdir(background_dir))
        bg = np.asarray(Image.open(rnd.choice(bgs)).convert("RGB"))[..., ::-1]
        x = R.merge_background(x, R.resize_linear_u8(bg, cw, ch), m)
    aug = {}
    if not rnd.random() > 0.8:
        aug["blur_k"] = rnd.randint(1, 3)
        for key, (p, iv) in zip(("sharp", "contr", "bright", "col"),
                                ((0.3, (0., 50.)), (0.3, (0.2, 50.)), (0.5, (0.1, 6.0)), (0.3, (0., 20.)))):
            if rnd.random() <= p:
                aug[key] = rnd.uniform(*iv)
    x = np.ascontiguousarray(R.cosypose(x[..., ::-1], **aug)[..., ::-1])
    flip = nprnd.choice(["horizontal", None], p=[0.5, 0.5]) is not None
    if flip:
        boxes = np.stack([cw - boxes[:, 2], boxes[:, 1], cw - boxes[:, 0], boxes[:, 3]], axis=1)
        x, m = np.ascontiguousarray(x[:, ::-1]), om.flip(m)
    if dm == "mask":
        maps = om.pad(m, CROP)
    else:
        from radet_amd.datasets import PIPELINES
        from radet_amd.utils import build_from_cfg
        random.setstate(rnd.getstate())                       # GenerateDistanceMap draws from the global `random`
        res = build_from_cfg(DM[dm], PIPELINES)(dict(img=x, img_shape=(ch, cw, 3), gt_bboxes=boxes))
        rnd.setstate(random.getstate())
        maps = np.zeros((len(boxes), *CROP), np.float32)
        maps[:, :ch, :cw] = res["distance_maps"].cpu().numpy()
    out = np.zeros((3, *CROP), np.float32)
    out[:, :ch, :cw] = R.normalize(x, NORM["mean"], NORM["std"])
    p2g, pw = oa.assign_points(boxes, labels, maps, (*CROP, 3), rng=nprnd)
    return dict(img=out, gt_bboxes=boxes, gt_labels=labels, p2g=p2g, pw=pw, flip=flip, img_shape=(ch, cw, 3), scale_factor=sf,
                windowed=(h, w) != (ch, cw), up=ratio > 1, whole=(h, w) == (ch, cw), bg=bg is not None,
                whole_merged=(h, w) == (ch, cw) and bg is not None,
                whole_merged_flipped=(h, w) == (ch, cw) and bg is not None and flip)


@pytest.fixture(scope="module")
def png(tree):
    return _dataset(tree)


_RESTATED = {}


def restated(png, idx, dm, background_dir):
    """restate_sample, computed once per (sample, sampler) and shared by the variants that must all equal it"""
    if (idx, dm) not in _RESTATED:
        _RESTATED[(idx, dm)] = restate_sample(png, idx, dm, background_dir)
    return _RESTATED[(idx, dm)]


VARIANTS = {"png": dict(), "runs": dict(ann="rle"), "device-decode-cache": dict(image_decode="device", sample_cache="device", cache_bytes=64 << 20),
            "mask-free-mbd": dict(dm="mbd")}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_loader_equals_host_restatement(tree, png, variant):
    from radet_amd.datasets import build_dataloader
    kw = dict(VARIANTS[variant])
    dm = kw.get("dm", "mask")
    ds = _dataset(tree, **kw)
    loader = build_dataloader(ds, samples_per_gpu=4, workers=4, seed=SEED)
    n, kinds = 0, set()
    for batch, idxs in zip(loader, loader.batches()):
        assert batch["img"].shape == (4, 3, *CROP) and batch["img"].is_cuda                 # the shape is constant
        img = batch["img"].cpu().numpy()
        for j, idx in enumerate(idxs):
            ref = restated(png, idx, dm, tree["background_dir"])
            what = f"sample {idx}: {ref['img_shape']} flip {ref['flip']} bg {ref['bg']}"
            np.testing.assert_array_equal(img[j], ref["img"], err_msg=what)
            np.testing.assert_array_equal(batch["gt_bboxes"][j].numpy(), ref["gt_bboxes"], err_msg=what)
            np.testing.assert_array_equal(batch["gt_labels"][j].numpy(), ref["gt_labels"], err_msg=what)
            np.testing.assert_array_equal(batch["points_to_gt_index"][j].cpu().numpy(), ref["p2g"], err_msg=what)
            np.testing.assert_array_equal(batch["points_weight"][j].cpu().numpy(), ref["pw"], err_msg=what)
            meta = batch["img_metas"][j]
            assert meta["flip"] == ref["flip"] and tuple(meta["img_shape"]) == ref["img_shape"], what
            assert tuple(meta["pad_shape"]) == (*CROP, 3) and np.array_equal(meta["scale_factor"], ref["scale_factor"]), what
            kinds |= {k for k in ("windowed", "up", "whole", "flip", "bg", "whole_merged", "whole_merged_flipped") if ref[k]}
            n += 1
    loader.close()
    # (whole_merged: a sample smaller than the pad whose merge reads the padded masks through the mask pitch)
    assert n == 8 and {"windowed", "up", "whole", "whole_merged", "whole_merged_flipped"} <= kinds, kinds
    if "cache" in variant:
        assert ds.pipeline.decode_stats["device"] > 0 and ds.pipeline.cache_stats["inserted"] > 0


def test_cached_epoch_equals_the_first(tree):
    """sample_cache='device': the second visit of the files (cache hits, other scales and windows) equals the uncached pipeline"""
    from radet_amd.datasets.loader import sample_generators
    plain, cached = _dataset(tree), _dataset(tree, image_decode="device", sample_cache="device", cache_bytes=64 << 20)
    for epoch in range(2):
        a = plain.pipeline.run([plain.plan_sample(i, *sample_generators(SEED, epoch, i)) for i in range(4)], collate=True)
        b = cached.pipeline.run([cached.plan_sample(i, *sample_generators(SEED, epoch, i)) for i in range(4)], collate=True)
        assert torch.equal(a["img"], b["img"])
        for k in ("gt_bboxes", "points_to_gt_index", "points_weight"):
            assert all(torch.equal(x, y) for x, y in zip(a[k], b[k]))
    assert cached.pipeline.cache_stats["hits"] > 0


def test_launch_log(tree):
    """a jitter batch launches what the same files launch through the fixed-scale pipeline, entry point for entry point"""
    from radet_amd import _lib
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.datasets import build_dataset
    logs = {}
    for ann in ("png", "rle"):
        jit = _dataset(tree, ann=ann)
        fixed_pipe = [t for t in jitter_pipeline(tree["background_dir"], ann=ann) if t["type"] != "RandomCrop"]
        fixed_pipe[2] = dict(type="Resize", img_scale=(640, 480), keep_ratio=True)
        fixed = build_dataset(dict(type="BOPDataset", img_prefix=tree["img_prefix"], pipeline=fixed_pipe,
                                   **(dict(ann_file=tree["ann_file"], seg_prefix=tree["seg_prefix"]) if ann == "png"
                                      else dict(ann_file=tree["rle"], mask_source="annotation"))))
        # four up-scaled (windowed) samples of the jitter pipeline, and the fixed pipeline's samples with the same flips and
        # backgrounds (what decides the optional launches)
        plans = []
        for i in range(4):
            for epoch in range(200):
                s = jit.plan_sample(i, *sample_generators(SEED, epoch, i))
                want_both = not plans                       # the first: flipped AND merged (both mask orientations are needed)
                if s["resize_hw"][0] > CROP[0] and s["crop_window"][2:] == CROP and \
                        (not want_both or (s["flip"] and "background" in s and len(s["gt_bboxes"]))):
                    plans.append(s)
                    break
        assert len(plans) == 4
        ref = []
        for i, s in enumerate(plans):
            for epoch in range(200):
                f = fixed.plan_sample(i, *sample_generators(SEED, epoch, i))
                if bool(f["flip"]) == bool(s["flip"]) and ("background" in f) == ("background" in s):
                    ref.append(f)
                    break
        assert len(ref) == 4 and plans[0]["flip"] and "background" in plans[0]
        seen, call = [], _lib.call
        _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
        try:
            out = jit.pipeline.run(plans, collate=True)
            jit_seen = list(seen)
            del seen[:]
            fixed.pipeline.run(ref, collate=True)
            fixed_seen = list(seen)
        finally:
            _lib.call = call
        assert out["img"].shape == (4, 3, *CROP)
        assert jit_seen == fixed_seen, (jit_seen, fixed_seen)
        logs[ann] = jit_seen
    assert logs["png"].count("radet_mask_transform") == 2 and logs["rle"].count("radet_rle_masks") == 1      # both mask passes
    assert not any("window" in n for n in jit_seen + fixed_seen)


@pytest.mark.parametrize("ann", ["png", "rle"])
def test_mixed_batch_launches_what_a_windowed_batch_does(tree, ann):
    """samples of many scales in one batch, kept whole and windowed, merged and flipped: the entry points of a batch whose
    samples all fill the crop -- one mask group, one assigner launch, nothing per sample"""
    from radet_amd import _lib
    from radet_amd.datasets.loader import sample_generators
    ds = _dataset(tree, ann=ann)
    plans = [ds.plan_sample(i, *sample_generators(SEED, 0, i)) for i in range(8)]
    sizes = {tuple(s["crop_window"][2:]) for s in plans}
    assert len(sizes) > 2 and CROP in sizes
    assert any("background" in s and s["flip"] and tuple(s["crop_window"][2:]) != CROP for s in plans)
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        ds.pipeline.run(plans, collate=True)
    finally:
        _lib.call = call
    mask_stage = ["radet_mask_max", "radet_mask_transform", "radet_mask_transform"] if ann == "png" else ["radet_rle_masks"]
    assert seen == ["radet_resize_linear_u8", "radet_resize_linear_u8", *mask_stage, "radet_augment_merge_hblur",
                    "radet_augment_vblur", "radet_augment_sharp", "radet_augment_finish", "radet_assign_points"], seen


# ------------------------------------------------------------------------------------------------ training
def test_train_detector_on_the_jitter_config(tree):
    from oracle import synth
    from radet_amd.apis import train_detector
    from radet_amd.datasets import build_dataloader, build_dataset
    from radet_amd.models import build_detector
    from _jitter_cfg import jitter_train_cfg
    cfg, train = jitter_train_cfg(tree)
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    synth.fill_state_dict(det.state_dict(), seed=0)
    det = det.cuda()
    cfg.merge_from_dict({"lr_config.total_steps": 40, "log_config.interval": 1})
    loader = build_dataloader(build_dataset(train), samples_per_gpu=4, workers=4, seed=0)
    shapes = set()

    def batches():
        epoch = 0
        while True:
            loader.set_epoch(epoch)
            for b in loader:
                shapes.add((tuple(b["img"].shape), tuple(sorted({tuple(m["img_shape"]) for m in b["img_metas"]}))))
                yield b
            epoch += 1
    hist = train_detector(det, batches(), cfg, max_iters=6, log=lambda *_: None)
    loader.close()
    assert len(hist) == 6 and all(np.isfinite(h).all() for h in hist)
    assert {s[0] for s in shapes} == {(4, 3, *CROP)} and len({s[1] for s in shapes}) > 1     # one batch shape, many scales
    assert det.runtime().tape_stats()["replays"] > 0
