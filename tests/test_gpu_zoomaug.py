"""Zoom augmentation on the GPU: source windows (view rows) of the resize and of both mask kernels against the materialised
host chain (NumPy canvas / np.pad, paste, slice, then oracle/imgproc.py and oracle/masks.py), the pipeline on Expand +
MinIoURandomCrop + Resize against that chain built from each planned sample's recorded draws, and the launch log.  Every
comparison is array_equal / torch.equal."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _augment_ref as R  # noqa: E402
from oracle import imgproc, masks as om  # noqa: E402
from _maskfree_pipelines import ASSIGNER, NORM  # noqa: E402
from _rle_cases import edge_masks  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0xAB
FILL = (11, 140, 250)                                          # three distinct values: the channel order shows


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def src_windows(h, w):
    """(y0, x0, wh, ww) in the coordinates of an h x w image: strictly inside; overhanging each single side by 1 and by
    more than the image; holding the whole image; 1 x 1; entirely outside"""
    return [(2, 3, h - 5, w - 6),
            (-1, 2, h - 3, w - 5), (-(h + 2), 2, 2 * h, w - 5),                        # top
            (3, 2, h - 2, w - 5), (3, 2, 2 * h + 4, w - 5),                           # bottom
            (2, -1, h - 4, w - 3), (2, -(w + 3), h - 4, 2 * w),                        # left
            (2, 4, h - 4, w - 3), (2, 4, h - 4, 2 * w + 5),                           # right
            (-4, -7, h + 9, w + 11),                                                  # the whole image (Expand only)
            (3, 4, 1, 1), (h - 1, w - 1, 1, 1), (-1, -1, 1, 1),
            (h + 2, w + 3, 5, 6), (-20, -25, 5, 7), (1, w, 4, 3)]                     # outside


def host_window(src, win, fill):
    """the canvas that holds the image and the window, filled, the image pasted, the window sliced"""
    y0, x0, wh, ww = win
    h, w = src.shape[:2]
    top, left = max(0, -y0), max(0, -x0)
    canvas = np.empty((max(h, y0 + wh) + top, max(w, x0 + ww) + left, *src.shape[2:]), src.dtype)
    canvas[:] = fill
    canvas[top:top + h, left:left + w] = src
    return np.ascontiguousarray(canvas[y0 + top:y0 + top + wh, x0 + left:x0 + left + ww])


def test_windows_cover_what_they_claim():
    for h, w in ((13, 17), (60, 80)):
        wins = src_windows(h, w)
        inside = [0 <= y0 and 0 <= x0 and y0 + wh <= h and x0 + ww <= w for y0, x0, wh, ww in wins]
        outside = [y0 >= h or x0 >= w or y0 + wh <= 0 or x0 + ww <= 0 for y0, x0, wh, ww in wins]
        assert inside[0] and not any(inside[1:10]) and all(outside[-3:]) and not any(outside[:10])
        assert [(-y0, y0 + wh - h, -x0, x0 + ww - w) for y0, x0, wh, ww in wins[1:9:2]] == \
            [(1, -4, -2, -3), (-3, 1, -2, -3), (-2, -2, 1, -4), (-2, -2, -4, 1)]     # each single side by exactly 1
        assert wins[2][0] < -h and wins[4][0] + wins[4][2] > 2 * h and wins[6][1] < -w and wins[8][1] + wins[8][3] > 2 * w


# ------------------------------------------------------------------------------------------------ the resize
@pytest.fixture(scope="module")
def sources():
    rs = np.random.RandomState(0)
    return [rs.randint(0, 256, (13, 17, 3)).astype(np.uint8), rs.randint(0, 256, (60, 80, 3)).astype(np.uint8)]


def resize_rows(sources):
    """(source index, window, output (Hr, Wr)): every window up-scaled by about 2.3 and down-scaled by about 0.4, the x
    and y factors unequal"""
    rows = []
    for k, s in enumerate(sources):
        for win in src_windows(*s.shape[:2]):
            wh, ww = win[2:]
            rows.append((k, win, (max(int(wh * 2.3), 1), max(int(ww * 2.6 + 0.5), 1))))
            rows.append((k, win, (max(int(wh * 0.4 + 0.5), 1), max(int(ww * 0.45), 1))))
    return rows


@pytest.fixture(scope="module")
def resize_want(sources):
    return [imgproc.resize_linear_u8(host_window(sources[k], win, FILL), (Wr, Hr)) for k, win, (Hr, Wr) in resize_rows(sources)]


def view_rows(cases, fill=0):
    """the view rows of (Hr, Wr, y0, x0, wh, ww, flip) cases: the wh x ww window at (y0, x0) of the source resized to Hr x Wr,
    all of it written"""
    return np.array([(Hr, Wr, y0, x0, wh, ww, 0, 0, Hr, Wr, fl, fill) for Hr, Wr, y0, x0, wh, ww, fl in cases], np.int32)


def _src_window_resize(K, srcs, rows, align, fill=FILL, guard=64):
    """one launch over mixed rows; returns the per-row outputs and checks the guard bytes"""
    dev = _dev()
    soff = np.cumsum([0] + [s.shape[0] * s.shape[1] for s in srcs])
    sdesc = [(soff[k], srcs[k].shape[0], srcs[k].shape[1]) for k, _, _ in rows]
    wdesc, o = [], guard
    for k, (y0, x0, wh, ww), (Hr, Wr) in rows:
        wdesc.append((o, Hr, Wr))
        o += -(-Hr * Wr // align) * align
    total = o + guard
    dst = torch.full((total * 3,), GUARD, dtype=torch.uint8, device=dev)
    views = view_rows([(Hr, Wr, *win, 0) for _, win, (Hr, Wr) in rows], fill[0] | fill[1] << 8 | fill[2] << 16)
    K.resize_linear_u8(torch.from_numpy(np.concatenate([s.reshape(-1) for s in srcs])).to(dev),
                       torch.tensor(np.array(sdesc), dtype=torch.int32, device=dev), dst,
                       torch.tensor(np.array(wdesc), dtype=torch.int32, device=dev), len(rows),
                       max(hw[0] * hw[1] for _, _, hw in rows), 3, views=torch.from_numpy(views).to(dev))
    host = dst.cpu().numpy()
    written = np.zeros(total * 3, bool)
    outs = []
    for off, Hr, Wr, *_ in wdesc:
        assert off % align == 0
        outs.append(host[off * 3:(off + Hr * Wr) * 3].reshape(Hr, Wr, 3))
        written[off * 3:(off + Hr * Wr) * 3] = True
    assert (host[~written] == GUARD).all(), "bytes outside the outputs were written"
    return outs


@pytest.mark.parametrize("align", [1, 4])
def test_resize_src_window_equals_canvas_paste_slice_resize(sources, resize_want, align):
    from radet_amd import kernels as K
    rows = resize_rows(sources)
    assert len({Hr * Wr % 4 for _, _, (Hr, Wr) in rows}) > 1 and any(Hr * Wr > 256 and Hr * Wr % 256 for _, _, (Hr, Wr) in rows)
    for row, out, want in zip(rows, _src_window_resize(K, sources, rows, align), resize_want):
        np.testing.assert_array_equal(out, want, err_msg=str(row))
    # a window outside the image is the fill, whatever the scale
    for (k, win, _), want in zip(rows, resize_want):
        if win in src_windows(*sources[k].shape[:2])[-3:]:
            assert (want == np.array(FILL, np.uint8)).all()


def test_resize_src_window_of_the_whole_image_is_the_plain_resize(sources):
    """the window that is exactly the image (what a sample without a window gets): the plain kernel's bytes; rows without
    a window or without a source are not written"""
    from radet_amd import kernels as K
    dev = _dev()
    src = sources[1]
    h, w = src.shape[:2]
    got = _src_window_resize(K, sources, [(1, (0, 0, h, w), (138, 208)), (1, (0, 0, h, w), (24, 36))], 1)
    for out in got:
        Hr, Wr = out.shape[:2]
        dst = torch.empty(Hr * Wr * 3, dtype=torch.uint8, device=dev)
        desc = torch.tensor([[0, h, w], [0, Hr, Wr]], dtype=torch.int32, device=dev)
        K.resize_linear_u8(torch.from_numpy(src.reshape(-1)).to(dev), desc[:1], dst, desc[1:], 1, Hr * Wr, 3)
        np.testing.assert_array_equal(out, dst.cpu().numpy().reshape(Hr, Wr, 3))
    outs = _src_window_resize(K, sources, [(1, (0, 0, 0, w), (8, 8)), (1, (0, 0, h, -1), (8, 8)), (1, (2, 2, 8, 8), (8, 8))], 1)
    assert (outs[0] == GUARD).all() and (outs[1] == GUARD).all()
    np.testing.assert_array_equal(outs[2], src[2:10, 2:10])


# ------------------------------------------------------------------------------------------------ the masks
MH, MW = 23, 31


@pytest.fixture(scope="module")
def bitmaps():
    """G = 4: all zero; maximum 255 with a lower value; maximum 1; 0 / 255 whose only 255 pixels lie in the first two rows and
    columns (outside the windows that start at (2, 3)), a 7 elsewhere"""
    e = edge_masks(MH, MW)
    far = np.full((MH, MW), 7, np.uint8)
    far[:2, :] = 0
    far[:, :2] = 0
    far[0, 0] = far[1, 1] = 255
    m = np.stack([e["zeros"], e["random"] * 255, e["span"], far]).astype(np.uint8)
    m[1, 3, 4] = 7                                            # (a value below the maximum normalises to 0)
    m.setflags(write=False)
    return m


def mask_cases():
    """(Hr, Wr, y0, x0, wh, ww, flip): every window up- and down-scaled, both orientations"""
    out = []
    for y0, x0, wh, ww in src_windows(MH, MW):
        for Hr, Wr in ((max(int(wh * 2.3), 1), max(int(ww * 1.7 + 0.5), 1)), (max(int(wh * 0.4 + 0.5), 1), max(int(ww * 0.6), 1))):
            out += [(Hr, Wr, y0, x0, wh, ww, fl) for fl in (0, 1)]
    return out


def mask_want(normalised, case, out_hw, pad_val=0):
    """np.pad / slice of the masks as loaded (normalised by their own maximum), nearest resize, flip, pad"""
    Hr, Wr, y0, x0, wh, ww, fl = case
    m = om.resize_nearest(host_window(normalised.transpose(1, 2, 0), (y0, x0, wh, ww), 0).transpose(2, 0, 1), (Hr, Wr))
    return om.pad(om.flip(m) if fl else m, out_hw, pad_val)


def test_mask_transform_src_window_equals_pad_slice_transform(bitmaps):
    from radet_amd import kernels as K
    dev = _dev()
    cases = mask_cases()
    G = len(bitmaps)
    normalised = om.normalize(bitmaps)
    assert normalised[3].sum() == 2 and normalised[1].max() == 1 and normalised[0].max() == 0
    src = torch.from_numpy(bitmaps.copy()).to(dev)
    out_hw = (max(c[0] for c in cases) + 3, max(c[1] for c in cases) + 2)
    rows = torch.tensor(np.repeat(view_rows(cases), G, axis=0), device=dev)
    got = K.mask_transform(src.repeat(len(cases), 1, 1), out_hw, views=rows, pad_val=9, normalize=True).cpu().numpy()
    for n, case in enumerate(cases):
        np.testing.assert_array_equal(got[n * G:(n + 1) * G], mask_want(normalised, case, out_hw, 9), err_msg=str(case))
    # the mask whose maximum lies outside the window: all zero inside, normalised by the maximum of the whole mask
    n = cases.index((int((MH - 5) * 2.3), int((MW - 6) * 1.7 + 0.5), 2, 3, MH - 5, MW - 6, 0))
    Hr, Wr = cases[n][:2]
    assert (got[n * G + 3, :Hr, :Wr] == 0).all() and (bitmaps[3, 2:MH - 3, 3:MW - 3] == 7).all()
    # without normalisation: the bytes themselves, zeros around them
    case = (40, 50, -3, -2, MH + 5, MW + 6, 1)
    got = K.mask_transform(src, (40, 52), views=torch.from_numpy(view_rows([case] * G)).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got, mask_want(bitmaps, case, (40, 52)))
    assert got.max() == 255
    # a row whose output does not fit the destination, or without a window: pad_val only
    bad = [(41, 50, 0, 0, MH, MW, 0), (40, 53, 0, 0, MH, MW, 0), (40, 50, 0, 0, 0, MW, 0), (0, 50, 0, 0, MH, MW, 0)]
    got = K.mask_transform(src, (40, 52), views=torch.from_numpy(view_rows(bad)).to(dev), pad_val=5)
    assert bool((got == 5).all())


@pytest.mark.parametrize("with_plain", [True, False])
def test_rle_masks_src_window_equals_the_bitmap_variant(with_plain):
    from radet_amd import kernels as K
    from radet_amd.core import rle
    dev = _dev()
    e = edge_masks(MH, MW)
    # all zero (one run), all ones, a polygon segmentation of two parts, a compressed run list, columns that end in ones (a
    # sample right of or below the image must not land in the next column's run)
    compressed = dict(size=[MH, MW], counts=rle.string_from_counts(rle.rle_from_mask(e["random"])).decode("ascii"))
    checker = dict(size=[MH, MW], counts=rle.string_from_counts(rle.rle_from_mask(e["checker"])).decode("ascii"))
    ones = dict(size=[MH, MW], counts=rle.string_from_counts(rle.rle_from_mask(e["ones"])).decode("ascii"))
    segs = [dict(size=[MH, MW], counts=[MH * MW]), ones,
            [[3, 2, 10, 2, 10, 7, 3, 7], [8.5, 5, 29, 5.5, 20, 20.5]], compressed, checker]
    parts = [rle.parts_from_segmentation(s, MH, MW) for s in segs]
    decoded = np.stack([rle.mask_from_parts(p, MH, MW) for p in parts])
    assert decoded[0].max() == 0 and decoded[1].min() == 1 and decoded[2].sum() > 30 and len(parts[2]) == 2
    G = len(parts)
    cases = mask_cases()
    out_hw = (max(c[0] for c in cases) + 3, max(c[1] for c in cases) + 2)
    flips = np.repeat([bool(c[6]) for c in cases], G)
    ends, prows, mrows = rle.pack_runs([p for _ in cases for p in parts], MH, MW, flips)
    wrows = np.repeat(view_rows(cases), G, axis=0)
    bitmap = K.mask_transform(torch.from_numpy(decoded).to(dev).repeat(len(cases), 1, 1), out_hw, views=torch.from_numpy(wrows).to(dev),
                              pad_val=9, normalize=True).cpu().numpy()
    wrows[:, 10] = 0                                           # (the flip is the mask row's)
    res = K.rle_masks(torch.from_numpy(ends.view(np.int32)).to(dev), torch.from_numpy(prows).to(dev),
                      torch.from_numpy(mrows).to(dev), out_hw, views=torch.from_numpy(wrows).to(dev), pad_val=9,
                      with_plain=with_plain)
    got, plain = (res[0].cpu().numpy(), res[1].cpu().numpy()) if with_plain else (res.cpu().numpy(), None)
    np.testing.assert_array_equal(got, bitmap)
    for n, case in enumerate(cases):
        np.testing.assert_array_equal(got[n * G:(n + 1) * G], mask_want(decoded, case, out_hw, 9), err_msg=str(case))
        if case[6] and with_plain:                             # both orientations from one lookup
            np.testing.assert_array_equal(plain[n * G:(n + 1) * G], mask_want(decoded, (*case[:6], 0), out_hw, 9), err_msg=str(case))


# ------------------------------------------------------------------------------------------------ the pipeline
SEED = 7
OUT = (480, 640)
MEAN_BGR = (103, 116, 123)
ZOOM = [dict(type="Expand", mean=NORM["mean"], to_rgb=True, ratio_range=(1, 2), prob=0.5),
        dict(type="MinIoURandomCrop", min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3)]


def zoom_pipeline(background_dir, ann="png", zoom=True):
    """the zoom config's pipeline with the photometric stages off"""
    return [
        dict(type="LoadImageFromFile"),
        dict(type="LoadAnnotations", with_bbox=True, **(dict(with_bop_mask=True) if ann == "png" else dict(with_mask=True))),
        *(ZOOM if zoom else ()),
        dict(type="Resize", img_scale=(640, 480), keep_ratio=False),
        dict(type="RandomBackground", background_dir=background_dir, prob=0.5),
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
    from radet_amd.datasets.bop_convert import add_segmentation
    from tools.synth_bop import write_tree
    root = str(tmp_path_factory.mktemp("bop"))
    t = write_tree(root, n_frames=4, objects=(3, 5), n_backgrounds=2, seed=11)
    t["rle"] = os.path.join(root, "train_pbr_rle.json")
    json.dump(add_segmentation(json.load(open(t["ann_file"])), t["seg_prefix"], "rle"), open(t["rle"], "w"))
    return t


def _dataset(tree, ann="png", zoom=True, **kw):
    from radet_amd.datasets import build_dataset
    cfg = dict(type="BOPDataset", img_prefix=tree["img_prefix"], pipeline=zoom_pipeline(tree["background_dir"], ann, zoom), **kw)
    if ann == "png":
        return build_dataset(dict(cfg, ann_file=tree["ann_file"], seg_prefix=tree["seg_prefix"]))
    return build_dataset(dict(cfg, ann_file=tree["rle"], mask_source="annotation"))


def _plans(ds, epoch):
    from radet_amd.datasets.loader import sample_generators
    return [ds.plan_sample(i, *sample_generators(SEED, epoch, i)) for i in range(4)]


def host_chain(png, idx, s):
    """The reference's order for one sample, materialised on the host from the draws its plan recorded (s: the plan of the
    host-decoding dataset, before run): canvas, paste, slice, resize, background, flip, Normalize, assigner on the masks."""
    from PIL import Image
    from oracle import assigner as oa
    info, ann = png.data_infos[idx], png.get_ann_info(idx)
    x = np.asarray(Image.open(os.path.join(png.img_prefix, info["filename"])).convert("RGB"))[..., ::-1]
    m = om.normalize(np.stack([np.asarray(Image.open(os.path.join(png.seg_prefix, p))) for p in ann["masks"]]))
    boxes, labels = ann["bboxes"].astype(np.float32), ann["labels"]
    kinds = set()
    if "expand" in s:
        ratio, left, top = s["expand"]
        h, w = x.shape[:2]
        canvas = np.empty((int(h * ratio), int(w * ratio), 3), np.uint8)
        canvas[:] = MEAN_BGR
        canvas[top:top + h, left:left + w] = x
        mc = np.zeros((len(m), *canvas.shape[:2]), np.uint8)
        mc[:, top:top + h, left:left + w] = m
        x, m, boxes = canvas, mc, boxes + np.array([left, top, left, top], np.float32)
        kinds.add("expanded")
    if s["crop_mode"] != 1:
        px0, py0, px1, py1 = s["crop_patch"]
        c = (boxes[:, :2] + boxes[:, 2:]) / 2
        keep = (c[:, 0] > px0) & (c[:, 1] > py0) & (c[:, 0] < px1) & (c[:, 1] < py1)
        boxes = np.clip(boxes[keep], [px0, py0, px0, py0], [px1, py1, px1, py1]).astype(np.float32) - np.array([px0, py0, px0, py0], np.float32)
        labels, m, x = labels[keep], m[keep][:, py0:py1, px0:px1], x[py0:py1, px0:px1]
        kinds |= {"cropped", "dropped"} if not keep.all() else {"cropped"}
        if "expand" in s and not (left <= px0 and top <= py0 and px1 <= left + w and py1 <= top + h):
            kinds.add("crop_touches_fill")
    h, w = x.shape[:2]
    sf = np.array([640 / w, 480 / h, 640 / w, 480 / h], np.float32)
    boxes = boxes * sf
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, 640)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, 480)
    x, m = R.resize_linear_u8(np.ascontiguousarray(x), 640, 480), om.resize_nearest(np.ascontiguousarray(m), OUT)
    if "background" in s:
        x = R.merge_background(x, R.resize_linear_u8(s["background"], 640, 480), m)
        kinds.add("bg")
    if s["flip"]:
        boxes = np.stack([640 - boxes[:, 2], boxes[:, 1], 640 - boxes[:, 0], boxes[:, 3]], axis=1)
        x, m = np.ascontiguousarray(x[:, ::-1]), om.flip(m)
        kinds.add("flip")
    p2g, pw = oa.assign_points(boxes, labels, np.ascontiguousarray(m), (*OUT, 3), rng=copy.deepcopy(s["_nprnd"]))
    return dict(img=R.normalize(x, NORM["mean"], NORM["std"]), gt_bboxes=boxes, gt_labels=labels, p2g=p2g, pw=pw, sf=sf, kinds=kinds)


@pytest.fixture(scope="module")
def png(tree):
    return _dataset(tree)


@pytest.fixture(scope="module")
def chains(png):
    """the host chain of two batches (epochs 0 and 1 of the same four files: other draws), computed once"""
    out = {}
    for epoch in (0, 1):
        for idx, s in enumerate(_plans(png, epoch)):
            assert isinstance(s["img"], np.ndarray)
            out[(epoch, idx)] = host_chain(png, idx, s)
    kinds = set().union(*(c["kinds"] for c in out.values()))
    assert {"expanded", "cropped", "dropped", "crop_touches_fill", "bg", "flip"} <= kinds, kinds
    assert any(c["kinds"] >= {"expanded", "bg"} for c in out.values())          # the fill border merged as background
    return out


VARIANTS = {"host": dict(), "runs": dict(ann="rle"), "device-decode": dict(image_decode="device"),
            "sample-cache": dict(sample_cache="device", cache_bytes=64 << 20)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_pipeline_equals_the_materialised_host_chain(tree, chains, variant):
    ds = _dataset(tree, **VARIANTS[variant])
    shapes = set()
    for epoch in ((0, 1, 0) if variant == "sample-cache" else (0, 1)):          # (the third batch: cache hits)
        batch = ds.pipeline.run(_plans(ds, epoch), collate=True)
        shapes.add(tuple(batch["img"].shape))
        img = batch["img"].cpu().numpy()
        for j in range(4):
            ref, what = chains[(epoch, j)], f"epoch {epoch} sample {j}: {sorted(chains[(epoch, j)]['kinds'])}"
            np.testing.assert_array_equal(img[j], ref["img"], err_msg=what)
            np.testing.assert_array_equal(batch["gt_bboxes"][j].numpy(), ref["gt_bboxes"], err_msg=what)
            np.testing.assert_array_equal(batch["gt_labels"][j].numpy(), ref["gt_labels"], err_msg=what)
            np.testing.assert_array_equal(batch["points_to_gt_index"][j].cpu().numpy(), ref["p2g"], err_msg=what)
            np.testing.assert_array_equal(batch["points_weight"][j].cpu().numpy(), ref["pw"], err_msg=what)
            meta = batch["img_metas"][j]
            assert tuple(meta["img_shape"]) == tuple(meta["pad_shape"]) == (*OUT, 3) and np.array_equal(meta["scale_factor"], ref["sf"]), what
    assert shapes == {(4, 3, *OUT)}                                            # other draws, the same tensor shape
    if variant == "device-decode":
        assert ds.pipeline.decode_stats["device"] > 0
    if variant == "sample-cache":
        assert ds.pipeline.cache_stats["hits"] > 0


@pytest.mark.parametrize("ann", ["png", "rle"])
def test_launch_log(tree, ann):
    """a zoom batch launches what the same files launch through the fixed-scale pipeline, entry point for entry point"""
    from radet_amd import _lib
    from radet_amd.datasets.loader import sample_generators
    zoom, fixed = _dataset(tree, ann=ann), _dataset(tree, ann=ann, zoom=False)
    # four samples with a source window, the first flipped AND merged (both mask orientations are needed), and the fixed
    # pipeline's samples with the same flips and backgrounds (what decides the optional launches)
    plans = []
    for i in range(4):
        for epoch in range(200):
            s = zoom.plan_sample(i, *sample_generators(SEED, epoch, i))
            if "src_window" in s and (plans or (s["flip"] and "background" in s)):
                plans.append(s)
                break
    assert len(plans) == 4 and plans[0]["flip"] and "background" in plans[0]
    ref = []
    for i, s in enumerate(plans):
        for epoch in range(200):
            f = fixed.plan_sample(i, *sample_generators(SEED, epoch, i))
            if bool(f["flip"]) == bool(s["flip"]) and ("background" in f) == ("background" in s):
                ref.append(f)
                break
    assert len(ref) == 4
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        out = zoom.pipeline.run(plans, collate=True)
        zoom_seen = list(seen)
        del seen[:]
        fixed.pipeline.run(ref, collate=True)
        fixed_seen = list(seen)
    finally:
        _lib.call = call
    assert out["img"].shape == (4, 3, *OUT)
    assert zoom_seen == fixed_seen, (zoom_seen, fixed_seen)
    assert zoom_seen.count("radet_mask_transform" if ann == "png" else "radet_rle_masks") == (2 if ann == "png" else 1)   # both mask passes
    assert not any("window" in n for n in zoom_seen + fixed_seen)


def test_mix_and_mask_free_pipelines_take_source_windows(tree):
    """the mixpbr stages (images packed at multiples of 4 pixels) and the mask-free sampler (which only sees the finished
    image) on zoomed samples: the frames of such a batch equal the plain pipeline's, resized from the same windows"""
    from _maskfree_pipelines import DM, MIX
    from radet_amd.datasets import build_dataset
    base = zoom_pipeline(tree["background_dir"])
    ref = _dataset(tree)
    plans = _plans(ref, 0)
    want = ref.pipeline.run(_plans(ref, 0), collate=True)
    # the mix stages switched off by their probabilities: the batch goes through the mix kernels' packing untouched
    off = [dict(t, prob=0.0) for t in MIX]
    mix = build_dataset(dict(type="BOPDataset", img_prefix=tree["img_prefix"], ann_file=tree["ann_file"], seg_prefix=tree["seg_prefix"],
                             pipeline=base[:6] + off + base[6:]))
    assert mix.pipeline.mix
    got = mix.pipeline.run(_plans(mix, 0), collate=True)
    assert [s["src_window"] for s in _plans(mix, 0) if "src_window" in s] == [s["src_window"] for s in plans if "src_window" in s]
    assert torch.equal(got["img"], want["img"])
    for k in ("gt_bboxes", "points_to_gt_index", "points_weight"):
        assert all(torch.equal(a, b) for a, b in zip(got[k], want[k]))
    free = build_dataset(dict(type="BOPDataset", img_prefix=tree["img_prefix"], ann_file=tree["ann_file"], seg_prefix=tree["seg_prefix"],
                              pipeline=[DM["mbd"] if t["type"] == "GenerateDistanceMap" else t for t in base]))
    assert free.pipeline.mask_free is not None
    got = free.pipeline.run(_plans(free, 0), collate=True)
    assert torch.equal(got["img"], want["img"]) and all(torch.equal(a, b) for a, b in zip(got["gt_bboxes"], want["gt_bboxes"]))
    assert all(p.shape == q.shape and bool((p >= -1).all()) for p, q in zip(got["points_to_gt_index"], want["points_to_gt_index"]))
