"""Masks from run-length / polygon annotations on the GPU: radet_rle_masks against the bitmap path's own kernels
(radet_mask_max + radet_mask_transform on the decoded bitmaps) and against oracle/masks.py, and the image pipeline fed
from RLE-annotated files against the same pipeline fed from the visible-mask PNGs.  Every comparison is array_equal /
torch.equal."""
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import masks as om  # noqa: E402
from _maskfree_pipelines import train_pipeline  # noqa: E402
from _rle_cases import edge_masks  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def blobs(h, w, n, seed):
    """n random masks: unions of a few ellipses"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for _ in range(n):
        m = np.zeros((h, w), bool)
        for _ in range(rs.randint(1, 4)):
            cy, cx, ry, rx = rs.uniform(0, h), rs.uniform(0, w), rs.uniform(2, h / 2), rs.uniform(2, w / 2)
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        out.append(m.astype(np.uint8))
    return out


@pytest.fixture(scope="module")
def stacks():
    """(h, w) -> u8 [G, h, w] of 0 / 1: five blobs plus the codec's edge cases; computed once, never written to"""
    out = {}
    for h, w in ((37, 53), (96, 128)):
        out[(h, w)] = np.stack(blobs(h, w, 5, h) + list(edge_masks(h, w).values()))
        out[(h, w)].setflags(write=False)
    return out


def _from_rle(masks, **kw):
    from radet_amd.core import rle
    from radet_amd.core.mask import BitmapMasks
    h, w = masks.shape[1:]
    return BitmapMasks.from_rle([[rle.rle_from_mask(m)] for m in masks], h, w, **kw).masks


# what happens to a mask on its way to the assigner, and more: (source size, transform arguments)
CASES = [
    ((37, 53), dict()),                                                                   # identity
    ((96, 128), dict()),
    ((96, 128), dict(resized_hw=(72, 96))),                                               # downscale
    ((37, 53), dict(resized_hw=(61, 80))),                                                # upscale
    ((37, 53), dict(flip="horizontal")),
    ((96, 128), dict(resized_hw=(72, 96), flip="horizontal")),
    ((37, 53), dict(resized_hw=(61, 80), flip="horizontal", out_hw=(64, 80))),            # pad to a multiple of 16
    ((96, 128), dict(resized_hw=(72, 96), out_hw=(80, 96), pad_val=7)),
    ((37, 53), dict(resized_hw=(61, 77), flip="horizontal")),                             # width % 4 != 0
    ((96, 128), dict(resized_hw=(50, 1030), out_hw=(50, 1031))),                          # more words than a workgroup has threads
]


def test_rle_masks_equals_mask_transform(stacks):
    """one call sequence over both source sizes and G = 1, 5, all, 0"""
    from radet_amd import kernels as K
    for (h, w), kw in CASES:
        full = stacks[(h, w)]
        for G in (1, 5, len(full), 0):
            m = full[:G]
            got = _from_rle(m, **kw)
            src = torch.from_numpy(np.ascontiguousarray(m * 255)).to(_dev())
            want = K.mask_transform(src, kw.get("out_hw"), kw.get("resized_hw"), kw.get("flip"), kw.get("pad_val", 0), normalize=True)
            assert got.shape == want.shape and got.dtype == torch.uint8
            assert torch.equal(got, want), f"{(h, w)} {kw} G={G}"
            host = om.transform(m, resized_hw=kw.get("resized_hw"), flip_dir=kw.get("flip"), out_hw=kw.get("out_hw"),
                                pad_val=kw.get("pad_val", 0))
            np.testing.assert_array_equal(got.cpu().numpy().reshape(host.shape), host, err_msg=f"{(h, w)} {kw} G={G}")


def test_both_orientations_from_one_launch(stacks):
    """flip flags per mask and the second output: the flagged masks mirrored in the first result, unflipped in the second"""
    from radet_amd import _lib, kernels as K
    from radet_amd.core import rle
    m = stacks[(37, 53)]
    flips = np.arange(len(m)) % 2 == 1
    ends, prows, mrows = rle.pack_runs([[rle.rle_from_mask(x)] for x in m], 37, 53, flips)
    dev = _dev()
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        out, plain = K.rle_masks(torch.from_numpy(ends.view(np.int32)).to(dev), torch.from_numpy(prows).to(dev),
                                 torch.from_numpy(mrows).to(dev), (64, 77), resized_hw=(61, 77), with_plain=True)
    finally:
        _lib.call = call
    assert seen == ["radet_rle_masks"]
    res = om.transform(m, resized_hw=(61, 77), out_hw=(64, 77))
    fl = om.transform(m, resized_hw=(61, 77), flip_dir="horizontal", out_hw=(64, 77))
    np.testing.assert_array_equal(out.cpu().numpy(), np.where(flips[:, None, None], fl, res))
    np.testing.assert_array_equal(plain.cpu().numpy()[flips], res[flips])


def test_parts_are_united(stacks):
    from radet_amd.core import rle
    from radet_amd.core.mask import BitmapMasks
    a, b, c = (rle.rle_from_mask(m) for m in stacks[(37, 53)][:3])
    kw = dict(resized_hw=(61, 80), flip="horizontal", out_hw=(64, 80))
    single = BitmapMasks.from_rle([[a], [b], [c]], 37, 53, **kw).masks
    # next to a mask without parts (all polygons invalid) and a mask of two parts
    both = BitmapMasks.from_rle([[a, b, c], [], [c, a]], 37, 53, **kw).masks
    assert torch.equal(both[0], single[0] | single[1] | single[2])
    assert torch.equal(both[2], single[0] | single[2])
    assert int(both[1, :61].sum()) == 0


def test_many_runs_next_to_one_run():
    """a one-pixel checkerboard (1961 runs) and an empty mask (one run) in one launch"""
    from radet_amd.core import rle
    h, w = 37, 53
    e = edge_masks(h, w)
    m = np.stack([e["checker"], e["zeros"], e["ones"], e["checker"]])
    runs = [rle.rle_from_mask(x) for x in m]
    assert len(runs[0]) > 1900 and len(runs[1]) == 1
    for kw in (dict(), dict(resized_hw=(61, 80), flip="horizontal"), dict(resized_hw=(20, 31))):
        np.testing.assert_array_equal(_from_rle(m, **kw).cpu().numpy(),
                                      om.transform(m, resized_hw=kw.get("resized_hw"), flip_dir=kw.get("flip")))


def test_polygons_decode_on_the_device():
    from radet_amd.core import rle
    from radet_amd.core.mask import BitmapMasks
    h, w = 37, 53
    segs = [[[3, 2, 10, 2, 10, 7, 3, 7], [8, 5, 30, 5, 30, 20, 8, 20]], [[1.3, 1.2, 30.7, 5.5, 12.2, 28.9]]]
    parts = [rle.parts_from_segmentation(s, h, w) for s in segs]
    host = np.stack([rle.mask_from_parts(p, h, w) for p in parts])
    assert host[0, 2:7, 3:10].all() and host[0, 5:20, 8:30].all() and host[0].sum() == 5 * 7 + 15 * 22 - 2 * 2
    got = BitmapMasks.from_rle(parts, h, w, resized_hw=(61, 80)).masks.cpu().numpy()
    np.testing.assert_array_equal(got, om.transform(host, resized_hw=(61, 80)))


# ------------------------------------------------------------------------------------------------ the pipeline
SEED = 5


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """one tree, annotated three times: mask PNG paths, run lists, compressed run lists"""
    pytest.importorskip("PIL", reason="PIL decodes the generated JPEG / PNG files")
    from PIL import Image
    from radet_amd.datasets.bop_convert import add_segmentation
    from tools.synth_bop import write_tree
    root = str(tmp_path_factory.mktemp("bop"))
    # six frames of two sizes, frame 4 without objects
    t = write_tree(root, n_frames=6, objects=(3, 6), n_backgrounds=3, seed=17, sizes=[(640, 480), (600, 480)], empty_frames=(4,))
    # (the PNG path's mask / max is undefined for an empty mask and not under test: this seed writes none)
    pngs = sorted(os.listdir(os.path.join(t["seg_prefix"], "000000", "mask_visib")))
    assert pngs and all(np.asarray(Image.open(os.path.join(t["seg_prefix"], "000000", "mask_visib", p))).max() == 255 for p in pngs)
    coco = json.load(open(t["ann_file"]))
    for form in ("rle", "rle-string"):
        t[form] = os.path.join(root, f"train_pbr_{form}.json")
        json.dump(add_segmentation(coco, t["seg_prefix"], form), open(t[form], "w"))
    return t


def _dataset(tree, style, mix, kind="BOPDataset"):
    from radet_amd.datasets import build_dataset
    from tools.synth_bop import YCBV_NAMES
    pipe = train_pipeline(tree["background_dir"], "mask", mix=mix, bg_prob=0.5)
    cfg = dict(type=kind, img_prefix=tree["img_prefix"], filter_empty_gt=False, classes=YCBV_NAMES)
    if style == "png":
        return build_dataset(dict(cfg, ann_file=tree["ann_file"], seg_prefix=tree["seg_prefix"], pipeline=pipe))
    assert pipe[1]["type"] == "LoadAnnotations"
    pipe[1] = dict(type="LoadAnnotations", with_bbox=True, with_mask=True)
    if kind == "BOPDataset":
        cfg["mask_source"] = "annotation"
    return build_dataset(dict(cfg, ann_file=tree[style], pipeline=pipe))


KEYS = ("img", "gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight")


def _run(ds, no_sync_masks=False):
    from radet_amd.datasets.loader import sample_generators
    gens = [sample_generators(SEED, 0, i) for i in range(len(ds))]
    planned = [ds.plan_sample(i, *gens[i]) for i in range(len(ds))]
    pipe, calls = ds.pipeline, []
    if no_sync_masks:
        # the mask stage may not wait for the device: it runs with synchronising calls made an error
        inner = pipe._masks

        def no_sync(*a, **k):
            torch.cuda.set_sync_debug_mode("error")
            try:
                out = inner(*a, **k)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            calls.append(sum(len(m) for m in out[0] if m is not None))
            return out
        pipe._masks = no_sync
    try:
        out = pipe.run(planned)
    finally:
        if no_sync_masks:
            del pipe._masks
    return out, gens, planned, calls


@pytest.fixture(scope="module")
def png_runs(tree):
    return {mix: _run(_dataset(tree, "png", mix)) for mix in (False, True)}


@pytest.mark.parametrize("mix", [False, True], ids=["pbr", "mix"])
@pytest.mark.parametrize("style,kind", [("rle", "BOPDataset"), ("rle-string", "BOPDataset"), ("rle", "CocoDataset")])
def test_pipeline_equals_png_annotations(tree, png_runs, style, kind, mix):
    ref, ref_gens, ref_planned, _ = png_runs[mix]
    ds = _dataset(tree, style, mix, kind)
    assert len(ds) == 6
    out, gens, planned, calls = _run(ds, no_sync_masks=True)
    assert all("gt_masks_rle" in s and "gt_masks" not in s for s in planned)
    assert calls == [sum(len(s["gt_bboxes"]) for s in planned)]
    for i in range(6):
        for k in KEYS:
            assert torch.equal(out[i][k], ref[i][k]), f"sample {i}: {k}"
        assert gens[i][0].getstate() == ref_gens[i][0].getstate(), f"sample {i}: random.Random position"
        for a, b in zip(gens[i][1].get_state(), ref_gens[i][1].get_state()):
            assert np.array_equal(a, b), f"sample {i}: RandomState position"
    # the batch covers: both sizes, flipped and not, merged under the masks and not, a sample without objects
    assert len({tuple(s["resize_hw"]) for s in planned}) == 2 and {bool(s["flip"]) for s in planned} == {True, False}
    assert any("background" in s and len(s["gt_bboxes"]) and s["flip"] for s in planned)
    assert any("background" in s and len(s["gt_bboxes"]) and not s["flip"] for s in planned)
    assert [len(s["gt_bboxes"]) for s in planned].count(0) == 1
    assert max(int((o["points_to_gt_index"] > 0).sum()) for o in out) > 10


def test_launches(tree):
    """an RLE batch: one radet_rle_masks per size group and none of the bitmap path's launches; a PNG batch: the launches
    it issued before; a mixed batch (two annotation styles) equals the PNG batch"""
    from radet_amd import _lib
    from radet_amd.datasets.loader import sample_generators
    seen, call = [], _lib.call

    def spy(name, *a):
        seen.append(name)
        return call(name, *a)
    ds = {s: _dataset(tree, s, False) for s in ("png", "rle")}
    plans = {s: [d.plan_sample(i, *sample_generators(SEED, 0, i)) for i in range(6)] for s, d in ds.items()}
    mixed = [plans["rle" if i % 2 else "png"][i] for i in range(6)]
    _lib.call = spy
    try:
        ref = ds["png"].pipeline.run([dict(s, _nprnd=_copy(s["_nprnd"])) for s in plans["png"]])
        png_seen = [n for n in seen if "mask" in n]
        del seen[:]
        ds["rle"].pipeline.run([dict(s, _nprnd=_copy(s["_nprnd"])) for s in plans["rle"]])
        rle_seen = [n for n in seen if "mask" in n]
        del seen[:]
        out = ds["png"].pipeline.run([dict(s, _nprnd=_copy(s["_nprnd"])) for s in mixed])
    finally:
        _lib.call = call
    groups = len({tuple(s["resize_hw"]) for s in plans["png"] if len(s["gt_bboxes"])})
    assert groups == 2 and rle_seen == ["radet_rle_masks"] * groups
    assert set(png_seen) == {"radet_mask_max", "radet_mask_transform"} and png_seen.count("radet_mask_max") == groups
    assert "radet_rle_masks" in seen and "radet_mask_transform" in seen
    for i in range(6):
        for k in KEYS:
            assert torch.equal(out[i][k], ref[i][k]), f"sample {i}: {k}"


def _copy(rs):
    import copy
    return copy.deepcopy(rs)


@pytest.fixture(scope="module")
def tiny_tree(tmp_path_factory):
    """four frames of one size that all hold objects, as a training run needs them (the assigner's points follow the image
    shape, the head's the padded batch: they agree for 640 x 480), annotated with PNG paths and with run lists"""
    pytest.importorskip("PIL", reason="PIL decodes the generated JPEG / PNG files")
    from radet_amd.datasets.bop_convert import add_segmentation
    from tools.synth_bop import write_tree
    root = str(tmp_path_factory.mktemp("tiny"))
    t = write_tree(root, n_frames=4, objects=(2, 4), n_backgrounds=1, seed=23)
    t["rle"] = os.path.join(root, "train_pbr_rle.json")
    json.dump(add_segmentation(json.load(open(t["ann_file"])), t["seg_prefix"], "rle"), open(t["rle"], "w"))
    return t


def test_train_steps_equal_png_loader(tiny_tree):
    """two steps of train_detector from the RLE-annotated loader: the losses of the PNG-annotated loader, bit for bit"""
    tree = tiny_tree
    from radet_amd.apis import train_detector
    from radet_amd.datasets import build_dataloader
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill

    def run(style):
        cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
        cfg.model["pretrained"] = None
        cfg.merge_from_dict({"lr_config.total_steps": 40, "log_config.interval": 1})
        torch.manual_seed(0)
        det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda()
        synth_fill(det, seed=0)
        loader = build_dataloader(_dataset(tree, style, False), samples_per_gpu=4, workers=4, seed=0)

        def batches():
            epoch = 0
            while True:
                loader.set_epoch(epoch)
                yield from loader
                epoch += 1
        try:
            return train_detector(det, batches(), cfg, max_iters=2, log=lambda *_: None)
        finally:
            loader.close()
    a, b = run("png"), run("rle")
    assert len(a) == len(b) == 2 and np.isfinite(a).all() and a == b


def test_symbol_is_exported():
    from radet_amd import _lib
    assert hasattr(_lib.load(), "radet_rle_masks") and "radet_rle_masks" in _lib.SIGNATURES
