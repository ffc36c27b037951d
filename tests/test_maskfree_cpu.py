"""Host side of the mask-free sampler inside an image pipeline (GenerateDistanceMap(with_gt_mask=False), reference
loading.py:586-645): the pipeline is accepted, the factored crop geometry equals the reference's per-box loop, and planning
draws the fill colours where the reference's random.randint calls fall."""
import math
import os
import random
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _maskfree_pipelines import DM, boxes_on_borders as _boxes, train_pipeline  # noqa: E402


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL writes and decodes the generated JPEG / PNG files")
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=4, objects=(3, 6), n_backgrounds=2, seed=3)


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("dm", ["gdt", "mbd"])
def test_image_pipeline_accepts_mask_free_sampler(tree, dm, mix):
    from radet_amd.datasets.loading import ImagePipeline
    pipe = ImagePipeline(train_pipeline(tree["background_dir"], dm, mix=mix))
    assert pipe.mask_free is not None and not pipe.mask_free.with_gt_mask
    assert ImagePipeline(train_pipeline(tree["background_dir"], "mask", mix=mix)).mask_free is None


def test_image_pipeline_refuses_host_edge_callbacks(tree):
    from radet_amd.datasets.loading import ImagePipeline
    cfg = train_pipeline(tree["background_dir"], "gdt")
    at = cfg.index(DM["gdt"])
    cfg[at] = dict(type="GenerateDistanceMap", with_gt_mask=False, distance_transform="gdt")
    with pytest.raises(NotImplementedError):            # the reference default edge_mode='sed' needs cv2.ximgproc's model
        ImagePipeline(cfg)
    cfg[at] = dict(cfg[at], extract_edge_func=lambda im: np.zeros(im.shape[:2], np.float32))
    with pytest.raises(NotImplementedError):            # a host callback cannot run inside the device pipeline
        ImagePipeline(cfg)


def reference_loop(gt_bboxes, img_h, img_w, pad_ratio, small_object_size, rnd):
    """loading.py:595-634 restated box by box: (maskenable, per box (canvas h, w, fill, box_img rect, refined rect), regions)"""
    areas = (gt_bboxes[:, 2] - gt_bboxes[:, 0] + 1) * (gt_bboxes[:, 3] - gt_bboxes[:, 1] + 1)
    maskenable = areas > small_object_size
    bak = gt_bboxes.copy().astype(np.int_)
    region = np.zeros_like(bak)
    per_box = []
    for i, xyxy in enumerate(bak):
        pad_x = math.ceil((xyxy[2] - xyxy[0]) * pad_ratio)
        pad_y = math.ceil((xyxy[3] - xyxy[1]) * pad_ratio)
        bh, bw = xyxy[3] - xyxy[1] + 2 * pad_y, xyxy[2] - xyxy[0] + 2 * pad_x
        colour = [rnd.randint(0, 255) for _ in range(3)]
        o = xyxy.copy()
        xyxy += np.array([-pad_x, -pad_y, pad_x, pad_y], dtype=xyxy.dtype)
        rx1, ry1 = np.clip(xyxy[0], 0, img_w - 1), np.clip(xyxy[1], 0, img_h - 1)
        rx2, ry2 = np.clip(xyxy[2], 0, img_w - 1), np.clip(xyxy[3], 0, img_h - 1)
        bx1, by1 = rx1 - xyxy[0], ry1 - xyxy[1]
        bx2, by2 = bw - (xyxy[-2] - rx2), bh - (xyxy[-1] - ry2)
        region[i] = [o[0] - xyxy[0], o[1] - xyxy[1], bw - (xyxy[2] - o[2]), bh - (xyxy[-1] - o[-1])]
        per_box.append((bh, bw, colour, (bx1, by1, bx2, by2), (rx1, ry1, rx2, ry2), (xyxy[0], xyxy[1])))
    return maskenable, per_box, region


@pytest.mark.parametrize("H,W,pad_ratio", [(480, 640, 0.05), (333, 517, 0.05), (480, 600, 0.2)])
def test_crop_geometry_equals_reference_loop(H, W, pad_ratio):
    from radet_amd.datasets.pipelines import crop_geometry, draw_fill_colours
    rs = np.random.RandomState(H)
    boxes = _boxes(rs, H, W, 40)
    g = crop_geometry(boxes, (H, W), pad_ratio, 32 ** 2)
    fill = draw_fill_colours(random.Random(9), len(boxes))
    enable, per_box, region = reference_loop(boxes, H, W, pad_ratio, 32 ** 2, random.Random(9))
    assert np.array_equal(g.large, enable) and not enable.all() and enable.any()
    assert np.array_equal(g.regions, region)
    assert np.array_equal(g.corners, boxes.astype(np.int_))
    for k, (bh, bw, colour, dst, src, win) in enumerate(per_box):
        assert tuple(g.canvas_wh[k]) == (bw, bh)
        assert fill[k].tolist() == colour
        assert (*g.dst_lo[k], *g.dst_hi[k]) == dst
        assert (*g.src_lo[k], *g.src_hi[k]) == src
        assert tuple(g.win_lo[k]) == win
    # windows leave the image on every side somewhere, and on two sides at once in the corners
    assert (g.win_lo < 0).any(axis=0).all() and (g.win_lo.min(axis=1) < 0).any()
    assert ((g.win_lo[:, 0] < 0) & (g.win_lo[:, 1] < 0)).any()


def test_crop_boxes_uses_the_shared_geometry():
    """GenerateDistanceMap.crop_boxes (the host path) == the reference loop, canvases included"""
    pytest.importorskip("torch")
    from radet_amd.datasets.pipelines import GenerateDistanceMap
    H, W = 240, 320
    rs = np.random.RandomState(1)
    img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    boxes = _boxes(rs, H, W, 10)
    gdm = GenerateDistanceMap(with_gt_mask=False, distance_transform="mbd")
    random.seed(4)
    canvases, large, regions = gdm.crop_boxes(img, (H, W), boxes)
    state = random.getstate()
    enable, per_box, region = reference_loop(boxes, H, W, gdm.pad_ratio, gdm.small_object_size, random.Random(4))
    assert np.array_equal(large, enable) and np.array_equal(regions, region)
    for c, (bh, bw, colour, dst, src, _) in zip(canvases, per_box):
        ref = np.zeros((bh, bw, 3), np.uint8)
        ref[:, :, :] = colour
        ref[dst[1]:dst[3], dst[0]:dst[2]] = img[src[1]:src[3], src[0]:src[2]]
        assert np.array_equal(c, ref)
    r = random.Random(4)
    [r.randint(0, 255) for _ in range(3 * len(boxes))]
    assert state == r.getstate()


@pytest.mark.parametrize("mix", [False, True])
def test_plan_draws_fill_colours_after_the_flip(tree, mix):
    """after planning, the sample's random.Random stands where the same stages followed by 3 * G randint(0, 255) leave
    it, the fill colours are those draws, and the RandomState is where the mask pipeline leaves it"""
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators

    def ds(dm):
        return build_dataset(dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"],
                                  seg_prefix=tree["seg_prefix"], pipeline=train_pipeline(tree["background_dir"], dm, mix=mix)))
    free, mask = ds("gdt"), ds("mask")
    for i in range(len(free)):
        rnd, nprnd = sample_generators(7, 0, i)
        s = free.plan_sample(i, rnd, nprnd)
        rnd2, nprnd2 = sample_generators(7, 0, i)
        s2 = mask.plan_sample(i, rnd2, nprnd2)                 # the same stages without the fill colours
        G = len(s["gt_bboxes"])
        assert G > 0 and "_crop_plan" not in s2
        by_hand = [rnd2.randint(0, 255) for _ in range(3 * G)]
        assert rnd.getstate() == rnd2.getstate()
        geom, fill = s["_crop_plan"]
        assert fill.reshape(-1).tolist() == by_hand and fill.dtype == np.uint8
        for a, b in zip(nprnd.get_state(), nprnd2.get_state()):
            assert np.array_equal(a, b)
        # the geometry is that of the resized / flipped boxes
        assert np.array_equal(s["gt_bboxes"], s2["gt_bboxes"]) and s["flip"] == s2["flip"]
        assert np.array_equal(geom.corners, s["gt_bboxes"].astype(np.int_))


def test_descriptor_widths_match_the_header():
    """kernels.CROP_DESC_INTS / PASTE_DESC_INTS restate the header's defines"""
    import re
    from radet_amd import kernels as K
    hdr = open(os.path.join(REPO, "include", "radet_hip.h")).read()
    for name in ("CROP_DESC_INTS", "PASTE_DESC_INTS"):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == getattr(K, name)
