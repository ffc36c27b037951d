"""Run-length masks on the host (radet_amd.core.rle), the stages and datasets that accept them, and the converter that
writes them.  No device.  Every mask comparison is array_equal.  pycocotools is absent: the list form is checked against
its definition, the string form against a string decoded by hand, the polygon rasteriser against rectangles (whose pixels
follow from the rule) and against the shoelace area of convex polygons."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from radet_amd.core import rle  # noqa: E402
from _rle_cases import edge_masks  # noqa: E402


@pytest.mark.parametrize("name", ["zeros", "ones", "first", "checker", "span", "random"])
def test_list_form_round_trip(name):
    h, w = 37, 53
    m = edge_masks(h, w)[name]
    c = rle.rle_from_mask(m)
    assert c.sum() == h * w and (c[1:] > 0).all()
    np.testing.assert_array_equal(rle.mask_from_rle(c, h, w), m)
    if name == "zeros":
        assert c.tolist() == [h * w]
    if name == "ones":
        assert c.tolist() == [0, h * w]
    if name == "first":
        assert c[0] == 0 and c[1] == 1
    if name == "checker":
        assert len(c) >= h * w - w and set(c[1:-1].tolist()) <= {1, 2}            # single-pixel runs (2 where a column turns)
    if name == "span":
        assert c.max() > 3 * h                                                     # one run over several columns


def test_list_form_is_column_major():
    m = np.zeros((3, 4), np.uint8)
    m[1:, 0] = 1
    m[0, 1] = 1                      # positions 1, 2 (column 0) and 3 (column 1): one run of three
    assert rle.rle_from_mask(m).tolist() == [1, 3, 8]


def test_string_form_round_trip():
    # counts >= 2^15; a large run followed two places later by a small one (a negative difference: the sign bit);
    # differences of -16 / 15 / 16 / -17 (the 5-bit sign boundary)
    counts = np.array([0, 40000, 3, 5, 100000, 2, 1, 70000, 31, 32, 15, 16, 47, 0, 30, 1 << 20, 1, 2], np.int64)
    s = rle.string_from_counts(counts)
    assert isinstance(s, bytes) and all(48 <= b < 112 for b in s)
    np.testing.assert_array_equal(rle.counts_from_string(s), counts)
    np.testing.assert_array_equal(rle.counts_from_string(s.decode("ascii")), counts)
    assert rle.counts_from_string(b"").size == 0


def test_string_form_by_hand():
    """counts [5, 40, 3, 7, 2, 100]: stored values 5, 40, 3, 7 - 40 = -33, 2 - 3 = -1, 100 - 7 = 93.
    5   = 00101                       -> one group, sign bit clear, no more:          chr(5 + 48)            = '5'
    40  = 01000 | 00001 (low first)   -> 8 + continuation (0x20) = 40 -> chr(88) 'X'; then 1 -> chr(49)      = '1'
    3                                  -> chr(51)                                                             = '3'
    -33 = ...1011111: low 5 bits 11111 = 31, rest -2 (not -1 although bit 4 is set) -> 31 | 0x20 = 63 -> chr(111) 'o';
          -2 = ...11110: low 5 bits 30, rest -1 and bit 4 set -> stop: chr(78)                                = 'N'
    -1  = low 5 bits 31, rest -1, bit 4 set -> stop: chr(79)                                                  = 'O'
    93  = 11101 | 00010: 29 has bit 4 set and the rest (2) is not -1 -> 29 | 0x20 = 61 -> chr(109) 'm'; 2 -> '2'"""
    s = b"5X13oNOm2"
    assert rle.counts_from_string(s).tolist() == [5, 40, 3, 7, 2, 100]
    assert rle.string_from_counts([5, 40, 3, 7, 2, 100]) == s
    with pytest.raises(ValueError):
        rle.counts_from_string(b"5X")                  # ends inside a count


def _rect(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def test_polygon_rectangles():
    h, w = 37, 53
    for x0, y0, x1, y1 in [(3, 2, 10, 7), (0, 0, 53, 37), (20, 30, 21, 31), (0, 5, 9, 37), (40, 0, 53, 4)]:
        want = np.zeros((h, w), np.uint8)
        want[y0:y1, x0:x1] = 1
        parts = rle.rle_from_polygons([_rect(x0, y0, x1, y1)], h, w)
        assert len(parts) == 1 and parts[0].sum() == h * w
        np.testing.assert_array_equal(rle.mask_from_parts(parts, h, w), want, err_msg=str((x0, y0, x1, y1)))
        rev = np.asarray(_rect(x0, y0, x1, y1)).reshape(-1, 2)[::-1].reshape(-1).tolist()
        np.testing.assert_array_equal(rle.mask_from_parts(rle.rle_from_polygons([rev], h, w), h, w), want)


def test_polygon_parts_union_and_invalid_parts():
    h, w = 37, 53
    a, b = _rect(3, 2, 10, 7), _rect(8, 5, 30, 20)
    want = np.zeros((h, w), np.uint8)
    want[2:7, 3:10] = 1
    want[5:20, 8:30] = 1
    parts = rle.parts_from_segmentation([a, b, [1, 2, 3, 4], [1, 2, 3, 4, 5, 6, 7]], h, w)      # 4 values / an odd number: dropped
    assert len(parts) == 2
    np.testing.assert_array_equal(rle.mask_from_parts(parts, h, w), want)
    assert rle.parts_from_segmentation([[1, 2, 3, 4]], h, w) == []


@pytest.mark.parametrize("poly", [
    [1.3, 1.2, 30.7, 5.5, 12.2, 28.9],
    [5.5, 3.25, 47.75, 2.1, 50.2, 33.9, 2.4, 30.6],
    [10.1, 0.4, 22.6, 6.3, 27.9, 18.2, 20.4, 30.1, 8.7, 33.3, 1.2, 17.5],
    [0.49, 0.49, 52.51, 0.49, 52.51, 36.51, 0.49, 36.51],
])
def test_polygon_area(poly):
    """a rasteriser differs from the true area by no more than its boundary pixels: |pixels - area| <= perimeter + 4"""
    h, w = 37, 53
    p = np.asarray(poly).reshape(-1, 2)
    q = np.roll(p, -1, axis=0)
    area = 0.5 * abs(float((p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]).sum()))
    perimeter = float(np.hypot(*(q - p).T).sum())
    m = rle.mask_from_parts(rle.rle_from_polygons([poly], h, w), h, w)
    assert abs(int(m.sum()) - area) <= perimeter + 4, (int(m.sum()), area, perimeter)
    ys, xs = np.nonzero(m)                                       # and it lies where the polygon lies (not transposed)
    assert p[:, 0].min() - 1 <= xs.min() and xs.max() <= p[:, 0].max() + 1
    assert p[:, 1].min() - 1 <= ys.min() and ys.max() <= p[:, 1].max() + 1


def test_bad_records_raise():
    h, w = 37, 53
    with pytest.raises(ValueError):
        rle.mask_from_rle([10, 20], h, w)
    with pytest.raises(ValueError, match="img7.jpg, record 12"):
        rle.parts_from_segmentation(dict(size=[h, w], counts=[10, 20]), h, w, "img7.jpg, record 12")
    with pytest.raises(ValueError, match="record 12"):
        rle.parts_from_segmentation(dict(size=[w, h], counts=[h * w]), h, w, "img7.jpg, record 12")
    good = rle.string_from_counts([h * w - 5, 5]).decode()
    with pytest.raises(ValueError):
        rle.parts_from_segmentation(dict(size=[h, w], counts=good[:-1] + "1"), h, w)
    assert rle.parts_from_segmentation(dict(size=[h, w], counts=good), h, w)[0].tolist() == [h * w - 5, 5]
    with pytest.raises(ValueError):
        rle.pack_runs([[np.array([10, 20])]], h, w)
    with pytest.raises(ValueError):
        rle.pack_runs([[np.array([1 << 32])]], 1 << 16, 1 << 16)


def test_pack_runs_layout():
    h, w = 5, 4
    a, b, c = np.array([3, 2, 15]), np.array([20]), np.array([0, 20])
    ends, prows, mrows = rle.pack_runs([[a, b], [], [c]], h, w, [True, False, True])
    assert ends.dtype == np.uint32 and ends.tolist() == [3, 5, 20, 20, 0, 20]
    assert prows.tolist() == [[0, 3], [3, 1], [4, 2]]
    assert mrows.tolist() == [[0, 2, 5, 4, 1], [2, 0, 5, 4, 0], [2, 1, 5, 4, 1]]


# ------------------------------------------------------------------------------------------------ stages and datasets
def test_load_annotations_construction():
    from radet_amd.datasets.loading import LoadAnnotations
    st = LoadAnnotations(with_bbox=True, with_mask=True)
    assert st.with_mask and not st.with_bop_mask
    assert LoadAnnotations(with_mask=True, poly2mask=True).with_mask
    with pytest.raises(NotImplementedError):
        LoadAnnotations(with_mask=True, poly2mask=False)
    with pytest.raises(NotImplementedError):
        LoadAnnotations(with_mask=True, with_bop_mask=True)
    with pytest.raises(NotImplementedError):
        LoadAnnotations(with_seg=True)


def test_load_annotations_plans_run_lists():
    """polygons, a run list and a compressed run list in one image: plan leaves run lists, no pixels"""
    from radet_amd.datasets.loading import LoadAnnotations
    h, w = 37, 53
    m = edge_masks(h, w)["random"]
    counts = rle.rle_from_mask(m)
    segs = [[_rect(3, 2, 10, 7), _rect(8, 5, 30, 20)], dict(size=[h, w], counts=counts.tolist()),
            dict(size=[h, w], counts=rle.string_from_counts(counts).decode())]
    s = dict(img_info=dict(filename="a/rgb/000001.jpg", height=h, width=w), bbox_fields=[], mask_fields=[],
             ann_info=dict(bboxes=np.zeros((3, 4), np.float32), labels=np.zeros(3, np.int64), masks=segs, ann_ids=[4, 5, 6]))
    LoadAnnotations(with_mask=True).plan(s, None, None)
    parts, hw = s["gt_masks_rle"]
    assert hw == (h, w) and [len(p) for p in parts] == [2, 1, 1] and "gt_masks" not in s and s["mask_fields"] == ["gt_masks"]
    assert all(isinstance(c, np.ndarray) and c.dtype.kind == "i" for p in parts for c in p)
    np.testing.assert_array_equal(rle.mask_from_parts(parts[1], h, w), m)
    np.testing.assert_array_equal(rle.mask_from_parts(parts[2], h, w), m)
    s["ann_info"]["masks"][1] = dict(size=[h, w], counts=[1, 2, 3])
    s["mask_fields"] = []
    with pytest.raises(ValueError, match="a/rgb/000001.jpg, record 5"):
        LoadAnnotations(with_mask=True).plan(s, None, None)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL writes and reads the generated JPEG / PNG files")
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=3, objects=(2, 4), n_backgrounds=1, seed=5)


def _thresholded(path):
    from PIL import Image
    m = np.asarray(Image.open(path))
    return ((m == m.max()) & (m.max() != 0)).astype(np.uint8)


@pytest.mark.parametrize("form", ["rle", "rle-string"])
def test_bop_to_coco_writes_the_masks(tree, form):
    from radet_amd.datasets.bop_convert import add_segmentation, bop_to_coco
    coco = bop_to_coco(tree["img_prefix"], tree["image_list"], "ycbv", segmentation=form)
    plain = bop_to_coco(tree["img_prefix"], tree["image_list"], "ycbv")
    assert len(coco["annotations"]) == len(plain["annotations"]) > 0 and "segmentation" not in plain["annotations"][0]
    coco = json.loads(json.dumps(coco))                                       # what a file holds
    names = {im["id"]: im["file_name"] for im in coco["images"]}
    seen = {}
    for a, b in zip(coco["annotations"], plain["annotations"]):
        assert {k: v for k, v in a.items() if k != "segmentation"} == b
        k = seen[a["image_id"]] = seen.get(a["image_id"], -1) + 1
        frame = int(os.path.splitext(os.path.basename(names[a["image_id"]]))[0])
        png = os.path.join(tree["seg_prefix"], "000000", "mask_visib", f"{frame:06d}_{k:06d}.png")
        seg = a["segmentation"]
        assert seg["size"] == [480, 640] and isinstance(seg["counts"], list if form == "rle" else str)
        np.testing.assert_array_equal(rle.mask_from_parts(rle.parts_from_segmentation(seg, 480, 640), 480, 640), _thresholded(png))
    # the same records added to the tree's own annotation file
    own = add_segmentation(json.load(open(tree["ann_file"])), tree["seg_prefix"], form)
    assert [a["segmentation"] for a in own["annotations"]] == [a["segmentation"] for a in coco["annotations"]]
    with pytest.raises(ValueError):
        bop_to_coco(tree["img_prefix"], tree["image_list"], "ycbv", segmentation="polygon")


def test_datasets_take_masks_from_the_annotations(tree, tmp_path):
    from radet_amd.datasets import BOPDataset, CocoDataset, build_dataset
    from radet_amd.datasets.bop_convert import add_segmentation
    from tools.synth_bop import YCBV_NAMES
    coco = add_segmentation(json.load(open(tree["ann_file"])), tree["seg_prefix"], "rle")
    coco["annotations"][0]["iscrowd"] = 1
    ann = str(tmp_path / "rle.json")
    json.dump(coco, open(ann, "w"))
    ds = build_dataset(dict(type="CocoDataset", ann_file=ann, img_prefix=tree["img_prefix"], classes=YCBV_NAMES, pipeline=[]))
    assert isinstance(ds, CocoDataset) and len(ds) == 3
    files = BOPDataset(tree["ann_file"], pipeline=[])
    a, f = ds.get_ann_info(0), files.get_ann_info(0)
    n = len(f["bboxes"])
    assert len(a["bboxes"]) == n - 1 and len(a["bboxes_ignore"]) == 1 and len(a["masks"]) == n - 1      # the crowd record
    np.testing.assert_array_equal(a["bboxes"], f["bboxes"][1:])
    np.testing.assert_array_equal(a["bboxes_ignore"], f["bboxes"][:1])
    assert all(isinstance(m, dict) and m["size"] == [480, 640] for m in a["masks"])
    b = BOPDataset(ann, pipeline=[], mask_source="annotation", min_visib_frac=0.5).get_ann_info(0)      # keeps its visibility rule
    v = BOPDataset(tree["ann_file"], pipeline=[], min_visib_frac=0.5).get_ann_info(0)
    np.testing.assert_array_equal(b["bboxes"], v["bboxes"])
    np.testing.assert_array_equal(b["bboxes_ignore"], v["bboxes_ignore"])
    assert len(b["masks"]) == len(v["masks"]) and all(isinstance(m, dict) for m in b["masks"])
    for seg, path in zip(b["masks"], v["masks"]):
        np.testing.assert_array_equal(rle.mask_from_parts(rle.parts_from_segmentation(seg, 480, 640), 480, 640),
                                      _thresholded(os.path.join(tree["seg_prefix"], path)))
    with pytest.raises(ValueError):
        BOPDataset(ann, pipeline=[], mask_source="polygons")
    # CocoDataset needs no BOP file layout and no visib_fract
    for im in coco["images"]:
        im["file_name"] = os.path.basename(im["file_name"])
    for r in coco["annotations"]:
        del r["visib_fract"]
    json.dump(coco, open(ann, "w"))
    flat = CocoDataset(ann, pipeline=[], classes=YCBV_NAMES)
    assert len(flat.get_ann_info(1)["masks"]) == len(files.get_ann_info(1)["masks"])
