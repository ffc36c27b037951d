"""CutOut, host side: the planning against the reference's stage run under the same seeds and the NumPy restatement
(tests/_cutout_ref.py) against the reference's own output images (tests/golden/cutout_aug.npz, made by
tests/golden/gen_cutout_aug.py), bare and inside AutoAugment policies; the argument checks, the refusals, the places the
stage may stand in, and the cutout configs."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _cutout_ref as C  # noqa: E402
from _jitter_cfg import jitter_train_cfg  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden", "cutout_aug.npz")
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def _args(d):
    """the stage arguments as they were before JSON: {"tuple": [...]} / {"list": [[...], ...]} candidates, tuple for the rest"""
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            v = tuple(v["tuple"]) if "tuple" in v else [tuple(c) for c in v["list"]]
        elif isinstance(v, list):
            v = tuple(v)
        out[k] = v
    return out


def _candidates(args):
    with_ratio = args.get("cutout_ratio") is not None
    cand = args["cutout_ratio"] if with_ratio else args["cutout_shape"]
    return (cand if isinstance(cand, list) else [cand]), with_ratio


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    g["cases"] = [_args(a) for a in json.loads(str(g["cases"]))]
    g["policies"] = [[_args(t) for t in p] for p in json.loads(str(g["policies"]))]
    return g


def _sample_image(g):
    """the generator's image: RandomState(1).randint(0, 256, (H, W, 3)) (tests/golden/gen_scale_jitter.py: sample)"""
    H, W = (int(v) for v in g["src_hw"])
    return np.random.RandomState(1).randint(0, 256, (H, W, 3)).astype(np.uint8)


def _bare_rows(g):
    """per recorded bare run: (row, args, draws)"""
    o = 0
    for n in range(len(g["seed"])):
        nd = int(g["n_draws"][n])
        yield n, g["cases"][g["case"][n]], g["draws"][o:o + nd]
        o += nd
    assert o == len(g["draws"])


def test_fixture_holds_the_edge_cases(gold):
    g = gold
    H, W = (int(v) for v in g["src_hw"])
    img = _sample_image(g)
    assert g["images"].shape == (len(g["seed"]), H, W, 3) and g["images"].dtype == np.uint8
    cases = g["cases"]
    assert any(isinstance(c.get("cutout_shape"), tuple) for c in cases) and any(isinstance(c.get("cutout_shape"), list) for c in cases)
    assert any(isinstance(c.get("cutout_ratio"), tuple) for c in cases) and any(isinstance(c.get("cutout_ratio"), list) for c in cases)
    assert any(isinstance(c["n_holes"], int) for c in cases) and any(isinstance(c["n_holes"], tuple) and c["n_holes"][0] == 0 for c in cases)
    seen = dict(none=0, right=0, bottom=0, zero_area=0, several=0, changed=0, second=0)
    for n, args, draws in _bare_rows(g):
        cand, with_ratio = _candidates(args)
        rects = C.holes_from_draws(draws, cand, with_ratio, H, W)
        seen["none"] += len(rects) == 0
        seen["several"] += len(rects) > 1
        seen["second"] += any(int(d) > 0 for d in draws[3::3])
        seen["changed"] += not np.array_equal(g["images"][n], img)
        for k, (x1, y1, x2, y2) in enumerate(rects):
            cw, ch = cand[int(draws[3 + 3 * k])]
            cw, ch = (int(cw * W), int(ch * H)) if with_ratio else (cw, ch)
            seen["right"] += x1 + cw > W and x2 == W
            seen["bottom"] += y1 + ch > H and y2 == H
            seen["zero_area"] += with_ratio and cw == 0 and x2 == x1
        if len(rects) == 0:
            assert np.array_equal(g["images"][n], img)
    assert all(seen.values()), seen
    # AutoAugment: every policy drawn, a hole before and after a warp, holes alone, a warp alone, nothing at all
    assert set(g["auto_policy"]) == set(range(len(g["policies"])))
    orders = set(str(v) for v in g["auto_order"])
    assert {"cw", "wc", "c", "w", ""} <= orders, orders


def test_restatement_reproduces_the_reference_images(gold):
    g = gold
    H, W = (int(v) for v in g["src_hw"])
    img = _sample_image(g)
    for n, args, draws in _bare_rows(g):
        cand, with_ratio = _candidates(args)
        rects = C.holes_from_draws(draws, cand, with_ratio, H, W)
        got = C.apply_holes(img, rects, np.array(args.get("fill_in", (0, 0, 0)), np.uint8))
        assert np.array_equal(got, g["images"][n]), f"row {n}: {args}"


@pytest.mark.parametrize("late", [False, True])
def test_planning_reproduces_the_reference(gold, late):
    from radet_amd.datasets.loading import CutOut
    g = gold
    H, W = (int(v) for v in g["src_hw"])
    img = _sample_image(g)
    for n, args, draws in _bare_rows(g):
        what = f"row {n}: {args} seed {g['seed'][n]}"
        rs = np.random.RandomState(int(g["seed"][n]))
        boxes = g["boxes"].copy()
        s = dict(img_shape=(H, W, 3), bbox_fields=["gt_bboxes"], gt_bboxes=boxes.copy(), gt_labels=g["labels"].copy())
        stage = CutOut(**args)
        stage.late = late
        stage.plan(s, None, rs)
        assert rs.random_sample() == g["next"][n], what                # the generator stands where the reference's does
        cand, with_ratio = _candidates(args)
        want = C.holes_from_draws(draws, cand, with_ratio, H, W)
        assert np.array_equal(s["gt_bboxes"], boxes) and np.array_equal(s["gt_labels"], g["labels"]), what
        if not len(want):
            assert not any(k in s for k in ("cutout", "block_ops", "cutout_late")), what
            continue
        if late:
            rects, fill = s["cutout_late"]
            assert "cutout" not in s and "block_ops" not in s
        else:
            (rects, fill), = s["cutout"]
            assert s["block_ops"] == [("cutout", 0)] and "affine" not in s and "cutout_late" not in s, what
        assert rects.dtype == np.int32 and np.array_equal(rects, want), what
        assert fill == tuple(args.get("fill_in", (0, 0, 0))), what
        # and the planned holes give the reference's pixels
        assert np.array_equal(C.apply_holes(img, rects, np.array(fill, np.uint8)), g["images"][n]), what


def test_autoaugment_planning_reproduces_the_reference(gold):
    from radet_amd.datasets.loading import AutoAugment
    g = gold
    H, W = (int(v) for v in g["src_hw"])
    stage = AutoAugment(policies=[[dict(t) for t in p] for p in g["policies"]])
    oc = od = om = ob = 0
    for n in range(len(g["auto_seed"])):
        what = f"seed {g['auto_seed'][n]}"
        rs = np.random.RandomState(int(g["auto_seed"][n]))
        s = dict(img_shape=(H, W, 3), bbox_fields=["gt_bboxes_ignore", "gt_bboxes"], gt_bboxes=g["boxes"].copy(),
                 gt_bboxes_ignore=g["ignore"].copy(), gt_labels=g["labels"].copy())
        stage.plan(s, None, rs)
        assert rs.random_sample() == g["auto_next"][n], what
        assert s["policy"] == g["auto_policy"][n], what
        policy = g["policies"][s["policy"]]
        cut_args = [t for t in policy if t["type"] == "CutOut"]
        want_holes = []
        for k in range(int(g["auto_n_cutouts"][n])):
            nd = int(g["auto_n_draws"][oc + k])
            cand, with_ratio = _candidates(cut_args[k])
            rects = C.holes_from_draws(g["auto_draws"][od:od + nd], cand, with_ratio, H, W)
            if len(rects):
                want_holes.append((rects, tuple(cut_args[k].get("fill_in", (0, 0, 0)))))
            od += nd
        oc += int(g["auto_n_cutouts"][n])
        nw = int(g["auto_n_warps"][n])
        order = str(g["auto_order"][n])
        # the entries in the order the reference ran them; s["affine"] holds the warps only, as before
        ops = s.get("block_ops", [("warp", k) for k in range(len(s.get("affine", ())))])
        assert "".join(kind[0] for kind, _ in ops) == order, what
        assert [k for kind, k in ops if kind == "warp"] == list(range(nw)) == list(range(len(s.get("affine", ())))), what
        assert [k for kind, k in ops if kind == "cutout"] == list(range(len(want_holes))) == list(range(len(s.get("cutout", ())))), what
        assert ("block_ops" in s) == ("c" in order), what
        for (rects, fill), (want, want_fill) in zip(s.get("cutout", ()), want_holes):
            assert np.array_equal(rects, want) and fill == want_fill, what
        for k in range(nw):
            assert np.array_equal(s["affine"][k][0], g["auto_matrices"][om + k]), what
        om += nw
        nb = int(g["auto_n_boxes"][n])
        assert np.array_equal(s["gt_bboxes"], g["auto_gt_bboxes"][ob:ob + nb]), what
        ob += nb
    assert od == len(g["auto_draws"]) and om == len(g["auto_matrices"]) and ob == len(g["auto_gt_bboxes"])


def test_kernel_batch_holds_the_cases():
    """the batch tests/test_gpu_cutout.py runs radet_cutout_u8 on: its expected buffer shows every case the kernel must get right"""
    frames, rows, offs, packed, want = C.u8_kernel_cases()
    assert len(rows[5][0]) == C.U8_MAX_HOLES and [f.shape[:2] for f in frames] == C.U8_SIZES
    guard = np.ones(len(want), bool)
    for f, o in zip(frames, offs):
        guard[o * 3:o * 3 + f.size] = False
    assert guard.sum() >= 15 * len(frames) and (want[guard] == C.U8_GUARD).all() and (packed[guard] == C.U8_GUARD).all()
    got = [want[o * 3:o * 3 + f.size].reshape(f.shape) for f, o in zip(frames, offs)]
    assert (got[0] == np.array(rows[0][1], np.uint8)).all()                                     # the whole image
    assert (got[1][0, 200:] == np.array(rows[1][1], np.uint8)).all() and (got[1][0, :4] == np.array(rows[1][1], np.uint8)).all()
    assert np.array_equal(got[1][0, 4:200], frames[1][0, 4:200])
    assert np.array_equal(got[2][:250], frames[2][:250]) and (got[2][250:] == 255).all()        # only the hole with area
    assert np.array_equal(got[3], frames[3]) and np.array_equal(got[4], frames[4])              # no holes; skipped
    hit = (got[5] == np.array(rows[5][1], np.uint8)).all(-1)
    assert 0.2 < hit.mean() < 0.95 and hit[299, 199] and hit[0, 0] and C.hole_mask(rows[5][0], 300, 200).sum() == hit.sum()


# ------------------------------------------------------------------------------------------------ arguments and refusals
def test_argument_checks():
    from radet_amd.datasets.loading import CUTOUT_MAX_HOLES, CutOut
    assert CUTOUT_MAX_HOLES == 64
    assert CutOut(3, cutout_shape=(4, 5)).n_holes == (3, 3)
    assert CutOut((0, 2), cutout_ratio=[(0.1, 0.2), (0.3, 0.4)]).candidates == [(0.1, 0.2), (0.3, 0.4)]
    assert CutOut(1, cutout_shape=[(4, 5)], fill_in=[1, 2, 255]).fill == (1, 2, 255)
    for bad in (dict(n_holes=1), dict(n_holes=1, cutout_shape=(4, 5), cutout_ratio=(0.1, 0.1)), dict(n_holes=1, cutout_shape=7),
                dict(n_holes=(2, 2), cutout_shape=(4, 5)), dict(n_holes=(3, 1), cutout_shape=(4, 5)), dict(n_holes=(-1, 2), cutout_shape=(4, 5)),
                dict(n_holes=(1, 2, 3), cutout_shape=(4, 5)), dict(n_holes=-1, cutout_shape=(4, 5)), dict(n_holes=1.5, cutout_shape=(4, 5)),
                dict(n_holes=1, cutout_shape=(4, 5, 6)), dict(n_holes=1, cutout_shape=[]), dict(n_holes=1, cutout_shape=(4.5, 5)),
                dict(n_holes=1, cutout_shape=((4, 5), (6, 7))), dict(n_holes=1, cutout_ratio=["a", "b"])):
        with pytest.raises(ValueError, match="CutOut"):
            CutOut(**bad)
    # fill_in: three integers in [0, 255]; the reference's assignment into the u8 image would wrap or truncate the rest
    for fill in ((0, 0), (0, 0, 0, 0), 0, (256, 0, 0), (-1, 0, 0), (0.5, 0, 0), (0, 0, "0"), (True, 0, 0), None):
        with pytest.raises(ValueError, match="fill_in"):
            CutOut(1, cutout_shape=(4, 5), fill_in=fill)
    assert CutOut(1, cutout_shape=(4, 5), fill_in=(128.0, 0, 255)).fill == (128, 0, 255)
    with pytest.raises(NotImplementedError, match="CUTOUT_MAX_HOLES"):
        CutOut(CUTOUT_MAX_HOLES + 1, cutout_shape=(4, 5))
    with pytest.raises(NotImplementedError, match="CUTOUT_MAX_HOLES"):
        CutOut((1, CUTOUT_MAX_HOLES + 1), cutout_shape=(4, 5))
    CutOut((0, CUTOUT_MAX_HOLES), cutout_shape=(4, 5))
    with pytest.raises(NotImplementedError, match="seg_fields"):
        CutOut(1, cutout_shape=(4, 5)).plan(dict(img_shape=(48, 64, 3), seg_fields=["gt_semantic_seg"]), None, np.random.RandomState(0))


def _pipeline(*middle, first="LoadImageFromFile", dm=None):
    return [dict(type=first), *middle, *([dm] if dm else []), dict(type="Normalize", **NORM), dict(type="Pad", size_divisor=32),
            dict(type="Collect", keys=["img"])]


CUT = dict(type="CutOut", n_holes=(1, 3), cutout_ratio=(0.1, 0.1))
ROTATE, TRANSLATE = dict(type="Rotate", level=10), dict(type="Translate", level=1)
RESIZE, ANN = dict(type="Resize", img_scale=(640, 480), keep_ratio=True), dict(type="LoadAnnotations")
FLIP = dict(type="RandomFlip", flip_ratio=0.5)
COSY = dict(type="CosyPoseAug", p=0.8, pipelines=[dict(type="PillowBlur")])
CROP = dict(type="RandomCrop", crop_size=(480, 640))
EXPAND = dict(type="Expand", mean=NORM["mean"], ratio_range=(1, 2))


def test_places_the_stage_may_stand_in(tmp_path):
    from radet_amd.datasets.loading import CutOut, ImagePipeline
    (tmp_path / "bg.jpg").write_bytes(b"")                                   # (RandomBackground lists the directory only)
    bg = dict(type="RandomBackground", background_dir=str(tmp_path))

    def lates(*middle, **kw):
        return [t.late for t in ImagePipeline(_pipeline(*middle, **kw)).transforms if isinstance(t, CutOut)]

    # (a) in the block after Resize: bare, mixed with bare affine stages in any order, inside AutoAugment policies
    assert lates(ANN, RESIZE, CUT, bg, COSY, FLIP) == [False]
    assert lates(ANN, RESIZE, CUT, ROTATE, CUT, TRANSLATE, bg, FLIP) == [False, False]
    assert lates(ANN, RESIZE, ROTATE, CUT, FLIP) == [False]
    ImagePipeline(_pipeline(ANN, RESIZE, dict(type="AutoAugment", policies=[[ROTATE, CUT], [CUT], [TRANSLATE]]), bg, FLIP))
    # (b) late: behind the photometric stages, in front of RandomFlip; both at once
    assert lates(ANN, RESIZE, bg, COSY, CUT, FLIP) == [True]
    assert lates(ANN, RESIZE, ROTATE, bg, dict(type="RandomHSV", h_ratio=0.1, s_ratio=0.1, v_ratio=0.1), CUT, FLIP) == [True]
    assert lates(ANN, RESIZE, CUT, bg, COSY, CUT, FLIP) == [False, True]
    # a CutOut-only block is pointwise: it stands behind RandomCrop and together with the zoom stages
    assert lates(ANN, RESIZE, CROP, CUT, CUT, bg, FLIP) == [False, False]
    assert lates(ANN, EXPAND, dict(type="MinIoURandomCrop"), RESIZE, CUT, FLIP) == [False]
    ImagePipeline(_pipeline(ANN, EXPAND, RESIZE, dict(type="AutoAugment", policies=[[CUT], [CUT, CUT]]), FLIP))
    assert lates(ANN, RESIZE, CROP, bg, CUT, FLIP) == [True] and lates(ANN, EXPAND, RESIZE, bg, COSY, CUT, FLIP) == [True]
    # a block that holds a warp stage is refused with them, in today's words
    for warp in ((ROTATE, CUT), (CUT, ROTATE), (dict(type="AutoAugment", policies=[[CUT], [TRANSLATE]]),)):
        with pytest.raises(NotImplementedError, match="together with RandomCrop \\(a warp composed with a window is left out\\)"):
            ImagePipeline(_pipeline(ANN, RESIZE, CROP, *warp))
        with pytest.raises(NotImplementedError, match="together with Expand \\(a warp composed with a window is left out\\)"):
            ImagePipeline(_pipeline(ANN, EXPAND, RESIZE, *warp))
        with pytest.raises(NotImplementedError, match="together with MinIoURandomCrop"):
            ImagePipeline(_pipeline(ANN, dict(type="MinIoURandomCrop"), RESIZE, *warp))
    # anywhere else, twice late, more than 4 entries, in test pipelines
    with pytest.raises(NotImplementedError, match="subsequence"):
        ImagePipeline(_pipeline(ANN, CUT, RESIZE))
    with pytest.raises(NotImplementedError, match="subsequence"):
        ImagePipeline(_pipeline(ANN, RESIZE, FLIP, CUT))
    with pytest.raises(NotImplementedError, match="subsequence"):
        ImagePipeline(_pipeline(ANN, RESIZE, bg, CUT, CUT, FLIP))
    with pytest.raises(NotImplementedError, match="at most 4"):
        ImagePipeline(_pipeline(ANN, RESIZE, CUT, ROTATE, CUT, TRANSLATE, CUT))
    with pytest.raises(NotImplementedError, match="at most 4"):
        ImagePipeline(_pipeline(ANN, RESIZE, dict(type="AutoAugment", policies=[[CUT, ROTATE, CUT, TRANSLATE, CUT]])))
    with pytest.raises(NotImplementedError, match="one AutoAugment"):
        ImagePipeline(_pipeline(ANN, RESIZE, dict(type="AutoAugment", policies=[[CUT]]), CUT))
    with pytest.raises(NotImplementedError, match="LoadImageFromWebcam"):
        ImagePipeline(_pipeline(RESIZE, CUT, first="LoadImageFromWebcam"))
    for inner in ((RESIZE, CUT, FLIP), (RESIZE, FLIP, CUT)):
        with pytest.raises(NotImplementedError, match="MultiScaleFlipAug"):
            ImagePipeline([dict(type="LoadImageFromFile"),
                           dict(type="MultiScaleFlipAug", img_scale=(640, 480), flip=False,
                                transforms=[*inner, dict(type="Normalize", **NORM), dict(type="Pad", size_divisor=32),
                                            dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])])])
    # the colour stages stay refused inside policies
    from radet_amd.datasets.loading import AutoAugment
    with pytest.raises(NotImplementedError, match="ColorTransform"):
        AutoAugment(policies=[[CUT], [dict(type="ColorTransform", prob=0.5)]])


def test_late_cutout_with_the_mask_free_sampler_is_refused(tmp_path):
    from _maskfree_pipelines import ASSIGNER, DM
    from radet_amd.datasets.loading import ImagePipeline
    tail = [FLIP, DM["mbd"], ASSIGNER, dict(type="Normalize", **NORM), dict(type="Pad", size_divisor=32),
            dict(type="Collect", keys=["img", "gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight"])]
    with pytest.raises(NotImplementedError, match="with_gt_mask=False"):
        ImagePipeline([dict(type="LoadImageFromFile"), ANN, RESIZE, COSY, CUT, *tail])
    p = ImagePipeline([dict(type="LoadImageFromFile"), ANN, RESIZE, CUT, COSY, *tail])          # in the block: built
    assert p.mask_free is not None


def test_entry_limit_counts_holes_and_warps_together():
    from radet_amd.datasets.loading import CutOut, Translate
    rs = np.random.RandomState(0)
    s = dict(img_shape=(48, 64, 3), bbox_fields=[])
    CUTOUT_HOLES = 5
    cut, move = CutOut(CUTOUT_HOLES, cutout_shape=(4, 5)), Translate(level=1, prob=1)
    move.plan(s, None, rs)
    assert "block_ops" not in s and len(s["affine"]) == 1                      # a warp alone plans as before
    cut.plan(s, None, rs)
    move.plan(s, None, rs)
    cut.plan(s, None, rs)
    assert s["block_ops"] == [("warp", 0), ("cutout", 0), ("warp", 1), ("cutout", 1)]
    assert len(s["affine"]) == 2 and [len(r) for r, _ in s["cutout"]] == [CUTOUT_HOLES] * 2    # one entry however many holes
    for stage in (cut, move):
        with pytest.raises(NotImplementedError, match="more than 4"):
            stage.plan(dict(s, block_ops=list(s["block_ops"])), None, rs)


# ------------------------------------------------------------------------------------------------ the pipeline and the configs
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL writes and decodes the generated JPEG / PNG files")
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=8, seed=3)


def test_pipeline_without_cutout_plans_as_before(tree):
    """a stage that draws no hole leaves no key behind; it draws once from the NumPy generator"""
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    cfg, train = jitter_train_cfg(tree, name="r50_ycbv_pbr_rotate.py")
    k = [t["type"] for t in train["pipeline"]].index("Rotate")
    never = dict(train, pipeline=train["pipeline"][:k + 1] + [dict(type="CutOut", n_holes=0, cutout_shape=(9, 9))] + train["pipeline"][k + 1:])
    a, b = build_dataset(train), build_dataset(never)
    fired = 0
    for i in range(8):
        p = a.plan_sample(i, *sample_generators(0, 0, i))
        q = b.plan_sample(i, *sample_generators(0, 0, i))
        assert not any(key in p or key in q for key in ("block_ops", "cutout", "cutout_late"))
        assert set(p) == set(q)
        fired += "affine" in p
        if "affine" in p:                                                     # (the Rotate in front of the stage drew the same)
            assert np.array_equal(p["affine"][0][0], q["affine"][0][0]) and p["affine_draws"] == q["affine_draws"]
            assert np.array_equal(p["gt_bboxes"], q["gt_bboxes"]) or p["flip"] != q["flip"]
    assert fired


def test_cutout_configs_build(tree):
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.datasets.loading import ImagePipeline
    from radet_amd.utils import Config
    base = Config.fromfile(os.path.join(REPO, "configs", "base", "datasets", "bop_detection_cutout.py"))
    cfg, train = jitter_train_cfg(tree, name="r50_ycbv_pbr_cutout.py")
    plain = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    assert cfg.model == plain.model and cfg.train_cfg == plain.train_cfg and cfg.test_cfg == plain.test_cfg
    assert cfg.data.train.pipeline == base.data.train.pipeline == base.train_pipeline
    names = [t["type"] for t in cfg.data.train.pipeline]
    assert names[2:5] == ["Resize", "AutoAugment", "RandomBackground"]
    assert [[t["type"] for t in p] for p in cfg.data.train.pipeline[3]["policies"]] == [["Rotate", "CutOut"], ["CutOut"], ["Translate"]]
    cut = cfg.data.train.pipeline[3]["policies"][1][0]
    assert cut == dict(type="CutOut", n_holes=(1, 4), cutout_ratio=[(0.1, 0.1), (0.2, 0.15)], fill_in=(0, 0, 0))
    ds = build_dataset(train)
    assert isinstance(ds.pipeline, ImagePipeline) and len(ds) == 8
    orders = set()
    for epoch in range(3):
        for i in range(8):
            s = ds.plan_sample(i, *sample_generators(0, epoch, i))
            assert s["img_shape"] == s["pad_shape"] == (480, 640, 3)
            assert len(s["gt_bboxes"]) == len(s["gt_labels"]) == len(s["gt_masks"])
            ops = s.get("block_ops", [("warp", k) for k in range(len(s.get("affine", ())))])
            order = "".join(kind[0] for kind, _ in ops)
            orders.add((s["policy"], order))
            assert order in {0: ("wc", "c"), 1: ("c",), 2: ("w", "")}[s["policy"]]
            for rects, fill in s.get("cutout", ()):
                assert 1 <= len(rects) <= 4 and fill == (0, 0, 0)
                assert (rects[:, 2] - rects[:, 0] <= 128).all() and (rects[:, 3] - rects[:, 1] <= 72).all()
                assert (rects[:, 0] >= 0).all() and (rects[:, 2] <= 640).all() and (rects[:, 3] <= 480).all()
    assert {(0, "wc"), (0, "c"), (1, "c"), (2, "w")} <= orders, orders
