"""Affine augmentation, host side: the planning of Rotate, Shear, Translate and AutoAugment against the reference's stages
run under the same seeds (tests/golden/affine_aug.npz, made by tests/golden/gen_affine_aug.py), the NumPy restatement of
cv2.warpAffine (tests/_affine_ref.py) against hand-checked values, the refusals and the rotate configs."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _affine_ref as A  # noqa: E402
from _affine_cfg import rotate_train_cfg  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden", "affine_aug.npz")
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def _args(d):
    """the tuples that JSON made lists of (policies stay lists of lists of dicts)"""
    if isinstance(d, dict):
        return {k: _args(v) if k == "policies" else (tuple(v) if isinstance(v, list) else v) for k, v in d.items()}
    return [_args(v) for v in d]


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    g["cases"] = [(name, _args(a)) for name, a in json.loads(str(g["cases"]))]
    return g


def test_fixture_holds_the_edge_cases(gold):
    g = gold
    assert (np.bincount(g["case"]) >= 8).all() and len(np.bincount(g["case"])) == len(g["cases"])
    assert (g["n_entries"] == 0).any() and (g["n_entries"] == 1).any() and (g["n_entries"] == 2).any()      # skipped, fired, two stages
    assert (np.copysign(1, g["values"]) < 0).any() and (np.copysign(1, g["values"]) > 0).any()             # both signs
    assert ((g["n_boxes"] > 0) & (g["n_boxes"] < len(g["boxes"]))).any()                                   # a box dropped
    assert ((g["n_boxes"] == 0) & (g["n_ignore"] > 0)).any()                                               # gt emptied, an ignore box left
    assert set(g["policy"]) == {-1, 0, 1}                                                                  # each policy chosen
    for name in ("Rotate", "Shear", "Translate"):
        assert {a["prob"] for n, a in g["cases"] if n == name} >= {0, 0.5, 1}
        assert any(a["level"] == 0 for n, a in g["cases"] if n == name)
    assert {a.get("direction", "horizontal") for n, a in g["cases"] if n == "Shear"} == {"horizontal", "vertical"}
    assert {a.get("direction", "horizontal") for n, a in g["cases"] if n == "Translate"} == {"horizontal", "vertical"}
    assert any(a.get("center") == (5, 40) and a.get("scale") == 0.8 for n, a in g["cases"] if n == "Rotate")
    assert any(a.get("min_size", 0) > 0 for n, a in g["cases"] if n == "Translate")
    assert len(g["matrices"]) == len(g["values"]) == g["n_entries"].sum()


@pytest.mark.parametrize("masks_as", ["bitmap", "runs"])
def test_planning_reproduces_the_reference(gold, masks_as):
    from radet_amd.datasets import loading as L
    g = gold
    H, W = (int(v) for v in g["src_hw"])
    ob = oi = om = 0
    for n in range(len(g["seed"])):
        name, args = g["cases"][g["case"][n]]
        rs = np.random.RandomState(int(g["seed"][n]))
        nb0 = len(g["boxes"])
        s = dict(img=np.zeros((H, W, 3), np.uint8), img_shape=(H, W, 3), bbox_fields=["gt_bboxes_ignore", "gt_bboxes"],
                 mask_fields=["gt_masks"], gt_bboxes=g["boxes"].copy(), gt_bboxes_ignore=g["ignore"].copy(), gt_labels=g["labels"].copy())
        if masks_as == "bitmap":                 # mask k is filled with k: the surviving rows name themselves
            s["gt_masks"] = np.arange(nb0, dtype=np.uint8)[:, None, None] * np.ones((1, H, W), np.uint8)
        else:
            s["gt_masks_rle"] = (list(range(nb0)), (H, W))
        what = f"sample {n}: {name} {args} seed {g['seed'][n]}"
        getattr(L, name)(**args).plan(s, None, rs)
        assert rs.random_sample() == g["next"][n], what                  # the generator stands where the reference's does
        ne = int(g["n_entries"][n])
        assert len(s.get("affine", ())) == ne and ("affine" in s) == (ne > 0), what          # fired
        assert s.get("policy", -1) == g["policy"][n], what
        for k in range(ne):
            M, fill = s["affine"][k]
            assert M.dtype == np.float64 and M.shape == (2, 3) and np.array_equal(M, g["matrices"][om + k]), what
            value = s["affine_draws"][k][1]
            assert value == g["values"][om + k], what
            if isinstance(value, float):                                                     # the sign drawn (an int has no -0)
                assert np.copysign(1, value) == np.copysign(1, g["values"][om + k]), what
            stage_args = args if name != "AutoAugment" else \
                [t for t in args["policies"][s["policy"]] if t["type"] == s["affine_draws"][k][0]][0]
            want_fill = stage_args.get("img_fill_val", 128)
            want_fill = (want_fill,) * 3 if not isinstance(want_fill, (tuple, list)) else want_fill
            assert fill == tuple(int(v) for v in want_fill), what
        nb, ni = int(g["n_boxes"][n]), int(g["n_ignore"][n])
        for key, want in (("gt_bboxes", g["gt_bboxes"][ob:ob + nb]), ("gt_bboxes_ignore", g["gt_bboxes_ignore"][oi:oi + ni]),
                          ("gt_labels", g["gt_labels"][ob:ob + nb])):
            assert s[key].dtype == want.dtype and np.array_equal(s[key], want), f"{what}: {key}"
        kept = s["gt_masks"][:, 0, 0] if masks_as == "bitmap" else s["gt_masks_rle"][0]
        assert list(kept) == list(g["kept"][ob:ob + nb]), what
        assert tuple(s["img_shape"]) == (H, W, 3)                        # the output size is the input size
        ob, oi, om = ob + nb, oi + ni, om + ne
    assert ob == len(g["gt_bboxes"]) and oi == len(g["gt_bboxes_ignore"]) and om == len(g["matrices"])


# ------------------------------------------------------------------------------------------------ the restatement
def test_inverse_and_tables_by_hand():
    # the inverse of a translation by (+3, -2) is the translation by (-3, +2); of a scale by 2 about the origin, 1 / 2
    assert np.array_equal(A.invert([[1, 0, 3], [0, 1, -2]]), [1, 0, -3, 0, 1, 2])
    assert np.array_equal(A.invert([[2, 0, 0], [0, 2, 0]]), [0.5, 0, 0, 0, 0.5, 0])
    assert np.array_equal(A.invert([[0, 0, 5], [0, 0, 7]]), [0, 0, 0, 0, 0, 0])            # singular: D = 0, as cv2
    # the kernel's copy of the inverse is the same arithmetic
    from radet_amd import kernels as K
    M = A.rotation_matrix((5, 40), -17.5, 0.8)
    assert np.array_equal(K.invert_affine(M), A.invert(M))
    # X = ((x - 3) * 1024 + 16) >> 5 = (x - 3) * 32: whole pixels, no fraction; the half-pixel shift: fraction 16 / 32
    X, Y = A.tables(np.array([[1, 0, 3], [0, 1, -2]], np.float64), 4, 6)
    assert np.array_equal(X, np.tile((np.arange(6) - 3) * 32, (4, 1))) and np.array_equal(Y, np.tile(((np.arange(4) + 2) * 32)[:, None], (1, 6)))
    X, _ = A.tables(np.array([[1, 0, 0.5], [0, 1, 0]], np.float64), 1, 3)
    assert list(X[0]) == [-16, 16, 48] and list(X[0] >> 5) == [-1, 0, 1] and list(X[0] & 31) == [16, 16, 16]
    # round half to even at the table set-up: (1 / 2048) * 1024 = 0.5 -> 0, (3 / 2048) * 1024 = 1.5 -> 2
    X, _ = A.tables(np.array([[1, 0, -1 / 2048], [0, 1, 0]], np.float64), 1, 1)
    assert X[0, 0] == (0 + 16) >> 5
    X, _ = A.tables(np.array([[1, 0, -3 / 2048 - 16 / 1024], [0, 1, 0]], np.float64), 1, 1)
    assert X[0, 0] == (np.rint(1.5 + 16) + 16) // 32 == 1


def test_blend_by_hand():
    img = np.array([[10, 20], [30, 50]], np.uint8)
    # a shift by half a pixel to the right: dst(x) = (src(x - 1) + src(x)) / 2 with the fill 100 on the left, rounded half up
    out = A.warp_affine_u8(img, np.array([[1, 0, 0.5], [0, 1, 0]], np.float64), 100)
    assert out.tolist() == [[(100 * 512 + 10 * 512 + 512) >> 10, 15], [(100 * 512 + 30 * 512 + 512) >> 10, 40]]
    # a quarter pixel in both directions: weights (8 | 24) x (8 | 24)
    out = A.warp_affine_u8(img, np.array([[1, 0, 0.25], [0, 1, 0.25]], np.float64), 0)
    assert out[1, 1] == (8 * 8 * 10 + 24 * 8 * 20 + 8 * 24 * 30 + 24 * 24 * 50 + 512) >> 10
    # on 0 / 1 masks the blend yields 0 / 1
    m = (np.random.RandomState(0).rand(23, 31) > 0.5).astype(np.uint8)
    assert set(np.unique(A.warp_affine_u8(m, A.rotation_matrix((15, 11), 33, 1.1), 0))) <= {0, 1}


def test_restatement_on_exact_cases():
    rs = np.random.RandomState(1)
    img = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    fill = (0, 37, 255)
    assert np.array_equal(A.warp_affine_u8(img, np.array([[1, 0, 0], [0, 1, 0]], np.float64), fill), img)       # identity
    for off in (7, -7):
        for direction in ("horizontal", "vertical"):
            want = np.empty_like(img)
            want[:] = fill
            if direction == "horizontal":
                want[:, max(off, 0):53 + min(off, 0)] = img[:, max(-off, 0):53 - max(off, 0)]
            else:
                want[max(off, 0):37 + min(off, 0)] = img[max(-off, 0):37 - max(off, 0)]
            assert np.array_equal(A.warp_affine_u8(img, A.translate_matrix(off, direction), fill), want), (off, direction)
    for off in (100, -100):                                                                                      # more than the width
        assert (A.warp_affine_u8(img, A.translate_matrix(off), fill) == np.array(fill, np.uint8)).all()
    sq = rs.randint(0, 256, (31, 31, 3)).astype(np.uint8)
    # getRotationMatrix2D(centre, 90, 1) turns the image counter-clockwise, as np.rot90 does; -90 the other way
    assert np.array_equal(A.warp_affine_u8(sq, A.rotation_matrix((15, 15), 90, 1), fill), np.rot90(sq))
    assert np.array_equal(A.warp_affine_u8(sq, A.rotation_matrix((15, 15), -90, 1), fill), np.rot90(sq, -1))
    one = rs.randint(0, 256, (31, 31)).astype(np.uint8)                                                          # one channel
    assert np.array_equal(A.warp_affine_u8(one, A.rotation_matrix((15, 15), 90, 1), 0), np.rot90(one))


def test_matrix_builders_match_the_pipelines():
    from radet_amd.datasets import loading as L
    assert np.array_equal(L.rotation_matrix((5, 40), -17.5, 0.8), A.rotation_matrix((5, 40), -17.5, 0.8))
    for d in ("horizontal", "vertical"):
        assert np.array_equal(L.shear_matrix(-0.3, d), A.shear_matrix(-0.3, d))
        assert np.array_equal(L.translate_matrix(-7, d), A.translate_matrix(-7, d))
    assert L.shear_matrix(0.3, "horizontal")[0, 1] == float(np.float32(0.3))                # float32 entries, widened


# ------------------------------------------------------------------------------------------------ the pipeline
def _pipeline(*middle, first="LoadImageFromFile"):
    return [dict(type=first), *middle, dict(type="Normalize", **NORM), dict(type="Pad", size_divisor=32),
            dict(type="Collect", keys=["img"])]


ROTATE, SHEAR, TRANSLATE = dict(type="Rotate", level=10), dict(type="Shear", level=5), dict(type="Translate", level=1)
AUTO = dict(type="AutoAugment", policies=[[SHEAR, ROTATE], [TRANSLATE]])


def test_refusals():
    from radet_amd.datasets.loading import AutoAugment, ImagePipeline, Rotate, Shear, Translate
    resize = dict(type="Resize", img_scale=(640, 480), keep_ratio=True)
    ann = dict(type="LoadAnnotations")
    bg = dict(type="RandomFlip", flip_ratio=0.5)
    for middle in ((ann, resize, ROTATE), (ann, resize, SHEAR, TRANSLATE, ROTATE), (ann, resize, AUTO, bg), (ann, resize, TRANSLATE, bg),
                   (ann, resize, ROTATE, SHEAR, ROTATE, SHEAR)):                              # (a stage may stand twice, as in the reference)
        ImagePipeline(_pipeline(*middle))
    for stage in (ROTATE, SHEAR, TRANSLATE, AUTO):
        with pytest.raises(NotImplementedError, match="directly after Resize"):              # anywhere else
            ImagePipeline(_pipeline(ann, stage, resize))
        with pytest.raises(NotImplementedError, match="directly after Resize"):
            ImagePipeline(_pipeline(ann, resize, bg, stage))
        with pytest.raises(NotImplementedError, match="directly after Resize"):
            ImagePipeline(_pipeline(ann, stage))
        with pytest.raises(NotImplementedError, match="LoadImageFromWebcam"):
            ImagePipeline(_pipeline(resize, stage, first="LoadImageFromWebcam"))
        with pytest.raises(NotImplementedError, match="MultiScaleFlipAug"):
            ImagePipeline([dict(type="LoadImageFromFile"),
                           dict(type="MultiScaleFlipAug", img_scale=(640, 480), flip=False,
                                transforms=[dict(type="Resize", keep_ratio=True), stage, dict(type="RandomFlip"),
                                            dict(type="Normalize", **NORM), dict(type="Pad", size_divisor=32),
                                            dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])])])
        with pytest.raises(NotImplementedError, match="RandomCrop"):
            ImagePipeline(_pipeline(ann, resize, dict(type="RandomCrop", crop_size=(480, 640)), stage))
        with pytest.raises(NotImplementedError, match="Expand"):
            ImagePipeline(_pipeline(ann, dict(type="Expand", mean=NORM["mean"], ratio_range=(1, 2)), resize, stage))
        with pytest.raises(NotImplementedError, match="MinIoURandomCrop"):
            ImagePipeline(_pipeline(ann, dict(type="MinIoURandomCrop"), resize, stage))
    with pytest.raises(NotImplementedError, match="one AutoAugment"):
        ImagePipeline(_pipeline(ann, resize, AUTO, ROTATE))
    with pytest.raises(NotImplementedError, match="at most 4"):
        ImagePipeline(_pipeline(ann, resize, ROTATE, SHEAR, TRANSLATE, ROTATE, SHEAR))
    with pytest.raises(NotImplementedError, match="with_seg"):                               # seg fields cannot be loaded at all
        ImagePipeline(_pipeline(dict(type="LoadAnnotations", with_seg=True), resize, ROTATE))
    with pytest.raises(NotImplementedError, match="bilinear"):
        Shear(level=5, interpolation="nearest")
    with pytest.raises(NotImplementedError, match="scale=0"):
        Rotate(level=5, scale=0)
    for name in ("ColorTransform", "EqualizeTransform", "BrightnessTransform", "ContrastTransform"):
        with pytest.raises(NotImplementedError, match=name):
            AutoAugment(policies=[[ROTATE], [dict(type=name, prob=0.5)]])
    with pytest.raises(NotImplementedError, match="at most 4"):                              # more than 4 entries per sample
        AutoAugment(policies=[[ROTATE, SHEAR, TRANSLATE, ROTATE, SHEAR]])
    s = dict(img_shape=(48, 64, 3), bbox_fields=[], affine=[(np.eye(2, 3), (0, 0, 0))] * 4)
    with pytest.raises(NotImplementedError, match="more than 4"):
        Translate(level=1, prob=1).plan(s, None, np.random.RandomState(0))
    for stage in (Rotate(level=5, prob=1), Shear(level=5, prob=1), Translate(level=5, prob=1)):       # seg fields
        with pytest.raises(NotImplementedError, match="seg_fields"):
            stage.plan(dict(img_shape=(48, 64, 3), bbox_fields=[], seg_fields=["gt_semantic_seg"]), None, np.random.RandomState(0))
    # a matrix entry too large for the kernel's 32-bit fixed point: at build time, and again when planned
    with pytest.raises(NotImplementedError, match="fixed point"):
        ImagePipeline(_pipeline(ann, resize, dict(type="Translate", level=10, max_translate_offset=1e7)))
    with pytest.raises(NotImplementedError, match="fixed point"):
        ImagePipeline(_pipeline(ann, resize, dict(type="Rotate", level=10, scale=1e-4)))
    with pytest.raises(NotImplementedError, match="fixed point"):
        ImagePipeline(_pipeline(ann, resize, dict(type="AutoAugment", policies=[[dict(type="Rotate", level=1, scale=1e-4)]])))
    with pytest.raises(NotImplementedError, match="fixed point"):
        Rotate(level=10, scale=1e-4, prob=1).plan(dict(img_shape=(480, 640, 3), bbox_fields=[]), None, np.random.RandomState(0))
    with pytest.raises(ValueError):
        Rotate(level=11)
    with pytest.raises(ValueError):
        Shear(level=5, img_fill_val=(300., 0., 0.))
    with pytest.raises(ValueError):
        Translate(level=5, direction="diagonal")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL writes and decodes the generated JPEG / PNG files")
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=8, seed=3)


def test_pipeline_without_affine_stages_plans_as_before(tree):
    """same keys and values with and without a stage that never fires; no affine key in either"""
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    cfg, train = rotate_train_cfg(tree)
    without = dict(train, pipeline=[t for t in train["pipeline"] if t["type"] != "Rotate"])
    never = dict(train, pipeline=[dict(t, prob=0) if t["type"] == "Rotate" else t for t in train["pipeline"]])
    a, b = build_dataset(without), build_dataset(never)
    for i in range(4):
        p = a.plan_sample(i, *sample_generators(0, 0, i))
        assert "affine" not in p and "affine_draws" not in p and "policy" not in p
        # the stage that never fires draws once from the NumPy generator; the planned keys are the same
        q = b.plan_sample(i, *sample_generators(0, 0, i))
        assert set(p) == set(q) and "affine" not in q
        assert p["img_shape"] == q["img_shape"] and len(p["gt_bboxes"]) == len(q["gt_bboxes"])     # (its one draw moves the flip's)


def test_rotate_configs_build(tree):
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.datasets.loading import ImagePipeline
    from radet_amd.utils import Config
    base = Config.fromfile(os.path.join(REPO, "configs", "base", "datasets", "bop_detection_rotate.py"))
    cfg, train = rotate_train_cfg(tree)
    plain = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    assert cfg.model == plain.model and cfg.train_cfg == plain.train_cfg and cfg.test_cfg == plain.test_cfg
    assert cfg.data.train.pipeline == base.data.train.pipeline == base.train_pipeline
    names = [t["type"] for t in cfg.data.train.pipeline]
    assert names[2:5] == ["Resize", "Rotate", "RandomBackground"]
    assert cfg.data.train.pipeline[3] == dict(type="Rotate", level=10, max_rotate_angle=30, prob=0.5, img_fill_val=128)
    ds = build_dataset(train)
    assert isinstance(ds.pipeline, ImagePipeline) and len(ds) == 8
    fired = []
    for epoch in range(3):
        for i in range(8):
            s = ds.plan_sample(i, *sample_generators(0, epoch, i))
            assert s["img_shape"] == s["pad_shape"] == (480, 640, 3)
            assert len(s["gt_bboxes"]) == len(s["gt_labels"]) == len(s["gt_masks"])
            fired.append(len(s.get("affine", ())))
            if "affine" in s:
                (M, fill), = s["affine"]
                angle = s["affine_draws"][0][1]
                assert abs(angle) == 30.0 and fill == (128, 128, 128)
                assert np.array_equal(M, A.rotation_matrix((319.5, 239.5), -angle, 1))
    assert set(fired) == {0, 1} and 4 < sum(fired) < 20
