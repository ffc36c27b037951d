"""AutoAugment's colour stages, host side: the planning of ColorTransform / EqualizeTransform / BrightnessTransform /
ContrastTransform against the reference's stages run under the same seeds (tests/golden/color_aug.npz, made by
tests/golden/gen_color_aug.py), bare and inside the policies of an AutoAugment(color_stages=True) that order colour, warp and CutOut entries every way
round; the NumPy restatement of the pixel rules (tests/_color_ref.py) against hand-worked cases; the argument checks, the
refusals, the places the stages may stand in, and the configs."""
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _color_ref as C  # noqa: E402
import _cutout_ref as CUTREF  # noqa: E402
from _jitter_cfg import jitter_train_cfg  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden", "color_aug.npz")
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
LETTER = dict(warp="w", cutout="c", color="k")
# the stub that recorded a stage's call -> the kind the stage plans
KIND_OF = dict(adjust_color="color", imequalize="equalize", adjust_brightness="brightness", adjust_contrast="contrast")
STAGE_KIND = dict(ColorTransform="color", EqualizeTransform="equalize", BrightnessTransform="brightness", ContrastTransform="contrast")


def _tuples(t):
    """a stage config as it was before JSON: lists of pairs stay lists of tuples, other lists become tuples"""
    out = {}
    for k, v in t.items():
        if isinstance(v, list):
            v = [tuple(c) for c in v] if v and isinstance(v[0], list) else tuple(v)
        out[k] = v
    return out


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    g["cases"] = json.loads(str(g["cases"]))
    g["policies"] = [[_tuples(t) for t in p] for p in json.loads(str(g["policies"]))]
    g["names"] = json.loads(str(g["names"]))
    return g


def _sample(g):
    H, W = (int(v) for v in g["src_hw"])
    return dict(img_shape=(H, W, 3), bbox_fields=["gt_bboxes_ignore", "gt_bboxes"], gt_bboxes=g["boxes"].copy(),
                gt_bboxes_ignore=g["ignore"].copy(), gt_labels=g["labels"].copy())


# ------------------------------------------------------------------------------------------------ planning
def test_fixture_holds_the_cases(gold):
    g = gold
    assert {name for name, _ in g["cases"]} == set(STAGE_KIND)
    assert {a["prob"] for _, a in g["cases"]} == {0, 0.5, 1} and {a.get("level") for _, a in g["cases"]} == {None, 0, 3, 7.5, 10}
    fired = g["fired"].astype(bool)
    assert fired.any() and (~fired).any() and np.isnan(g["factor"][~fired]).all()
    orders = set(str(v) for v in g["auto_order"])
    assert {"wck", "wkc", "cwk", "ckw", "kwc", "kcw", "", "k"} <= orders, orders
    assert set(g["auto_policy"]) == set(range(len(g["policies"])))


def test_bare_planning_reproduces_the_reference(gold):
    from radet_amd.datasets import loading as L
    g = gold
    for n in range(len(g["seed"])):
        name, args = g["cases"][g["case"][n]]
        what = f"row {n}: {name} {args} seed {g['seed'][n]}"
        rs = np.random.RandomState(int(g["seed"][n]))
        s = _sample(g)
        stage = getattr(L, name)(**args)
        stage.plan(s, None, rs)
        assert rs.random_sample() == g["next"][n], what                    # one draw, whatever the gate said
        assert np.array_equal(s["gt_bboxes"], g["boxes"]) and np.array_equal(s["gt_bboxes_ignore"], g["ignore"]), what
        assert np.array_equal(s["gt_labels"], g["labels"]) and "img" not in s, what
        if not g["fired"][n]:
            assert not any(k in s for k in ("color", "block_ops", "affine", "cutout")), what
            continue
        (op,), kind = s["color"], STAGE_KIND[name]
        assert s["block_ops"] == [("color", 0)] and isinstance(op, L.ColorOp) and op.kind == kind, what
        assert isinstance(op.factor, float) and op.factor == g["factor"][n], what     # bit for bit: both are float64
        if kind != "equalize":
            assert op.factor == (args["level"] / 10) * 1.8 + 0.1 == L.enhance_level_to_value(args["level"]), what
        assert L._block_list(s) == [op]


def test_autoaugment_planning_reproduces_the_reference(gold):
    from radet_amd.datasets.loading import AutoAugment, _block_list
    g = gold
    H, W = (int(v) for v in g["src_hw"])
    stage = AutoAugment(policies=[[dict(t) for t in p] for p in g["policies"]], color_stages=True)
    ok = oc = od = om = ob = 0
    for n in range(len(g["auto_seed"])):
        what = f"seed {g['auto_seed'][n]}"
        rs = np.random.RandomState(int(g["auto_seed"][n]))
        s = _sample(g)
        stage.plan(s, None, rs)
        assert rs.random_sample() == g["auto_next"][n], what
        assert s["policy"] == g["auto_policy"][n], what
        policy, order = g["policies"][s["policy"]], str(g["auto_order"][n])
        ops = s.get("block_ops", [("warp", k) for k in range(len(s.get("affine", ())))])
        assert "".join(LETTER[kind] for kind, _ in ops) == order, what
        assert ("block_ops" in s) == ("c" in order or "k" in order), what
        for kind in LETTER:                                                # each list holds its own entries, in order
            key = dict(warp="affine", cutout="cutout", color="color")[kind]
            assert [k for q, k in ops if q == kind] == list(range(len(s.get(key, ())))), what
        nk, nw = int(g["auto_n_colours"][n]), int(g["auto_n_warps"][n])
        assert len(s.get("color", ())) == nk and len(s.get("affine", ())) == nw, what
        for k, op in enumerate(s.get("color", ())):
            assert op.kind == KIND_OF[g["names"][g["auto_colour_names"][ok + k]]], what
            assert op.factor == g["auto_colour_factors"][ok + k], what
        ok += nk
        cut_args, want_holes = [t for t in policy if t["type"] == "CutOut"], []
        for k in range(int(g["auto_n_cutouts"][n])):
            nd = int(g["auto_n_draws"][oc + k])
            rects = CUTREF.holes_from_draws(g["auto_draws"][od:od + nd], cut_args[k]["cutout_ratio"], True, H, W)
            if len(rects):
                want_holes.append(rects)
            od += nd
        oc += int(g["auto_n_cutouts"][n])
        assert len(want_holes) == len(s.get("cutout", ())), what
        for (rects, fill), want in zip(s.get("cutout", ()), want_holes):
            assert np.array_equal(rects, want) and fill == tuple(cut_args[0]["fill_in"]), what
        for k in range(nw):
            assert np.array_equal(s["affine"][k][0], g["auto_matrices"][om + k]), what
        om += nw
        nb = int(g["auto_n_boxes"][n])
        assert np.array_equal(s["gt_bboxes"], g["auto_gt_bboxes"][ob:ob + nb]), what     # moved by the warps alone
        ob += nb
        assert len(_block_list(s)) == len(order)
    assert ok == len(g["auto_colour_factors"]) and od == len(g["auto_draws"]) and om == len(g["auto_matrices"])
    assert ob == len(g["auto_gt_bboxes"])


# ------------------------------------------------------------------------------------------------ the restatement
def _gray_image(values, shape):
    """an image whose pixels are gray (b = g = r), so gray(pixel) is the value itself"""
    v = np.asarray(values, np.uint8).reshape(shape)
    return np.ascontiguousarray(np.stack([v, v, v], -1))


def test_exact_fp32_arithmetic():
    """the integer fma against cases where float64 is exact, and one where a float64 sum rounds twice"""
    rs = np.random.RandomState(0)
    for _ in range(2000):
        x, a, m = int(rs.randint(0, 256)), np.float32(rs.uniform(0.1, 1.9)), np.float32(rs.uniform(0, 255))
        n, u = C.fma_f32(x, a, m)
        exact = Fraction(x) * Fraction(float(a)) + Fraction(float(m))
        got = Fraction(n) * Fraction(2) ** u
        assert float(got) == float(np.float32(float(got)))                     # an fp32 value
        lo, hi = np.nextafter(np.float32(float(got)), np.float32(-np.inf)), np.nextafter(np.float32(float(got)), np.float32(np.inf))
        assert abs(exact - got) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi))))
        assert C.mul_f32(x, a) == np.float32(np.float64(x) * np.float64(a))    # (8 x 24 bits: the double product is exact)
    # a tie between 1 and 1 + 2^-23: alone it goes to even (down); with 2^-64 more it goes up, where a float64 sum, which
    # first rounds the 2^-64 away, still says down
    tie = Fraction(1) + Fraction(1, 2 ** 24)
    assert C._round_f32(tie.numerator, 24) == (2 ** 23, -23)
    assert C._round_f32(tie.numerator * 2 ** 40 + 1, 64) == (2 ** 23 + 1, -23)
    assert np.float32(np.float64(float(tie)) + np.float64(2.0 ** -64)) == np.float32(1)
    # and through the fma: 3 * a = 1 + 2^-24 exactly needs 26 bits of a, so build the tie with x = 1: a = 1, m = 2^-24
    assert C.fma_f32(1, np.float32(1), np.float32(2.0 ** -24)) == (2 ** 23, -23)
    assert C.fma_f32(1, np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24)) == (2 ** 23 + 2, -23)       # odd + half: up to even


def test_hand_worked_cases():
    # Equalize: 15 x 17 = 255 pixels: step = (255 - count of the highest value) // 255 = 0 whatever the image: identity
    img = np.random.RandomState(2).randint(0, 256, (15, 17, 3)).astype(np.uint8)
    assert all(C.equalize_lut(img[..., c])[1] == 0 for c in range(3)) and np.array_equal(C.imequalize(img), img)
    # a constant image: the highest value holds every pixel, step = 0
    const = np.full((48, 64, 3), (17, 130, 250), np.uint8)
    assert np.array_equal(C.imequalize(const), const)
    # a two-valued channel: the lower value maps to (0 + step // 2) // step = 0, the higher to count_low // step >= 255 -> 255
    two = C.kernel_frames(4096)[6]
    assert all(len(np.unique(two[..., c])) == 2 for c in range(3))
    out = C.imequalize(two)
    for c in range(3):
        lo, hi = np.unique(two[..., c])
        assert (out[..., c][two[..., c] == lo] == 0).all() and (out[..., c][two[..., c] == hi] == 255).all()
    # 20 x 26 from RandomState(0): 520 pixels, step = 2: the unclamped lut passes 255 and is clamped
    img = np.random.RandomState(0).randint(0, 256, (20, 26, 3)).astype(np.uint8)
    clamped = 0
    for c in range(3):
        lut, step, raw = C.equalize_lut(img[..., c])
        assert step == 2 and lut.max() == 255 and lut[0] == 0
        clamped += int((raw > 255).sum())
    assert clamped >= 3
    eq = C.imequalize(img)
    assert eq.dtype == np.uint8 and not np.array_equal(eq, img)
    # Contrast: means that land exactly on .5 go to the even neighbour, both parities
    for values, mean in (([10, 11], 10), ([11, 12], 12), ([0, 1], 0), ([254, 255], 254), ([7, 7, 8, 8], 8), ([1, 2, 2, 3, 2, 3], 2)):
        g = _gray_image(values, (1, len(values)))
        assert C.gray_mean(g) == mean == C.gray_mean_int(g), values
    # ... and the map: factor 0.5, mean 12 -> m = 6: x / 2 + 6, truncated
    g = _gray_image([11, 12], (1, 2))
    assert C.adjust_contrast(g, 0.5)[0, :, 0].tolist() == [11, 12] and C.adjust_contrast(_gray_image([11, 12, 255, 0], (1, 4)), 0.5).shape == (1, 4, 3)
    # Brightness: truncation, clipping
    ramp = _gray_image(np.arange(256), (16, 16))
    assert np.array_equal(C.adjust_brightness(ramp, 0.5)[..., 0].reshape(-1), np.arange(256) // 2)
    assert np.array_equal(C.adjust_brightness(ramp, 1.5)[..., 1].reshape(-1), np.minimum(255, np.arange(256) * 3 // 2))
    # Color: factor 0 is the gray image, rounded half to even (gray * 1.0 is an integer: no rounding left)
    rnd = np.random.RandomState(3).randint(0, 256, (9, 11, 3)).astype(np.uint8)
    assert np.array_equal(C.adjust_color(rnd, 0.0), np.repeat(C.bgr2gray(rnd)[..., None], 3, -1))
    # a tie: x = 1, g = 2, factor 0.5 -> 1.5 -> 2; x = 2, g = 3 -> 2.5 -> 2
    assert C._color_table(np.float32(0.5), np.float32(0.5))[2, 1] == 2 and C._color_table(np.float32(0.5), np.float32(0.5))[3, 2] == 2
    # factor 1.0 is the identity for all three blends
    for fn in (C.adjust_brightness, C.adjust_contrast, C.adjust_color):
        assert np.array_equal(fn(rnd, 1.0), rnd), fn.__name__
    # the gray weights sum to 2^15: gray of a gray pixel is itself, 255 stays 255
    assert np.array_equal(C.bgr2gray(ramp).reshape(-1), np.arange(256))


def test_integer_mean_equals_pythons_round():
    """the kernel's integer rule against round(float64(S) / N) on random S, N up to 8192 x 8192, and at exact halves"""
    rs = np.random.RandomState(1)
    for _ in range(20000):
        N = int(rs.randint(1, 8192 * 8192 + 1))
        S = int(rs.randint(0, 255 * N + 1))
        q, r = divmod(S, N)
        assert q + (2 * r > N or (2 * r == N and q % 2 == 1)) == round(np.float64(S) / N), (S, N)
    for N in (2, 4, 6, 8192 * 8192, 8192 * 8190):
        for q in (0, 1, 2, 127, 128, 253, 254):
            S = q * N + N // 2
            assert q + (q % 2 == 1) == round(np.float64(S) / N), (S, N)


def test_kernel_batch_holds_the_cases():
    """the batch tests/test_gpu_color.py runs the kernels on"""
    from radet_amd import kernels as K
    frames = C.kernel_frames(K.COLOR_CHUNK_PX)
    assert [f.shape[:2] for f in frames[:7]] == [(1, 1), (3, 5), (15, 17), (20, 26), (60, 80), (48, 64), (48, 64)]
    h, w = frames[7].shape[:2]
    assert w % 2 == 1 and 2 * K.COLOR_CHUNK_PX < h * w < 3 * K.COLOR_CHUNK_PX and (3 * w) % 16
    offs, packed = C.pack(frames)
    assert {(3 * o) % 4 for o in offs} == {0, 1, 2, 3} and len({(3 * o) % 16 for o in offs}) >= 6
    guard = np.ones(len(packed), bool)
    for f, o in zip(frames, offs):
        guard[o * 3:o * 3 + f.size] = False
    assert guard.sum() >= 15 * len(frames) and (packed[guard] == C.GUARD).all()
    for kind in C.KINDS:                                                   # every kind changes the large image
        assert not np.array_equal(C.apply(frames[7], kind, 0.64), frames[7]), kind


# ------------------------------------------------------------------------------------------------ arguments and refusals
def test_argument_checks():
    from radet_amd.datasets import loading as L
    assert L._POLICY_STAGES + L._COLOR_STAGES == ("Rotate", "Shear", "Translate", "CutOut", "ColorTransform", "EqualizeTransform",
                                                  "BrightnessTransform", "ContrastTransform")
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="color_stages"):
            L.AutoAugment(policies=[[dict(type="Rotate", level=1)]], color_stages=bad)
    for name in ("ColorTransform", "BrightnessTransform", "ContrastTransform"):
        cls = getattr(L, name)
        assert cls(level=6).prob == 0.5 and cls(6, 0.25).factor == (6 / 10) * 1.8 + 0.1
        for bad in (dict(level=-1), dict(level=10.5), dict(level="3"), dict(level=None), dict(level=True), dict(level=3, prob=1.5),
                    dict(level=3, prob=-0.1), dict(level=3, prob="1")):
            with pytest.raises(ValueError, match=name):
                cls(**bad)
        with pytest.raises(TypeError):
            cls()
    assert L.EqualizeTransform().prob == 0.5
    for bad in (1.5, -0.1, None):
        with pytest.raises(ValueError, match="EqualizeTransform"):
            L.EqualizeTransform(prob=bad)
    for stage in (L.ColorTransform(3, prob=1), L.EqualizeTransform(prob=1), L.BrightnessTransform(3, prob=1), L.ContrastTransform(3, prob=1)):
        with pytest.raises(NotImplementedError, match="seg_fields"):
            stage.plan(dict(img_shape=(48, 64, 3), seg_fields=["gt_semantic_seg"]), None, np.random.RandomState(0))


def _pipeline(*middle, first="LoadImageFromFile"):
    return [dict(type=first), *middle, dict(type="Normalize", **NORM), dict(type="Pad", size_divisor=32),
            dict(type="Collect", keys=["img"])]


COL, EQ = dict(type="ColorTransform", level=6), dict(type="EqualizeTransform")
BRI, CON = dict(type="BrightnessTransform", level=3), dict(type="ContrastTransform", level=7)
CUT = dict(type="CutOut", n_holes=(1, 3), cutout_ratio=(0.1, 0.1))
ROTATE, TRANSLATE = dict(type="Rotate", level=10), dict(type="Translate", level=1)
RESIZE, ANN = dict(type="Resize", img_scale=(640, 480), keep_ratio=True), dict(type="LoadAnnotations")
FLIP = dict(type="RandomFlip", flip_ratio=0.5)
COSY = dict(type="CosyPoseAug", p=0.8, pipelines=[dict(type="PillowBlur")])
CROP = dict(type="RandomCrop", crop_size=(480, 640))
EXPAND = dict(type="Expand", mean=NORM["mean"], ratio_range=(1, 2))


def test_places_the_stages_may_stand_in(tmp_path):
    from radet_amd.datasets.loading import AutoAugment, ImagePipeline
    (tmp_path / "bg.jpg").write_bytes(b"")                                   # (RandomBackground lists the directory only)
    bg = dict(type="RandomBackground", background_dir=str(tmp_path))
    # in the block after Resize: bare, mixed with the other block stages in any order, inside the policies of an
    # AutoAugment(color_stages=True)
    ImagePipeline(_pipeline(ANN, RESIZE, COL, bg, COSY, FLIP))
    ImagePipeline(_pipeline(ANN, RESIZE, EQ, ROTATE, CUT, BRI, bg, FLIP))
    ImagePipeline(_pipeline(ANN, RESIZE, ROTATE, CON, FLIP))
    ImagePipeline(_pipeline(ANN, RESIZE, dict(type="AutoAugment", policies=[[ROTATE, COL], [EQ], [BRI, CON], [CUT]], color_stages=True), bg, FLIP))
    AutoAugment(policies=[[CUT], [dict(type="ColorTransform", level=5, prob=0.5)]], color_stages=True)
    # a block without a warp stage is pointwise: behind RandomCrop, together with the zoom stages
    ImagePipeline(_pipeline(ANN, RESIZE, CROP, COL, EQ, bg, FLIP))
    ImagePipeline(_pipeline(ANN, EXPAND, dict(type="MinIoURandomCrop"), RESIZE, CON, CUT, FLIP))
    ImagePipeline(_pipeline(ANN, EXPAND, RESIZE, dict(type="AutoAugment", policies=[[EQ], [BRI, CUT]], color_stages=True), FLIP))
    for warp in ((ROTATE, COL), (EQ, ROTATE), (dict(type="AutoAugment", policies=[[EQ], [TRANSLATE]], color_stages=True),)):
        with pytest.raises(NotImplementedError, match="together with RandomCrop \\(a warp composed with a window is left out\\)"):
            ImagePipeline(_pipeline(ANN, RESIZE, CROP, *warp))
        with pytest.raises(NotImplementedError, match="together with Expand"):
            ImagePipeline(_pipeline(ANN, EXPAND, RESIZE, *warp))
    # anywhere else: refused, and the message says where the stage belongs
    for stage in (COL, EQ, BRI, CON):
        for middle in ((ANN, stage, RESIZE), (ANN, RESIZE, bg, stage, FLIP), (ANN, RESIZE, FLIP, stage), (ANN, RESIZE, bg, COSY, stage)):
            with pytest.raises(NotImplementedError, match=f"{stage['type']} at position .* directly after Resize .* move it there"):
                ImagePipeline(_pipeline(*middle))
        with pytest.raises(NotImplementedError, match="LoadImageFromWebcam"):
            ImagePipeline(_pipeline(RESIZE, stage, first="LoadImageFromWebcam"))
        with pytest.raises(NotImplementedError, match=f"{stage['type']} in a MultiScaleFlipAug"):
            ImagePipeline([dict(type="LoadImageFromFile"),
                           dict(type="MultiScaleFlipAug", img_scale=(640, 480), flip=False,
                                transforms=[RESIZE, stage, FLIP, dict(type="Normalize", **NORM), dict(type="Pad", size_divisor=32),
                                            dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])])])
    with pytest.raises(NotImplementedError, match="at most 4"):
        ImagePipeline(_pipeline(ANN, RESIZE, COL, EQ, BRI, CON, COL))
    with pytest.raises(NotImplementedError, match="at most 4"):
        AutoAugment(policies=[[COL, ROTATE, EQ, CUT, CON]], color_stages=True)
    with pytest.raises(NotImplementedError, match="one AutoAugment"):
        ImagePipeline(_pipeline(ANN, RESIZE, dict(type="AutoAugment", policies=[[EQ]], color_stages=True), COL))
    with pytest.raises(NotImplementedError, match="PhotoMetricDistortion"):                    # stays out
        AutoAugment(policies=[[EQ], [dict(type="PhotoMetricDistortion")]], color_stages=True)
    # without the switch a policy that names a colour stage is refused as before, and the message names the switch
    for stage in (COL, EQ, BRI, CON):
        for kw in ({}, dict(color_stages=False)):
            with pytest.raises(NotImplementedError, match=f"{stage['type']} .*pass color_stages=True"):
                AutoAugment(policies=[[ROTATE], [stage]], **kw)
        with pytest.raises(NotImplementedError, match="pass color_stages=True"):
            ImagePipeline(_pipeline(ANN, RESIZE, dict(type="AutoAugment", policies=[[ROTATE, stage]]), FLIP))


def test_entry_limit_counts_every_kind():
    from radet_amd.datasets import loading as L
    rs = np.random.RandomState(0)
    s = dict(img_shape=(48, 64, 3), bbox_fields=[])
    col, move, cut = L.ColorTransform(6, prob=1), L.Translate(level=1, prob=1), L.CutOut(2, cutout_shape=(4, 5))
    move.plan(s, None, rs)
    assert "block_ops" not in s
    col.plan(s, None, rs)
    cut.plan(s, None, rs)
    L.EqualizeTransform(prob=1).plan(s, None, rs)
    assert s["block_ops"] == [("warp", 0), ("color", 0), ("cutout", 0), ("color", 1)]
    assert [type(x).__name__ for x in L._block_list(s)] == ["tuple", "ColorOp", "CutHoles", "ColorOp"]
    assert s["color"] == [L.ColorOp("color", (6 / 10) * 1.8 + 0.1), L.ColorOp("equalize", 1.0)]
    for stage in (col, move, cut):
        with pytest.raises(NotImplementedError, match="more than 4"):
            stage.plan(dict(s, block_ops=list(s["block_ops"])), None, rs)


# ------------------------------------------------------------------------------------------------ the configs
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL writes and decodes the generated JPEG / PNG files")
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=8, seed=3)


def test_color_configs_build(tree):
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.datasets.loading import ImagePipeline
    from radet_amd.utils import Config
    base = Config.fromfile(os.path.join(REPO, "configs", "base", "datasets", "bop_detection_color.py"))
    cfg, train = jitter_train_cfg(tree, name="r50_ycbv_pbr_color.py")
    plain = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    assert cfg.model == plain.model and cfg.train_cfg == plain.train_cfg and cfg.test_cfg == plain.test_cfg
    assert cfg.data.train.pipeline == base.data.train.pipeline == base.train_pipeline
    names = [t["type"] for t in cfg.data.train.pipeline]
    assert names[2:5] == ["Resize", "AutoAugment", "RandomBackground"]
    policies = cfg.data.train.pipeline[3]["policies"]
    assert [[t["type"] for t in p] for p in policies] == [["Rotate", "ColorTransform"], ["EqualizeTransform"],
                                                          ["BrightnessTransform", "ContrastTransform"], ["CutOut"]]
    assert policies[0] == [dict(type="Rotate", level=10, max_rotate_angle=30, prob=0.5, img_fill_val=128),
                           dict(type="ColorTransform", level=6, prob=0.6)]
    assert policies[1] == [dict(type="EqualizeTransform", prob=0.8)]
    assert policies[2] == [dict(type="BrightnessTransform", level=3, prob=0.6), dict(type="ContrastTransform", level=7, prob=0.6)]
    cutout = Config.fromfile(os.path.join(REPO, "configs", "base", "datasets", "bop_detection_cutout.py")).train_pipeline
    assert policies[3] == cutout[3]["policies"][1]
    assert cfg.data.train.pipeline[3]["color_stages"] is True and set(cfg.data.train.pipeline[3]) == {"type", "policies", "color_stages"}
    # everything but the AutoAugment is the cutout config's pipeline
    assert [t for t in cfg.data.train.pipeline if t["type"] != "AutoAugment"] == [t for t in cutout if t["type"] != "AutoAugment"]
    ds = build_dataset(train)
    assert isinstance(ds.pipeline, ImagePipeline) and len(ds) == 8
    orders = set()
    for epoch in range(6):
        for i in range(8):
            s = ds.plan_sample(i, *sample_generators(0, epoch, i))
            assert s["img_shape"] == s["pad_shape"] == (480, 640, 3)
            ops = s.get("block_ops", [("warp", k) for k in range(len(s.get("affine", ())))])
            order = "".join(LETTER[kind] for kind, _ in ops)
            orders.add((s["policy"], order, tuple(op.kind for op in s.get("color", ()))))
            assert order in {0: ("wk", "w", "k", ""), 1: ("k", ""), 2: ("kk", "k", ""), 3: ("c",)}[s["policy"]]
            for op in s.get("color", ()):
                assert op.factor == dict(color=(6 / 10) * 1.8 + 0.1, equalize=1.0, brightness=(3 / 10) * 1.8 + 0.1,
                                         contrast=(7 / 10) * 1.8 + 0.1)[op.kind]
    assert {(0, "wk", ("color",)), (1, "k", ("equalize",)), (2, "kk", ("brightness", "contrast")), (3, "c", ())} <= orders, orders


def test_other_configs_carry_no_colour_entries(tree):
    """a sanity check, not a comparison with the parent commit: no other config holds a colour stage, so its samples carry no
    colour key, _block_list gives what the lists of warps and holes alone give (the formula from before the colour entries),
    and two plans under one seed are equal.  (It passes without the colour stages too.)"""
    import glob
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.datasets.loading import _block_list
    from radet_amd.utils import Config
    seen = 0
    for path in sorted(glob.glob(os.path.join(REPO, "configs", "bop", "*.py"))):
        name = os.path.basename(path)
        if name == "r50_ycbv_pbr_color.py" or "train" not in Config.fromfile(path).data:      # (the others carry no data pipeline)
            continue
        cfg, train = jitter_train_cfg(tree, name=name)
        ds = build_dataset(train)
        for i in range(4):
            s = ds.plan_sample(i, *sample_generators(0, 0, i))
            t = ds.plan_sample(i, *sample_generators(0, 0, i))
            assert "color" not in s and all(kind in ("warp", "cutout") for kind, _ in s.get("block_ops", ())), name
            before = ([s["affine" if kind == "warp" else "cutout"][j] for kind, j in s["block_ops"]] if "block_ops" in s
                      else list(s.get("affine", ())))
            got = _block_list(s)
            assert len(got) == len(before) and all(a is b for a, b in zip(got, before)), name
            assert s.get("block_ops") == t.get("block_ops") and s.get("policy") == t.get("policy"), name
            assert np.array_equal(s["gt_bboxes"], t["gt_bboxes"]) and s["img_shape"] == t["img_shape"], name
            seen += 1
    assert seen >= 16
