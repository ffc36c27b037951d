"""Drawing detections, the host side (no GPU): the two NumPy restatements of radet_draw_detections agree bit for bit on every
table of the GPU test, the style's refusals, colour names, the palette against the reference's NumPy draws, the atlas, the
score text, and the constants of the three declarations."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import _draw_cases as C  # noqa: E402
import _draw_ref as R  # noqa: E402
from radet_amd import _lib, kernels as K  # noqa: E402
from radet_amd.ops import draw as D  # noqa: E402


def test_constants_and_declarations():
    hdr = open(os.path.join(REPO, "include", "radet_hip.h")).read()
    src = open(os.path.join(REPO, "radet_amd", "csrc", "draw.hip")).read()

    def define(name, text=hdr):
        return int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert define("DRAW_MAX_DETS") == K.DRAW_MAX_DETS == 256
    assert define("DRAW_MAX_THICKNESS") == K.DRAW_MAX_THICKNESS
    assert define("DRAW_MAX_TEXT_W") == K.DRAW_MAX_TEXT_W
    assert define("DRAW_MAX_GLYPH_H") == K.DRAW_MAX_GLYPH_H
    assert define("DRAW_MAX_PAD") == K.DRAW_MAX_PAD
    assert define("DRAW_INPLACE") == K.DRAW_INPLACE == 1
    assert (define("DRAW_STRIP_DOT", src), define("DRAW_STRIP_BAR", src), define("DRAW_STRIP_CLASS", src),
            define("DRAW_STRIP_NAME0", src)) == (K.DRAW_STRIP_DOT, K.DRAW_STRIP_BAR, K.DRAW_STRIP_CLASS, K.DRAW_STRIP_NAME0) \
        == (R.DOT, R.BAR, R.CLASS, R.NAME0)
    proto = re.search(r"int radet_draw_detections\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["radet_draw_detections"][1]) == 27


@pytest.mark.parametrize("thickness", C.THICKNESSES)
@pytest.mark.parametrize("case", sorted(C.CASES))
def test_restatements_agree(case, thickness):
    frames, _ = C.frames_host()
    want = C.expected(case, thickness)
    got = R.painter(frames, *C.padded(case), C.style_for(case, thickness), C.atlas_for(case))
    for b, (w, g, f) in enumerate(zip(want, got, frames)):
        assert w.shape == f.shape and np.array_equal(w, g), (case, b, int((w != g).sum()))
    if C.CASES[case]["counts"][0] == 0:
        assert np.array_equal(want[0], frames[0])                                  # a count of 0 draws nothing
    assert any((w != f).any() for w, f in zip(want, frames))                       # (not vacuous: pixels did change)


def test_tables_are_what_they_claim():
    """the crossing sets are non-empty, max_dets cuts, the labels shift, the wide label is wider than its frame"""
    frames, _ = C.frames_host()
    st = C.style_for("crossing", 2)
    b, s, l, c = C.padded("crossing")
    d = R._drawn_gather(b[1], s[1], l[1], c[1], st)
    h, w = C.SHAPES[1]
    Y, X = np.mgrid[0:h, 0:w]

    def outline(x1, y1, x2, y2):
        outer = (X >= x1 - 1) & (X <= x2) & (Y >= y1 - 1) & (Y <= y2)
        return outer & ~((X > x1) & (X < x2 - 1) & (Y > y1) & (Y < y2 - 1))
    cross = outline(*d[0][:4]) & outline(*d[1][:4])
    assert cross.any() and tuple(st.palette[0]) != tuple(st.palette[1])
    want = C.expected("crossing", 2)[1]
    # rank 0 is on top where only outlines show (outside every label rectangle)
    cov, widths = C.atlas_for("crossing")
    free = cross.copy()
    for x1, y1, x2, y2, lab, sc in d:
        Wt = sum(int(widths[i]) for i in R._strips(lab, sc, st.n_names))
        lx, ly = max(0, min(x1, w - Wt - 2 * st.pad)), max(0, min(y1, h - cov.shape[1] - 2 * st.pad))
        free &= ~((X >= lx) & (X < lx + Wt + 2 * st.pad) & (Y >= ly) & (Y < ly + cov.shape[1] + 2 * st.pad))
    assert free.any() and (want[free] == st.palette[0]).all()
    # overlapping labels on frame 2
    d2 = R._drawn_gather(b[2], s[2], l[2], c[2], st)
    assert abs(d2[0][0] - d2[1][0]) < 10 and abs(d2[0][1] - d2[1][1]) < 10
    # max_dets
    st = C.style_for("max_dets", 2)
    b, s, l, c = C.padded("max_dets")
    assert [len(R._drawn_gather(b[i], s[i], l[i], c[i], st)) for i in range(3)] == [0, 2, 2]
    assert len(R._drawn_gather(b[1], s[1], l[1], c[1], st._replace(max_dets=256))) == 4
    # the invalid table keeps exactly: the +-1e9 box and the last one
    st = C.style_for("invalid", 2)
    b, s, l, c = C.padded("invalid")
    assert [v[4] for v in R._drawn_gather(b[1], s[1], l[1], c[1], st)] == [1, 3]
    assert [v[:4] for v in R._drawn_gather(b[2], s[2], l[2], c[2], st)] == [(10, 10, 10, 10)]
    # 130 hits on the origin tile
    st = C.style_for("many", 2)
    b, s, l, c = C.padded("many")
    d = R._drawn_gather(b[1], s[1], l[1], c[1], st)
    assert len(d) == 130 and all(v[0] - 1 <= 127 and v[1] - 1 <= 7 and v[2] >= 0 and v[3] >= 0 for v in d)
    # the wide label
    cov, widths = C.atlas_for("wide")
    assert int(widths[R.NAME0 + 1]) + 2 > C.SHAPES[1][1]


def test_score_text():
    assert R.score_text(0.125) == "0.13"                         # ties round up (Python's ':.02f' gives 0.12)
    assert f"{0.125:.02f}" == "0.12"
    assert R.score_text(np.float32(0.995)) == "1.00"
    assert R.score_text(1.0) == "1.00" and R.score_text(0.004) == "0.00"
    assert R.score_text(0.0051) == "0.01" and R.score_text(7.0) == "1.00" and R.score_text(0.005) == "0.00"   # (0.005f < 0.005)
    for v in (0.125, np.float32(0.995), 1.0, 0.004, 0.005, 0.3, 0.999):
        assert "%03d" % R._half_up_cents(v) == R.score_text(v).replace(".", "")
    assert R._strips(3, 0.125, 5) == [R.NAME0 + 3, R.BAR, 0, R.DOT, 1, 3]
    assert R._strips(1203, 0.995, 0) == [R.CLASS, 1, 2, 0, 3, R.BAR, 1, R.DOT, 0, 0]


def test_colours():
    assert D.COLORS == dict(red=(0, 0, 255), green=(0, 255, 0), blue=(255, 0, 0), cyan=(255, 255, 0), yellow=(0, 255, 255),
                            magenta=(255, 0, 255), white=(255, 255, 255), black=(0, 0, 0))
    assert D.color_val("cyan") == (255, 255, 0) and D.color_val((72, 101, 241)) == (72, 101, 241)
    assert D.color_val(np.array([1, 2, 3])) == (1, 2, 3)
    for bad in ("orange", (1, 2), (1, 2, 256), (0.5, 0.5, 0.5), (-1, 0, 0), None, 7, (True, 0, 0)):
        with pytest.raises(ValueError):
            D.color_val(bad)
    from radet_amd.core.visualization import color_val_matplotlib
    assert color_val_matplotlib("red") == (1.0, 0.0, 0.0) and color_val_matplotlib((255, 0, 51)) == (0.2, 0.0, 1.0)


def test_palette_is_the_references_draws():
    state = np.random.get_state()
    pal = D.class_palette(21)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]   # the global generator
    np.random.seed(42)
    want = [np.random.randint(0, 256, (1, 3), dtype=np.uint8) for _ in range(21)]    # radet/core/visualization/image.py:97-101
    np.random.set_state(state)
    assert pal.dtype == np.uint8 and pal.shape == (21, 3) and np.array_equal(pal, np.concatenate(want))
    assert D.class_palette(0).shape == (0, 3)
    assert np.array_equal(C.style_for("crossing", 1).palette, pal[:5])


def test_spec_refusals():
    ok = D.draw_spec(class_names=["a", "b"], thickness=3, font_size=13, label_alpha=0.8, max_dets=7)
    assert ok == D.DrawSpec(3, 0x00FF00, 0x00FF00, 204, 0.3, 7, 2, 2)
    assert D.draw_spec(bbox_color="class").colour is None and D.draw_spec().max_dets == K.DRAW_MAX_DETS
    assert D.draw_spec(font_size=0).pad == 1 and D.draw_spec(bbox_color=(72, 101, 241)).colour == 72 | 101 << 8 | 241 << 16
    for kw in (dict(max_dets=K.DRAW_MAX_DETS + 1), dict(max_dets=-1), dict(thickness=0), dict(thickness=1.5), dict(thickness=True),
               dict(thickness=K.DRAW_MAX_THICKNESS + 1), dict(bbox_color="orange"), dict(text_color=(1, 2, 300)),
               dict(text_color="class"), dict(score_thr=float("nan")), dict(label_alpha=1.5), dict(font_size=-1),
               dict(font_size=8 * K.DRAW_MAX_PAD), dict(class_names=[])):
        with pytest.raises(ValueError):
            D.draw_spec(**kw)
    # a text wider than the kernel's limit
    cov = np.zeros((R.NAME0 + 1, 4, K.DRAW_MAX_TEXT_W), np.uint8)
    widths = np.full(R.NAME0 + 1, 3, np.int32)
    widths[R.NAME0] = K.DRAW_MAX_TEXT_W
    with pytest.raises(ValueError, match="wider than the kernel's limit"):
        D.check_atlas((cov, widths), 1)
    widths[R.NAME0] = 100
    assert D.check_atlas((cov, widths), 1).widths.dtype == np.int32
    with pytest.raises(ValueError):
        D.check_atlas((cov, widths), 2)                          # fewer strips than names
    with pytest.raises(ValueError):
        D.check_atlas((cov.astype(np.float32), widths), 1)
    # frames: host arrays in place, wrong shapes / dtypes
    f = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="in place"):
        D.check_device_frames([f], "inplace=True")
    from radet_amd.ops.crops import check_frames
    for bad in ([np.zeros((8, 8), np.uint8)], [np.zeros((8, 8, 3), np.float32)], ["a.png"], []):
        with pytest.raises(ValueError):
            check_frames(bad)


def test_atlas_shapes_widths_and_cache():
    names = ["can", "cracker_box", "i"]
    a = D.build_atlas(names, 13)
    assert a is D.build_atlas(list(names), 13) and a is D.build_atlas(tuple(names), 13)       # cached per (names, size, font)
    assert a is not D.build_atlas(names, 9) and a is not D.build_atlas(names[:2], 13)
    S, Hc, Wa = a.coverage.shape
    assert S == R.NAME0 + 3 == a.widths.size and a.coverage.dtype == np.uint8 and a.widths.dtype == np.int32
    assert Hc >= 1 and (a.widths >= 1).all() and a.widths.max() == Wa
    for s in range(S):
        assert not a.coverage[s, :, a.widths[s]:].any()                                    # nothing beyond a strip's width
        assert a.coverage[s].any() or s == R.CLASS                                         # every glyph has ink
    assert a.coverage[R.CLASS].any()
    assert a.widths[R.NAME0 + 1] > a.widths[R.NAME0] > a.widths[R.NAME0 + 2]
    assert D.check_atlas(a, 3).coverage.shape == (S, Hc, Wa)
    b = D.build_atlas(None, 13)
    assert b.coverage.shape[0] == R.NAME0 and D.text_width_bound(b.widths, 0) <= K.DRAW_MAX_TEXT_W
    with pytest.raises(ValueError):
        D.build_atlas(names, 0)


def test_visualization_refusals(tmp_path):
    from radet_amd.core import visualization as V
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="mask"):
        V.imshow_det_bboxes(img, np.zeros((0, 5), np.float32), np.zeros(0, np.int64), segms=np.zeros((0, 8, 8)), show=False)
    with pytest.raises(NotImplementedError, match="mask"):
        V.imshow_det_bboxes(img, np.zeros((0, 5), np.float32), np.zeros(0, np.int64), mask_color="red", show=False)
    with pytest.raises(ValueError):
        V.imshow_det_bboxes(img, np.zeros((2, 5), np.float32), np.zeros(3, np.int64), show=False)
    import inspect
    ref = ["img", "bboxes", "labels", "segms", "class_names", "score_thr", "bbox_color", "text_color", "mask_color", "thickness",
           "font_scale", "font_size", "win_name", "fig_size", "show", "wait_time", "out_file"]
    assert list(inspect.signature(V.imshow_det_bboxes).parameters) == ref
    from radet_amd.models.radet import RADet
    ref = ["self", "img", "result", "score_thr", "bbox_color", "text_color", "mask_color", "thickness", "font_scale", "font_size",
           "win_name", "fig_size", "show", "wait_time", "out_file"]
    assert list(inspect.signature(RADet.show_result).parameters) == ref
    from radet_amd import apis
    assert callable(apis.draw_frames) and callable(apis.show_result_pyplot)
