"""The loader's sample -> view mapping (radet_amd.datasets.loading.sample_view): the one row {Hr, Wr, wy0, wx0, wh, ww, oy, ox,
h, w, flip, fill} that the resize and both mask kernels take per image or mask, from what RandomCrop (s["crop_window"]) and
Expand / MinIoURandomCrop (s["src_window"]) planned."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

IMG = np.zeros((48, 64, 3), np.uint8)


def test_view_ints_match_the_header():
    import re
    from radet_amd import kernels as K
    hdr = open(os.path.join(REPO, "include", "radet_hip.h")).read()
    assert int(re.search(r"#define RADET_VIEW_INTS (\d+)", hdr).group(1)) == K.VIEW_INTS == 12


def test_a_sample_with_neither_window_is_the_whole_source_and_the_whole_output():
    from radet_amd.datasets.loading import sample_view
    assert sample_view(dict(img=IMG)) == (48, 64, 0, 0, 48, 64, 0, 0, 48, 64, 0, 0)
    assert sample_view(dict(img=IMG, resize_hw=(96, 100))) == (96, 100, 0, 0, 48, 64, 0, 0, 96, 100, 0, 0)
    # a mask row: the whole source is the mask's own size
    assert sample_view(dict(img=IMG, resize_hw=(96, 100)), src_hw=(24, 32)) == (96, 100, 0, 0, 24, 32, 0, 0, 96, 100, 0, 0)


def test_a_crop_window_sets_the_output_window_only():
    from radet_amd.datasets.loading import sample_view
    s = dict(img=IMG, resize_hw=(77, 102), crop_window=(5, 38, 60, 64))
    assert sample_view(s) == (77, 102, 0, 0, 48, 64, 5, 38, 60, 64, 0, 0)
    assert sample_view(s, src_hw=(48, 64)) == sample_view(s)
    v = sample_view(dict(s, crop_window=(np.int64(17), np.int64(0), 60, 64)))
    assert v[6:10] == (17, 0, 60, 64) and all(type(x) is int for x in v)


def test_a_source_window_sets_the_source_side_and_the_fill():
    """negative origin and overhang past the far edge: the window goes into the row as planned, in image coordinates"""
    from radet_amd.datasets.loading import sample_view
    s = dict(img=IMG, src_window=(-7, -11, 70, 90, (11, 140, 250)), resize_hw=(480, 640))
    fill = 11 | 140 << 8 | 250 << 16
    assert sample_view(s) == (480, 640, -7, -11, 70, 90, 0, 0, 480, 640, 0, fill)
    assert sample_view(s, src_hw=(48, 64)) == sample_view(s)                # (a mask row: the same window, masks ignore the fill)
    assert -7 + 70 > 48 and -11 + 90 > 64
    # entirely outside the image, and without a Resize behind it (the window is the output)
    s = dict(img=IMG, src_window=(50, 70, 5, 6, (1, 2, 3)), resize_hw=(5, 6))
    assert sample_view(s) == (5, 6, 50, 70, 5, 6, 0, 0, 5, 6, 0, 1 | 2 << 8 | 3 << 16)


def test_the_stages_plans_go_through():
    """what Expand and RandomCrop leave in the sample is what the row says"""
    from radet_amd.datasets.loading import _set_src_window, sample_view
    s = dict(img=IMG)
    _set_src_window(s, -3, -4, 60, 80, (9, 8, 7))
    assert sample_view(s)[:10] == (60, 80, -3, -4, 60, 80, 0, 0, 60, 80)
    s["resize_hw"] = (480, 640)
    assert sample_view(s)[:10] == (480, 640, -3, -4, 60, 80, 0, 0, 480, 640)
