"""The view row of the resize and of both mask kernels ({Hr, Wr, wy0, wx0, wh, ww, oy, ox, h, w, flip, fill}): the whole-source /
whole-output row against the call without rows, and a source window that overhangs composed with an output window against
the materialised host chain -- paste on a filled canvas, slice the source window, resize (oracle/imgproc.py, oracle/masks.py),
slice the output window, flip.  Every comparison is array_equal."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import imgproc, masks as om  # noqa: E402
from _rle_cases import edge_masks  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0xAB
FILL = (11, 140, 250)
SOURCES = [(13, 17), (9, 31)]
VIRTUAL = [(23, 29), (7, 11)]
FLIPS = [None, "horizontal", "vertical", "diagonal"]


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def src_windows(h, w):
    """(wy0, wx0, wh, ww) that overhang an h x w source: negative origin; past the far edge; both; entirely outside"""
    return [(-3, -2, h, w), (2, 3, h + 1, w + 4), (-2, -5, h + 5, w + 7), (h + 2, w + 1, 5, 6)]


def out_windows(Hr, Wr):
    """(oy, ox, h, w) inside Hr x Wr: at the origin, in the far corner, one row high, one column wide"""
    return [(0, 0, Hr // 2 + 1, Wr // 2 + 1), (Hr - 3, Wr - 5, 3, 5), (Hr // 2, 0, 1, Wr), (0, Wr // 3, Hr, 1)]


def host_window(src, win, fill):
    """the canvas that holds the image and the window, filled, the image pasted, the window sliced"""
    y0, x0, wh, ww = win
    h, w = src.shape[:2]
    top, left = max(0, -y0), max(0, -x0)
    canvas = np.empty((max(h, y0 + wh) + top, max(w, x0 + ww) + left, *src.shape[2:]), src.dtype)
    canvas[:] = fill
    canvas[top:top + h, left:left + w] = src
    return np.ascontiguousarray(canvas[y0 + top:y0 + top + wh, x0 + left:x0 + left + ww])


def composed(src_hw):
    """every (source window, virtual size, output window) of one source size"""
    return [(sw, hw, ow) for sw in src_windows(*src_hw) for hw in VIRTUAL for ow in out_windows(*hw)]


def row(sw, hw, ow, flip=0, fill=0):
    return (*hw, *sw, *ow, flip, fill)


# ------------------------------------------------------------------------------------------------ the whole view
@pytest.mark.parametrize("channels", [1, 3])
def test_whole_view_resize_equals_no_rows(channels):
    from radet_amd import kernels as K
    rs = np.random.RandomState(1)
    srcs = [rs.randint(0, 256, (*hw, channels)).astype(np.uint8) for hw in SOURCES]
    jobs = [(k, hw) for k in range(len(srcs)) for hw in VIRTUAL]                     # an up-scale and a down-scale of each
    soff = np.cumsum([0] + [s.shape[0] * s.shape[1] for s in srcs])
    doff = np.cumsum([0] + [h * w for _, (h, w) in jobs])
    sdesc = _t(np.array([(soff[k], *srcs[k].shape[:2]) for k, _ in jobs], np.int32))
    ddesc = _t(np.array([(doff[j], h, w) for j, (_, (h, w)) in enumerate(jobs)], np.int32))
    views = _t(np.array([row((0, 0, *srcs[k].shape[:2]), hw, (0, 0, *hw), fill=0x123456) for k, hw in jobs], np.int32))
    src = _t(np.concatenate([s.reshape(-1) for s in srcs]))
    got = []
    for v in (None, views):
        dst = torch.full((int(doff[-1]) * channels,), GUARD, dtype=torch.uint8, device=_dev())
        K.resize_linear_u8(src, sdesc, dst, ddesc, len(jobs), max(h * w for _, (h, w) in jobs), channels, views=v)
        got.append(dst.cpu().numpy())
    np.testing.assert_array_equal(got[1], got[0])
    for j, (k, (h, w)) in enumerate(jobs):                                           # (and the plain call is the oracle's resize)
        want = imgproc.resize_linear_u8(srcs[k] if channels == 3 else srcs[k][..., 0], (w, h))
        np.testing.assert_array_equal(got[0][doff[j] * channels:doff[j + 1] * channels], want.reshape(-1))


@pytest.mark.parametrize("normalize", [False, True])
def test_whole_view_mask_transform_equals_no_rows(normalize):
    from radet_amd import kernels as K
    for (H, W), hw, out_hw in zip(SOURCES, VIRTUAL, [(24, 32), (9, 13)]):
        e = edge_masks(H, W)
        m = np.stack([e["zeros"], e["random"] * 255, e["span"]]).astype(np.uint8)
        m[1, 3, 4] = 7
        src = _t(m)
        for fl, name in enumerate(FLIPS):
            plain = K.mask_transform(src, out_hw, hw, name, 9, normalize)
            views = _t(np.array([row((0, 0, H, W), hw, (0, 0, *hw), flip=fl)] * len(m), np.int32))
            assert torch.equal(K.mask_transform(src, out_hw, pad_val=9, normalize=normalize, views=views), plain), (hw, name)


def _runs(H, W):
    """run-list parts of three masks and their decoded bitmaps: a compressed random mask, a checkerboard, all ones (columns
    that end in ones: a sample below or right of the image must not land in the next column's run)"""
    from radet_amd.core import rle
    e = edge_masks(H, W)
    segs = [dict(size=[H, W], counts=rle.string_from_counts(rle.rle_from_mask(e[k])).decode("ascii")) for k in ("random", "checker", "ones")]
    parts = [rle.parts_from_segmentation(s, H, W) for s in segs]
    return parts, np.stack([rle.mask_from_parts(p, H, W) for p in parts])


def _rle(K, parts, H, W, flips, out_hw, with_plain, **kw):
    from radet_amd.core import rle
    ends, prows, mrows = rle.pack_runs(parts, H, W, flips)
    return K.rle_masks(_t(ends.view(np.int32)), _t(prows), _t(mrows), out_hw, pad_val=9, with_plain=with_plain, **kw)


@pytest.mark.parametrize("with_plain", [False, True])
def test_whole_view_rle_masks_equals_no_rows(with_plain):
    from radet_amd import kernels as K
    for (H, W), hw, out_hw in zip(SOURCES, VIRTUAL, [(24, 32), (9, 13)]):
        parts, _ = _runs(H, W)
        parts, flips = parts * 2, np.repeat([False, True], len(parts))
        views = _t(np.array([row((0, 0, H, W), hw, (0, 0, *hw))] * len(parts), np.int32))
        plain = _rle(K, parts, H, W, flips, out_hw, with_plain, resized_hw=hw)
        got = _rle(K, parts, H, W, flips, out_hw, with_plain, views=views)
        if not with_plain:
            assert torch.equal(got, plain)
        else:                                                  # (the second result is defined for the flipped masks only)
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1][flips], plain[1][flips])


# ------------------------------------------------------------------------------------------------ the composed case
@pytest.mark.parametrize("align", [1, 4])
def test_composed_resize_equals_the_host_chain(align):
    from radet_amd import kernels as K
    rs = np.random.RandomState(2)
    srcs = [rs.randint(0, 256, (*hw, 3)).astype(np.uint8) for hw in SOURCES]
    jobs = [(k, *c) for k, s in enumerate(srcs) for c in composed(s.shape[:2])]
    soff = np.cumsum([0] + [s.shape[0] * s.shape[1] for s in srcs])
    ddesc, o = [], 64
    for _, _, _, (_, _, h, w) in jobs:
        ddesc.append((o, h, w))
        o += -(-h * w // align) * align
    total = o + 64
    assert len({d[1] * d[2] % 4 for d in ddesc}) > 1
    dst = torch.full((total * 3,), GUARD, dtype=torch.uint8, device=_dev())
    fill = FILL[0] | FILL[1] << 8 | FILL[2] << 16
    K.resize_linear_u8(_t(np.concatenate([s.reshape(-1) for s in srcs])), _t(np.array([(soff[k], *srcs[k].shape[:2]) for k, *_ in jobs], np.int32)),
                       dst, _t(np.array(ddesc, np.int32)), len(jobs), max(d[1] * d[2] for d in ddesc), 3,
                       views=_t(np.array([row(sw, hw, ow, fill=fill) for _, sw, hw, ow in jobs], np.int32)))
    host = dst.cpu().numpy()
    written = np.zeros(total * 3, bool)
    resized = {}
    for (k, sw, (Hr, Wr), (oy, ox, h, w)), (off, _, _) in zip(jobs, ddesc):
        assert off % align == 0
        if (k, sw, Hr, Wr) not in resized:
            resized[(k, sw, Hr, Wr)] = imgproc.resize_linear_u8(host_window(srcs[k], sw, FILL), (Wr, Hr))
        want = resized[(k, sw, Hr, Wr)][oy:oy + h, ox:ox + w]
        np.testing.assert_array_equal(host[off * 3:(off + h * w) * 3].reshape(h, w, 3), want, err_msg=str((k, sw, (Hr, Wr), (oy, ox, h, w))))
        written[off * 3:(off + h * w) * 3] = True
    assert (host[~written] == GUARD).all(), "bytes outside the outputs were written"
    outside = [resized[(k, sw, Hr, Wr)] for k, sw, (Hr, Wr), _ in jobs if sw[0] >= srcs[k].shape[0]]
    assert outside and all((r == np.array(FILL, np.uint8)).all() for r in outside)


def mask_want(m, sw, hw, ow, flip, out_hw):
    """np.pad / slice of the masks, nearest resize, slice, flip inside the window, pad"""
    oy, ox, h, w = ow
    r = om.resize_nearest(host_window(m.transpose(1, 2, 0), sw, 0).transpose(2, 0, 1), hw)[:, oy:oy + h, ox:ox + w]
    return om.pad(om.flip(r, FLIPS[flip]) if flip else r, out_hw, 9)


@pytest.mark.parametrize("Wd", [32, 33])
def test_composed_mask_transform_equals_the_host_chain(Wd):
    from radet_amd import kernels as K
    out_hw = (24, Wd)
    for H, W in SOURCES:
        e = edge_masks(H, W)
        m = np.stack([e["random"] * 255, e["span"], e["ones"] * 3]).astype(np.uint8)
        m[0, 3, 4] = 7                                         # (a value below the maximum normalises to 0)
        G = len(m)
        cases = [(*c, fl) for c in composed((H, W)) for fl in range(4)]
        views = _t(np.repeat(np.array([row(*c) for c in cases], np.int32), G, axis=0))
        got = K.mask_transform(_t(m).repeat(len(cases), 1, 1), out_hw, pad_val=9, normalize=True, views=views).cpu().numpy()
        raw = K.mask_transform(_t(m).repeat(len(cases), 1, 1), out_hw, pad_val=9, views=views).cpu().numpy()
        for n, case in enumerate(cases):
            np.testing.assert_array_equal(got[n * G:(n + 1) * G], mask_want(om.normalize(m), *case, out_hw), err_msg=str(case))
            np.testing.assert_array_equal(raw[n * G:(n + 1) * G], mask_want(m, *case, out_hw), err_msg=str(case))


@pytest.mark.parametrize("Wd", [32, 33])
def test_composed_rle_masks_equals_the_bitmap_kernel(Wd):
    from radet_amd import kernels as K
    out_hw = (24, Wd)
    for H, W in SOURCES:
        parts, decoded = _runs(H, W)
        G = len(parts)
        cases = [(*c, fl) for c in composed((H, W)) for fl in (0, 1)]
        rows = np.repeat(np.array([row(*c) for c in cases], np.int32), G, axis=0)
        bitmap = K.mask_transform(_t(decoded).repeat(len(cases), 1, 1), out_hw, pad_val=9, normalize=True, views=_t(rows)).cpu().numpy()
        flips = rows[:, 10].astype(bool)
        rows[:, 10] = 0                                        # (the flip is the mask row's)
        got, plain = _rle(K, parts * len(cases), H, W, flips, out_hw, True, views=_t(rows))
        got, plain = got.cpu().numpy(), plain.cpu().numpy()
        np.testing.assert_array_equal(got, bitmap)
        for n, case in enumerate(cases):
            np.testing.assert_array_equal(got[n * G:(n + 1) * G], mask_want(decoded, *case, out_hw), err_msg=str(case))
            if case[3]:                                        # both orientations from one lookup
                np.testing.assert_array_equal(plain[n * G:(n + 1) * G], mask_want(decoded, *case[:3], 0, out_hw), err_msg=str(case))
        assert np.array_equal(_rle(K, parts * len(cases), H, W, flips, out_hw, False, views=_t(rows)).cpu().numpy(), got)
