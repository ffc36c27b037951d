"""Tiled inference, host side: the properties of the tile plan, the descriptor rows of a tiled batch (fake addresses), the
edge masks, set_tiling's validation and the refusals that need no device, and the NumPy restatement of the merge held to its
own bookkeeping."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _tiles_ref as R  # noqa: E402

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])


def _pipe(loader, **msfa):
    msfa.setdefault("flip", False)
    inner = [dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", **NORM),
             dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])]
    return [dict(type=loader), dict(type="MultiScaleFlipAug", transforms=inner, **msfa)]


# ------------------------------------------------------------------------------------------- 1. the plan
def _axis_cases():
    cases = []
    for t in (1, 2, 7, 48, 640):
        for o in sorted({0, 1, t // 4, t // 2, t - 1}):
            if not 0 <= o < t:
                continue
            for L in sorted({1, t - 1, t, t + 1, t + 2, 2 * t - o, 2 * t - o + 1, 3 * t, 3 * t + 5, 1000, 1920}):
                if L >= 1:
                    cases.append((L, t, o))
    return cases


def test_plan_tiles_properties():
    from radet_amd.ops import plan_tiles
    cases = _axis_cases()
    assert any(L < t for L, t, o in cases) and any(L == t for L, t, o in cases) and any(L == t + 1 for L, t, o in cases)
    assert any(o == 0 for L, t, o in cases) and any(o == t - 1 and t > 1 for L, t, o in cases)
    other = (37, 11, 3)                                            # the other axis: a fixed case of its own
    for L, t, o in cases:
        for tiles, ax in ((plan_tiles(other[0], L, (t, other[1]), (o, other[2])), 0),
                          (plan_tiles(L, other[0], (other[1], t), (other[2], o)), 1)):
            assert tiles.dtype == np.int32 and tiles.ndim == 2 and tiles.shape[1] == 4
            starts = np.unique(tiles[:, ax])
            per_axis = len(starts)
            assert len(tiles) == per_axis * len(np.unique(tiles[:, 1 - ax]))
            assert (tiles[:, 2 + ax] == min(t, L)).all()                         # the size is min(t, L)
            assert starts[0] == 0 and starts[-1] + min(t, L) == L                # first at 0, last ends at L
            assert (tiles[:, ax] >= 0).all() and (tiles[:, ax] + tiles[:, 2 + ax] <= L).all()      # inside the frame
            covered = np.zeros(L, bool)
            for s in starts:
                covered[s:s + min(t, L)] = True
            assert covered.all()                                                 # every pixel is covered
            if per_axis > 1:
                assert (starts[:-1] + t - starts[1:] >= o).all(), (L, t, o)      # consecutive overlap >= o
                assert per_axis == -(-(L - o) // (t - o))
            else:
                assert L <= t
            assert [tuple(r) for r in tiles] == [tuple(r) for r in R.plan(*((other[0], L) if ax == 0 else (L, other[0])),
                                                                          (t, other[1]) if ax == 0 else (other[1], t),
                                                                          (o, other[2]) if ax == 0 else (other[2], o))]
    # row-major, y outer and x inner
    tiles = plan_tiles(75, 100, (48, 36), (16, 12))
    assert [tuple(r) for r in tiles] == [(x, y, 48, 36) for y in (0, 19, 39) for x in (0, 26, 52)]


def test_plan_tiles_full_hd_example():
    from radet_amd.ops import plan_tiles
    tiles = plan_tiles(1080, 1920, (640, 480), 0.25)
    assert tiles.shape == (12, 4)
    assert [tuple(r) for r in tiles] == [(x, y, 640, 480) for y in (0, 300, 600) for x in (0, 426, 853, 1280)]
    assert np.array_equal(tiles, plan_tiles(1080, 1920, (640, 480), (160, 120)))
    assert np.array_equal(tiles, R.plan(1080, 1920, (640, 480), 0.25))
    for bad in ((640, 480), (-1, 0), 1.0, -0.1, (640, 0), "a", 3):
        with pytest.raises(ValueError):
            plan_tiles(1080, 1920, (640, 480), bad)
    for bad in ((0, 480), (640,), 640, (640.0, 480)):
        with pytest.raises(ValueError):
            plan_tiles(1080, 1920, bad, 0)


# ------------------------------------------------------------------------------------------- 2. rows, addresses, masks
def test_edge_masks():
    from radet_amd import kernels as K
    from radet_amd.ops.tiles import edge_masks, tile_rows
    L, T, Rr, B = K.TILE_EDGE_L, K.TILE_EDGE_T, K.TILE_EDGE_R, K.TILE_EDGE_B
    assert (L, T, Rr, B) == (R.L_, R.T_, R.R_, R.B_) == (1, 2, 4, 8)
    rects, edges, row_start = tile_rows([(75, 100), (30, 40)], dict(tile=(48, 36), overlap=(16, 12)))
    assert row_start.tolist() == [0, 10, 12] and rects.shape == (12, 4) and edges.dtype == np.int32
    assert tuple(rects[0]) == (0, 0, 100, 75) and edges[0] == 0                  # the full-frame row
    want = [Rr | B, L | Rr | B, L | B,                                           # top corners and border: no T
            T | Rr | B, L | T | Rr | B, L | T | B,                               # the inner tile: all four
            T | Rr, L | T | Rr, L | T]                                           # bottom: no B
    assert edges[1:10].tolist() == want
    assert tuple(rects[10]) == (0, 0, 40, 30) and tuple(rects[11]) == (0, 0, 40, 30)      # a frame smaller than the tile:
    assert edges[10:].tolist() == [0, 0]                                          # one tile, every side a side of the frame
    for r, e in zip(rects[:10], edges[:10]):
        assert e == R.edge_mask(r, 75, 100)
    assert edge_masks([(0, 0, 5, 5)], 5, 5).tolist() == [0]
    # without the full-frame rows
    rects2, edges2, rs2 = tile_rows([(75, 100), (30, 40)], dict(tile=(48, 36), overlap=(16, 12), full_frame=False))
    assert rs2.tolist() == [0, 9, 10] and np.array_equal(rects2[:9], rects[1:10]) and np.array_equal(edges2[:9], edges[1:10])
    with pytest.raises(NotImplementedError, match="enlarge the tile"):           # 8 x 8 + 1 = 65 rows
        tile_rows([(64, 64)], dict(tile=(8, 8), overlap=0))
    assert len(tile_rows([(64, 64)], dict(tile=(8, 8), overlap=0, full_frame=False))[0]) == 64


def test_descriptor_rows_of_a_tiled_batch():
    from radet_amd import kernels as K
    from radet_amd.datasets.loading import frame_desc_rows, tile_desc_rows
    from radet_amd.ops.tiles import tile_rows
    rng = np.random.RandomState(3)
    host = rng.randint(0, 256, (75, 100, 3)).astype(np.uint8)
    big = torch.zeros(90, 128, 3, dtype=torch.uint8)
    view = big[7:37, 11:51]                                       # a strided view 30 x 40 (row stride 384) into a larger tensor
    frames = [host, view]
    rects, edges, row_start = tile_rows([f.shape[:2] for f in frames], dict(tile=(48, 36), overlap=(16, 12)))
    dst = [(480 + r, 640 - r) for r in range(len(rects))]
    base = 0x7F1200003000
    src, rows, offs, nbytes = tile_desc_rows(frames, rects, row_start, dst, True, base)
    want_src, want_offs, want_bytes = frame_desc_rows(frames, [(75, 100), (30, 40)], True, base)
    assert np.array_equal(src, want_src) and offs == want_offs == [0, None] and nbytes == want_bytes == host.size   # once
    assert rows.shape == (12, K.PREP_DESC_INTS) and rows.dtype == np.int32
    addr_of = [base, view.data_ptr()]
    stride_of = [300, 384]
    assert view.data_ptr() == big.data_ptr() + 7 * 384 + 33
    for b in range(2):
        for r in range(row_start[b], row_start[b + 1]):
            x0, y0, tw, th = (int(v) for v in rects[r])
            row = rows[r]
            addr = int(row[:2].view(np.uint32)[0]) | int(row[:2].view(np.uint32)[1]) << 32
            assert addr == addr_of[b] + y0 * stride_of[b] + 3 * x0               # the frame's address, shifted
            assert tuple(row[2:5]) == (stride_of[b], th, tw)                     # the frame's stride, the tile's h and w
            assert tuple(row[5:7]) == dst[r] and row[7] == K.PREP_TO_RGB
    assert any(int(r[0]) and int(r[1]) for r in rects)                           # (some tile is shifted in both axes)
    with pytest.raises(ValueError, match="leaves"):
        tile_desc_rows(frames, np.array([[60, 0, 48, 36]] * 12), row_start, dst, True, base)
    with pytest.raises(ValueError):
        tile_desc_rows(frames, rects, row_start[:2], dst, True, base)


# ------------------------------------------------------------------------------------------- 3. the public interface
def test_set_tiling_validation_and_refusals():
    from radet_amd.apis import inference as I, set_tiling, set_tta
    from radet_amd.ops.tiles import TileSpec
    from radet_amd.utils import Config
    import radet_amd.apis
    import radet_amd.ops
    assert "set_tiling" in radet_amd.apis.__all__ and {"plan_tiles", "merge_tile_candidates"} <= set(radet_amd.ops.__all__)

    class Model:
        cfg = Config(dict(data=dict(test=dict(pipeline=_pipe("LoadImageFromFile", img_scale=(640, 480))))))
    m = set_tiling(Model(), dict(tile=(640, 480)))
    assert m.tiling == TileSpec((640, 480), (160, 120), True, 0.0, 16, None)
    full = dict(tile=[48, 36], overlap=(16, 12), full_frame=False, edge_margin=1.5, batch=5, nms_pre=200)
    assert set_tiling(m, full).tiling == TileSpec((48, 36), (16, 12), False, 1.5, 5, 200)
    assert set_tiling(m, None).tiling is None
    for bad in (dict(tile=(48, 36), overlaps=0.25), dict(overlap=0.25), dict(), dict(tile=(48, 36), overlap=(48, 0)),
                dict(tile=(48, 36), overlap=(0, 36)), dict(tile=(48, 36), overlap=1.0), dict(tile=(48, 36), overlap=-0.5),
                dict(tile=(48, 36), overlap=(-1, 0)), dict(tile=(0, 36)), dict(tile=48), dict(tile=(48, 36), edge_margin=-1.0),
                dict(tile=(48, 36), edge_margin=float("nan")), dict(tile=(48, 36), batch=0), dict(tile=(48, 36), nms_pre=0),
                "tiles"):
        with pytest.raises(ValueError):
            set_tiling(m, bad)
    assert m.tiling is None                                        # (a refused request leaves the model as it was)
    set_tiling(m, dict(tile=(48, 36)))
    frame = np.zeros((75, 100, 3), np.uint8)
    for names in ("a.png", ["a.png", "b.png"], [frame, "a.png"]):
        with pytest.raises(NotImplementedError, match="file names"):
            I.inference_detector(m, names)
    with pytest.raises(NotImplementedError, match="normalised"):
        I.inference_detector(m, torch.zeros(1, 3, 64, 64))
    set_tta(m, dict(img_scale=[(64, 48), (96, 80)], flip=False))
    with pytest.raises(NotImplementedError, match="set_tta"):     # tiling + a set_tta override
        I.inference_detector(m, frame)
    with pytest.raises(NotImplementedError, match="set_tta"):
        next(I.detect_frames(m, [frame]))
    set_tta(m, None)

    class Views:                                                   # tiling + a multi-view config
        cfg = Config(dict(data=dict(test=dict(pipeline=_pipe("LoadImageFromFile", img_scale=(64, 48), flip=True)))))
    v = set_tiling(Views(), dict(tile=(48, 36)))
    with pytest.raises(NotImplementedError, match="views"):
        I.inference_detector(v, frame)
    with pytest.raises(NotImplementedError, match="views"):
        next(I.detect_frames(v, [frame]))
    assert I.inference_detector(m, []) == []                       # (an empty list has no rows to run)


# ------------------------------------------------------------------------------------------- 4. the restatement, against itself
def test_merge_restatement_consistency():
    rng = np.random.RandomState(2)
    rows_per_image = [1, 4]
    shapes = [(36, 48, 3)] * 5
    sfs = [np.array([0.48, 0.5, 0.48, 0.5], np.float32)] + [np.ones(4, np.float32)] * 4
    offsets = [(0, 0), (0, 0), (26, 0), (0, 19), (26, 19)]
    masks = [0, R.R_ | R.B_, R.L_ | R.B_, R.T_ | R.R_, R.L_ | R.T_]
    caps, counts = [6, 9, 9, 9, 9], [6, 9, 12, -3, 4]
    boxes, scores, ctr, labels = [], [], [], []
    for c in caps:
        p = rng.random_sample((c, 4)).astype(np.float32) * np.array([48, 36, 48, 36], np.float32)
        b = np.concatenate([np.minimum(p[:, :2], p[:, 2:]), np.maximum(p[:, :2], p[:, 2:])], -1)
        b[::3, 2] = 48.0                                           # every third box lies on the right side of its row
        b[1::3, 1] = 0.0                                           # ... and every third on the top
        boxes.append(b)
        scores.append(rng.random_sample(c).astype(np.float32))
        ctr.append(rng.random_sample(c).astype(np.float32))
        labels.append(rng.randint(0, 21, c).astype(np.int64))
    out = R.merge(boxes, scores, ctr, labels, counts, rows_per_image, shapes, sfs, offsets, masks)
    clamped = [min(max(n, 0), c) for n, c in zip(counts, caps)]
    assert [len(o[0]) + o[4] for o in out] == [clamped[0], sum(clamped[1:])]     # kept + dropped = the clamped counts
    assert out[0][4] == 0 and len(out[0][0]) == 6                                # mask 0 keeps everything, on an edge or not
    assert out[1][4] > 0 and len(out[1][0]) > 0
    # the full-frame row: mapped back by the division alone; a tile: by its offset alone
    assert np.array_equal(out[0][0], (boxes[0] / sfs[0]).astype(np.float32))
    kept1 = R.keep_mask(boxes[1], shapes[1], masks[1], 0.0)
    assert not kept1[::3].any() and kept1[1::3].all()                             # row 1: R is a cut, T is the frame's side
    n1 = int(kept1.sum())
    assert np.array_equal(out[1][0][:n1], boxes[1][kept1]) and np.array_equal(out[1][1][:n1], scores[1][kept1])   # stable
    # a margin only ever drops more
    wide = R.merge(boxes, scores, ctr, labels, counts, rows_per_image, shapes, sfs, offsets, masks, 4.0)
    assert wide[1][4] >= out[1][4] and wide[0][4] == 0
    assert [len(o[0]) + o[4] for o in wide] == [clamped[0], sum(clamped[1:])]
