"""Tiled inference on the device: the rows of a tiled batch against the single-view frame pipeline on copied slices,
radet_merge_tiles against the NumPy restatement, its argument errors, the composition of rows against an oracle built from
existing pieces, inference_detector / detect_frames / crops= with a tiling set on the model (set_tiling), and the refusals."""
import contextlib
import os
import random
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _tiles_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
SCALE = (640, 480)
# frames 75 x 100 and 30 x 40 (smaller than the tile): 1 + 9 and 1 + 1 rows, and every row resizes to 480 x 640
TILING = dict(tile=(48, 36), overlap=(16, 12))
NMS_PRE, MAX_PER_IMG = 200, 100
FRAME_SEED = 11


def _pipe(loader, **msfa):
    msfa.setdefault("flip", False)
    return [dict(type=loader),
            dict(type="MultiScaleFlipAug", transforms=[
                dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", **NORM),
                dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])],
                **msfa)]


def _pipeline():
    from radet_amd.datasets.loading import ImagePipeline
    return ImagePipeline(_pipe("LoadImageFromWebcam", img_scale=SCALE))


@pytest.fixture(scope="module")
def frames():
    rng = np.random.RandomState(FRAME_SEED)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((75, 100), (30, 40))]


# ------------------------------------------------------------------------------------------- 1. the rows of a tiled batch
@pytest.fixture(scope="module")
def slice_rows(frames):
    """what the existing single-view frame pipeline writes for the 12 copied slices, passed as frames: computed once"""
    from radet_amd.ops.tiles import tile_rows
    rects, _, row_start = tile_rows([f.shape[:2] for f in frames], TILING)
    assert row_start.tolist() == [0, 10, 12]
    p = _pipeline()
    copies = [np.ascontiguousarray(frames[b][y0:y0 + th, x0:x0 + tw]).copy()
              for b in range(2) for x0, y0, tw, th in rects[row_start[b]:row_start[b + 1]].tolist()]
    planned = [p.plan(dict(img=c, bbox_fields=[], mask_fields=[], seg_fields=[]), random, np.random) for c in copies]
    data = p.run(planned, collate=True)
    img = data["img"][0] if isinstance(data["img"], (list, tuple)) else data["img"]
    metas = data["img_metas"][0] if isinstance(data["img"], (list, tuple)) else data["img_metas"]
    torch.cuda.synchronize()
    assert img.shape == (12, 3, 480, 640)
    return img.clone(), metas


@pytest.mark.parametrize("kind", ["ndarray", "device", "strided"])
def test_tile_rows_equal_single_view_pipeline(frames, slice_rows, kind):
    want, want_metas = slice_rows
    keep = []
    if kind == "ndarray":
        given = frames
    elif kind == "device":
        given = [torch.from_numpy(f).cuda() for f in frames]
    else:
        given = []
        for f in frames:
            big = torch.full((f.shape[0] + 9, f.shape[1] + 15, 3), 201, dtype=torch.uint8, device="cuda")
            view = big[4:4 + f.shape[0], 7:7 + f.shape[1]]
            view.copy_(torch.from_numpy(f).cuda())
            assert not view.is_contiguous()
            keep.append(big)
            given.append(view)
    plan = _pipeline().run_tile_rows(given, TILING)
    torch.cuda.synchronize()
    assert plan["img"].shape == (12, 3, 480, 640) and plan["row_start"].tolist() == [0, 10, 12]
    assert plan["table"].shape == (2 + 12, 8)
    for r in range(12):
        assert torch.equal(plan["img"][r], want[r]), (kind, r)           # bit for bit
        for k in ("img_shape", "pad_shape", "ori_shape"):
            assert tuple(plan["img_metas"][r][k]) == tuple(want_metas[r][k])
        assert np.array_equal(plan["img_metas"][r]["scale_factor"], want_metas[r]["scale_factor"])
    assert not torch.equal(plan["img"][1], plan["img"][2])              # (neighbouring tiles differ)


# ------------------------------------------------------------------------------------------- 2. the merge kernel
CAPS = [[300], [1, 7, 64, 257, 300], [64, 257, 7]]                        # B = 3 with 1, 5 and 3 rows
SENTINEL = 7.0


def _merge_case(variant):
    """synthetic lists for B = 3 images with 1, 5 and 3 rows.  Variants 0 and 1 (margins 0 and 1.5) cover the 16 edge masks
    between them and hold counts of 0, cap, above cap and below 0; variant 2 keeps every candidate of image 1, whose
    capacities add up to cap_out."""
    rng = np.random.RandomState(40 + variant)
    masks = [[0, 1, 2, 3, 4, 5, 6, 7, 8], [15, 9, 10, 11, 12, 13, 14, 3, 15], [5, 0, 0, 0, 0, 0, 10, 12, 15]][variant]
    margin = [0.0, 1.5, 0.0][variant]
    caps = [c for img in CAPS for c in img]
    counts = [[300, 1, 7, 70, 257, 150, 64, 0, -3], [120, 1, 3, 64, 300, 300, 64, 257, 9],
              [290, 1, 7, 64, 257, 300, -1, 200, 7]][variant]
    shapes = [(480, 640, 3), (36, 48, 3), (45, 64, 3), (37, 53, 3), (480, 640, 3), (67, 96, 3), (36, 48, 3), (480, 640, 3),
              (55, 80, 3)]
    sfs = [np.array([6.4, 6.4, 6.4, 6.4], np.float32), np.array([48 / 37, 36 / 29, 48 / 37, 36 / 29], np.float32),
           np.array([64 / 53, 45 / 37, 64 / 53, 45 / 37], np.float32), np.ones(4, np.float32),
           np.array([640 / 48, 480 / 36, 640 / 48, 480 / 36], np.float32), np.array([0.7, 0.71, 0.7, 0.71], np.float32),
           np.array([1.06, 1.0576923, 1.06, 1.0576923], np.float32), np.array([3.0, 3.0, 3.0, 3.0], np.float32),
           np.array([96 / 53, 67 / 37, 96 / 53, 67 / 37], np.float32)]
    offsets = [(0, 0), (0, 0), (26, 0), (853, 300), (1280, 600), (7, 19), (0, 0), (426, 39), (52, 1)]
    boxes, scores, ctr, labels = [], [], [], []
    for r, cap in enumerate(caps):
        h, w = np.float32(shapes[r][0]), np.float32(shapes[r][1])
        lo = rng.uniform(3.0, 12.0, (cap, 2)).astype(np.float32)
        hi = (np.array([w, h], np.float32) - rng.uniform(3.0, 12.0, (cap, 2)).astype(np.float32)).astype(np.float32)
        b = np.concatenate([lo, hi], -1)                           # strictly inside, further than any margin here
        tiny = np.nextafter(np.float32(0), np.float32(1))
        m = np.float32(1.5)
        special = [(0, np.float32(0)), (1, np.float32(0)), (2, w), (3, h),                                  # exactly on an edge
                   (0, tiny), (1, tiny), (2, np.nextafter(w, np.float32(0))), (3, np.nextafter(h, np.float32(0))),   # one ulp inside
                   (0, m), (2, np.float32(w - m)), (1, np.nextafter(m, np.float32(2))),                     # at / just inside 1.5
                   (3, np.nextafter(np.float32(h - m), np.float32(0))), (0, np.float32(1.0)), (3, np.float32(h - 1.0))]
        if variant != 2 or not 1 <= r <= 5:
            for i in range(cap):
                k, v = special[(i + r) % len(special)]
                if i % 2 == 0:
                    b[i, k] = v
        boxes.append(b)
        scores.append(rng.random_sample(cap).astype(np.float32))
        ctr.append(rng.random_sample(cap).astype(np.float32))
        labels.append(rng.randint(0, 21, cap).astype(np.int64))
    case = dict(boxes=boxes, scores=scores, ctr=ctr, labels=labels, counts=counts, rows_per_image=[len(c) for c in CAPS],
                img_shapes=shapes, scale_factors=sfs, offsets=offsets, edge_masks=masks, edge_margin=margin)
    want = R.merge(**case)
    # checked on the CPU, when the case is built: every image with an inner edge both keeps and drops
    r0 = 0
    for b, img in enumerate(CAPS):
        if any(masks[r0:r0 + len(img)]) and not (variant == 2 and b == 1):
            assert len(want[b][0]) > 0 and want[b][4] > 0, (variant, b)
        r0 += len(img)
    return case, want


def test_merge_cases_cover_what_they_claim():
    masks, counts_seen = set(), set()
    caps = [c for img in CAPS for c in img]
    for variant in (0, 1):
        case, want = _merge_case(variant)
        masks |= set(case["edge_masks"])
        for n, c in zip(case["counts"], caps):
            counts_seen.add("zero" if n == 0 else "neg" if n < 0 else "cap" if n == c else "above" if n > c else "part")
    assert masks == set(range(16)) and counts_seen == {"zero", "neg", "cap", "above", "part"}
    case, want = _merge_case(2)
    assert len(want[1][0]) == sum(CAPS[1]) == 629 and want[1][4] == 0            # kept == cap_out
    # the division and the add both round: neither float32 step is exact on row 4 (scale 13.33, offset (1280, 600))
    case, want = _merge_case(0)
    b, sf = case["boxes"][4][1::2], case["scale_factors"][4]
    q = (b / sf).astype(np.float32)
    assert (q.astype(np.float64) != b.astype(np.float64) / sf.astype(np.float64)).any()
    off = np.array([1280, 600, 1280, 600], np.float64)
    assert ((q + off.astype(np.float32)).astype(np.float32).astype(np.float64) != q.astype(np.float64) + off).any()


def _launch_merge(case, prefill=SENTINEL):
    """radet_merge_tiles through kernels.merge_tiles on buffers of the test's own, prefilled with a sentinel"""
    from radet_amd import kernels as K
    dev = torch.device("cuda")
    caps = np.array([len(s) for s in case["scores"]], np.int64)
    Rn, B = len(caps), len(case["rows_per_image"])
    row_start = np.concatenate([[0], np.cumsum(case["rows_per_image"])]).astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(caps)])[:Rn]
    cap_out = max(int(caps[row_start[b]:row_start[b + 1]].sum()) for b in range(B))
    desc = K.tile_desc_rows(np.array([s[:2] for s in case["img_shapes"]], np.float32), np.stack(case["scale_factors"]),
                            np.array(case["offsets"], np.float32), np.array(case["edge_masks"], np.int32), starts, caps)
    pb = torch.from_numpy(np.concatenate(case["boxes"])).to(dev)
    ps, pc = (torch.from_numpy(np.concatenate(case[k])).to(dev) for k in ("scores", "ctr"))
    pl = torch.from_numpy(np.concatenate(case["labels"])).to(dev)
    cnt = torch.tensor(case["counts"], dtype=torch.int32, device=dev)
    ob = torch.full((B, cap_out, 4), prefill, device=dev)
    osc, oct_ = torch.full((B, cap_out), prefill, device=dev), torch.full((B, cap_out), prefill, device=dev)
    ol = torch.full((B, cap_out), int(prefill), dtype=torch.long, device=dev)
    oc, od = torch.full((B,), -9, dtype=torch.int32, device=dev), torch.full((B,), -9, dtype=torch.int32, device=dev)
    K.merge_tiles(desc, torch.from_numpy(desc).to(dev), row_start, torch.from_numpy(row_start).to(dev), B, pb, ps, pc, pl, cnt,
                  case["edge_margin"], cap_out, ob, osc, oct_, ol, oc, od)
    torch.cuda.synchronize()
    return ob, osc, oct_, ol, oc, od, cap_out


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_merge_tiles_equals_restatement(variant):
    case, want = _merge_case(variant)
    ob, osc, oct_, ol, oc, od, cap_out = _launch_merge(case)
    assert cap_out == 629
    assert oc.cpu().tolist() == [len(w[0]) for w in want]
    assert od.cpu().tolist() == [w[4] for w in want]
    print(f"variant {variant}: kept {oc.cpu().tolist()}, dropped {od.cpu().tolist()}")
    for b, (wb, ws, wc, wl, _) in enumerate(want):
        n = len(wb)
        assert np.array_equal(ob[b, :n].cpu().numpy().view(np.uint32), wb.view(np.uint32)), b      # bit for bit
        assert np.array_equal(osc[b, :n].cpu().numpy(), ws) and np.array_equal(oct_[b, :n].cpu().numpy(), wc)
        assert np.array_equal(ol[b, :n].cpu().numpy(), wl)
        # slots at and beyond the count are not written
        assert (ob[b, n:] == SENTINEL).all() and (osc[b, n:] == SENTINEL).all() and (oct_[b, n:] == SENTINEL).all()
        assert (ol[b, n:] == int(SENTINEL)).all()
    if variant == 2:
        assert int(oc[1]) == cap_out


def test_merge_tile_candidates_stand_alone():
    from radet_amd import ops
    case, want = _merge_case(1)
    ob, osc, oct_, ol, oc, od = ops.merge_tile_candidates(**case)
    torch.cuda.synchronize()
    assert ob.shape == (3, 629, 4) and ol.dtype == torch.int64 and oc.dtype == od.dtype == torch.int32
    assert oc.cpu().tolist() == [len(w[0]) for w in want] and od.cpu().tolist() == [w[4] for w in want]
    for b, (wb, ws, wc, wl, _) in enumerate(want):
        n = len(wb)
        assert np.array_equal(ob[b, :n].cpu().numpy().view(np.uint32), wb.view(np.uint32))
        assert np.array_equal(osc[b, :n].cpu().numpy(), ws) and np.array_equal(ol[b, :n].cpu().numpy(), wl)
    with pytest.raises(ValueError):
        ops.merge_tile_candidates(**dict(case, rows_per_image=[1, 5, 2]))


# ------------------------------------------------------------------------------------------- 3. argument errors
def test_merge_tiles_argument_errors():
    from radet_amd import _lib, kernels as K
    lib = _lib.load()
    dev = torch.device("cuda")
    B, cap = 2, 4
    row_start = np.array([0, 1, 3], np.int32)
    Rn = 3
    pool = Rn * cap
    desc = K.tile_desc_rows(np.full((Rn, 2), 32.0), np.ones((Rn, 4)), np.zeros((Rn, 2)), [0, 4, 1], np.arange(Rn) * cap, [cap] * Rn)
    ddev, rdev = torch.from_numpy(desc).to(dev), torch.from_numpy(row_start).to(dev)
    pb = torch.full((pool, 4), 5.0, device=dev)
    ps, pc = torch.zeros(pool, device=dev), torch.zeros(pool, device=dev)
    pl, cnt = torch.zeros(pool, dtype=torch.long, device=dev), torch.full((Rn,), cap, dtype=torch.int32, device=dev)
    cap_out = 2 * cap
    ob = torch.full((B, cap_out, 4), 7.0, device=dev)
    osc, oct_ = torch.full((B, cap_out), 7.0, device=dev), torch.full((B, cap_out), 7.0, device=dev)
    ol = torch.full((B, cap_out), 7, dtype=torch.long, device=dev)
    oc, od = torch.full((B,), 7, dtype=torch.int32, device=dev), torch.full((B,), 7, dtype=torch.int32, device=dev)

    def args(desc_host=desc, rs=row_start, B=B, pool=pool, cap_out=cap_out, boxes=pb, margin=0.0, dropped=od, rs_dev=rdev):
        return (desc_host.ctypes.data, ddev.data_ptr(), rs.ctypes.data, None if rs_dev is None else rs_dev.data_ptr(), B, pool,
                None if boxes is None else boxes.data_ptr(), ps.data_ptr(), pc.data_ptr(), pl.data_ptr(), cnt.data_ptr(), margin,
                cap_out, ob.data_ptr(), osc.data_ptr(), oct_.data_ptr(), ol.data_ptr(), oc.data_ptr(),
                None if dropped is None else dropped.data_ptr(), None)

    def changed(col, row, value):
        d = desc.copy()
        d[row, col] = value
        return d
    many = np.array([0, 1, 1 + K.TILE_MAX_ROWS + 1], np.int32)
    many_desc = np.concatenate([desc[:1]] + [desc[1:2]] * (K.TILE_MAX_ROWS + 1))
    bad = [dict(boxes=None), dict(dropped=None), dict(rs_dev=None),                     # a NULL pointer with B > 0
           dict(B=65536), dict(B=-1), dict(cap_out=0), dict(cap_out=65537),
           dict(rs=many, desc_host=many_desc, cap_out=65536),                           # 65 rows for an image
           dict(rs=np.array([0, 0, 3], np.int32)), dict(rs=np.array([0, 3, 3], np.int32)),      # an image with no row
           dict(rs=np.array([1, 2, 3], np.int32)),                                      # rows that do not start at 0
           dict(desc_host=changed(9, 2, pool - cap + 1)), dict(desc_host=changed(9, 0, -1)), dict(pool=pool - 1),   # a row leaves the pool
           dict(desc_host=changed(10, 1, -1)),                                          # a negative cap
           dict(cap_out=cap_out - 1),                                                   # the caps of image 1 exceed cap_out
           dict(desc_host=changed(8, 1, 16)), dict(desc_host=changed(8, 2, -1)),        # edge bits outside 0..15
           dict(margin=-0.5), dict(margin=float("nan")), dict(margin=float("inf"))]
    assert K.TILE_MAX_ROWS == 64 and K.TILE_DESC_INTS == 11
    for kw in bad:
        assert lib.radet_merge_tiles(*args(**kw)) == -1, kw
    assert lib.radet_merge_tiles(*args(B=0)) == 0                  # no images: OK, no launch
    # through the package: the error surfaces, and it is the only call that was made
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        with pytest.raises(_lib.RadetHipError):
            K.merge_tiles(changed(8, 1, 16), ddev, row_start, rdev, B, pb, ps, pc, pl, cnt, 0.0, cap_out, ob, osc, oct_, ol, oc, od)
    finally:
        _lib.call = call
    assert seen == ["radet_merge_tiles"]
    torch.cuda.synchronize()
    for t in (ob, osc, oct_, ol, oc, od):
        assert (t == 7).all()                                      # nothing was launched
    assert lib.radet_merge_tiles(*args()) == 0
    torch.cuda.synchronize()
    # row 1 (mask R, x2 = 5 < 32) and row 2 (mask L, x1 = 5 > 0) keep everything
    assert oc.cpu().tolist() == [cap, 2 * cap] and od.cpu().tolist() == [0, 0] and (ob[1] == 5).all() and (ob[0, cap:] == 7).all()


# ------------------------------------------------------------------------------------------- the tiny detector
@pytest.fixture(scope="module")
def det():
    """the detector of tests/test_gpu_tta.py: synthetic weights, cls bias + 2"""
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    d = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().eval()
    synth_fill(d, seed=0)
    with torch.no_grad():
        d.bbox_head.atss_cls.bias += 2.0                       # (scores above the threshold: the comparisons are not vacuous)
    d.cfg = Config(dict(data=dict(test=dict(pipeline=_pipe("LoadImageFromFile", img_scale=SCALE)))))
    return d


@contextlib.contextmanager
def _tiling(det, tiling):
    """the tiling on the (module-wide) detector for the length of a block"""
    from radet_amd.apis import set_tiling
    set_tiling(det, tiling)
    try:
        yield det
    finally:
        set_tiling(det, None)


def _same_results(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert len(ra) == len(rb)
        for ca, cb in zip(ra, rb):
            assert ca.dtype == cb.dtype and np.array_equal(ca, cb)


# ------------------------------------------------------------------------------------------- 4. the composition of rows
NMS_CFGS = dict(
    vote=dict(type="vote", iou_threshold=0.65, cluster_score=["cls", "iou"], vote_score=["iou", "cls"], iou_enable=False),
    nms=dict(type="nms", iou_threshold=0.5),
    soft_nms=dict(type="soft_nms", iou_threshold=0.3, method="linear", min_score=0.05, split_thr=-1),
)


@pytest.fixture(scope="module")
def rows(det, frames):
    """the 12 rows of the two frames and, per forward batching (one batch of 12; 5 + 5 + 2), the candidates an existing
    forward pass + radet_decode_candidates call give per row (row coordinates), computed once for the three NMS types"""
    from radet_amd import kernels as K
    plan = _pipeline().run_tile_rows(frames, dict(TILING, nms_pre=NMS_PRE))
    rt = det.runtime()
    e = rt.engine
    Rn = 12
    hw_all = torch.tensor([[float(m["img_shape"][0]), float(m["img_shape"][1])] for m in plan["img_metas"]], device="cuda")
    cands = {}
    with torch.no_grad():
        for batch in (16, 5):
            per_row = []
            for i0 in range(0, Rn, batch):
                n = min(batch, Rn - i0)
                rt.forward(plan["img"][i0:i0 + n])
                nlvl = e.nlvl
                cap = nlvl * NMS_PRE
                bx, sc = torch.zeros(n, cap, 4, device="cuda"), torch.zeros(n, cap, device="cuda")
                ct, lb = torch.zeros(n, cap, device="cuda"), torch.zeros(n, cap, dtype=torch.long, device="cuda")
                cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
                ws = torch.empty(K.decode_ws_bytes(n, nlvl, NMS_PRE), dtype=torch.uint8, device="cuda")
                K.decode_candidates(e.buf["cls"], e.buf["reg_u"], e.buf["iou"], e.scales_tensor(), e.ldesc, nlvl, n,
                                    rt.num_classes, float(det.test_cfg["score_thr"]), NMS_PRE, hw_all[i0:i0 + n], None, bx, sc, ct,
                                    lb, cnt, ws)
                torch.cuda.synchronize()
                for i in range(n):
                    per_row.append(tuple(t[i].cpu().numpy() for t in (bx, sc, ct, lb, cnt)))
            cands[batch] = per_row
    return dict(plan=plan, cands=cands)


def _oracle_nms(boxes, scores, ctr, labels, ncfg, limit=MAX_PER_IMG):
    """the existing NMS op on one image's candidate list -> (dets [k, 5], labels [k]) on the device; limit: max_per_img
    (0: no limit)"""
    from radet_amd import ops
    b, s, c, lab = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (boxes, scores, ctr, labels))
    if ncfg["type"] == "vote":
        return ops.vote_nms(b, s, lab, {k: v for k, v in ncfg.items() if k != "type"}, score_factor=c, max_num=limit)
    dets, keep = ops.batched_nms(b, s * c, lab, ncfg)
    limit = limit or dets.shape[0]
    return dets[:limit], lab[keep][:limit]


def _ref_args(plan, cands, rows_sel=None):
    sel = range(len(cands)) if rows_sel is None else rows_sel
    m = plan["img_metas"]
    return dict(boxes=[cands[r][0] for r in sel], scores=[cands[r][1] for r in sel], ctr=[cands[r][2] for r in sel],
                labels=[cands[r][3] for r in sel], counts=[int(cands[r][4]) for r in sel],
                img_shapes=[m[r]["img_shape"] for r in sel], scale_factors=[m[r]["scale_factor"] for r in sel],
                offsets=[tuple(plan["rects"][r][:2]) for r in sel], edge_masks=[int(plan["edges"][r]) for r in sel])


@pytest.mark.parametrize("batch", [16, 5])
@pytest.mark.parametrize("nms", sorted(NMS_CFGS))
def test_composition_equals_oracle(det, rows, nms, batch):
    ncfg = NMS_CFGS[nms]
    cfg = dict(det.test_cfg, nms_pre=1000, max_per_img=MAX_PER_IMG, nms=ncfg)      # (the plan's nms_pre = 200 replaces it)
    plan, cands = rows["plan"], rows["cands"][batch]
    assert plan["nms_pre"] == NMS_PRE and plan["row_start"].tolist() == [0, 10, 12]
    counts = [int(c[4]) for c in cands]
    assert all(n > 0 for n in counts), counts                      # every row contributes candidates
    merged = R.merge(**_ref_args(plan, cands), rows_per_image=[10, 2])
    # the 75 x 100 frame: the edge rule drops candidates, and every tile keeps some
    per_tile = [R.merge(**_ref_args(plan, cands, [r]), rows_per_image=[1])[0] for r in range(12)]
    print(f"{nms} batch {batch}: counts {counts}, kept {[len(t[0]) for t in per_tile]}, dropped {[t[4] for t in per_tile]}")
    assert merged[0][4] >= 1 and all(len(per_tile[r][0]) >= 1 for r in range(1, 10))
    assert per_tile[0][4] == 0 and merged[1][4] == 0               # full-frame rows and the single-tile frame drop nothing
    rt = det.runtime()
    got = rt.detect_tiles(plan["img"], dict(plan, batch=batch), cfg)
    torch.cuda.synchronize()
    assert len(got) == 2
    for b in range(2):
        want_d, want_l = _oracle_nms(*merged[b][:4], ncfg)
        assert want_d.shape[0] > 0
        assert got[b][0].shape == want_d.shape and torch.equal(got[b][0], want_d) and torch.equal(got[b][1], want_l)
    # NMS suppresses across rows: without a limit per image the union keeps fewer than the rows' own lists one by one
    union = _oracle_nms(*merged[0][:4], ncfg, limit=0)[0].shape[0]
    one_by_one = sum(_oracle_nms(*per_tile[r][:4], ncfg, limit=0)[0].shape[0] for r in range(10))
    print(f"   kept without a limit: {union} of the union, {one_by_one} of the rows one by one")
    assert 0 < union < one_by_one, (union, one_by_one)


# ------------------------------------------------------------------------------------------- 5. the public interface
API_TILING = dict(TILING, nms_pre=NMS_PRE, batch=5)


def _want(det, group):
    from radet_amd.core.bbox import bbox2result
    plan = _pipeline().run_tile_rows(group, API_TILING)
    dets = det.runtime().detect_tiles(plan["img"], plan, det.test_cfg)
    return dets, [bbox2result(b, l, det.bbox_head.num_classes) for b, l in dets]


def test_public_interface_with_tiling(det, frames):
    from radet_amd import _lib
    from radet_amd.apis import detect_frames, inference_detector

    def logged(fn):
        seen, call = [], _lib.call
        _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
        try:
            return fn(), seen
        finally:
            _lib.call = call
    inference_detector(det, frames)                                # (first use: geometries are tuned once, outside the logs)
    single, before = logged(lambda: inference_detector(det, frames))
    assert sum(len(c) for r in single for c in r) > 0 and "radet_merge_tiles" not in before
    with _tiling(det, API_TILING):
        raw2, want2 = _want(det, frames)
        want1 = [_want(det, [f]) for f in frames]
        res, during = logged(lambda: inference_detector(det, frames))
        _same_results(res, want2)
        assert during.count("radet_merge_tiles") == 1 and during.count("radet_preprocess_frames") == 1
        assert during.count("radet_decode_candidates") == 3       # 12 rows as 5 + 5 + 2
        assert any(not np.array_equal(x, y) for ra, rb in zip(res, single) for x, y in zip(ra, rb))   # (tiles change the result)
        _same_results([inference_detector(det, frames[0])], want1[0][1])
        _same_results(list(detect_frames(det, iter(frames), batch_size=2)), want2)
        _same_results(list(detect_frames(det, iter(frames), batch_size=1)), [w[1][0] for w in want1])
        for bs, want in ((2, raw2), (1, [w[0][0] for w in want1])):
            on_dev = list(detect_frames(det, frames, batch_size=bs, on_device=True))
            assert len(on_dev) == 2
            for (b0, l0), (b1, l1) in zip(on_dev, want):
                assert b0.is_cuda and torch.equal(b0, b1) and torch.equal(l0, l1)
        assert inference_detector(det, []) == []
    after, log_after = logged(lambda: inference_detector(det, frames))
    _same_results(after, single)                                   # cleared: the untouched single-view results, bit for bit
    assert log_after == before                                     # ... through the same calls


def test_crops_with_tiling(det, frames):
    from radet_amd import ops
    from radet_amd.apis import detect_frames, inference_detector
    req = dict(size=(16, 12), scale=1.3, fill=(5, 6, 7))
    with _tiling(det, API_TILING):
        raw = list(detect_frames(det, frames, batch_size=2, on_device=True))
        assert sum(int(b.shape[0]) for b, _ in raw) > 0
        want = ops.crop_detections(frames, raw, (16, 12), scale=1.3, fill=(5, 6, 7), normalize=NORM)
        res, crops = inference_detector(det, frames, crops=req)
        _same_results(res, inference_detector(det, frames))
        assert crops.n_total == want.n_total and crops.images.shape[0] > 0
        assert torch.equal(crops.windows, want.windows) and torch.equal(crops.index, want.index)
        assert torch.equal(crops.images, want.images)
        both = list(detect_frames(det, frames, batch_size=2, on_device=True, crops=req))
        dev_frames = [torch.from_numpy(f).cuda() for f in frames]
        res_dev, crops_dev = inference_detector(det, dev_frames, crops=req)
        _same_results(res_dev, res)
        assert torch.equal(crops_dev.images, want.images)
    for k, ((b0, l0), ((b1, l1), c)) in enumerate(zip(raw, both)):
        assert torch.equal(b0, b1) and torch.equal(l0, l1)
        one = ops.crop_detections([frames[k]], [(b1, l1)], (16, 12), scale=1.3, fill=(5, 6, 7), normalize=NORM)
        assert torch.equal(c.images, one.images) and torch.equal(c.windows, one.windows)


# ------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(det, frames):
    from radet_amd import _lib
    from radet_amd.apis import inference_detector, set_tta
    plan = _pipeline().run_tile_rows(frames, TILING)
    torch.cuda.synchronize()
    rt = det.runtime()
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        with pytest.raises(NotImplementedError, match="nms_pre"):      # 10 rows x 5 levels x 1400 > 65536
            rt.detect_tiles(plan["img"], dict(plan, nms_pre=1400), det.test_cfg)
        with pytest.raises(NotImplementedError, match="nms_pre"):      # test_cfg's own nms_pre, when the plan has none
            rt.detect_tiles(plan["img"], plan, dict(det.test_cfg, nms_pre=1400))
        with pytest.raises(NotImplementedError, match="detect_tiles"):
            rt.detect_graph(plan["img"], plan, det.test_cfg)
        with pytest.raises(ValueError):                                # a row tensor that is not the plan's
            rt.detect_tiles(plan["img"][:5], plan, det.test_cfg)
        with _tiling(det, TILING):
            set_tta(det, dict(img_scale=[SCALE], flip=True, flip_direction="horizontal"))
            try:
                with pytest.raises(NotImplementedError, match="set_tta"):
                    inference_detector(det, frames)
            finally:
                set_tta(det, None)
    finally:
        _lib.call = call
    assert seen == []                                                  # refused before any launch
