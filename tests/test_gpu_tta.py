"""Test-time augmentation on the device: the flip flags of radet_preprocess_frames, radet_merge_views against the NumPy
restatement, the single-view identity, the composition of views against an oracle built from existing pieces, detect_frames
and crops with a test-time-augmentation override set on the model (set_tta), and the refusals."""
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

import _tta_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])


def _pipe(loader, **msfa):
    msfa.setdefault("flip", False)
    return [dict(type=loader),
            dict(type="MultiScaleFlipAug", transforms=[
                dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", **NORM),
                dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])],
                **msfa)]


def _norm_consts():
    mean = np.array(NORM["mean"], np.float32)
    stdinv = (1.0 / np.array(NORM["std"], np.float32).astype(np.float64)).astype(np.float32)
    return mean, stdinv


def _batch(cfg, imgs):
    from radet_amd.datasets.loading import ImagePipeline
    p = ImagePipeline(cfg)
    planned = [p.plan(dict(img=f, bbox_fields=[], mask_fields=[], seg_fields=[]), random, np.random) for f in imgs]
    return p.run(planned, collate=True)


# ------------------------------------------------------------------------------------------- 1. the flip flags
def test_preprocess_frames_flips():
    from radet_amd import kernels as K
    from radet_amd.datasets.loading import frame_desc_rows
    dev = torch.device("cuda")
    rng = np.random.RandomState(5)
    src = [(5, 7), (1, 3), (37, 53)]
    dst = [(11, 13), (4, 1), (45, 64)]                           # an upscale, a destination with w == 1, a resize by 1.2
    Hp = Wp = 64                                                 # padded to a multiple of 32
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in src]
    B, V = len(imgs), 4
    flags = [0, K.PREP_FLIP_H, K.PREP_FLIP_V, K.PREP_FLIP_H | K.PREP_FLIP_V]
    buf = torch.from_numpy(np.concatenate([f.reshape(-1) for f in imgs])).to(dev)
    rows, _, nbytes = frame_desc_rows(imgs, dst * V, True, buf.data_ptr(), views=V, flips=np.repeat(flags, B).tolist())
    assert nbytes == buf.numel() and rows.shape[0] == V * B
    out = torch.full((V * B, 3, Hp, Wp), float("nan"), device=dev)
    K.preprocess_frames(torch.from_numpy(rows).to(dev), V * B, Hp, Wp, *_norm_consts(), out)
    plain = torch.full((B, 3, Hp, Wp), float("nan"), device=dev)
    K.preprocess_frames(torch.from_numpy(rows[:B].copy()).to(dev), B, Hp, Wp, *_norm_consts(), plain)
    torch.cuda.synchronize()
    out = out.view(V, B, 3, Hp, Wp)
    assert not torch.isnan(out).any()
    assert torch.equal(out[0], plain)                            # the unflipped rows write what a launch without flips writes
    dims = {1: (2,), 2: (1,), 3: (1, 2)}
    for v in (1, 2, 3):
        for b, (h, w) in enumerate(dst):
            want = torch.flip(out[0, b, :, :h, :w], dims[v])
            assert torch.equal(out[v, b, :, :h, :w], want), (v, b)
            assert (out[v, b, :, h:, :] == 0).all() and (out[v, b, :, :, w:] == 0).all()      # the padding stays zero
    assert not torch.equal(out[1, 2], out[0, 2])                 # (a flip of random pixels is not the identity)


# ------------------------------------------------------------------------------------------- 2. the merge kernel
def _merge_case():
    rng = np.random.RandomState(8)
    V, B = 4, 3
    caps = [8, 12, 8, 12]
    flips = [None, "horizontal", "vertical", "diagonal"]
    shapes = [[(45, 64, 3), (48, 64, 3), (37, 53, 3)]] * 2 + [[(67, 96, 3), (72, 96, 3), (55, 80, 3)]] * 2
    sfs = [[np.array([64 / 53, 45 / 37, 64 / 53, 45 / 37], np.float32), np.ones(4, np.float32),
            np.array([0.7, 0.71, 0.7, 0.71], np.float32)]] * 2
    sfs += [[np.array([96 / 53, 67 / 37, 96 / 53, 67 / 37], np.float32), np.full(4, 1.5, np.float32),
             np.array([1.06, 1.0576923, 1.06, 1.0576923], np.float32)]] * 2
    counts = [np.array([0, 8, 0], np.int32), np.array([12, 5, 0], np.int32), np.array([3, 0, 0], np.int32),
              np.array([7, 12, 0], np.int32)]                   # 0, full rows, partial rows; image 2 has no candidate at all
    boxes, scores, ctr, labels = [], [], [], []
    for v in range(V):
        h, w = shapes[v][0][:2]
        p = rng.random_sample((B, caps[v], 4)).astype(np.float32) * np.array([w, h, w, h], np.float32)
        boxes.append(np.concatenate([np.minimum(p[..., :2], p[..., 2:]), np.maximum(p[..., :2], p[..., 2:])], -1))
        scores.append(rng.random_sample((B, caps[v])).astype(np.float32))
        ctr.append(rng.random_sample((B, caps[v])).astype(np.float32))
        labels.append(rng.randint(0, 21, (B, caps[v])).astype(np.int64))
    return dict(boxes=boxes, scores=scores, ctr=ctr, labels=labels, counts=counts, img_shapes=shapes, scale_factors=sfs, flips=flips)


def test_merge_view_candidates_equals_restatement():
    from radet_amd import ops
    c = _merge_case()
    ob, osc, oct_, ol, oc = ops.merge_view_candidates(**c)
    torch.cuda.synchronize()
    want = R.merge(**c)
    assert ob.shape == (3, 40, 4) and ol.dtype == torch.int64
    assert oc.cpu().tolist() == [len(w[0]) for w in want] == [22, 25, 0]
    for b, (wb, ws, wc, wl) in enumerate(want):
        n = len(wb)
        assert np.array_equal(ob[b, :n].cpu().numpy().view(np.uint32), wb.view(np.uint32)), b
        assert np.array_equal(osc[b, :n].cpu().numpy(), ws) and np.array_equal(oct_[b, :n].cpu().numpy(), wc)
        assert np.array_equal(ol[b, :n].cpu().numpy(), wl)


def test_merge_views_argument_errors():
    from radet_amd import _lib, kernels as K
    lib = _lib.load()
    dev = torch.device("cuda")
    V, B, cap = 2, 2, 4
    pool = V * B * cap
    desc = K.merge_desc_rows(np.full((V * B, 2), 32.0), np.ones((V * B, 4)), [0, 0, 0, 0], np.arange(V * B) * cap, [cap] * (V * B))
    ddev = torch.from_numpy(desc).to(dev)
    pb, ps, pc = torch.zeros(pool, 4, device=dev), torch.zeros(pool, device=dev), torch.zeros(pool, device=dev)
    pl, cnt = torch.zeros(pool, dtype=torch.long, device=dev), torch.full((V * B,), cap, dtype=torch.int32, device=dev)
    cap_out = V * cap
    ob = torch.full((B, cap_out, 4), 7.0, device=dev)
    osc, oct_ = torch.full((B, cap_out), 7.0, device=dev), torch.full((B, cap_out), 7.0, device=dev)
    ol, oc = torch.full((B, cap_out), 7, dtype=torch.long, device=dev), torch.full((B,), 7, dtype=torch.int32, device=dev)

    def call(desc_host=desc, V=V, B=B, pool=pool, cap_out=cap_out, boxes=pb):
        return lib.radet_merge_views(desc_host.ctypes.data, ddev.data_ptr(), V, B, pool, None if boxes is None else boxes.data_ptr(),
                                     ps.data_ptr(), pc.data_ptr(), pl.data_ptr(), cnt.data_ptr(), cap_out, ob.data_ptr(),
                                     osc.data_ptr(), oct_.data_ptr(), ol.data_ptr(), oc.data_ptr(), None)
    bad_flip = desc.copy()
    bad_flip[3, 6] = 4
    neg_flip = desc.copy()
    neg_flip[0, 6] = -1
    outside = desc.copy()
    outside[3, 7] = pool - cap + 1
    for kw in (dict(V=0), dict(V=K.TTA_MAX_VIEWS + 1), dict(cap_out=0), dict(cap_out=65537), dict(desc_host=bad_flip),
               dict(desc_host=neg_flip), dict(desc_host=outside), dict(boxes=None), dict(cap_out=cap_out - 1)):
        assert call(**kw) == -1, kw
    assert call(B=0) == 0                                        # no images: OK, no launch
    torch.cuda.synchronize()
    assert (ob == 7).all() and (osc == 7).all() and (ol == 7).all() and (oc == 7).all()       # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert oc.cpu().tolist() == [cap_out, cap_out] and (ob == 0).all()


# ------------------------------------------------------------------------------------------- the tiny detector
# The detector of tests/test_gpu_frames.py: img_scale (640, 480) on small landscape frames; batches of 1, 2 and 4 images
# padded to 480 x 640 are geometries whose conv tile picks are pinned.  Two frames with an unflipped and a flipped view run
# as one forward batch of 4.  The second scale's geometry (240 x 320) is tuned once when it first runs; every comparison
# below runs both of its sides in this process, on the same picks.
SCALE_A, SCALE_B = (640, 480), (320, 240)


@pytest.fixture(scope="module")
def det():
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
    d.cfg = Config(dict(data=dict(test=dict(pipeline=_pipe("LoadImageFromFile", img_scale=SCALE_A)))))
    return d


@pytest.fixture(scope="module")
def frames():
    rng = np.random.RandomState(11)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (48, 64), (60, 80), (30, 40), (75, 100))]


@contextlib.contextmanager
def _tta(det, tta):
    """the override on the (module-wide) detector for the length of a block"""
    from radet_amd.apis import set_tta
    set_tta(det, tta)
    try:
        yield det
    finally:
        set_tta(det, None)


def _same_results(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert len(ra) == len(rb)
        for ca, cb in zip(ra, rb):
            assert ca.dtype == cb.dtype and np.array_equal(ca, cb)


# ------------------------------------------------------------------------------------------- 3. one view is today's path
def test_single_view_identity(det, frames):
    from radet_amd.apis import inference_detector
    want = inference_detector(det, frames[:2])
    assert sum(len(c) for r in want for c in r) > 0
    with _tta(det, dict(img_scale=[SCALE_A], flip=False)):
        _same_results(inference_detector(det, frames[:2]), want)
    data = _batch(_pipe("LoadImageFromWebcam", img_scale=SCALE_A), frames[:2])
    x, m = data["img"][0], data["img_metas"][0]
    with torch.no_grad():
        simple = det.simple_test(x, [dict(k) for k in m], rescale=True)
        listed = det(img=[x], img_metas=[[dict(k) for k in m]], return_loss=False, rescale=True)
    _same_results(listed, simple)
    _same_results(listed, want)
    dets = det.runtime().detect_aug([x], [m], det.test_cfg, True)
    from radet_amd.core.bbox import bbox2result
    _same_results([bbox2result(b, l, det.bbox_head.num_classes) for b, l in dets], want)


# ------------------------------------------------------------------------------------------- 4. the composition of views
NMS_CFGS = dict(
    vote=dict(type="vote", iou_threshold=0.65, cluster_score=["cls", "iou"], vote_score=["iou", "cls"], iou_enable=False),
    nms=dict(type="nms", iou_threshold=0.5),
    soft_nms=dict(type="soft_nms", iou_threshold=0.3, method="linear", min_score=0.05, split_thr=-1),
)
NMS_PRE, MAX_PER_IMG = 200, 100


@pytest.fixture(scope="module")
def views(det, frames):
    """views {scale A, scale A + horizontal flip, scale B} of two frames, and per view the candidates an existing forward
    pass + radet_decode_candidates call give (view coordinates), computed once for the three NMS types"""
    from radet_amd import kernels as K
    a = _batch(_pipe("LoadImageFromWebcam", img_scale=SCALE_A, flip=True, flip_direction="horizontal"), frames[:2])
    b = _batch(_pipe("LoadImageFromWebcam", img_scale=SCALE_B), frames[:2])
    imgs = [a["img"][0], a["img"][1], b["img"][0]]
    metas = [a["img_metas"][0], a["img_metas"][1], b["img_metas"][0]]
    assert [m[0]["flip"] for m in metas] == [False, True, False] and metas[1][0]["flip_direction"] == "horizontal"
    assert imgs[0].shape == imgs[1].shape == (2, 3, 480, 640) and imgs[2].shape == (2, 3, 256, 320)
    rt = det.runtime()
    e = rt.engine
    B, cands = 2, []
    with torch.no_grad():
        # the flipped view next to the unflipped one, as one batch of 4: the geometry detect_aug runs them at
        for group in ([0, 1], [2]):
            rt.forward(torch.cat([imgs[v] for v in group]).cuda())
            n, nlvl = len(group) * B, e.nlvl
            cap = nlvl * NMS_PRE
            hw = torch.tensor([[float(m["img_shape"][0]), float(m["img_shape"][1])] for v in group for m in metas[v]], device="cuda")
            bx, sc = torch.zeros(n, cap, 4, device="cuda"), torch.zeros(n, cap, device="cuda")
            ct, lb = torch.zeros(n, cap, device="cuda"), torch.zeros(n, cap, dtype=torch.long, device="cuda")
            cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
            ws = torch.empty(K.decode_ws_bytes(n, nlvl, NMS_PRE), dtype=torch.uint8, device="cuda")
            K.decode_candidates(e.buf["cls"], e.buf["reg_u"], e.buf["iou"], e.scales_tensor(), e.ldesc, nlvl, n, rt.num_classes,
                                float(det.test_cfg["score_thr"]), NMS_PRE, hw, None, bx, sc, ct, lb, cnt, ws)
            torch.cuda.synchronize()
            for i in range(len(group)):
                sl = slice(i * B, (i + 1) * B)
                cands.append(tuple(t[sl].cpu().numpy() for t in (bx, sc, ct, lb, cnt)))
    return dict(imgs=imgs, metas=metas, cands=cands)


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


@pytest.mark.parametrize("nms", sorted(NMS_CFGS))
def test_composition_equals_oracle(det, views, nms):
    ncfg = NMS_CFGS[nms]
    cfg = dict(det.test_cfg, nms_pre=NMS_PRE, max_per_img=MAX_PER_IMG, nms=ncfg)
    imgs, metas, cands = views["imgs"], views["metas"], views["cands"]
    V, B = 3, 2
    assert all((c[4] > 0).all() for c in cands)                   # every view contributes candidates, for every image
    merged = R.merge([c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], [c[3] for c in cands],
                     [c[4] for c in cands], [[m["img_shape"] for m in metas[v]] for v in range(V)],
                     [[m["scale_factor"] for m in metas[v]] for v in range(V)],
                     [m[0]["flip_direction"] if m[0]["flip"] else None for m in metas])
    rt = det.runtime()
    got = rt.detect_aug(imgs, metas, cfg, True)
    plain = rt.detect_aug(imgs, metas, cfg, False)
    torch.cuda.synchronize()
    assert len(got) == B
    for b in range(B):
        want_d, want_l = _oracle_nms(*merged[b], ncfg)
        print(f"{nms} image {b}: {[int(c[4][b]) for c in cands]} candidates per view, {want_d.shape[0]} detections")
        assert want_d.shape[0] > 0
        assert got[b][0].shape == want_d.shape and torch.equal(got[b][0], want_d) and torch.equal(got[b][1], want_l)
        # NMS suppresses across views: without a limit per image the union keeps fewer than the views' own lists together
        per_view = sum(_oracle_nms(*R.merge(*[[c[k]] for k in range(5)], [[metas[v][i]["img_shape"] for i in range(B)]],
                                            [[metas[v][i]["scale_factor"] for i in range(B)]],
                                            [metas[v][0]["flip_direction"] if metas[v][0]["flip"] else None])[b],
                                   ncfg, limit=0)[0].shape[0]
                       for v, c in enumerate(cands))
        union = _oracle_nms(*merged[b], ncfg, limit=0)[0].shape[0]
        print(f"   kept without a limit: {union} of the union, {per_view} of the views one by one")
        assert 0 < union < per_view, (union, per_view)
        # rescale=False: the kept boxes times view 0's scale factor
        sf0 = torch.from_numpy(np.asarray(metas[0][b]["scale_factor"], np.float32)).cuda()
        assert torch.equal(plain[b][0][:, :4], got[b][0][:, :4] * sf0) and torch.equal(plain[b][0][:, 4], got[b][0][:, 4])
        assert torch.equal(plain[b][1], got[b][1])
    # the model entry point takes the same road
    from radet_amd.core.bbox import bbox2result
    if nms == "vote":
        old = det.test_cfg
        det.test_cfg = cfg
        try:
            with torch.no_grad():
                res = det(img=imgs, img_metas=[[dict(m) for m in view] for view in metas], return_loss=False, rescale=True)
        finally:
            det.test_cfg = old
        _same_results(res, [bbox2result(d, l, det.bbox_head.num_classes) for d, l in got])


# ------------------------------------------------------------------------------------------- 5. / 6. the public interface
TTA = dict(img_scale=[SCALE_A], flip=True, flip_direction="horizontal")


def test_detect_frames_with_tta(det, frames):
    from radet_amd.apis import detect_frames, inference_detector
    single = inference_detector(det, frames[:2])
    with _tta(det, TTA):
        want = [r for lo in (0, 2, 4) for r in inference_detector(det, frames[lo:lo + 2])]
        assert len(want) == 5 and sum(len(c) for r in want for c in r) > 0
        assert any(not np.array_equal(x, y) for ra, rb in zip(want[:2], single) for x, y in zip(ra, rb))   # (the views change the result)
        got = list(detect_frames(det, iter(frames), batch_size=2))
        _same_results(got, want)
        # a generator dropped after its first result: the second batch is in flight; the runtime stays usable
        it = detect_frames(det, frames, batch_size=2)
        _same_results([next(it)], want[:1])
        it.close()
    _same_results(inference_detector(det, frames[:2]), single)         # (the override is cleared: a single-view call again)
    # a config whose MultiScaleFlipAug makes the views is honoured without an override
    from radet_amd.utils import Config
    old = det.cfg
    det.cfg = Config(dict(data=dict(test=dict(pipeline=_pipe("LoadImageFromFile", **TTA)))))
    try:
        _same_results(inference_detector(det, frames[:2]), want[:2])
    finally:
        det.cfg = old


def test_crops_with_tta(det, frames):
    from radet_amd import ops
    from radet_amd.apis import detect_frames, inference_detector
    req = dict(size=(16, 12), scale=1.3, fill=(5, 6, 7))
    with _tta(det, TTA):
        raw = list(detect_frames(det, frames[:2], batch_size=2, on_device=True))
        assert sum(int(b.shape[0]) for b, _ in raw) > 0
        want = ops.crop_detections(frames[:2], raw, (16, 12), scale=1.3, fill=(5, 6, 7), normalize=NORM)
        res, crops = inference_detector(det, frames[:2], crops=req)
        _same_results(res, inference_detector(det, frames[:2]))
        assert crops.n_total == want.n_total and crops.images.shape[0] > 0
        assert torch.equal(crops.windows, want.windows) and torch.equal(crops.index, want.index)
        assert torch.equal(crops.images, want.images)
        both = list(detect_frames(det, frames[:2], batch_size=2, on_device=True, crops=req))
    for k, ((b0, l0), ((b1, l1), c)) in enumerate(zip(raw, both)):
        assert torch.equal(b0, b1) and torch.equal(l0, l1)
        one = ops.crop_detections([frames[k]], [(b1, l1)], (16, 12), scale=1.3, fill=(5, 6, 7), normalize=NORM)
        assert torch.equal(c.images, one.images) and torch.equal(c.windows, one.windows)


# ------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(det, frames):
    from radet_amd import _lib
    data = _batch(_pipe("LoadImageFromWebcam", **TTA), frames[:2])
    imgs, metas = data["img"], data["img_metas"]
    rt = det.runtime()
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        with pytest.raises(NotImplementedError, match="nms_pre"):      # 2 views x 5 levels x 7000 > 65536
            rt.detect_aug(imgs, metas, dict(det.test_cfg, nms_pre=7000), True)
        with pytest.raises(ValueError):                                # views that disagree in B
            rt.detect_aug([imgs[0], imgs[1][:1]], [metas[0], metas[1][:1]], det.test_cfg, True)
        other = [dict(m) for m in metas[1]]
        other[0]["ori_shape"] = (11, 12, 3)
        with pytest.raises(ValueError, match="ori_shape"):
            rt.detect_aug(imgs, [metas[0], other], det.test_cfg, True)
    finally:
        _lib.call = call
    assert seen == []                                                  # refused before any launch
    with pytest.raises(NotImplementedError):
        rt.detect_graph(imgs, metas, det.test_cfg, True)
