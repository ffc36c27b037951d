"""radet_soft_nms on the GPU against the NumPy restatement (tests/_softnms_ref.py): keep, order and score BITS are equal
for the naive, linear and gaussian methods -- the gaussian weight is exp in double of the fp32 argument, rounded once, on
both sides.  Sizes straddle the kernel's thresholds (64-lane waves, 1024 lanes per workgroup, 8192 register-resident
candidates).  Then the Python layers (ops.soft_nms, ops.batched_nms, core.multiclass_nms) and the detector path
(get_bboxes, detect, detect_graph)."""
import os

import numpy as np
import pytest
import torch

from _softnms_ref import METHODS, batched_soft_nms, soft_nms_fast

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(METHODS)
REG_CAP = 8192          # SOFT_NMS_REG_CAP of radet_amd/csrc/soft_nms.hip


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_dev(boxes, scores, labels, counts, method, thr=0.3, sigma=0.5, min_score=1e-3, class_agnostic=False, max_out=None):
    """boxes [B, cap, 4], scores [B, cap], labels [B, cap], counts [B] -> per image (keep, scores, boxes, labels)"""
    from radet_amd import kernels as K
    boxes = np.asarray(boxes, np.float32)
    B, cap = boxes.shape[:2]
    k = cap if max_out is None else max_out
    dev = torch.device("cuda")
    ob = torch.full((B, k, 4), -1.0, device=dev)
    osc = torch.full((B, k), -1.0, device=dev)
    ol = torch.full((B, k), -1, dtype=torch.long, device=dev)
    okp = torch.full((B, k), -1, dtype=torch.long, device=dev)
    oc = torch.full((B,), -1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(K.soft_nms_ws_bytes(B, cap), 1), dtype=torch.uint8, device=dev)
    K.soft_nms(torch.from_numpy(boxes).to(dev), torch.from_numpy(np.asarray(scores, np.float32)).to(dev),
               torch.from_numpy(np.asarray(labels, np.int64)).to(dev), torch.from_numpy(np.asarray(counts, np.int32)).to(dev),
               B, cap, METHODS[method], thr, sigma, min_score, class_agnostic, k, ob, osc, ol, okp, oc, ws)
    torch.cuda.synchronize()
    out = []
    for b in range(B):
        c = int(oc[b])
        assert 0 <= c <= k
        assert bool((okp[b, c:] == -1).all()) and bool((osc[b, c:] == -1).all())       # nothing written past the count
        out.append((okp[b, :c].cpu().numpy(), osc[b, :c].cpu().numpy(), ob[b, :c].cpu().numpy(), ol[b, :c].cpu().numpy()))
    return out


def check(boxes, scores, labels, method, thr=0.3, sigma=0.5, min_score=1e-3, class_agnostic=False, max_out=None):
    """one image, cap = n: device == reference; returns the reference's (keep, scores)"""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    scores = np.asarray(scores, np.float32).reshape(-1)
    labels = np.asarray(labels, np.int64).reshape(-1)
    n = len(scores)
    rk, rs = batched_soft_nms(boxes, scores, labels, METHODS[method], thr, sigma, min_score, class_agnostic, max_out)
    pad = max(n, 1) - n
    (k, s, b, l), = run_dev(np.pad(boxes, ((0, pad), (0, 0)))[None], np.pad(scores, (0, pad))[None],
                            np.pad(labels, (0, pad))[None], [n], method, thr, sigma, min_score, class_agnostic, max_out)
    assert np.array_equal(k, rk), (k[:10], rk[:10])
    assert np.array_equal(bits(s), bits(rs))
    assert np.array_equal(bits(b), bits(boxes[rk])) and np.array_equal(l, labels[rk])
    assert np.all(np.diff(rs) <= 0)
    return rk, rs


def crowd(rng, n, classes=1, span=100.0):
    """n heavily overlapping boxes with distinct scores"""
    c = rng.uniform(0.1 * span, 0.9 * span, (n, 2))
    wh = rng.uniform(0.04 * span, 0.4 * span, (n, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    scores = rng.permutation(np.linspace(0.02, 0.99, n)).astype(np.float32)
    return boxes, scores, rng.integers(0, classes, n)


# ---------------------------------------------------------------------------------------------- must fail without the feature
def test_batched_nms_soft_linear_keeps_and_decays_the_overlapping_box():
    """two boxes of one class with IoU 0.6, scores 0.9 / 0.8, linear, thr 0.3: hard NMS returns one box, Soft-NMS both, the
    second with 0.8f * (1 - ovr)"""
    from radet_amd import ops
    boxes = torch.tensor([[0.0, 0, 10, 10], [0, 0, 10, 6]])
    dets, keep = ops.batched_nms(boxes, torch.tensor([0.9, 0.8]), torch.tensor([3, 3]),
                                 dict(type="soft_nms", iou_threshold=0.3, method="linear"))
    ovr = np.float32(60) / (np.float32(100) + np.float32(60) - np.float32(60))
    assert keep.tolist() == [0, 1] and tuple(dets.shape) == (2, 5)
    assert torch.equal(dets[:, :4], boxes)
    assert np.array_equal(bits(dets[:, 4].numpy()), bits([np.float32(0.9), np.float32(0.8) * (np.float32(1) - ovr)]))


# ---------------------------------------------------------------------------------------------- smallest cases
@pytest.mark.parametrize("method", ALL)
def test_smallest_cases(method):
    B1, B2, FAR = [0, 0, 2, 2], [0, 0, 2, 1], [50, 50, 60, 60]
    k, _ = check(np.zeros((0, 4)), [], [], method)                                        # n = 0
    assert len(k) == 0
    check([B1], [0.5], [0], method)                                                       # n = 1
    check([B1, FAR], [0.5, 0.6], [0, 0], method)                                          # n = 2
    k, s = check([B1, B1], [0.9, 0.8], [1, 1], method)                                    # identical boxes: ovr = 1
    assert (len(k) == 2) == (method == "gaussian")
    k, s = check([B1, B2], [0.9, 0.8], [0, 0], method, thr=0.5)                           # IoU exactly at thr: >= decays
    if method == "linear":
        assert s[1] == np.float32(0.8) * np.float32(0.5)
    if method == "naive":
        assert k.tolist() == [0]
    k, _ = check([B1, FAR, [80, 80, 90, 90]], [0.5, 0.7, 0.7], [0, 0, 0], method)         # equal scores: lower index first
    assert k.tolist() == [1, 2, 0]
    k, _ = check([FAR, B1, B1], [0.3, 0.6, 0.6], [0, 2, 1], method)                       # ... across classes too
    assert k.tolist() == [1, 2, 0]
    k, _ = check([B1, FAR], [5e-4, 4e-4], [0, 0], method)                                 # first pick below min_score
    assert k.tolist() == [0]
    k, _ = check([B1, FAR, B2, FAR], [2e-4, 5e-4, 1e-4, 3e-4], [0, 1, 2, 1], method)      # all below min_score
    assert k.tolist() == [1]
    k, _ = check([B1, B2, FAR], [0.9, 0.8, 5e-4], [0, 0, 4], method)                      # low box of another class vanishes
    assert 2 not in k.tolist()
    check([B1, FAR], [0.9, 0.8], [0, 0], method, min_score=0.85)                          # a multiply by exactly 1 prunes
    for thr in (0.0, -1.0):                                                               # 0 >= thr holds without any overlap
        k, _ = check([B1, FAR, B2], [0.9, 0.8, 0.7], [0, 0, 1], method, thr=thr)
        assert (k.tolist() == [0]) == (method == "naive")


def test_zero_area_boxes_under_gaussian():
    Z = [3, 3, 3, 3]
    k, s = check([Z, Z], [0.9, 0.8], [0, 0], "gaussian")                                  # NaN IoU, same class: weight 1
    assert k.tolist() == [0, 1] and s[1] == np.float32(0.8)
    k, s = check([Z, Z, [0, 0, 6, 6]], [0.9, 0.8, 0.7], [0, 1, 0], "gaussian")            # cross class: offset boxes, still NaN
    assert k.tolist() == [0, 1, 2] and s[1] == np.float32(0.8)
    k, _ = check([[0, 0, 0, 0], [0, 0, 0, 0]], [0.9, 0.8], [0, 5], "gaussian")            # the largest coordinate is 0: unit 1
    assert k.tolist() == [0, 1]
    for method in ("naive", "linear"):
        check([Z, Z, [3, 3, 3, 9]], [0.9, 0.8, 0.7], [0, 0, 0], method)


@pytest.mark.parametrize("method", ALL)
def test_large_coordinates_with_30_labels(method):
    """coordinates near 1e4 and 30 labels: the fp32 class offset (up to 3e5) loses low bits of the coordinates, on both sides
    alike"""
    rng = np.random.default_rng(5)
    boxes, scores, _ = crowd(rng, 400, span=60.0)
    boxes = (boxes + np.float32(9900.0) + rng.uniform(0, 1, (400, 1)).astype(np.float32)).astype(np.float32)
    labels = rng.integers(0, 30, 400)
    k, _ = check(boxes, scores, labels, method)
    assert len(k) >= 20


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("method", ALL)
@pytest.mark.parametrize("n", [63, 64, 65, 257, 1023, 1024, 1025])
def test_one_label_sizes(method, n):
    rng = np.random.default_rng(n)
    boxes, scores, labels = crowd(rng, n)
    k, _ = check(boxes, scores, labels + 2, method)
    assert 1 <= len(k) <= n


@pytest.mark.parametrize("method", ALL)
@pytest.mark.parametrize("n", [REG_CAP, REG_CAP + 1, 9000])
def test_one_label_around_register_capacity(method, n):
    """n <= 8192 runs out of registers and LDS, above through the workspace; naive prunes fast, so its full sequence is
    compared, the other methods' first 300 picks (the reference costs one pass over n per pick)"""
    rng = np.random.default_rng(n)
    boxes, scores, labels = crowd(rng, n, span=1000.0)
    k, _ = check(boxes, scores, labels + 1, method, max_out=None if method == "naive" else 300)
    assert len(k) >= 20


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2048, 2049])
def test_disjoint_boxes_all_survive(n):
    """no overlaps: every box is picked, in score order -- pick counts on both sides of the kernel's 1024-pick output stage"""
    rng = np.random.default_rng(n)
    i = np.arange(n)
    xy = np.stack([(i % 64) * 20.0, (i // 64) * 20.0], 1)
    boxes = np.concatenate([xy, xy + 10.0], 1).astype(np.float32)
    scores = rng.permutation(np.linspace(0.02, 0.99, n)).astype(np.float32)
    k, s = check(boxes, scores, rng.integers(0, 3, n), "linear")
    assert len(k) == n and np.array_equal(k, np.argsort(-scores, kind="stable"))
    k, _ = check(boxes, scores, np.zeros(n, np.int64), "gaussian", max_out=1024)
    assert len(k) == min(n, 1024)


def test_general_pass_equals_register_pass():
    """the same 8192 candidates through both passes: cap = n (registers) and, followed by one pruned-at-once candidate of
    another class, n = 8193 (workspace)"""
    rng = np.random.default_rng(77)
    boxes, scores, labels = crowd(rng, REG_CAP, classes=3, span=1000.0)
    a, sa = check(boxes, scores, labels, "gaussian", max_out=200)
    boxes2 = np.concatenate([boxes, [[0, 0, 1, 1]]]).astype(np.float32)
    b, sb = check(boxes2, np.append(scores, np.float32(1e-5)), np.append(labels, 0), "gaussian", max_out=200)
    assert np.array_equal(a, b) and np.array_equal(bits(sa), bits(sb))


@pytest.mark.parametrize("method", ALL)
def test_21_labels_random_lengths(method):
    rng = np.random.default_rng(21)
    lens = rng.integers(1, 160, 21)
    n = int(lens.sum())
    boxes, scores, _ = crowd(rng, n, span=300.0)
    labels = rng.permutation(np.repeat(np.arange(21), lens))
    k, s = check(boxes, scores, labels, method)
    assert len(set(labels[k].tolist())) == 21
    k5, s5 = check(boxes, scores, labels, method, max_out=5)                              # the first 5 rows of the sequence
    assert np.array_equal(k5, k[:5]) and np.array_equal(bits(s5), bits(s[:5]))
    assert np.bincount(labels).max() > 5
    ka, _ = check(boxes, scores, labels, method, class_agnostic=True)
    assert not np.array_equal(ka, k)
    kz, sz = batched_soft_nms(boxes, scores, np.zeros(n, np.int64), METHODS[method], 0.3, 0.5, 1e-3)
    assert np.array_equal(ka, kz)


@pytest.mark.parametrize("counts", [(300, 0, 7), (250, 0, 7)])
def test_batch_of_three_images(counts):
    """B = 3, cap = 300: a full image, an empty one and a short one; the rows past counts[b] hold huge coordinates and scores
    that must not be read (they would move the class offset and win every pick)"""
    rng = np.random.default_rng(3)
    cap = 300
    boxes = np.full((3, cap, 4), 1e6, np.float32)
    scores = np.full((3, cap), 9.0, np.float32)
    labels = np.full((3, cap), 7, np.int64)
    for b, c in enumerate(counts):
        boxes[b, :c], scores[b, :c], labels[b, :c] = crowd(rng, c, classes=4)
    for method in ALL:
        res = run_dev(boxes, scores, labels, counts, method)
        for b, c in enumerate(counts):
            rk, rs = batched_soft_nms(boxes[b, :c], scores[b, :c], labels[b, :c], METHODS[method], 0.3, 0.5, 1e-3)
            k, s, bx, l = res[b]
            assert np.array_equal(k, rk) and np.array_equal(bits(s), bits(rs))
            assert np.array_equal(bits(bx), bits(boxes[b, rk])) and np.array_equal(l, labels[b, rk])


# ---------------------------------------------------------------------------------------------- Python layers
@pytest.mark.parametrize("method", ALL)
def test_ops_layers_agree(method):
    """ops.soft_nms == the single-class loop; ops.batched_nms(type='soft_nms') == ops.soft_nms on the offset boxes;
    core.multiclass_nms inherits it"""
    from _softnms_ref import offset_boxes
    from radet_amd import ops
    from radet_amd.core import multiclass_nms
    rng = np.random.default_rng(8)
    boxes, scores, labels = crowd(rng, 500, classes=6)
    cfg = dict(type="soft_nms", iou_threshold=0.4, sigma=0.7, min_score=2e-3, method=method)
    dets, inds = ops.soft_nms(boxes, torch.from_numpy(scores), 0.4, 0.7, 2e-3, method)
    rk, rs = soft_nms_fast(boxes, scores, METHODS[method], 0.4, 0.7, 2e-3)
    assert not dets.is_cuda and np.array_equal(inds.numpy(), rk) and np.array_equal(bits(dets[:, 4].numpy()), bits(rs))
    assert np.array_equal(bits(dets[:, :4].numpy()), bits(boxes[rk]))

    bd, bk = ops.batched_nms(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda(), cfg)
    od, oi = ops.soft_nms(offset_boxes(boxes, labels), scores, 0.4, 0.7, 2e-3, method)
    assert bd.is_cuda and torch.equal(bk.cpu(), oi) and np.array_equal(bits(bd[:, 4].cpu().numpy()), bits(od[:, 4].numpy()))
    assert np.array_equal(bits(bd[:, :4].cpu().numpy()), bits(boxes[oi.numpy()]))
    ad, ak = ops.batched_nms(boxes, scores, labels, dict(cfg, class_agnostic=True))       # class_agnostic from the config
    ad2, ak2 = ops.batched_nms(boxes, scores, labels, cfg, class_agnostic=True)
    assert torch.equal(ak, inds) and torch.equal(ak2, inds) and torch.equal(ad, dets) and torch.equal(ad2, dets)
    hd, hk = ops.batched_nms(boxes, scores, labels, dict(iou_threshold=0.4))              # no type: hard NMS as before
    hd2, hk2 = ops.batched_nms(boxes, scores, labels, dict(type="nms", iou_threshold=0.4))
    assert torch.equal(hk, hk2) and torch.equal(hd, hd2) and len(hk) <= len(bk)
    assert np.array_equal(bits(hd[:, 4].numpy()), bits(scores[hk.numpy()]))

    C = 6
    multi_scores = np.zeros((500, C + 1), np.float32)
    multi_scores[np.arange(500), labels] = scores
    md, ml, mi = multiclass_nms(torch.from_numpy(boxes), torch.from_numpy(multi_scores), 0.01, cfg, max_num=50, return_inds=True)
    assert np.array_equal(mi.numpy(), bk.cpu().numpy()[:50]) and np.array_equal(ml.numpy(), labels[bk.cpu().numpy()[:50]])
    assert np.array_equal(bits(md.numpy()), bits(bd.cpu().numpy()[:50]))


def test_bad_arguments_launch_nothing():
    from radet_amd import kernels as K
    from radet_amd import ops
    from radet_amd._lib import RadetHipError
    dev = torch.device("cuda")
    n = 4
    boxes = torch.tensor([[0.0, 0, 4, 4]] * n, device=dev)
    scores, labels = torch.rand(n, device=dev), torch.zeros(n, dtype=torch.long, device=dev)
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    ob, osc = torch.full((1, n, 4), -1.0, device=dev), torch.full((1, n), -1.0, device=dev)
    ol, okp = torch.full((1, n), -1, dtype=torch.long, device=dev), torch.full((1, n), -1, dtype=torch.long, device=dev)
    oc = torch.full((1,), -1, dtype=torch.int32, device=dev)
    ws = torch.empty(K.soft_nms_ws_bytes(1, n), dtype=torch.uint8, device=dev)

    def call(cap=n, method=1, sigma=0.5, max_out=n):
        K.soft_nms(boxes, scores, labels, cnt, 1, cap, method, 0.3, sigma, 1e-3, False, max_out, ob, osc, ol, okp, oc, ws)

    for kw in (dict(method=3), dict(method=-1), dict(method=2, sigma=0.0), dict(method=2, sigma=-1.0), dict(max_out=0),
               dict(max_out=-5), dict(cap=0), dict(cap=65537)):
        with pytest.raises(RadetHipError):
            call(**kw)
    torch.cuda.synchronize()
    assert int(oc[0]) == -1 and bool((okp == -1).all()) and bool((osc == -1).all())
    call(method=1, sigma=0.0)                                                             # sigma only matters to gaussian
    torch.cuda.synchronize()
    assert int(oc[0]) >= 1
    with pytest.raises(ValueError):
        ops.soft_nms(boxes, scores, method="gaussian", sigma=0.0)
    with pytest.raises(NotImplementedError):
        ops.soft_nms(boxes, scores, offset=1)
    big = torch.zeros(10000, 4, device=dev)
    with pytest.raises(NotImplementedError):
        ops.batched_nms(big, torch.ones(10000, device=dev), torch.zeros(10000, dtype=torch.long, device=dev), dict(type="soft_nms"))
    d, k = ops.batched_nms(big, torch.ones(10000, device=dev), torch.zeros(10000, dtype=torch.long, device=dev),
                           dict(type="soft_nms", method="naive", split_thr=-1))
    assert torch.equal(k.cpu(), torch.arange(10000))     # identical zero-area boxes: NaN IoU, weight 1, equal scores in index order
    assert bool((d[:, 4] == 1).all())


# ---------------------------------------------------------------------------------------------- detector path
@pytest.fixture(scope="module")
def det():
    from oracle import synth
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr_softnms.py"))
    cfg.model["pretrained"] = None
    d = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    synth.fill_state_dict(d.state_dict(), seed=0)
    d = d.cuda().eval()
    with torch.no_grad():
        d.bbox_head.atss_cls.bias += 2.0           # enough detections on random images
    return d


@pytest.fixture(scope="module")
def candidates(det):
    """every candidate of the API tests' synthetic head outputs: hard NMS at IoU 1.0 (IoU > 1 never holds), max_per_img = cap"""
    from oracle import synth
    from test_gpu_api import synth_head_outputs
    cls, reg, iou = synth_head_outputs(9, 2, cls_mean=-4.0)
    metas = synth.img_metas(2)
    cfg = dict(det.test_cfg)
    cap = 5 * int(cfg["nms_pre"])
    cfg.update(nms=dict(type="nms", iou_threshold=1.0), max_per_img=cap)
    res = det.bbox_head.get_bboxes(cls, reg, iou, metas, cfg=cfg, rescale=True)
    out = []
    for db, dl in res:
        db, dl = db.cpu().numpy(), dl.cpu().numpy()
        assert 1000 < len(db) <= cap
        assert len(np.unique(db[:, 4])) == len(db)                                        # no equal scores
        out.append((db[:, :4].copy(), db[:, 4].copy(), dl))
    return (cls, reg, iou, metas), out


@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_get_bboxes_soft_config(det, candidates, method):
    (cls, reg, iou, metas), cands = candidates
    cfg = dict(det.test_cfg)
    assert cfg["nms"]["type"] == "soft_nms" and int(cfg["max_per_img"]) == 100
    cfg["nms"] = dict(cfg["nms"], method=method)
    res = det.bbox_head.get_bboxes(cls, reg, iou, metas, cfg=cfg, rescale=True)
    assert len(res) == 2
    for (db, dl), (boxes, scores, labels) in zip(res, cands):
        rk, rs = batched_soft_nms(boxes, scores, labels, METHODS[method], 0.3, 0.5, 1e-3, max_out=100)
        assert len(rk) == 100 and tuple(db.shape) == (100, 5)
        db = db.cpu().numpy()
        assert np.array_equal(bits(db[:, :4]), bits(boxes[rk])) and np.array_equal(dl.cpu().numpy(), labels[rk])
        assert np.array_equal(bits(db[:, 4]), bits(rs))
    rt = det.runtime()
    soft = [v for k, v in rt._posts.items() if k[-1] == "soft"]
    assert soft and not any("aux0" in v or v["nws"].numel() > 2 * 24 * 5000 + 512 for v in soft)   # no dense-mask workspace


@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_detect_graph_soft_matches_eager(det, method):
    rt = det.runtime()
    cfg = dict(det.test_cfg)
    cfg["nms"] = dict(cfg["nms"], method=method)
    metas = [dict(img_shape=(160, 192, 3), scale_factor=np.ones(4, np.float32)) for _ in range(2)]
    g = torch.Generator().manual_seed(4)
    for rep in range(2):                                                                  # capture + replay, then replay
        img = torch.randn(2, 3, 160, 192, generator=g).cuda()
        a = rt.detect(img, metas, cfg, rescale=True)
        b = rt.detect_graph(img, metas, cfg, rescale=True)
        assert len(a) == len(b) == 2
        for (da, la), (db, lb) in zip(a, b):
            assert torch.equal(da, db) and torch.equal(la, lb)
        assert sum(d.shape[0] for d, _ in a) > 0
