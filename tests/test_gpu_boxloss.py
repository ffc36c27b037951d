"""IoULoss (-log / linear), DIoULoss and CIoULoss on the GPU: the registered modules (radet_box_loss / radet_box_loss_bwd)
and the fused head loss (radet_head_loss, kind in flags bits 1-3) against tests/golden/box_losses.npz -- the reference's
own classes run on the CPU (tests/golden/gen_box_losses.py) --, the module path against the fused one, GIoU unchanged,
bad arguments, empty batches and train steps from configs/bop/r50_ycbv_pbr_ciou.py."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4   # BASELINE.json north_star (tests/test_gpu_api.py)
KINDS = dict(iou=dict(type="IoULoss"), iou_linear=dict(type="IoULoss", linear=True), diou=dict(type="DIoULoss"),
             ciou=dict(type="CIoULoss"))
LEVEL_HW = [(60, 80), (30, 40), (15, 20), (8, 10), (4, 5)]
STRIDES = (8, 16, 32, 64, 128)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def run_loss(mod, x, *args, **kw):
    x = x.clone().requires_grad_(True)
    loss = mod(x, *args, **kw)
    (loss.sum() if loss.dim() else loss).backward()
    return loss.detach().cpu().numpy(), x.grad.cpu().numpy()


def judge(got, g, key, rtol, atol):
    """against the reference's fp32 result; where the fixture's mask says that result is itself off the reference's fp64
    one, against fp64 with 4 x the reference's own fp32 error as the bound (at most 2 % of a tensor: a cap)."""
    ref, ref64, m = g[key], g[key + "_64"], g[key + "_m"]
    assert m.mean() <= 0.02, key
    got = np.asarray(got)
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{key}: max |d| / tol = {float((err / (atol + rtol * np.abs(ref))).max()):.3g}, fp64-judged {int(m.sum())}")
    assert np.allclose(got[~m], ref[~m], rtol=rtol, atol=atol), key
    assert (np.abs(got[m].astype(np.float64) - ref64[m]) <= 4 * np.abs(ref[m].astype(np.float64) - ref64[m])).all(), key


def inputs(g, kind):
    return T(g["pred_ciou"] if kind == "ciou" else g["pred"]), T(g["tgt"]), T(g["w"])


# ------------------------------------------------------------------------------------------------ modules
@pytest.mark.parametrize("red", ["mean", "avg_w", "none_w", "sum"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_module_vs_reference(golden, kind, red):
    from radet_amd.models import build_loss
    g = golden("box_losses")
    p, t, w = inputs(g, kind)
    kw = dict(mean={}, avg_w=dict(weight=w, avg_factor=w.sum()), none_w=dict(weight=w, reduction_override="none"),
              sum=dict(reduction_override="sum"))[red]
    loss, grad = run_loss(build_loss(dict(KINDS[kind], loss_weight=2.0)), p, t, **kw)
    judge(loss, g, f"{kind}_{red}", TOL, 1e-7)                        # close() of test_gpu_api.py
    judge(grad, g, f"{kind}_{red}_g", 2e-4, 1e-7)                     # the GIoU module test's gradient tolerance


@pytest.mark.parametrize("kind", list(KINDS))
def test_module_weight_contract(golden, kind):
    """all-zero weights -> exactly 0 (IoULoss: not under reduction 'none', iou_loss.py:264-266); weight [n, 4] == its
    row mean; inputs on the device give results on the device; sum + avg_factor is refused"""
    from radet_amd.models import build_loss
    g = golden("box_losses")
    p, t, w = inputs(g, kind)
    mod = build_loss(dict(KINDS[kind], loss_weight=2.0))
    z, zg = run_loss(mod, p, t, weight=torch.zeros(120))
    assert float(z) == 0.0 and not zg.any()
    zn = mod(p, t, weight=torch.zeros(120), reduction_override="none")
    assert (tuple(zn.shape) == (120,) and not zn.any()) if kind.startswith("iou") else (zn.dim() == 0 and float(zn) == 0.0)
    w4 = torch.stack([w * 0.5, w * 1.5, w * 0.25, w * 1.75], 1)
    a, ag = run_loss(mod, p, t, weight=w4, avg_factor=7.0)
    b, bg = run_loss(mod, p, t, weight=w4.mean(-1), avg_factor=7.0)
    assert np.array_equal(a, b) and np.array_equal(ag, bg)
    x = p.cuda().requires_grad_(True)
    out = mod(x, t.cuda(), weight=w.cuda(), avg_factor=w.sum().cuda())
    out.backward()
    assert out.is_cuda and x.grad.is_cuda
    assert np.array_equal(out.detach().cpu().numpy(), run_loss(mod, p, t, weight=w, avg_factor=w.sum())[0])   # deterministic
    with pytest.raises(ValueError):
        mod(p, t, avg_factor=3.0, reduction_override="sum")


def test_clamp_at_equality_and_ciou_identical_pairs(golden):
    """IoU == eps exactly: the clamp passes the gradient, as torch's does.  CIoU on identical pairs: 0 / 0 in the penalty, NaN
    in the reference's own fp32 run and here (the formulas are followed to the letter)."""
    from radet_amd.models import build_loss
    g = golden("box_losses")
    for kind in ("iou", "iou_linear"):
        loss, grad = run_loss(build_loss(dict(KINDS[kind], eps=float(g["eq_eps"]))), T(g["eq_pred"]), T(g["eq_tgt"]))
        assert np.allclose(loss, g[kind + "_eq"], rtol=TOL, atol=1e-7) and np.allclose(grad, g[kind + "_eq_g"], rtol=2e-4, atol=1e-7)
    loss, grad = run_loss(build_loss(dict(type="CIoULoss", loss_weight=2.0)), T(g["pred"][:5]), T(g["tgt"][:5]),
                          reduction_override="none")
    assert np.array_equal(np.isnan(loss), np.isnan(g["ciou_ident"])) and np.isnan(loss).all()
    assert np.array_equal(np.isnan(grad), np.isnan(g["ciou_ident_g"]))


def test_box_loss_giou_kind_is_the_giou_kernel(golden):
    """radet_box_loss(kind = GIoU) == radet_giou_loss bit for bit on the 120 boxes: elements, partial sums, gradient"""
    from radet_amd import kernels as K
    g = golden("box_losses")
    p, t, w = (x.cuda() for x in inputs(g, "giou"))
    n = p.shape[0]
    outs = []
    for via_kind in (False, True):
        elem, part, dp = torch.full((n,), 7.0, device="cuda"), torch.full((K.loss_partials(n),), 7.0, device="cuda"), \
            torch.full((n, 4), 7.0, device="cuda")
        gs = torch.tensor([0.75], device="cuda")
        if via_kind:
            K.box_loss("giou", p, t, w, n, 1e-6, elem, part, 2.0)
            K.box_loss_bwd("giou", p, t, w, n, 1e-6, None, gs, None, 2.0, dp)
        else:
            K.giou_loss(p, t, w, n, 1e-6, elem, part, 2.0)
            K.giou_loss_bwd(p, t, w, n, 1e-6, None, gs, None, 2.0, dp)
        outs.append((elem.cpu(), part.cpu(), dp.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b) and not (a == 7.0).all()


def test_box_loss_unknown_kind_stores_nothing(golden):
    from radet_amd import _lib, kernels as K
    g = golden("box_losses")
    p, t, _ = (x.cuda() for x in inputs(g, "iou"))
    n = p.shape[0]
    elem, part, dp = torch.full((n,), 7.0, device="cuda"), torch.full((K.loss_partials(n),), 7.0, device="cuda"), \
        torch.full((n, 4), 7.0, device="cuda")
    lib = _lib.load()
    for kind in (5, 7, -1, 100):
        assert lib.radet_box_loss(kind, p.data_ptr(), t.data_ptr(), None, n, 1e-6, 0.0, elem.data_ptr(), 1.0, part.data_ptr(), None) == -1
        assert lib.radet_box_loss_bwd(kind, p.data_ptr(), t.data_ptr(), None, n, 1e-6, 0.0, None, None, None, 1.0, dp.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (elem == 7.0).all() and (part == 7.0).all() and (dp == 7.0).all()


# ------------------------------------------------------------------------------------------------ fused head loss
def synth_head_outputs(seed, B, cls_mean=-2.0):
    g = torch.Generator().manual_seed(seed)
    cls, reg, iou = [], [], []
    for (h, w) in LEVEL_HW:
        cls.append(torch.randn(B, 21, h, w, generator=g) * 1.5 + cls_mean)
        reg.append(torch.relu(torch.randn(B, 4, h, w, generator=g) * 2.0 + 2.5))
        iou.append(torch.randn(B, 1, h, w, generator=g))
    return cls, reg, iou


def flat(ts):
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in ts])


def targets(golden, tags=("g8", "g3")):
    a = golden("assigner")
    return ([T(a[t + "_boxes"]) for t in tags], [T(a[t + "_labels"]) for t in tags],
            [T(a[t + "_p2g"].astype(np.int64)) for t in tags], [T(a[t + "_w"]) for t in tags])


def pack(gt_b, gt_l, p2g, pw, dev="cuda"):
    off = np.zeros(len(gt_b) + 1, np.int32)
    off[1:] = np.cumsum([b.shape[0] for b in gt_b])
    return dict(boxes=torch.cat(gt_b).to(dev), labels=torch.cat(gt_l).to(dev), off=T(off).to(dev),
                p2g=torch.stack(p2g).to(dev), pw=torch.stack(pw).to(dev))


def run_head_loss(cls, reg, iou, tg, B, flags=0, eps=1e-6, fill=0.0, dumps=False):
    from radet_amd import kernels as K
    dev = "cuda"
    lv = K.Levels(LEVEL_HW, B)
    ld, nl = K.level_desc(lv, STRIDES)
    R = lv.rows
    fc, fr, fi = flat(cls).to(dev), flat(reg).to(dev), flat(iou).reshape(-1).contiguous().to(dev)
    out = dict(losses=torch.full((3,), fill, device=dev), dcls=torch.full((R, 21), fill, device=dev),
               dreg=torch.full((R, 4), fill, device=dev), diou=torch.full((R,), fill, device=dev),
               dsc=torch.full((5,), fill, device=dev))
    ws = torch.zeros(K.head_loss_ws_ints(R), dtype=torch.int32, device=dev)
    tgt = torch.zeros(R, 4, device=dev) if dumps else None
    K.head_loss(fc, fr, fi, torch.ones(5, device=dev), tg["boxes"], tg["labels"], tg["off"], tg["p2g"], tg["pw"], ld, nl, B, 21,
                0.25, 2.0, 2.0, eps, None, out["losses"], out["dcls"], 21, out["dreg"], 4, out["diou"], 1, out["dsc"], ws, None,
                tgt, flags=flags)
    out["ws"], out["tgt"], out["reg"] = ws, tgt, fr
    return out


@pytest.fixture(scope="module")
def head_case(golden):
    """the inputs of test_head_loss_vs_reference_golden and the GIoU run every kind is held against"""
    cls, reg, iou = synth_head_outputs(7, 2)
    tg = pack(*targets(golden))
    return cls, reg, iou, tg, run_head_loss(cls, reg, iou, tg, 2, dumps=True)


@pytest.mark.parametrize("kind", list(KINDS))
def test_fused_head_loss_vs_reference(golden, head_case, kind):
    from radet_amd import kernels as K
    g, h = golden("box_losses"), golden("head_loss")
    cls, reg, iou, tg, base = head_case
    o = run_head_loss(cls, reg, iou, tg, 2, flags=K.head_loss_flags(kind))
    L = o["losses"].cpu().numpy()
    for i, k in enumerate(("loss_cls", "loss_bbox", "loss_iou")):
        ref = float(g[f"h_{kind}_{k}"])
        print(kind, k, L[i], ref)
        assert abs(L[i] - ref) <= TOL * max(1.0, abs(ref)), (k, L[i], ref)
    pos = T(h["pos"])
    dr, di, dc = o["dreg"].cpu(), o["diou"].cpu(), o["dcls"].cpu()
    live = (flat(reg)[pos] > 0).numpy()               # the golden gradient is w.r.t. the post-ReLU tensor (relu'(0) = 0 here)
    ref = g[f"h_{kind}_g_reg_pos"]
    print(kind, "dreg max |d| / tol", float((np.abs(dr[pos].numpy() - ref) / (1e-8 + TOL * np.abs(ref)))[live].max()))
    assert np.allclose(dr[pos].numpy()[live], ref[live], rtol=TOL, atol=1e-8)
    assert float(np.abs(dr[pos].numpy()[~live]).sum()) == 0.0
    assert np.allclose(di[pos].numpy(), g[f"h_{kind}_g_iou_pos"].reshape(-1), rtol=TOL, atol=1e-9)
    assert np.allclose(dc[pos].numpy(), g[f"h_{kind}_g_cls_pos"], rtol=TOL, atol=1e-9)
    outside = torch.ones(dr.shape[0], dtype=torch.bool)
    outside[pos] = False
    assert float(dr[outside].abs().sum()) == 0.0 and float(di[outside].abs().sum()) == 0.0
    # the classification and IoU branches do not see the kind: bit for bit the GIoU run
    assert L[0] == float(base["losses"][0]) and L[2] == float(base["losses"][2]) and L[1] != float(base["losses"][1])
    assert torch.equal(dc, base["dcls"].cpu()) and torch.equal(di, base["diou"].cpu())
    assert not torch.equal(dr, base["dreg"].cpu())
    # two runs are bit-identical
    o2 = run_head_loss(cls, reg, iou, tg, 2, flags=K.head_loss_flags(kind))
    assert all(torch.equal(o[k], o2[k]) for k in ("losses", "dcls", "dreg", "diou", "dsc"))


def test_fused_giou_unchanged(golden, head_case):
    """kind 0 through the templated kernel: two runs bit-identical, explicit kind 0 == flags 0, and head_loss.npz as before"""
    from radet_amd import kernels as K
    h = golden("head_loss")
    cls, reg, iou, tg, base = head_case
    assert K.head_loss_flags("giou") == 0
    o = run_head_loss(cls, reg, iou, tg, 2, flags=K.head_loss_flags("giou"))
    assert all(torch.equal(o[k], base[k]) for k in ("losses", "dcls", "dreg", "diou", "dsc"))
    L = o["losses"].cpu().numpy()
    for i, k in enumerate(("loss_cls", "loss_bbox", "loss_iou")):
        assert abs(L[i] - float(h[k])) <= TOL * max(1.0, abs(float(h[k]))), (k, L[i], float(h[k]))
    pos = T(h["pos"])
    live = (flat(reg)[pos] > 0).numpy()
    assert np.allclose(o["dreg"].cpu()[pos].numpy()[live], h["g_reg_pos"][live], rtol=TOL, atol=1e-8)
    assert np.allclose(o["diou"].cpu()[pos].numpy(), h["g_iou_pos"].reshape(-1), rtol=TOL, atol=1e-9)
    assert np.allclose(o["dcls"].cpu()[pos].numpy(), h["g_cls_pos"], rtol=TOL, atol=1e-9)


def test_fused_unknown_kind_stores_nothing(head_case):
    from radet_amd._lib import RadetHipError
    cls, reg, iou, tg, _ = head_case
    for kind in (5, 6, 7):
        for postact in (0, 1):
            with pytest.raises(RadetHipError, match="radet_head_loss"):
                run_head_loss(cls, reg, iou, tg, 2, flags=(kind << 1) | postact, fill=7.0)
    # the same call again, by hand, to look at the buffers it was given
    from radet_amd import kernels as K
    lv = K.Levels(LEVEL_HW, 2)
    ld, nl = K.level_desc(lv, STRIDES)
    R = lv.rows
    bufs = [torch.full(s, 7.0, device="cuda") for s in ((3,), (R, 21), (R, 4), (R,), (5,))]
    ws = torch.full((K.head_loss_ws_ints(R),), 7, dtype=torch.int32, device="cuda")
    with pytest.raises(RadetHipError):
        K.head_loss(flat(cls).cuda(), flat(reg).cuda(), flat(iou).reshape(-1).cuda(), torch.ones(5, device="cuda"), tg["boxes"],
                    tg["labels"], tg["off"], tg["p2g"], tg["pw"], ld, nl, 2, 21, 0.25, 2.0, 2.0, 1e-6, None, bufs[0], bufs[1], 21,
                    bufs[2], 4, bufs[3], 1, bufs[4], ws, flags=5 << 1)
    torch.cuda.synchronize()
    assert all((b == 7.0).all() for b in bufs) and (ws == 7).all()


@pytest.mark.parametrize("kind", list(KINDS))
def test_fused_no_gt(golden, kind):
    from radet_amd import kernels as K
    h = golden("head_loss")
    cls, reg, iou = synth_head_outputs(8, 2)
    dev = "cuda"
    tg = dict(boxes=torch.zeros(1, 4, device=dev), labels=torch.zeros(1, dtype=torch.long, device=dev),
              off=torch.zeros(3, dtype=torch.int32, device=dev), p2g=torch.full((2, 6400), -1, dtype=torch.long, device=dev),
              pw=torch.ones(2, 6400, device=dev))
    o = run_head_loss(cls, reg, iou, tg, 2, flags=K.head_loss_flags(kind), fill=3.0)
    L = o["losses"].cpu().numpy()
    assert abs(L[0] - float(h["e_loss_cls"])) <= TOL * float(h["e_loss_cls"]) and L[1] == 0.0 and L[2] == 0.0
    assert float(o["dreg"].abs().sum()) == 0.0 and float(o["diou"].abs().sum()) == 0.0 and float(o["dsc"].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ fused == modules
@pytest.fixture(scope="module")
def det():
    from oracle import synth
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr_ciou.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    d = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    synth.fill_state_dict(d.state_dict(), seed=0)
    return d.cuda().train()


@pytest.mark.parametrize("kind", list(KINDS))
def test_fused_equals_module_path(golden, head_case, det, kind):
    """radet_head_loss(kind) == RADetHead.loss with that `loss_bbox` built by the registry (NCHW lists in, autograd out; the
    tolerances of test_head_loss_method_vs_reference_golden), and its loss_bbox == the registered class itself evaluated by
    the stand-alone kernels on the decoded positive boxes, as radet_head.py:262-274 calls it."""
    from oracle import synth
    from radet_amd import kernels as K
    from radet_amd.core import bbox_overlaps
    from radet_amd.models import build_loss
    h = golden("head_loss")
    cls, reg, iou, tg, base = head_case
    o = run_head_loss(cls, reg, iou, tg, 2, flags=K.head_loss_flags(kind))
    head = det.bbox_head
    keep = head.loss_bbox
    head.loss_bbox = build_loss(dict(KINDS[kind], loss_weight=2.0))
    try:
        c, r, i = ([t.clone().requires_grad_(True) for t in ts] for ts in (cls, reg, iou))
        losses = head.loss(c, r, i, *targets(golden), synth.img_metas(2))
        assert det.runtime().loss_hparams["box_kind"] == kind
        sum(losses.values()).backward()
    finally:
        head.loss_bbox = keep
    L = o["losses"].cpu().numpy()
    for j, k in enumerate(("loss_cls", "loss_bbox", "loss_iou")):
        assert abs(losses[k].item() - L[j]) <= TOL * max(1.0, abs(L[j])), (k, losses[k].item(), L[j])
    pos = T(h["pos"])
    g_cls, g_reg, g_iou = flat([t.grad for t in c]), flat([t.grad for t in r]), flat([t.grad for t in i])
    live = (flat(reg)[pos] > 0).numpy()
    assert np.allclose(g_reg[pos].numpy()[live], o["dreg"].cpu()[pos].numpy()[live], rtol=TOL, atol=1e-8)
    assert np.allclose(g_iou[pos].numpy().reshape(-1), o["diou"].cpu()[pos].numpy(), rtol=TOL, atol=1e-9)
    assert np.allclose(g_cls[pos].numpy(), o["dcls"].cpu()[pos].numpy(), rtol=TOL, atol=1e-9)
    # the class on its own
    B = 2
    anchors = torch.cat([a.repeat(B, 1) for a in head.anchor_generator.grid_anchors(LEVEL_HW, "cuda")])[pos.cuda()]
    dp = head.bbox_coder.decode(anchors, o["reg"][pos.cuda()])
    dt = head.bbox_coder.decode(anchors, base["tgt"][pos.cuda()])
    iou_t = bbox_overlaps(dp, dt, is_aligned=True)
    pwt = torch.cat([tg["pw"][:, a:b].reshape(-1) for a, b in zip(np.cumsum([0] + [hh * ww for hh, ww in LEVEL_HW])[:-1],
                                                                  np.cumsum([hh * ww for hh, ww in LEVEL_HW]))])[pos.cuda()]
    wgt = iou_t.clamp(min=1e-12) * pwt
    lb = build_loss(dict(KINDS[kind], loss_weight=2.0))(dp, dt, weight=wgt, avg_factor=wgt.sum())
    assert abs(float(lb) - L[1]) <= TOL * max(1.0, abs(L[1])), (float(lb), L[1])


# ------------------------------------------------------------------------------------------------ train steps
def small_batch(H=224, W=224, B=2):
    """the small synthetic batch of tests/test_gpu_configs.py"""
    from oracle import assigner as oa, synth
    img = synth.synth_images(5, B, H, W)
    gt_b, gt_l, p2g, pw = [], [], [], []
    for i in range(B):
        g = (3, 2)[i % 2]
        rng = np.random.RandomState(40 + i)
        boxes = np.zeros((g, 4), np.float32)
        masks = np.zeros((g, H, W), np.uint8)
        for k in range(g):
            w, h = rng.randint(30, W // 2), rng.randint(30, H // 2)
            x, y = rng.randint(0, W - w), rng.randint(0, H - h)
            boxes[k] = (x, y, x + w, y + h)
            masks[k, y:y + h, x + w // 4:x + w] = 1
        labels = rng.randint(0, 21, g).astype(np.int64)
        a, wt = oa.assign_points(boxes, labels, masks, (H, W, 3), rng=np.random.RandomState(i))
        gt_b.append(torch.from_numpy(boxes)); gt_l.append(torch.from_numpy(labels))
        p2g.append(torch.from_numpy(a)); pw.append(torch.from_numpy(wt))
    return img, gt_b, gt_l, p2g, pw


def build(config, math=None):
    from oracle import synth
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", config))
    cfg.model["pretrained"] = None
    d = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    synth.fill_state_dict(d.state_dict(), seed=1)
    d = d.cuda().train()
    rt = d.runtime(math=math) if math else d.runtime()
    rt.set_loss_from_head(d.bbox_head)
    return d, rt


def steps(config, tape, n):
    d, rt = build(config)
    rt.tape_mode = tape
    rt.init_optimizer()
    img, gt_b, gt_l, p2g, pw = small_batch()
    tg = rt.pack_targets(gt_b, gt_l, p2g, pw)
    img = img.cuda()
    losses = [rt.train_step(img, tg, lr=4e-4 * (1 + 0.1 * i)).clone() for i in range(n)]
    torch.cuda.synchronize()
    return d, rt, torch.stack(losses).cpu(), rt.flat.params.clone().cpu()


@functools.lru_cache(maxsize=None)
def eager_ciou():
    return steps("r50_ycbv_pbr_ciou.py", "0", 6)


def test_ciou_config_train_step(golden):
    """set_loss_from_head picks CIoU from the config; the step's loss_bbox is not GIoU's and is the module path's"""
    from oracle import synth
    d, rt, losses, _ = eager_ciou()
    assert rt.loss_hparams["box_kind"] == "ciou" and rt.loss_hparams["box_eps"] == 1e-6 and rt.loss_hparams["lbw"] == 2.0
    _, rtg, lg, _ = steps("r50_ycbv_pbr.py", "0", 1)
    assert rtg.loss_hparams["box_kind"] == "giou"
    assert torch.isfinite(losses).all() and losses[0, 0] == lg[0, 0] and losses[0, 2] == lg[0, 2]      # same weights, same batch
    assert abs(float(losses[0, 1]) - float(lg[0, 1])) > 1e-3 * float(lg[0, 1])
    # module path on a detector with the step-0 parameters: RADetHead.forward -> RADetHead.loss with the registry's CIoULoss
    d0, _ = build("r50_ycbv_pbr_ciou.py")
    img, gt_b, gt_l, p2g, pw = small_batch()
    with torch.no_grad():
        outs = d0.bbox_head(d0.extract_feat(img.cuda()))
    lm = d0.bbox_head.loss(*outs, gt_b, gt_l, p2g, pw, synth.img_metas(2, 224, 224))
    for j, k in enumerate(("loss_cls", "loss_bbox", "loss_iou")):
        assert abs(float(lm[k]) - float(losses[0, j])) <= 1e-6 * max(1.0, abs(float(losses[0, j]))), (k, float(lm[k]), losses[0])


def test_ciou_taped_steps_equal_eager_and_repeat():
    """the kind and eps are scalars on the launch tape like the other loss hyper-parameters: taped == eager bit for bit, and a
    second taped run == the first"""
    _, _, le, pe = eager_ciou()
    runs = [steps("r50_ycbv_pbr_ciou.py", "1", 6) for _ in range(2)]
    for _, rt, _, _ in runs:
        st = rt.tape_stats()
        assert st is not None and st["replays"] >= 2, (st, rt._tape["failed"])
    assert torch.equal(le, runs[0][2]) and torch.equal(pe, runs[0][3])
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])


def test_ciou_bf16_storage_step_is_finite():
    d, rt = build("r50_ycbv_pbr_ciou.py", math="bf16-storage")
    assert rt.engine.h16 and rt.loss_hparams["box_kind"] == "ciou"
    rt.init_optimizer()
    img, gt_b, gt_l, p2g, pw = small_batch()
    out = rt.train_step(img.cuda(), rt.pack_targets(gt_b, gt_l, p2g, pw))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and float(out[1]) > 0
    assert torch.isfinite(rt.flat.params).all()
