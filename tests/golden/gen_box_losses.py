"""Generates tests/golden/box_losses.npz by RUNNING THE REFERENCE's IoULoss (-log and linear), DIoULoss and CIoULoss
(radet/models/losses/iou_loss.py) on the CPU, for tests/test_boxloss_cpu.py and tests/test_gpu_boxloss.py.

    python tests/golden/gen_box_losses.py

Only data is written.  The reference is imported at generation time through ref_import, exactly like gen_golden.py.

Function level: the 90 boxes of ops2.npz (g_pred / g_tgt / g_w: random pairs, identical pairs, disjoint pairs) plus 30
hand-made pairs (EDGE below; CIoU runs on `pred_ciou`, see gen_functions).  Per kind and per reduction of the GIoU
module test -- `mean`, weight + avg_factor, `none` + weight, `sum` -- the loss and d loss / d pred of the reference
CLASS in fp32 (`<kind>_<red>`, `..._g`) and of the same functions in fp64 (`..._64`, `..._g_64`).  Where the reference's own fp32 result is off its fp64 result by
more than the test tolerance the element is recorded in a mask (`..._m`, `..._g_m`); the tests judge those elements
against fp64.  At most 2 % of a tensor may be masked: asserted here, and if an input set fails it the inputs change.

Head level: RADetHead.loss on the inputs of test_head_loss_vs_reference_golden (synth_head_outputs(7, 2), assigner tags
g8 / g3) with each of the four `loss_bbox` configs: the three losses and the gradients at the positive rows, keys of
head_loss.npz prefixed with the kind (`h_<kind>_...`).

Ties: what the installed torch does at max / min / clamp ties is checked here before anything is written (ties_on_this_torch)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ref_import  # noqa: E402
from oracle import synth  # noqa: E402

torch.set_num_threads(8)
ref_import.install()

from radet.models import build_detector, build_loss  # noqa: E402

KINDS = dict(iou=dict(type="IoULoss"), iou_linear=dict(type="IoULoss", linear=True), diou=dict(type="DIoULoss"),
             ciou=dict(type="CIoULoss"))
LOSS_WEIGHT = 2.0
TOL_LOSS = dict(rtol=1e-4, atol=1e-7)          # close() of tests/test_gpu_api.py
TOL_GRAD = dict(rtol=2e-4, atol=1e-7)          # the GIoU module test's gradient tolerance
MASK_CAP = 0.02

# (pred, target, what the pair is there for); integer coordinates so that the ties are exact in fp32
EDGE = [
    ([10, 10, 50, 40], [50, 10, 90, 40], "touching: shared vertical edge, overlap width exactly 0"),
    ([10, 10, 50, 40], [10, 40, 50, 80], "touching: shared horizontal edge"),
    ([10, 10, 50, 40], [50, 40, 90, 80], "touching: one corner"),
    ([20, 20, 60, 50], [0, 0, 100, 100], "nested: pred inside target"),
    ([0, 0, 100, 100], [20, 20, 60, 50], "nested: target inside pred"),
    ([0, 0, 60, 50], [0, 0, 100, 100], "nested, two shared edges (max / min ties on x1, y1)"),
    ([40, 50, 100, 100], [0, 0, 100, 100], "nested, ties on x2, y2"),
    ([0, 20, 100, 60], [0, 0, 100, 100], "nested, ties on x1, x2"),
    ([30, 10, 30, 70], [10, 10, 60, 70], "zero-width pred inside the target"),
    ([80, 10, 80, 70], [10, 10, 60, 70], "zero-width pred outside the target"),
    ([10, 30, 60, 30], [10, 10, 60, 70], "zero-height pred inside the target"),
    ([10, 90, 60, 90], [10, 10, 60, 70], "zero-height pred outside the target"),
    ([30, 30, 30, 30], [10, 10, 60, 70], "zero-size pred"),
    ([10, 10, 60, 70], [30, 30, 30, 30], "zero-size target"),
    ([30, 30, 30, 30], [30, 30, 30, 30], "both zero-size and identical"),
    ([20, 15, 70, 75], [10, 10, 60, 70], "same width and height, shifted: v = 0 exactly"),
    ([10, 40, 60, 100], [10, 10, 60, 70], "same width and height, shifted along y with an x tie: v = 0"),
    ([200, 200, 250, 260], [10, 10, 60, 70], "same width and height, disjoint: v = 0"),
    ([0, 0, 100, 120], [10, 10, 60, 70], "same aspect ratio, doubled: v ~ 0 (eps in the heights)"),
    ([20, 22, 45, 52], [10, 10, 60, 70], "same aspect ratio, halved: v ~ 0"),
    ([0, 0, 1000, 1000], [999.5, 999.5, 2000, 2000], "IoU 1.25e-7 < eps: the clamp of IoULoss holds the gradient"),
    ([0, 0, 2000, 1000], [1999, 999, 4000, 2000], "IoU 2.5e-7 < eps"),
    ([0, 0, 200, 10], [0, 0, 10, 200], "elongated, crossed"),
    ([5, 0, 15, 300], [0, 0, 10, 200], "elongated, tall both"),
    ([0, 5, 300, 15], [0, 0, 200, 10], "elongated, wide both"),
    ([0, 0, 3, 400], [100, 0, 500, 4], "elongated, disjoint, opposite aspect"),
    ([12.5, 7.25, 80.75, 33.5], [10.25, 9.5, 70.5, 40.75], "generic non-integer pair"),
    ([100, 100, 101, 101], [100.5, 100.5, 101.5, 101.5], "unit boxes, quarter overlap"),
    ([0, 0, 640, 480], [1, 1, 639, 479], "near-identical large boxes"),
    ([300, 200, 308, 206], [301, 201, 307, 207], "small boxes"),
]


def ties_on_this_torch():
    """What autograd does at the ties the kernels restate (csrc/box_loss.h): binary max / min split 1/2 - 1/2,
    clamp(min=c) passes the gradient at x == c."""
    a = torch.tensor([1.0, 2.0], requires_grad=True)
    b = torch.tensor([1.0, 1.0])
    torch.max(a, b).sum().backward()
    g_max = a.grad.clone()
    a.grad = None
    torch.min(a, b).sum().backward()
    g_min = a.grad.clone()
    x = torch.tensor([0.0, -1.0, 1.0, 0.25], requires_grad=True)
    x.clamp(min=0).sum().backward()
    g_c0 = x.grad.clone()
    x.grad = None
    x.clamp(min=0.25).sum().backward()
    g_ceps = x.grad.clone()
    assert g_max.tolist() == [0.5, 1.0] and g_min.tolist() == [0.5, 0.0], (g_max, g_min)
    assert g_c0.tolist() == [1.0, 0.0, 1.0, 1.0], g_c0
    assert g_ceps.tolist() == [0.0, 0.0, 1.0, 1.0], g_ceps            # the 0.25 entry: equality passes
    return np.asarray([g_max[0], g_min[0], g_c0[0], g_ceps[3]], np.float32)


def run(mod, p, t, **kw):
    p = p.clone().requires_grad_(True)
    loss = mod(p, t, **kw)
    (loss.sum() if loss.dim() else loss).backward()
    return loss.detach().numpy(), p.grad.numpy().copy()


def off_mask(v32, v64, rtol, atol):
    return ~np.isclose(v32.astype(np.float64), v64, rtol=rtol, atol=atol)


def gen_functions(out):
    g2 = np.load(os.path.join(HERE, "ops2.npz"))
    gen = torch.Generator().manual_seed(21)
    pred = torch.cat([torch.from_numpy(g2["g_pred"]), torch.tensor([e[0] for e in EDGE], dtype=torch.float32)])
    tgt = torch.cat([torch.from_numpy(g2["g_tgt"]), torch.tensor([e[1] for e in EDGE], dtype=torch.float32)])
    w = torch.cat([torch.from_numpy(g2["g_w"]), torch.rand(len(EDGE), generator=gen) * 0.9 + 0.1])
    out.update(pred=pred.numpy(), tgt=tgt.numpy(), w=w.numpy(), n_ops2=np.int64(g2["g_pred"].shape[0]))
    # CIoU on an identical pair: in fp32 union + eps == union once the area exceeds a few units, so iou == 1, v == 0 and
    # the penalty v^2 / (1 - iou + v) is 0 / 0.  The reference returns NaN there (recorded below, `ciou_ident`), which
    # would swallow every reduced result, so CIoU gets the identical pairs of ops2 with x2 moved by half a pixel
    # (three of the four coordinates still tie).
    ident = (pred[:90] == tgt[:90]).all(1).nonzero().reshape(-1)
    assert ident.tolist() == [0, 1, 2, 3, 4]
    pred_ciou = pred.clone()
    pred_ciou[ident, 2] += 0.5
    nan_loss, nan_grad = run(build_loss(dict(KINDS["ciou"], loss_weight=LOSS_WEIGHT)), pred[ident], tgt[ident],
                             reduction_override="none")
    assert np.isnan(nan_loss).all()
    out.update(pred_ciou=pred_ciou.numpy(), ciou_ident=nan_loss, ciou_ident_g=nan_grad)
    t64, w64 = tgt.double(), w.double()
    for kind, cfg in KINDS.items():
        mod = build_loss(dict(cfg, loss_weight=LOSS_WEIGHT))
        pred, p64 = (pred_ciou, pred_ciou.double()) if kind == "ciou" else (pred, pred.double())
        for red, kw, kw64 in (("mean", {}, {}),
                              ("avg_w", dict(weight=w, avg_factor=w.sum()), dict(weight=w64, avg_factor=w64.sum())),
                              ("none_w", dict(weight=w, reduction_override="none"), dict(weight=w64, reduction_override="none")),
                              ("sum", dict(reduction_override="sum"), dict(reduction_override="sum"))):
            tag = f"{kind}_{red}"
            l32, g32 = run(mod, pred, tgt, **kw)
            l64, g64 = run(mod, p64, t64, **kw64)
            assert l32.dtype == np.float32 and g32.dtype == np.float32 and l64.dtype == np.float64 and g64.dtype == np.float64
            assert np.isfinite(l32).all() and np.isfinite(g32).all() and np.isfinite(l64).all() and np.isfinite(g64).all(), tag
            lm, gm = off_mask(l32, l64, **TOL_LOSS), off_mask(g32, g64, **TOL_GRAD)
            assert lm.mean() <= MASK_CAP and gm.mean() <= MASK_CAP, (tag, lm.mean(), gm.mean())
            print(f"{tag:18s} loss off fp64: {int(lm.sum())}/{lm.size}   grad off fp64: {int(gm.sum())}/{gm.size}")
            out.update({tag: l32, tag + "_g": g32, tag + "_64": l64, tag + "_g_64": g64, tag + "_m": lm, tag + "_g_m": gm})
    # the clamp of IoULoss at exact equality: IoU = 2 / 8 = eps = 0.25 (both exact in fp32) -> the gradient passes
    pe, te = torch.tensor([[0.0, 0.0, 2.0, 1.0]]), torch.tensor([[0.0, 0.0, 2.0, 4.0]])
    for kind in ("iou", "iou_linear"):
        le, ge = run(build_loss(dict(KINDS[kind], eps=0.25)), pe, te)
        assert np.abs(ge).sum() > 0
        out.update({f"{kind}_eq": le, f"{kind}_eq_g": ge})
    out.update(eq_pred=pe.numpy(), eq_tgt=te.numpy(), eq_eps=np.float32(0.25))


LEVEL_HW = [(60, 80), (30, 40), (15, 20), (8, 10), (4, 5)]


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


def gen_head(out):
    torch.manual_seed(0)
    model_cfg, train_cfg, test_cfg = ref_import.load_cfg()
    det = build_detector(model_cfg, train_cfg=train_cfg, test_cfg=test_cfg)
    head = det.bbox_head
    assign = np.load(os.path.join(HERE, "assigner.npz"))
    pos = torch.from_numpy(np.load(os.path.join(HERE, "head_loss.npz"))["pos"])
    tags, B = ["g8", "g3"], 2
    gt_b = [torch.from_numpy(assign[t + "_boxes"]) for t in tags]
    gt_l = [torch.from_numpy(assign[t + "_labels"]) for t in tags]
    p2g = [torch.from_numpy(assign[t + "_p2g"].astype(np.int64)) for t in tags]
    pw = [torch.from_numpy(assign[t + "_w"]) for t in tags]
    metas = synth.img_metas(B)
    for kind, cfg in KINDS.items():
        head.loss_bbox = build_loss(dict(cfg, loss_weight=LOSS_WEIGHT))
        cls, reg, iou = synth_head_outputs(7, B)
        for t in cls + reg + iou:
            t.requires_grad_(True)
        losses = head.loss(cls, reg, iou, gt_b, gt_l, p2g, pw, metas)
        sum(losses.values()).backward()
        g_cls, g_reg, g_iou = flat([t.grad for t in cls]), flat([t.grad for t in reg]), flat([t.grad for t in iou])
        outside = torch.ones(g_reg.shape[0], dtype=torch.bool)
        outside[pos] = False
        assert float(g_reg[outside].abs().sum()) == 0.0 and float(g_iou[outside].abs().sum()) == 0.0
        h = f"h_{kind}_"
        out.update({h + k: losses[k].detach().numpy() for k in ("loss_cls", "loss_bbox", "loss_iou")})
        out.update({h + "g_cls_pos": g_cls[pos].numpy(), h + "g_reg_pos": g_reg[pos].numpy(), h + "g_iou_pos": g_iou[pos].numpy(),
                    h + "g_reg_abs": g_reg.double().abs().sum().numpy()})
        print(h, {k: float(v) for k, v in losses.items()})


def main():
    out = dict(ties=ties_on_this_torch(), edge_notes=np.asarray([e[2] for e in EDGE]))
    gen_functions(out)
    gen_head(out)
    path = os.path.join(HERE, "box_losses.npz")
    np.savez_compressed(path, **out)
    print(f"box_losses.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
