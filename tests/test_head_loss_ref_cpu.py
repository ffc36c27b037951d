"""tests/_head_loss_ref.py and tests/_head_loss_cases.py, checked without a GPU: the restatement in fp32 equals
oracle.model.head_loss + autograd and tests/golden/head_loss.npz on the golden geometry, its box losses in fp64 equal the
fp64 columns of tests/golden/box_losses.npz, and every case of tests/test_gpu_head_loss.py holds what it claims to hold
(P, row blocks, the edge) with at most 2 % of its positive rows near a branch -- all read off the fp64 restatement."""
import numpy as np
import pytest
import torch

import _head_loss_cases as HC
import _head_loss_ref as HR

from test_gpu_kernels import LEVEL_HW, STRIDES, TOL, synth_head_outputs   # the inputs of test_head_loss_vs_reference_golden


def flat(ts):
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in ts])


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_fp32_restatement_equals_oracle_and_golden(golden):
    from oracle import model as om
    g, a = golden("head_loss"), golden("assigner")
    tags = ("g8", "g3")
    gt_b = [torch.from_numpy(a[t + "_boxes"]) for t in tags]
    gt_l = [torch.from_numpy(a[t + "_labels"]) for t in tags]
    p2g = [torch.from_numpy(a[t + "_p2g"].astype(np.int64)) for t in tags]
    pw = [torch.from_numpy(a[t + "_w"]) for t in tags]
    cls, reg, iou = synth_head_outputs(7, 2)
    for t in cls + reg + iou:
        t.requires_grad_(True)
    losses, (labels, tgts, _, pos) = om.head_loss(cls, reg, iou, gt_b, gt_l, p2g, pw)
    (losses["loss_cls"] + losses["loss_bbox"] + losses["loss_iou"]).backward()
    off = torch.tensor([0, gt_b[0].shape[0], gt_b[0].shape[0] + gt_b[1].shape[0]], dtype=torch.int32)
    levels = [(h, w, s) for (h, w), s in zip(LEVEL_HW, STRIDES)]
    scales = torch.tensor([0.8, 1.1, 0.9, 1.3, 0.7])
    # reg is post-ReLU already: relu(1 * reg) == reg and the gradient w.r.t. it is the oracle's where reg > 0
    o = HR.head_loss_ref(flat(cls).detach(), flat(reg).detach(), flat(iou).detach().reshape(-1), torch.ones(5), torch.cat(gt_b),
                         torch.cat(gt_l), off, torch.stack(p2g), torch.stack(pw), levels, 2, 21, dtype=torch.float32)
    for i, k in enumerate(("loss_cls", "loss_bbox", "loss_iou")):
        assert abs(float(o["losses"][i]) - losses[k].item()) <= 1e-6 * abs(losses[k].item()), k
        assert abs(float(o["losses"][i]) - float(g[k])) <= TOL * max(1.0, abs(float(g[k]))), k
    live = flat(reg).detach() > 0
    assert rel(o["dcls"], flat([t.grad for t in cls])) <= 1e-6
    assert rel(o["dreg"] * live, flat([t.grad for t in reg]) * live) <= 1e-6 and float((o["dreg"] * ~live).abs().sum()) == 0.0
    assert rel(o["diou"], flat([t.grad for t in iou]).reshape(-1)) <= 1e-6
    assert np.array_equal(o["labels"].numpy(), g["labels"].astype(np.int64)) and torch.equal(o["labels"], labels)
    assert np.array_equal(o["pos"].numpy(), g["pos"]) and torch.equal(o["pos"], pos)
    assert np.array_equal(o["targets"][o["pos"]].numpy(), g["bbox_targets_pos"]) and torch.equal(o["targets"], tgts)
    # the Scale parameters: relu(scale * u) in front of the oracle, as test_head_loss_no_gt_and_scales builds it
    gsc = torch.Generator().manual_seed(4)
    reg_u = [(torch.randn(r.shape, generator=gsc) * 2 + 1.5).requires_grad_(True) for r in reg]
    sc = scales.clone().requires_grad_(True)
    c2 = [t.detach().clone().requires_grad_(True) for t in cls]
    i2 = [t.detach().clone().requires_grad_(True) for t in iou]
    l2, _ = om.head_loss(c2, [torch.relu(u * sc[i]) for i, u in enumerate(reg_u)], i2, gt_b, gt_l, p2g, pw)
    up = [0.5, 2.0, 3.0]
    (l2["loss_cls"] * up[0] + l2["loss_bbox"] * up[1] + l2["loss_iou"] * up[2]).backward()
    o = HR.head_loss_ref(flat(c2).detach(), flat(reg_u).detach(), flat(i2).detach().reshape(-1), scales, torch.cat(gt_b),
                         torch.cat(gt_l), off, torch.stack(p2g), torch.stack(pw), levels, 2, 21, grad_scale=up, dtype=torch.float32)
    assert rel(o["dscales"], sc.grad) <= 1e-6 and rel(o["dreg"], flat([u.grad for u in reg_u])) <= 1e-6
    assert rel(o["dcls"], flat([t.grad for t in c2])) <= 1e-6 and rel(o["diou"], flat([t.grad for t in i2]).reshape(-1)) <= 1e-6
    assert rel(o["losses"], torch.stack([l2[k] for k in ("loss_cls", "loss_bbox", "loss_iou")]).detach()) <= 1e-6


@pytest.mark.parametrize("kind", ["iou", "iou_linear", "diou", "ciou"])
def test_fp64_box_losses_equal_the_fixture(golden, kind):
    """`<kind>_none_w_64` = loss_weight 2 x w x the per-pair loss, and its gradient, of the reference's functions in fp64"""
    g = golden("box_losses")
    p = torch.from_numpy(g["pred_ciou"] if kind == "ciou" else g["pred"]).double().requires_grad_(True)
    t, w = torch.from_numpy(g["tgt"]).double(), torch.from_numpy(g["w"]).double()
    loss = 2.0 * w * HR.box_loss(kind, p, t, 1e-6)
    loss.sum().backward()
    assert np.allclose(loss.detach().numpy(), g[f"{kind}_none_w_64"], rtol=1e-12, atol=1e-12)
    assert np.allclose(p.grad.numpy(), g[f"{kind}_none_w_g_64"], rtol=1e-12, atol=1e-12)


def test_giou_box_loss_equals_the_oracle(golden):
    from oracle import model as om
    g = golden("box_losses")
    p, t = torch.from_numpy(g["pred"]).double(), torch.from_numpy(g["tgt"]).double()
    assert torch.equal(HR.box_loss("giou", p, t, 1e-6), 1 - om.overlaps_aligned(p, t, "giou", eps=1e-6))
    assert torch.equal(HR.aligned_iou(p, t), om.overlaps_aligned(p, t))


def test_num_pos_zero_is_the_kernels_contract():
    """positives of weight 0 only: loss_bbox = loss_iou = 0, no gradient for reg / iou / scales; loss_cls over 0 + B"""
    c = HC.get("noweight")
    o = HC.reference(c, c.hp, torch.float64)
    assert o["pos"].numel() == c.claims["P"] and float(o["num_pos"]) == 0.0
    assert float(o["losses"][1]) == 0.0 and float(o["losses"][2]) == 0.0 and float(o["losses"][0]) > 0
    assert not o["dreg"].any() and not o["diou"].any() and not o["dscales"].any() and o["dcls"].abs().sum() > 0


# ------------------------------------------------------------------------------------------------ the cases
def hp_list(name):
    if name == "eight":
        return HC.eight_variants()
    if name == "many1500":
        return HC.kind_variants()
    if name == "ties":
        return [dict(HC.DEFAULTS, kind=k) for k in ("giou", "iou", "diou")]
    if name == "flat":
        return [dict(HC.DEFAULTS, kind=k) for k in HR.KINDS]
    return [dict(HC.DEFAULTS)]


@pytest.mark.parametrize("name", list(HC.CASES))
def test_case_claims_and_margin_cap(name):
    c = HC.get(name)
    R = sum(c.B * h * w for h, w, _ in c.levels)
    assert c.R == R and c.cls.shape == (R, c.C) and c.reg_u.shape == (R, 4) and c.cls.dtype == torch.float32
    first = None
    for hp in hp_list(name):
        o = HC.reference(c, hp, torch.float64)
        first = first or o
        assert all(torch.isfinite(o[k]).all() for k in ("losses", "dcls", "dreg", "diou", "dscales")), hp
        P = o["pos"].numel()
        assert torch.equal(o["pos"], o["pos"].sort().values)
        if name != "ties" and P:
            near = float((o["margin"] < HR.MARGIN_MIN).double().mean())
            print(name, HC.variant_id(hp), "P", P, "rows under the margin", int((o["margin"] < HR.MARGIN_MIN).sum()))
            assert near <= HR.MARGIN_CAP, (name, hp, near)
    o = first
    pos, P, cl = o["pos"], o["pos"].numel(), c.claims
    blocks = (R + 255) // 256
    w_pos = c.pw[c.geo["img"][pos], c.geo["pt"][pos]]
    if "P" in cl:
        assert P == cl["P"]
    if name not in ("noweight", "nopos"):
        assert float(o["num_pos"]) > 0 and int((w_pos == 0).sum()) >= (2 if P > 2 else 1)     # a few positives of weight exactly 0
        assert float(w_pos.max()) <= 2.0 and float(w_pos[w_pos > 0].min()) >= 0.1
    if name == "tiny":
        assert R == 6 and blocks == 1 and R * c.C < 256
    if name == "block":
        assert R == 256 and P == 256
    if name in ("eight", "saturated", "ties"):
        assert len(c.levels) == 8 and c.B == 3 and set(c.geo["lvl"][pos].tolist()) == set(range(8))
        assert sorted(s for _, _, s in c.levels) == [4, 8, 16, 32, 64, 128, 256, 512] and sum(h * w == 1 for h, w, _ in c.levels) == 4
        assert set(c.geo["img"][pos].tolist()) == {0, 1, 2}
    if name == "eight":
        assert len(set(c.scales.tolist())) == 8 and (o["dscales"] != 0).all()
    if name.startswith("many"):
        lo = HC.MANY_BLOCK * 256
        per_block = torch.bincount(pos // 256, minlength=blocks)
        assert R == 4000 and per_block[HC.MANY_BLOCK] == 256 and per_block[HC.MANY_BLOCK - 1] == 0 and per_block[HC.MANY_BLOCK + 1] == 0
        assert P in (256, 257, 1500) and (P == 256 or (pos < lo).any() or (pos >= lo + 256).any())
    if name == "long":
        assert R == 264000 and blocks == 1032 and (blocks + 1023) // 1024 == 2 and R % 256 == 64
        t = HC.LONG_THREAD
        per_block = torch.bincount(pos // 256, minlength=blocks)
        assert pos[0] == 0 and pos[-1] == R - 1 and per_block[2 * t] > 0 and per_block[2 * t + 1] > 0 and per_block[blocks - 1] >= 2
        assert set(cl["rows"]) <= set(pos.tolist())
    if name in ("engine", "engine_small", "flat"):
        assert c.C == 21 and c.B == 4 and len(c.levels) == 5
    if name == "saturated":
        lab = o["labels"]
        for k, x in enumerate(HC.SATURATED):
            r = int(cl["saturated_pos"][k])
            assert float(c.cls[r, lab[r]]) == x and lab[r] < c.C and abs(float(c.iou[r])) >= 30
            assert float(c.cls[int(cl["saturated_neg"][k]), k % c.C]) == x and lab[int(cl["saturated_neg"][k])] == c.C
    if name == "flat":
        sc = c.scales[c.geo["lvl"]]
        assert all((c.reg_u[r] <= 0).all() and o["labels"][r] < c.C for r in cl["neg"])
        assert all((c.reg_u[r] == 1e4).all() and o["labels"][r] < c.C for r in cl["big"])
        assert all(c.p2g[c.geo["img"][r], c.geo["pt"][r]] == 0 and not o["targets"][r].any() and o["labels"][r] < c.C for r in cl["ignore"])
        k = cl["flat_gt"]
        assert c.gt_boxes[k, 0] == c.gt_boxes[k, 2] and c.gt_boxes[k, 3] > c.gt_boxes[k, 1]
        n = int(torch.searchsorted(c.gt_off.long(), torch.tensor(k), right=True)) - 1
        assert int(((c.p2g[n] - 1 + c.gt_off[n]) == k).sum()) > 0                          # used by a positive row
        assert cl["both"] in cl["neg"] and cl["both"] in cl["ignore"] and float(sc.min()) > 0
        assert float(w_pos[[pos.tolist().index(r) for r in cl["neg"] + cl["big"] + cl["ignore"]]].min()) > 0
    if name == "ties":
        assert (c.scales == 1).all() and (c.gt_boxes == c.gt_boxes.round()).all()
        inside = (o["targets"][pos] >= 0).all(1)
        assert inside.float().mean() > 0.5
        eq = torch.equal(c.reg_u[pos][inside][1:].double(), o["targets"][pos][inside][1:])
        assert eq and pos[0] == 0 and float(o["margin"][inside][1:].max()) == 0.0
        # row 0: union == eps exactly, in fp64 as in fp32
        e = HR.f32(1e-6)
        for dt in (torch.float32, torch.float64):
            cx = torch.zeros(1, dtype=dt)
            p = HR.tblr_decode(cx, cx, torch.full((1,), 32.0, dtype=dt), c.reg_u[:1].to(dt))
            t = HR.tblr_decode(cx, cx, torch.full((1,), 32.0, dtype=dt), HC.fp32_targets(c)[:1].to(dt))
            inter, ap, ag = HR._overlap(p, t)
            assert float(ap + ag - inter) == e and float(inter) == 0.0 and float(ag) == 0.0
    if name == "noweight":
        assert P > 0 and float(w_pos.abs().sum()) == 0.0
    if name == "nopos":
        assert P == 0 and c.gt_boxes.shape[0] > 0 and (o["labels"] == c.C).all()
    if name == "emptyimage":
        n = cl["empty"]
        assert c.gt_off[n + 1] == c.gt_off[n] and (c.p2g[n] > -1).any() and (o["labels"][c.geo["img"] == n] == c.C).all()
        assert (c.geo["img"][pos] != n).all() and P > 0
    if name == "engine_small":
        assert P < HC.get("engine").claims["P"]
