"""A plain restatement of the head loss (RADetHead.get_targets + loss, radet_head.py:173-392) on the flat level-major row
tensors that radet_head_loss takes, as ordinary torch tensor code in a caller-chosen dtype.  The gradients come from
autograd: nothing here transcribes the analytic backward of csrc/loss.hip.

tests/test_head_loss_ref_cpu.py pins it (fp32 against oracle.model.head_loss and tests/golden/head_loss.npz, the box losses
in fp64 against tests/golden/box_losses.npz); tests/test_gpu_head_loss.py holds the kernel against its fp64 run and uses
its fp32 run as the yardstick of what fp32 arithmetic costs.

Two places where it follows the kernel's documented contract and not the reference:
  * num_pos (the sum of the positive rows' weights) not greater than 0: loss_bbox = loss_iou = 0 with zero gradients for
    reg / iou / scales.  The reference returns the plain sum of the positive rows' raw predictions there (radet_head.py:279-281,
    a device for keeping the parameters in the graph), which is not 0 when zero-weight positives exist.
  * postact: reg_u is the head's bbox_pred (after Scale + ReLU), read as it is; scales are not applied (the C header asks
    for scales = 1 there) and get no gradient.
The IoU target is bbox_overlaps' I / max(U, 1e-6) whatever the kind and the loss's eps, as in the reference (the GIoU
kernel shares its loss's union instead; the same number at eps = 1e-6, which is what the tests pass for GIoU unless I = 0).

The branch margin (branch_margin) departs from the letter of the issue that asked for it, which takes every |a - b| over
8 * stride: that is kept for lengths; a union, enclosing area or IoU held against eps is taken over the larger of the two
instead (an IoU of 0.3 over 8 * 512 would fall under 1e-4 without being near anything, and an area of exactly 0 cannot
cross eps).  This leaves fewer rows out, never more.

The scalars (alpha, gamma, lbw, eps, grad_scale) are rounded to fp32 first: those are the values the kernel receives."""
import numpy as np
import torch
import torch.nn.functional as F

KINDS = ("giou", "iou", "iou_linear", "diou", "ciou")
OVERLAPS_EPS = float(np.float32(1e-6))      # bbox_overlaps' own eps
WEIGHT_FLOOR = float(np.float32(1e-12))     # iou.clamp(min=1e-12) in front of the box weight
NORMALIZER = 0.125                          # TBLRBBoxCoder(normalizer=1/8)
MARGIN_MIN = 1e-4                           # rows below it leave the dreg / dscales groups
MARGIN_CAP = 0.02                           # ... and are at most this share of a case's positive rows


def f32(x):
    return float(np.float32(x))


def row_geometry(levels, B):
    """the level-major row order: per row its level, image, point index inside the image, grid x / y and stride (int64)"""
    lvl, img, pt, ix, iy, st = [], [], [], [], [], []
    pt_off = 0
    for l, (h, w, s) in enumerate(levels):
        pix = torch.arange(h * w)
        lvl.append(torch.full((B * h * w,), l, dtype=torch.long))
        img.append(torch.arange(B).repeat_interleave(h * w))
        pt.append((pt_off + pix).repeat(B))
        ix.append((pix % w).repeat(B))
        iy.append((pix // w).repeat(B))
        st.append(torch.full((B * h * w,), s, dtype=torch.long))
        pt_off += h * w
    g = dict(lvl=torch.cat(lvl), img=torch.cat(img), pt=torch.cat(pt), ix=torch.cat(ix), iy=torch.cat(iy), stride=torch.cat(st))
    g["N"] = pt_off
    g["R"] = g["lvl"].numel()
    return g


def labels_and_targets(geo, gt_boxes, gt_labels, gt_off, p2g, C, dtype):
    """labels i64 [R] (p2g == 0 -> the image's LAST label, G == 0 -> background), the matched gt row (or -1) and the TBLR
    targets [R, 4] on anchors of half-size 4 * stride: (cy - y1) / (8 stride) / normalizer, two divisions as the coder does"""
    gt_off = gt_off.long()
    G = (gt_off[1:] - gt_off[:-1])[geo["img"]]
    g = p2g.long()[geo["img"], geo["pt"]]
    first = gt_off[:-1][geo["img"]]
    labelled = (G > 0) & (g > -1)
    lab_idx = first + torch.where(g == 0, G - 1, g - 1)
    labels = torch.full((geo["R"],), C, dtype=torch.long)
    labels[labelled] = gt_labels.long()[lab_idx[labelled]]
    matched = (G > 0) & (g > 0)
    gi = torch.where(matched, first + g - 1, torch.full_like(g, -1))
    tgt = torch.zeros(geo["R"], 4, dtype=dtype)
    gb = gt_boxes.to(dtype)[gi[matched]]
    cx = (geo["ix"] * geo["stride"]).to(dtype)[matched]
    cy = (geo["iy"] * geo["stride"]).to(dtype)[matched]
    size = (8 * geo["stride"]).to(dtype)[matched]
    tgt[matched] = torch.stack([(cy - gb[:, 1]) / size, (gb[:, 3] - cy) / size, (cx - gb[:, 0]) / size,
                                (gb[:, 2] - cx) / size], 1) / NORMALIZER
    return labels, gi, tgt


def tblr_decode(cx, cy, size, tblr):
    d = tblr * NORMALIZER
    return torch.stack([cx - d[:, 2] * size, cy - d[:, 0] * size, cx + d[:, 3] * size, cy + d[:, 1] * size], 1)


def _overlap(p, t):
    lt = torch.max(p[:, :2], t[:, :2])
    rb = torch.min(p[:, 2:], t[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]
    ap = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    ag = (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    return inter, ap, ag


def aligned_iou(p, t, eps=OVERLAPS_EPS):
    inter, ap, ag = _overlap(p, t)
    return inter / torch.max(ap + ag - inter, inter.new_tensor(eps))


def box_loss(kind, p, t, eps):
    """per-pair loss of (x1, y1, x2, y2) boxes; eps enters where csrc/box_loss.h's header says the reference puts it:
    GIoU under union and enclosing area (torch.max: a tie splits the gradient), IoU under bbox_overlaps' own 1e-6 and
    then as clamp(min=eps), DIoU / CIoU added to the union, to c^2 and to CIoU's two heights."""
    inter, ap, ag = _overlap(p, t)
    if kind == "giou":
        union = torch.max(ap + ag - inter, inter.new_tensor(eps))
        iou = inter / union
        ewh = (torch.max(p[:, 2:], t[:, 2:]) - torch.min(p[:, :2], t[:, :2])).clamp(min=0)
        enclose = torch.max(ewh[:, 0] * ewh[:, 1], inter.new_tensor(eps))
        return 1 - (iou - (enclose - union) / enclose)
    if kind in ("iou", "iou_linear"):
        iou = (inter / torch.max(ap + ag - inter, inter.new_tensor(OVERLAPS_EPS))).clamp(min=eps)
        return 1 - iou if kind == "iou_linear" else -iou.log()
    assert kind in ("diou", "ciou"), kind
    iou = inter / (ap + ag - inter + eps)
    ewh = (torch.max(p[:, 2:], t[:, 2:]) - torch.min(p[:, :2], t[:, :2])).clamp(min=0)
    c2 = ewh[:, 0] ** 2 + ewh[:, 1] ** 2 + eps
    rho2 = ((t[:, 0] + t[:, 2]) - (p[:, 0] + p[:, 2])) ** 2 / 4 + ((t[:, 1] + t[:, 3]) - (p[:, 1] + p[:, 3])) ** 2 / 4
    if kind == "diou":
        return 1 - (iou - rho2 / c2)
    w1, h1 = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1] + eps
    w2, h2 = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1] + eps
    v = (4 / np.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    return 1 - (iou - (rho2 / c2 + v ** 2 / (1 - iou + v)))


def focal(logits, labels, alpha, gamma):
    """sigmoid focal loss per (row, class), label == C is background"""
    C = logits.shape[1]
    t = F.one_hot(labels.clamp(0, C), C + 1)[:, :C].to(logits.dtype)
    p = logits.sigmoid()
    pt = (1 - p) * t + p * (1 - t)
    ce = -(t * F.logsigmoid(logits) + (1 - t) * F.logsigmoid(-logits))
    return ce * (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)


def branch_margin(kind, postact, eps, v, p, t, size):
    """per pair: the smallest |a - b| between the two sides of any comparison the loss differentiates through (max / min /
    clamp / relu), as a pure number.  Lengths (corner against corner, overlap and enclosing width / height against 0,
    scale * reg_u against 0, which is a length in strides) are taken over the anchor size 8 * stride, the scale their
    rounding errors have.  A quantity held against eps (union, enclosing area, IoU) is taken over the larger of the two:
    an area of exactly 0 is as far from eps as it can be and no rounding moves it across.  fp64, no gradient."""
    def rel(a, b):
        return (a - b).abs() / torch.maximum(a.abs(), torch.full_like(a, abs(b)))

    with torch.no_grad():
        v, p, t, size = v.double(), p.double(), t.double(), size.double()
        m = ((p - t).abs() / size[:, None]).min(1).values                                 # max / min of the corners
        lt, rb = torch.max(p[:, :2], t[:, :2]), torch.min(p[:, 2:], t[:, 2:])
        m = torch.minimum(m, ((rb - lt).abs() / size[:, None]).min(1).values)              # overlap w, h against 0
        inter, ap, ag = _overlap(p, t)
        union = ap + ag - inter
        ewh = torch.max(p[:, 2:], t[:, 2:]) - torch.min(p[:, :2], t[:, :2])
        if kind == "giou":
            m = torch.minimum(m, rel(union, eps))
            m = torch.minimum(m, rel(ewh.clamp(min=0).prod(1), eps))
        if kind in ("giou", "diou", "ciou"):
            m = torch.minimum(m, (ewh.abs() / size[:, None]).min(1).values)                # enclosing w, h against 0
        if kind in ("iou", "iou_linear"):
            m = torch.minimum(m, rel(union, OVERLAPS_EPS))
            m = torch.minimum(m, rel(inter / union.clamp(min=OVERLAPS_EPS), eps))
        if not postact:
            m = torch.minimum(m, (v.abs() * NORMALIZER).min(1).values)
        return m


def head_loss_ref(cls, reg_u, iou, scales, gt_boxes, gt_labels, gt_off, p2g, pw, levels, B, C, *, alpha=0.25, gamma=2.0,
                  lbw=2.0, eps=1e-6, kind="giou", postact=False, grad_scale=None, dtype=torch.float64):
    """cls [R, C], reg_u [R, 4], iou [R], scales [nlvl], gt_boxes [sumG, 4], gt_labels [sumG], gt_off [B + 1], p2g / pw [B, N];
    levels = [(h, w, stride), ...].  Returns a dict: losses [3], dcls, dreg, diou, dscales (gradients of sum_i grad_scale[i]
    * losses[i]), labels, targets [R, 4], pos (ascending rows), num_pos, margin (per positive row, fp64)."""
    alpha, gamma, lbw, eps = f32(alpha), f32(gamma), f32(lbw), f32(eps)
    gs = [1.0, 1.0, 1.0] if grad_scale is None else [f32(x) for x in grad_scale]
    geo = row_geometry(levels, B)
    assert cls.shape == (geo["R"], C) and reg_u.shape == (geo["R"], 4) and iou.shape == (geo["R"],) and p2g.shape == (B, geo["N"])
    cls, reg_u, iou, scales = (x.detach().to(dtype).requires_grad_(True) for x in (cls, reg_u, iou, scales))
    labels, _, tgt = labels_and_targets(geo, gt_boxes, gt_labels, gt_off, p2g, C, dtype)
    w_row = pw.to(dtype)[geo["img"], geo["pt"]]
    pos = ((labels >= 0) & (labels < C)).nonzero().reshape(-1)
    pos_w = w_row[pos]
    num_pos = pos_w.sum()
    loss_cls = (focal(cls, labels, alpha, gamma) * w_row[:, None]).sum() / (num_pos + B)
    margin = torch.zeros(pos.numel(), dtype=torch.float64)
    if pos.numel():
        cx = (geo["ix"] * geo["stride"]).to(dtype)[pos]
        cy = (geo["iy"] * geo["stride"]).to(dtype)[pos]
        size = (8 * geo["stride"]).to(dtype)[pos]
        v = reg_u[pos] if postact else reg_u[pos] * scales[geo["lvl"][pos]][:, None]
        dp = tblr_decode(cx, cy, size, v if postact else torch.relu(v))
        dt = tblr_decode(cx, cy, size, tgt[pos])
        margin = branch_margin(kind, postact, eps, v.detach(), dp.detach(), dt, size)
    if num_pos > 0:
        iou_t = aligned_iou(dp, dt).detach()
        wgt = iou_t.clamp(min=WEIGHT_FLOOR) * pos_w
        loss_bbox = lbw * (box_loss(kind, dp, dt, eps) * wgt).sum() / wgt.sum()
        loss_iou = (F.binary_cross_entropy_with_logits(iou[pos], iou_t, reduction="none") * pos_w).sum() / pos_w.sum()
    else:
        loss_bbox = loss_iou = loss_cls.new_zeros(())
    total = gs[0] * loss_cls + gs[1] * loss_bbox + gs[2] * loss_iou
    grads = torch.autograd.grad(total, (cls, reg_u, iou, scales), allow_unused=True)
    dcls, dreg, diou, dscales = (torch.zeros_like(x) if g is None else g for g, x in zip(grads, (cls, reg_u, iou, scales)))
    return dict(losses=torch.stack([loss_cls, loss_bbox, loss_iou]).detach(), dcls=dcls, dreg=dreg, diou=diou, dscales=dscales,
                labels=labels, targets=tgt, pos=pos, num_pos=num_pos.detach(), margin=margin, geo=geo)
