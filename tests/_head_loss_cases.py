"""Inputs of the head-loss parity tests (tests/test_head_loss_ref_cpu.py, tests/test_gpu_head_loss.py): every case is made
by a function here from a fixed seed, as fp32 host tensors in the layout radet_head_loss takes.

Positive rows come in clusters of neighbouring grid points, as an assigner produces them; per (level, image) a twelfth of
them are seeds, each seed gets a ground-truth box around its own point (0.7 .. 5 strides to every side) and every positive
goes to the nearest seed, so most points lie inside their box and some outside (negative TBLR targets).  The box
prediction of a positive row is its target times 0.6 .. 1.4 plus noise: IoUs spread over (0, 1), some sides cut by the ReLU."""
import functools
import types

import numpy as np
import torch

from _head_loss_ref import KINDS, f32, labels_and_targets, row_geometry

EIGHT = [(9, 7, 4), (5, 4, 8), (3, 2, 16), (2, 1, 32), (1, 1, 64), (1, 1, 128), (1, 1, 256), (1, 1, 512)]
ENGINE = [(8, 12, 8), (4, 6, 16), (2, 3, 32), (1, 2, 64), (1, 1, 128)]
MANY = [(40, 40, 8), (20, 20, 16)]
LONG = [(400, 330, 8)]
MANY_BLOCK = 5                      # rows 1280 .. 1535 all positive, blocks 4 and 6 without one
LONG_THREAD = 100                   # scan thread 100 walks row blocks 200 and 201
SATURATED = (30.0, -30.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4)
DEFAULTS = dict(alpha=0.25, gamma=2.0, lbw=2.0, eps=1e-6, kind="giou", postact=False, grad_scale=None)


def row_offsets(levels, B):
    off = [0]
    for h, w, _ in levels:
        off.append(off[-1] + B * h * w)
    return off


def generate(name, levels, B, C, seed, n_pos, forced=(), forbidden=(), zero_w=3, int_boxes=False, unit_scales=False):
    rng = np.random.RandomState(seed)
    geo = row_geometry(levels, B)
    R, N = geo["R"], geo["N"]
    lvl, img, pt, ix, iy, st = (geo[k].numpy() for k in ("lvl", "img", "pt", "ix", "iy", "stride"))
    off = row_offsets(levels, B)
    allowed = np.ones(R, bool)
    allowed[list(forbidden)] = False
    chosen = dict.fromkeys(int(r) for r in forced)                      # insertion-ordered set
    assert n_pos >= len(chosen) and n_pos <= int(allowed.sum()) + len(chosen)
    while len(chosen) < n_pos:
        c = int(rng.randint(R))
        h, w, _ = levels[lvl[c]]
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                y, x = iy[c] + dy, ix[c] + dx
                if 0 <= y < h and 0 <= x < w and len(chosen) < n_pos:
                    r = off[lvl[c]] + img[c] * h * w + y * w + x
                    if allowed[r]:
                        chosen[int(r)] = None
    pos = np.array(sorted(chosen), np.int64)
    boxes, labels, gt_off = [], [], [0]
    gidx = np.zeros(R, np.int64)
    for n in range(B):
        cnt = 0
        for l, (h, w, s) in enumerate(levels):
            rows = pos[(img[pos] == n) & (lvl[pos] == l)]
            if not len(rows):
                continue
            seeds = rng.choice(rows, max(1, -(-len(rows) // 12)), replace=False)
            for sr in seeds:
                ext = rng.randint(3, 7, 4).astype(np.float64) if int_boxes else rng.uniform(0.7, 5.0, 4)
                cx, cy = float(ix[sr] * s), float(iy[sr] * s)
                boxes.append([cx - ext[0] * s, cy - ext[1] * s, cx + ext[2] * s, cy + ext[3] * s])
                labels.append(int(rng.randint(C)))
            d = np.maximum(np.abs(ix[rows][:, None] - ix[seeds][None]), np.abs(iy[rows][:, None] - iy[seeds][None]))
            gidx[rows] = cnt + d.argmin(1) + 1
            cnt += len(seeds)
        if cnt == 0:                                                     # every image has a ground truth unless a case removes it
            boxes.append([0.0, 0.0, 8.0, 8.0])
            labels.append(int(rng.randint(C)))
            cnt = 1
        gt_off.append(gt_off[-1] + cnt)
    p2g = np.full((B, N), -1, np.int64)
    p2g[img[pos], pt[pos]] = gidx[pos]
    pw = rng.uniform(0.1, 2.0, (B, N)).astype(np.float32)
    free = np.setdiff1d(pos, np.asarray(list(forced), np.int64))
    zero_rows = rng.choice(free, min(zero_w, len(free)), replace=False) if len(free) else np.zeros(0, np.int64)
    pw[img[zero_rows], pt[zero_rows]] = 0.0
    scales = np.ones(len(levels)) if unit_scales else np.sort(rng.uniform(0.6, 1.5, len(levels)))[::-1] + 0.01 * np.arange(len(levels))
    c = types.SimpleNamespace(
        name=name, levels=list(levels), B=B, C=C, R=R, N=N, seed=seed,
        cls=torch.from_numpy((rng.randn(R, C) * 1.5 - 2.0).astype(np.float32)),
        iou=torch.from_numpy(rng.randn(R).astype(np.float32)),
        scales=torch.from_numpy(scales.astype(np.float32).copy()),
        gt_boxes=torch.from_numpy(np.asarray(boxes, np.float32).reshape(-1, 4)),
        gt_labels=torch.from_numpy(np.asarray(labels, np.int64)),
        gt_off=torch.from_numpy(np.asarray(gt_off, np.int32)),
        p2g=torch.from_numpy(p2g), pw=torch.from_numpy(pw), hp=dict(DEFAULTS), zero_rows=torch.from_numpy(np.sort(zero_rows)),
        claims={})
    reg = rng.randn(R, 4) * 1.5 + 0.5
    _, _, tgt = labels_and_targets(geo, c.gt_boxes, c.gt_labels, c.gt_off, c.p2g, C, torch.float64)
    v = tgt[pos].numpy() * rng.uniform(0.6, 1.4, (len(pos), 4)) + rng.randn(len(pos), 4) * 0.15
    reg[pos] = v / scales[lvl[pos]][:, None]
    c.reg_u = torch.from_numpy(reg.astype(np.float32))
    c.geo = geo
    return c


def fp32_targets(c):
    return labels_and_targets(c.geo, c.gt_boxes, c.gt_labels, c.gt_off, c.p2g, c.C, torch.float32)[2]


def postact_inputs(c):
    """what RADetHead.loss receives: bbox_pred = relu(scale * reg_u), one fp32 multiply and one max, and scales of 1"""
    reg = torch.relu(c.reg_u * c.scales[c.geo["lvl"]][:, None])
    return reg, torch.ones_like(c.scales)


# ------------------------------------------------------------------------------------------------ the table's cases
def tiny():
    c = generate("tiny", [(2, 3, 8)], 1, 1, seed=1, n_pos=2, zero_w=1)
    c.claims = dict(P=2, blocks=1, focal_partials=1)
    return c


def block():
    c = generate("block", [(16, 16, 8)], 1, 3, seed=2, n_pos=256, forced=range(256), zero_w=0)
    c.pw[0, torch.tensor([17, 200])] = 0.0
    c.claims = dict(P=256, blocks=1, all_positive=True)
    return c


def eight(seed=3, n_pos=100, also=(), **kw):
    B = 3
    off = row_offsets(EIGHT, B)
    forced = list(also) + [off[l] + (l % B) * h * w + (h * w) // 2 for l, (h, w, _) in enumerate(EIGHT)]
    c = generate("eight", EIGHT, B, 5, seed=seed, n_pos=n_pos, forced=forced, **kw)
    c.claims = dict(P=n_pos, levels=8, every_level_positive=True, scales_differ=True)
    return c


def many(n_pos):
    lo = MANY_BLOCK * 256
    forced = range(lo, lo + 256)
    forbidden = list(range(lo - 256, lo)) + list(range(lo + 256, lo + 512))
    c = generate(f"many{n_pos}", MANY, 2, 21, seed=10 + n_pos % 7, n_pos=n_pos, forced=forced, forbidden=forbidden,
                 zero_w=0 if n_pos < 300 else 5)
    if n_pos < 300:
        c.pw[0, torch.tensor([lo + 3, lo + 250])] = 0.0              # image 0, level 0: the point index is the row
    c.claims = dict(P=n_pos, full_block=MANY_BLOCK)
    return c


def long():
    R = 2 * 400 * 330
    b = 2 * LONG_THREAD * 256
    forced = [0, R - 1, R - 30, b + 5, b + 255, b + 256, b + 256 + 7]
    c = generate("long", LONG, 2, 1, seed=5, n_pos=3000, forced=forced, zero_w=6)
    c.claims = dict(P=3000, blocks=1032, per=2, rows=forced)
    return c


def engine(seed=6, n_pos=150, **kw):
    c = generate("engine", ENGINE, 4, 21, seed=seed, n_pos=n_pos, **kw)
    c.claims = dict(P=n_pos, cls_pad=32)
    return c


# ------------------------------------------------------------------------------------------------ the edge cases
def saturated():
    """eight with class / IoU logits of +-30, +-88, +-104, +-1e4: at the labelled class and another class of eight positive
    rows, at two classes of eight background rows, and as the IoU logit of those positive rows"""
    c = eight()
    c.name = "saturated"
    labels = labels_and_targets(c.geo, c.gt_boxes, c.gt_labels, c.gt_off, c.p2g, c.C, torch.float64)[0]
    pos = (labels < c.C).nonzero().reshape(-1)
    neg = (labels == c.C).nonzero().reshape(-1)
    rows_p, rows_n = pos[3::11][:8], neg[5::17][:8]
    assert len(rows_p) == 8 and len(rows_n) == 8
    for k, x in enumerate(SATURATED):
        r = int(rows_p[k])
        c.cls[r, labels[r]] = x
        c.cls[r, (labels[r] + 1) % c.C] = SATURATED[(k + 3) % 8]
        c.iou[r] = SATURATED[(k + 5) % 8]
        c.cls[int(rows_n[k]), k % c.C] = x
        c.cls[int(rows_n[k]), (k + 2) % c.C] = -x
    c.claims.update(saturated_pos=rows_p, saturated_neg=rows_n)
    return c


def flat():
    """engine with more positives and: two rows whose four reg_u are <= 0 (one of them with p2g == 0: zero-area prediction
    AND zero-area target), two rows of reg_u = 1e4, one ground truth with x1 == x2, two p2g == 0 rows"""
    c = engine(seed=7, n_pos=400)
    c.name = "flat"
    labels, gi, _ = labels_and_targets(c.geo, c.gt_boxes, c.gt_labels, c.gt_off, c.p2g, c.C, torch.float64)
    pos = (labels < c.C).nonzero().reshape(-1)
    live = pos[c.pw[c.geo["img"][pos], c.geo["pt"][pos]] > 0]
    r_neg, r_both, r_ign, r_big1, r_big2 = (int(x) for x in live[4::37][:5])
    c.reg_u[r_neg] = torch.tensor([-0.3, -1.0, -0.2, -2.0])
    c.reg_u[r_both] = torch.tensor([-0.5, -0.1, -3.0, -0.7])
    c.reg_u[r_big1] = 1e4
    c.reg_u[r_big2] = 1e4
    for r in (r_both, r_ign):
        c.p2g[c.geo["img"][r], c.geo["pt"][r]] = 0
    others = gi[live][~torch.isin(live, torch.tensor([r_neg, r_both, r_ign, r_big1, r_big2]))]
    used, count = others.unique(return_counts=True)
    k = int(used[count.argmin()])                                         # the ground truth that the fewest other positive rows use
    c.gt_boxes[k, 2] = c.gt_boxes[k, 0]
    c.claims.update(neg=[r_neg, r_both], big=[r_big1, r_big2], ignore=[r_both, r_ign], both=r_both, flat_gt=k)
    return c


def ties():
    """eight with integer boxes of 3 .. 6 strides to every side, scales of 1 and reg_u = the fp32 TBLR targets (which the
    kernel's bbox_targets_out equals bit for bit): prediction == target in fp32 and in fp64 wherever the point lies inside its
    box.  Row 0 (level 0, image 0, the point at the origin) is remade so that its union is exactly eps = fp32(1e-6): a
    zero-width target [0, 0, 0, 5] and a prediction of 2^-10 x (eps * 2^10) pixels."""
    c = eight(seed=8, int_boxes=True, unit_scales=True, n_pos=100, also=[0])
    c.name = "ties"
    off = row_offsets(EIGHT, 3)
    gi = labels_and_targets(c.geo, c.gt_boxes, c.gt_labels, c.gt_off, c.p2g, c.C, torch.float64)[1]
    assert int(gi[0]) >= 0 and float(c.pw[0, 0]) > 0
    c.gt_boxes[int(gi[0])] = torch.tensor([0.0, 0.0, 0.0, 5.0])
    tgt = fp32_targets(c)
    pos = (tgt.abs().sum(1) > 0) | (c.p2g[c.geo["img"], c.geo["pt"]] > 0)
    c.reg_u[pos] = tgt[pos]
    e = np.float32(1e-6)
    c.reg_u[0] = torch.tensor([0.0, float(e * np.float32(2.0 ** 8)), 0.0, 2.0 ** -12])     # stride 4: 2^-10 wide, eps * 2^10 high
    c.claims.update(union_eps_row=0, off=off)
    return c


def no_weight_all_zero():
    c = engine(seed=9, n_pos=60, zero_w=0)
    c.name = "noweight"
    labels = labels_and_targets(c.geo, c.gt_boxes, c.gt_labels, c.gt_off, c.p2g, c.C, torch.float64)[0]
    pos = (labels < c.C).nonzero().reshape(-1)
    c.pw[c.geo["img"][pos], c.geo["pt"][pos]] = 0.0
    c.claims = dict(P=60, num_pos=0.0)
    return c


def no_positive():
    c = engine(seed=9, n_pos=60)
    c.name = "nopos"
    c.p2g[:] = -1
    c.claims = dict(P=0, num_pos=0.0)
    return c


def empty_image():
    """engine; image 1 loses its ground truths (G = 0) and keeps its p2g row: background everywhere in that image"""
    c = engine(seed=11, n_pos=120)
    c.name = "emptyimage"
    a, b = int(c.gt_off[1]), int(c.gt_off[2])
    assert b > a and int((c.p2g[1] > -1).sum()) > 0
    keep = torch.ones(c.gt_boxes.shape[0], dtype=torch.bool)
    keep[a:b] = False
    c.gt_boxes, c.gt_labels = c.gt_boxes[keep].contiguous(), c.gt_labels[keep].contiguous()
    c.gt_off = c.gt_off.clone()
    c.gt_off[2:] -= b - a
    c.claims = dict(empty=1)
    return c


CASES = dict(tiny=tiny, block=block, eight=eight, many256=lambda: many(256), many257=lambda: many(257),
             many1500=lambda: many(1500), long=long, engine=engine, saturated=saturated, flat=flat, ties=ties,
             noweight=no_weight_all_zero, nopos=no_positive, emptyimage=empty_image,
             engine_small=lambda: engine(seed=12, n_pos=40))


@functools.lru_cache(maxsize=None)
def get(name):
    """the case, built once; callers do not modify it"""
    return CASES[name]()


def eight_variants():
    """all five kinds x postact, the other hyper-parameters rotating through them: gamma in {2, 1.5, 0}, alpha 0.25 / 0.4,
    lbw 2 / 1.3, grad_scale None / [0.5, 2, 3]"""
    out = []
    for i, (kind, postact) in enumerate((k, p) for k in KINDS for p in (False, True)):
        out.append(dict(kind=kind, postact=postact, gamma=(2.0, 1.5, 0.0)[i % 3], alpha=0.4 if i % 2 else 0.25,
                        lbw=1.3 if i % 3 == 1 else 2.0, eps=1e-6, grad_scale=None if i % 4 < 2 else [0.5, 2.0, 3.0]))
    return out


def kind_variants():
    return [dict(DEFAULTS, kind=k, postact=p) for k in KINDS for p in (False, True)]


def variant_id(hp):
    return "-".join([hp["kind"], "post" if hp["postact"] else "pre", f"g{hp['gamma']}", f"a{hp['alpha']}", f"w{hp['lbw']}",
                     "gs" if hp["grad_scale"] else "nogs"])


def reference(c, hp, dtype):
    """head_loss_ref on a case: under postact the kernel's input is relu(scale * reg_u) with scales of 1"""
    from _head_loss_ref import head_loss_ref
    reg, scales = postact_inputs(c) if hp["postact"] else (c.reg_u, c.scales)
    return head_loss_ref(c.cls, reg, c.iou, scales, c.gt_boxes, c.gt_labels, c.gt_off, c.p2g, c.pw, c.levels, c.B, c.C,
                         dtype=dtype, **hp)
