"""radet_head_loss (csrc/loss.hip) against the fp64 run of the plain restatement tests/_head_loss_ref.py, on the cases of
tests/_head_loss_cases.py: geometries beyond the golden one (1 and 8 levels, 1 x 1 levels, R from 6 to 264000, P from 0 to
3000), the engine's padded and aliased output layout, a reused workspace, every box-loss kind with and without postact,
gamma / alpha / loss weight / grad_scale off their defaults, saturated logits, degenerate boxes, exact ties and zero
weights; and radet_scale_relu.

Integers (labels, positive list, P) and the TBLR targets are compared bit for bit (the targets with the restatement's fp32
run: the same two divisions).  Every float output is compared per group -- dcls on positive and on background rows, dreg
and diou on positive rows (exactly 0 elsewhere), dscales per level, each loss -- by max |got - ref64| / max |ref64| over the
group, against max(4 x e32, 2e-6), e32 being the same statistic of the restatement's fp32 run on the host: 4 x is the
margin test_gpu_boxloss.py::judge grants an fp32 implementation over the reference's own fp32 deviation, the floor covers
groups where the fp32 restatement happens to be exact.  Positive rows with a branch margin under 1e-4 (at most 2 % of a
case's, tests/test_head_loss_ref_cpu.py) are left out of the dreg group and subtracted from both sides of dscales.
Under postact (scales = 1, as the C header asks) dscales is held against the derivative w.r.t. a unit scale in front of
bbox_pred, the per-level sum of the reference's dreg * bbox_pred."""
import types

import pytest
import torch

import _head_loss_cases as HC
import _head_loss_ref as HR

pytestmark = pytest.mark.gpu

FLOOR, FACTOR = 2e-6, 4.0
SENTINEL = -777.25
DIRTY_WS = 0x7F7F7F7F
CLS_PAD = 32


@pytest.fixture(scope="module")
def K():
    from radet_amd import kernels
    return kernels


def bits(t):
    return t.contiguous().view(torch.int32)


def ldesc(K, levels):
    import ctypes as C
    flat = [int(x) for lv in levels for x in lv]
    return (C.c_int * len(flat))(*flat), len(levels)


def make_bufs(K, c, layout, fill):
    """fill: a float for every output cell (the workspace gets 0), or 'dirty': NaN outputs and a workspace of 0x7f7f7f7f"""
    dev, R, nl = "cuda", c.R, len(c.levels)
    val = float("nan") if fill == "dirty" else fill
    new = lambda *s: torch.empty(*s, device=dev).fill_(val)   # noqa: E731
    b = dict(layout=layout, losses=new(3), dsc=new(nl), labels=torch.full((R,), -5, dtype=torch.long, device=dev), tgt=new(R, 4),
             ws=torch.full((K.head_loss_ws_ints(R),), DIRTY_WS if fill == "dirty" else 0, dtype=torch.int32, device=dev))
    if layout == "engine":
        b.update(dcls=new(R, CLS_PAD), dri=new(R, 16))
    else:
        b.update(dcls=new(R, c.C), dreg=new(R, 4), diou=new(R))
    return b


def launch(K, c, hp, layout="packed", fill=0.0, bufs=None):
    """one radet_head_loss call on case c; returns what it wrote (device tensors; dcls / dreg / diou as [R, C] / [R, 4] / [R] views
    of the buffers it was given)"""
    dev = "cuda"
    b = bufs or make_bufs(K, c, layout, fill)
    reg, scales = HC.postact_inputs(c) if hp["postact"] else (c.reg_u, c.scales)
    ld, nl = ldesc(K, c.levels)
    gs = None if hp["grad_scale"] is None else torch.tensor(hp["grad_scale"], device=dev)
    ins = [t.to(dev).contiguous() for t in (c.cls, reg, c.iou, scales, c.gt_boxes, c.gt_labels, c.gt_off, c.p2g, c.pw)]
    if ins[4].numel() == 0:                                   # no ground truth at all: still a valid pointer
        ins[4], ins[5] = torch.zeros(1, 4, device=dev), torch.zeros(1, dtype=torch.long, device=dev)
    if b["layout"] == "engine":
        dcls, dcls_ld, dreg, dreg_ld, diou, diou_ld = b["dcls"], CLS_PAD, b["dri"], 16, b["dri"].view(-1)[4:], 16
    else:
        dcls, dcls_ld, dreg, dreg_ld, diou, diou_ld = b["dcls"], c.C, b["dreg"], 4, b["diou"], 1
    K.head_loss(*ins, ld, nl, c.B, c.C, hp["alpha"], hp["gamma"], hp["lbw"], hp["eps"], gs, b["losses"], dcls, dcls_ld, dreg,
                dreg_ld, diou, diou_ld, b["dsc"], b["ws"], b["labels"], b["tgt"], flags=K.head_loss_flags(hp["kind"], hp["postact"]))
    torch.cuda.synchronize()
    o = dict(bufs=b, losses=b["losses"], dsc=b["dsc"], labels=b["labels"], tgt=b["tgt"], ws=b["ws"], P=int(b["ws"][0]))
    if b["layout"] == "engine":
        o.update(dcls=b["dcls"][:, :c.C], dreg=b["dri"][:, :4], diou=b["dri"][:, 4])
    else:
        o.update(dcls=b["dcls"], dreg=b["dreg"], diou=b["diou"])
    o["pos"] = b["ws"][16:16 + max(o["P"], 0)].long().cpu() if 0 <= o["P"] <= c.R else None
    return o


def stat(got, ref, scale=0.0):
    got, ref = got.double().cpu().reshape(-1), ref.double().reshape(-1)
    if ref.numel() == 0:
        return 0.0
    top = max(float(ref.abs().max()), scale)
    d = float((got - ref).abs().max())
    return d / top if top > 0 else (0.0 if d == 0 else float("inf"))


def without_rows(dsc, dreg, c, hp, rows):
    """dscales minus the share of `rows`: a row adds sum(dreg * reg_u) / scale[level] to its level (under postact: of the
    reg and the unit scales the kernel was given)"""
    out = dsc.double().cpu().clone()
    if rows.numel():
        reg, scales = HC.postact_inputs(c) if hp["postact"] else (c.reg_u, c.scales)
        lv = c.geo["lvl"][rows]
        out.index_add_(0, lv, -(dreg.double().cpu()[rows] * reg[rows].double()).sum(1) / scales[lv].double())
    return out


def unit_scale_grad(dreg, c, pos):
    """postact: reg_u is bbox_pred and the header asks for scales = 1, which the kernel still multiplies in, so what it writes
    to dscales is the derivative w.r.t. a unit scale in front of bbox_pred: per level the sum of dreg * bbox_pred"""
    reg, _ = HC.postact_inputs(c)
    out = torch.zeros(len(c.levels), dtype=torch.float64)
    out.index_add_(0, c.geo["lvl"][pos], (dreg.double().cpu()[pos] * reg[pos].double()).sum(1))
    return out


def groups(o, ref64, c, hp, exclude):
    """name -> (values, reference values, least denominator) per group, for the kernel's output or the fp32 restatement's
    alike.  A level's dscales with the left-out rows subtracted keeps the whole level's |dscales| as its least denominator:
    where every positive row of a level is left out, what remains is the rounding residue of that subtraction.  Under postact
    the restatement has no scales; the reference for dscales is unit_scale_grad of its dreg."""
    pos = ref64["pos"]
    bg = torch.ones(c.R, dtype=torch.bool)
    bg[pos] = False
    near = ref64["margin"] < HR.MARGIN_MIN if exclude else torch.zeros(pos.numel(), dtype=torch.bool)
    keep, out_rows = pos[~near], pos[near]
    g = {f"loss{i}": (o["losses"][i:i + 1], ref64["losses"][i:i + 1], 0.0) for i in range(3)}
    g["dcls_pos"] = (o["dcls"].cpu()[pos], ref64["dcls"][pos], 0.0)
    g["dcls_bg"] = (o["dcls"].cpu()[bg], ref64["dcls"][bg], 0.0)
    g["dreg_pos"] = (o["dreg"].cpu()[keep], ref64["dreg"][keep], 0.0)
    g["diou_pos"] = (o["diou"].cpu()[pos], ref64["diou"][pos], 0.0)
    full = unit_scale_grad(ref64["dreg"], c, pos) if hp["postact"] else ref64["dscales"]
    a, b = without_rows(o["dsc"], o["dreg"], c, hp, out_rows), without_rows(full, ref64["dreg"], c, hp, out_rows)
    for l in range(len(c.levels)):
        g[f"dscale{l}"] = (a[l:l + 1], b[l:l + 1], abs(float(full[l])))
    return g


def as_output(r, c, hp):
    """a restatement's result under the kernel's output names"""
    return {**r, "dsc": unit_scale_grad(r["dreg"], c, r["pos"]) if hp["postact"] else r["dscales"]}


def judge(tag, o, c, hp, exclude=True, scale_from=None, scale_groups=()):
    """integers and targets bit for bit, every float group within max(4 x e32, 2e-6) of the fp64 restatement; prints the figures.
    scale_from: a second case whose fp64 groups give the statistic's denominator, where they are larger, for the groups whose
    names start with one of scale_groups (see test_ties); every other group keeps its own max |ref64|.  Returns the fp64
    reference and the least denominator used per group."""
    ref64, ref32 = HC.reference(c, hp, torch.float64), HC.reference(c, hp, torch.float32)
    pos = ref64["pos"]
    assert o["P"] == pos.numel() and torch.equal(o["pos"], pos), (tag, o["P"], pos.numel())
    assert torch.equal(o["labels"].cpu(), ref64["labels"]), tag
    assert torch.equal(bits(o["tgt"].cpu()), bits(ref32["targets"])), tag
    bg = torch.ones(c.R, dtype=torch.bool)
    bg[pos] = False
    assert not o["dreg"].cpu()[bg].any() and not o["diou"].cpu()[bg].any(), tag                  # exactly 0 off the positive rows
    assert all(torch.isfinite(o[k]).all() for k in ("losses", "dcls", "dreg", "diou", "dsc")), tag
    got, yard = groups(o, ref64, c, hp, exclude), groups(as_output(ref32, c, hp), ref64, c, hp, exclude)
    worst, bad, scale, used = 0.0, [], {}, {}
    if scale_from is not None:
        r = HC.reference(scale_from, hp, torch.float64)
        scale = {k: float(v[0].abs().max()) for k, v in groups(as_output(r, scale_from, hp), r, scale_from, hp, False).items()
                 if v[0].numel() and k.startswith(tuple(scale_groups))}
    for name in got:
        least = used[name] = max(got[name][2], scale.get(name, 0.0))
        s, e32 = stat(*got[name][:2], least), stat(*yard[name][:2], least)
        bound = max(FACTOR * e32, FLOOR)
        print(f"{tag:42s} {name:9s} kernel {s:9.3g}  e32 {e32:9.3g}  bound {bound:9.3g}{'   <-- over' if s > bound else ''}")
        worst = max(worst, s)
        if not s <= bound:
            bad.append((name, s, e32))
    print(f"{tag:42s} worst     {worst:9.3g}")
    assert not bad, (tag, bad)
    return ref64, used


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("name", ["tiny", "block", "many256", "many257", "long"])
def test_case_vs_fp64(K, name):
    c = HC.get(name)
    o = launch(K, c, c.hp)
    ref, _ = judge(name, o, c, c.hp)
    assert o["P"] == c.claims["P"] and torch.equal(o["pos"], o["pos"].sort().values)             # ascending
    assert int(ref["pos"].numel()) == c.claims["P"]


def test_engine_layout_vs_fp64(K):
    """dcls_ld = 32 > C, dreg / diou in one [R, 16] buffer at columns 0-3 and 4: every other column keeps its bits"""
    c = HC.get("engine")
    o = launch(K, c, c.hp, layout="engine", fill=SENTINEL)
    judge("engine", o, c, c.hp)
    b = o["bufs"]
    s = bits(torch.full((1,), SENTINEL))[0].item()
    assert (bits(b["dcls"][:, c.C:]) == s).all() and (bits(b["dri"][:, 5:]) == s).all()
    p = launch(K, c, c.hp)                                                                     # the packed layout computes the same bits
    assert all(torch.equal(bits(o[k]), bits(p[k])) for k in ("losses", "dcls", "dreg", "diou", "dsc"))


@pytest.mark.parametrize("hp", HC.eight_variants(), ids=HC.variant_id)
def test_eight_levels_variants_vs_fp64(K, hp):
    c = HC.get("eight")
    judge("eight " + HC.variant_id(hp), launch(K, c, hp), c, hp)


@pytest.mark.parametrize("hp", HC.kind_variants(), ids=HC.variant_id)
def test_many_positives_kinds_vs_fp64(K, hp):
    c = HC.get("many1500")
    judge("many1500 " + HC.variant_id(hp), launch(K, c, hp), c, hp)


# ------------------------------------------------------------------------------------------------ the edges
def test_saturated_logits(K):
    c = HC.get("saturated")
    o = launch(K, c, c.hp)
    judge("saturated", o, c, c.hp)
    rows = torch.cat([c.claims["saturated_pos"], c.claims["saturated_neg"]])
    assert torch.isfinite(o["dcls"].cpu()[rows]).all() and torch.isfinite(o["diou"].cpu()[rows]).all()


@pytest.mark.parametrize("kind", HR.KINDS)
def test_flat_boxes(K, kind):
    c = HC.get("flat")
    hp = dict(c.hp, kind=kind)
    judge("flat " + kind, launch(K, c, hp, layout="engine", fill=SENTINEL), c, hp)


@pytest.mark.parametrize("kind", ["giou", "iou", "diou"])
def test_ties(K, kind):
    """prediction == target in fp32 and in fp64: nothing is left out, the max / min ties and the union == eps row included.
    At exact equality the two one-sided derivatives of every box loss cancel (the loss is at its minimum) and DIoU's loss
    itself is 0, so dreg, dscales and loss_bbox are rounding residue around 0 in the reference too and a figure relative to
    them has nothing to stand on: the denominators of dreg and dscales, and of DIoU's loss_bbox, are those of the same case with
    the prediction moved 5 % off the target, the size of the terms that cancel; every other group keeps its own.  A tie value
    other than autograd's leaves one of those terms standing."""
    c = HC.get("ties")
    hp = dict(c.hp, kind=kind)
    o = launch(K, c, hp)
    moved = types.SimpleNamespace(**vars(c))
    moved.reg_u = c.reg_u * 1.05
    over = ("dreg_pos", "dscale") + (("loss1",) if kind == "diou" else ())
    ref, used = judge("ties " + kind, o, c, hp, exclude=False, scale_from=moved, scale_groups=over)
    own = [k for k in used if not k.startswith(over)]
    assert len(own) == (5 if kind == "diou" else 6) and all(used[k] == 0.0 for k in own)      # these keep their own max |ref64|
    assert ref["dreg"][0].abs().sum() > 0 or kind != "giou"                                   # the union == eps row has a gradient


def test_ties_ciou_identical_pairs_are_nan(K):
    """what test_gpu_boxloss.py::test_clamp_at_equality_and_ciou_identical_pairs establishes for the element kernel: 0 / 0 in
    the penalty of an identical pair, NaN as in the reference's fp32 run; the other two branches do not see the kind"""
    c = HC.get("ties")
    o, base = launch(K, c, dict(c.hp, kind="ciou")), launch(K, c, c.hp)
    assert torch.isnan(o["losses"][1]) and torch.isnan(o["dreg"]).any()
    assert torch.equal(o["losses"][[0, 2]], base["losses"][[0, 2]]) and torch.equal(o["dcls"], base["dcls"])
    assert torch.equal(o["diou"], base["diou"])


def test_no_weight(K):
    """P > 0 with every positive weight 0; P = 0 with ground truths present; an image with G = 0 and a non-negative p2g row"""
    c = HC.get("noweight")
    o = launch(K, c, c.hp, layout="engine", fill=3.0)
    ref = HC.reference(c, c.hp, torch.float64)
    assert o["P"] == c.claims["P"] > 0 and torch.equal(o["pos"], ref["pos"])
    assert float(o["losses"][1]) == 0.0 and float(o["losses"][2]) == 0.0
    assert not o["dreg"].any() and not o["diou"].any() and not o["dsc"].any()
    assert stat(o["losses"][:1], ref["losses"][:1]) <= FLOOR and stat(o["dcls"], ref["dcls"]) <= FLOOR      # over 0 + B
    c = HC.get("nopos")
    o = launch(K, c, c.hp, fill=3.0)
    ref = HC.reference(c, c.hp, torch.float64)
    assert o["P"] == 0 and (o["labels"] == c.C).all() and not o["tgt"].any()
    assert float(o["losses"][1]) == 0.0 and float(o["losses"][2]) == 0.0
    assert not o["dreg"].any() and not o["diou"].any() and not o["dsc"].any()
    assert stat(o["losses"][:1], ref["losses"][:1]) <= FLOOR and stat(o["dcls"], ref["dcls"]) <= FLOOR
    c = HC.get("emptyimage")
    o = launch(K, c, c.hp, fill=3.0)
    judge("emptyimage", o, c, c.hp)
    rows = c.geo["img"] == c.claims["empty"]
    assert (o["labels"].cpu()[rows] == c.C).all() and not o["tgt"].cpu()[rows].any()


def test_reused_workspace_and_outputs(K):
    """the engine allocates workspace and gradients once: a run on dirty buffers, and a second case on what the first left,
    equal runs on fresh zeroed buffers bit for bit; so do two runs of the same case"""
    x, y = HC.get("engine"), HC.get("engine_small")
    assert y.claims["P"] < x.claims["P"] and x.R == y.R
    keys = ("losses", "dcls", "dreg", "diou", "dsc", "labels", "tgt")

    def same(a, b):
        return all(torch.equal(bits(a[k].float()), bits(b[k].float())) for k in keys) and a["P"] == b["P"] and \
            torch.equal(a["pos"], b["pos"]) and int(a["ws"][1]) == int(b["ws"][1])

    fresh_x = launch(K, x, x.hp, layout="engine", fill=0.0)
    fresh_x = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in fresh_x.items()}
    fresh_y = launch(K, y, y.hp, layout="engine", fill=0.0)
    dirty = make_bufs(K, x, "engine", "dirty")
    ox = launch(K, x, x.hp, bufs=dirty)
    assert same(ox, fresh_x)
    oy = launch(K, y, y.hp, bufs=dirty)                      # fewer positives: the first run's rows must be gone
    assert same(oy, fresh_y)
    again = launch(K, y, y.hp, layout="engine", fill=0.0)
    assert same(again, fresh_y)
    judge("engine_small (reused buffers)", oy, y, y.hp)


def test_scale_relu(K):
    """radet_scale_relu == relu(reg_u * scale[level of row]) in fp32 on the host (one multiply, one max), bit for bit"""
    c = HC.get("eight")
    ld, nl = ldesc(K, c.levels)
    out = torch.full((c.R + 1, 4), SENTINEL, device="cuda")
    K.scale_relu(c.reg_u.cuda(), c.scales.cuda(), out, ld, nl, c.B)
    torch.cuda.synchronize()
    want = torch.relu(c.reg_u * c.scales[c.geo["lvl"]][:, None])
    assert torch.equal(bits(out[:c.R].cpu()), bits(want)) and (out[c.R] == SENTINEL).all()
    assert len(set(c.scales.tolist())) == 8 and (want == 0).any() and (want > 0).any()
