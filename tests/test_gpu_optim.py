"""Optimizer choices of the fused step on the GPU: the run-table AdamW, SGD and the gradient-accumulation kernel against
torch's optimizers in fp64 (judged per run), and the runtime / harness paths built on them -- parameter groups, accumulated
steps (eager, taped, with mmcv's remainder rule), learning-rate policies and an exact resume."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    from radet_amd import kernels
    return kernels


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


# ---------------------------------------------------------------------- kernels against torch in fp64
# case A: boundaries inside a 16-byte group, one-element runs, a scalar tail (1003 = 250 * 4 + 3); pairwise different
# multipliers with lr_mult = 0 and decay_mult = 0 among them
RUNS_A = [(0, 1, 0.0, 1.0), (1, 2, 2.0, 0.0), (2, 7, 0.5, 0.5), (7, 8, 1.5, 2.0), (8, 520, 1.0, 1.0), (520, 1003, 0.1, 3.0)]


def runs_b():
    """case B: 300 random runs over 100003 elements (98 blocks; more than one trip of a wave's span holds a boundary)"""
    rng = np.random.RandomState(5)
    n = 100003
    cuts = [0] + sorted(rng.choice(np.arange(1, n), 299, replace=False).tolist()) + [n]
    mult = rng.uniform(0.0, 2.0, size=(300, 2))
    return [(cuts[i], cuts[i + 1], float(mult[i, 0]), float(mult[i, 1])) for i in range(300)]


CASES = {"A": (1003, RUNS_A), "B": (100003, runs_b()), "C": (100003, [(0, 100003, 1.0, 1.0)])}


def device_table(runs):
    from radet_amd.runtime import OPT_RUN_DTYPE, check_opt_runs
    arr = np.array(runs, dtype=OPT_RUN_DTYPE)
    check_opt_runs(arr, runs[-1][1])
    return torch.from_numpy(arr.view(np.uint8).copy()).to(DEV)


def fp64_groups(p0, runs, lr, wd):
    """one fp64 Parameter per run, in a param_group with the run's lr and weight_decay"""
    ps = [torch.nn.Parameter(p0[b:e].clone().double()) for b, e, _, _ in runs]
    return ps, [dict(params=[p], lr=lr * lm, weight_decay=wd * dm) for p, (_, _, lm, dm) in zip(ps, runs)]


def three_steps(n, ps, opt, launch, gn, seed=9):
    """three steps with the clip (max_norm 35) active in the second: gradients of scale 0.05, 3.0, 0.05 as in
    test_gpu_kernels.py::test_adamw_clip_step.  launch(step, gradient on the device) runs the kernel under test."""
    g = torch.Generator().manual_seed(seed + 1)
    for step in range(1, 4):
        gr = torch.randn(n, generator=g) * (3.0 if step == 2 else 0.05)
        o = 0
        for p in ps:
            p.grad = gr[o:o + p.numel()].clone().double()
            o += p.numel()
        tn = torch.nn.utils.clip_grad_norm_(ps, 35.0)
        assert (tn > 35.0) == (step == 2)
        opt.step()
        launch(step, gr.to(DEV))
        assert abs(gn.item() - tn.item()) <= 1e-5 * tn.item()


def assert_per_run(p, ps, runs, what):
    """rel_err < 1e-6 (the bound of test_adamw_clip_step) on EACH run's slice: one wrong element of a one-element run
    does not hide behind the other runs"""
    errs = [rel_err(p[b:e], q.detach()) for (b, e, _, _), q in zip(runs, ps)]
    worst = int(np.argmax(errs))
    print(f"{what}: worst run {runs[worst][:2]} rel_err {errs[worst]:.3e}")
    assert errs[worst] < 1e-6, (what, runs[worst], errs[worst])


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_adamw_step_runs_equals_torch_param_groups(K, case):
    n, runs = CASES[case]
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(9))
    ps, groups = fp64_groups(p0, runs, 4e-4, 0.05)
    opt = torch.optim.AdamW(groups, lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    table = device_table(runs)
    p, m, v = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    parts, gn = torch.zeros(256, device=DEV), torch.zeros(1, device=DEV)
    plain = [p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)] if case == "C" else None

    def launch(step, gd):
        K.sqnorm_partials(gd, n, parts)
        K.adamw_step_runs(p, gd, m, v, n, 4e-4, (0.9, 0.999), 1e-8, 0.05, step, 35.0, 1.0, parts, gn, table, len(runs))
        if plain is not None:                      # a single run (0, n, 1, 1) is radet_adamw_step bit for bit
            K.adamw_step(plain[0], gd, plain[1], plain[2], n, 4e-4, (0.9, 0.999), 1e-8, 0.05, step, 35.0, 1.0, parts, gn)
            assert all(torch.equal(a, b) for a, b in zip((p, m, v), plain))
    three_steps(n, ps, opt, launch, gn)
    assert_per_run(p, ps, runs, f"adamw_step_runs {case}")
    if case == "A":                                # lr_mult = 0: p untouched, m and v still updated
        assert p[0].item() == p0[0].item() and m[0].item() != 0 and v[0].item() != 0
        assert abs(m[0].item() - opt.state[ps[0]]["exp_avg"].item()) < 1e-6 * abs(m[0].item())


SGD_MODES = [(0.0, 0.0, False), (0.9, 0.0, False), (0.9, 0.1, False), (0.9, 0.0, True)]


@pytest.mark.parametrize("with_table", [True, False], ids=["table", "notable"])
@pytest.mark.parametrize("mode", SGD_MODES, ids=["plain", "momentum", "dampening", "nesterov"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_sgd_step_equals_torch(K, case, mode, with_table):
    momentum, dampening, nesterov = mode
    n, runs = CASES[case]
    ref_runs = runs if with_table else [(0, n, 1.0, 1.0)]
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(9))
    ps, groups = fp64_groups(p0, ref_runs, 0.01, 1e-4)
    opt = torch.optim.SGD(groups, lr=0.01, momentum=momentum, dampening=dampening, nesterov=nesterov, weight_decay=1e-4)
    table = device_table(runs) if with_table else None
    p, buf = p0.clone().to(DEV), torch.zeros(n, device=DEV) if momentum else None
    parts, gn = torch.zeros(256, device=DEV), torch.zeros(1, device=DEV)

    def launch(step, gd):
        K.sqnorm_partials(gd, n, parts)
        K.sgd_step(p, gd, buf, n, 0.01, momentum, dampening, 1e-4, nesterov, step, 35.0, 1.0, parts, gn, table,
                   len(runs) if with_table else 0)
    three_steps(n, ps, opt, launch, gn)
    assert_per_run(p, ps, ref_runs, f"sgd_step {case} {mode}")
    if momentum:
        bufs = [opt.state[q]["momentum_buffer"] for q in ps]
        assert_per_run(buf, bufs, ref_runs, f"sgd_step momentum_buffer {case} {mode}")


def test_optimizer_argument_checks(K):
    """RADET_ERR_ARG (RadetHipError) before anything is launched"""
    from radet_amd import _lib
    n = 64
    t = [torch.zeros(n, device=DEV) for _ in range(4)]
    parts, gn = torch.zeros(256, device=DEV), torch.zeros(1, device=DEV)
    table = device_table([(0, n, 1.0, 1.0)])

    def adamw(n=n, step=1, grad_div=1.0, runs=table, nruns=1):
        K.adamw_step_runs(*t, n, 1e-3, (0.9, 0.999), 1e-8, 0.0, step, 0.0, grad_div, parts, gn, runs, nruns)

    def sgd(n=n, step=1, grad_div=1.0, runs=None, nruns=0, momentum=0.9, dampening=0.0, nesterov=False, buf=t[2]):
        K.sgd_step(t[0], t[1], buf, n, 1e-3, momentum, dampening, 0.0, nesterov, step, 0.0, grad_div, parts, gn, runs, nruns)
    adamw()
    sgd()
    sgd(runs=table, nruns=1)
    for bad in (dict(nruns=0), dict(nruns=K.OPT_MAX_RUNS + 1), dict(runs=None), dict(n=2 ** 32), dict(step=0), dict(grad_div=0.0)):
        with pytest.raises(_lib.RadetHipError):
            adamw(**bad)
    for bad in (dict(nruns=1), dict(runs=table, nruns=0), dict(runs=table, nruns=K.OPT_MAX_RUNS + 1), dict(n=2 ** 32), dict(step=0),
                dict(grad_div=-1.0), dict(nesterov=True, dampening=0.1), dict(nesterov=True, momentum=0.0), dict(buf=None)):
        with pytest.raises(_lib.RadetHipError):
            sgd(**bad)
    with pytest.raises(_lib.RadetHipError):
        K.grad_accumulate(t[0], t[1], n, 3)
    with pytest.raises(_lib.RadetHipError):
        K.grad_accumulate(t[0], t[1], n, -1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1003, 100003])
def test_grad_accumulate_is_torchs_fp32_add(K, n):
    g = torch.Generator().manual_seed(3)
    a0, b0 = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    acc, grad = torch.full((n,), 7.0, device=DEV), b0.clone()
    K.grad_accumulate(acc, grad, n, K.GRAD_ACC_SET)
    assert torch.equal(acc, b0) and torch.equal(grad, b0)
    acc, grad = a0.clone(), b0.clone()
    K.grad_accumulate(acc, grad, n, K.GRAD_ACC_ADD)
    assert torch.equal(acc, a0 + b0) and torch.equal(grad, b0)
    acc, grad = a0.clone(), b0.clone()
    K.grad_accumulate(acc, grad, n, K.GRAD_ACC_RESTORE)
    assert torch.equal(grad, a0 + b0) and torch.equal(acc, a0)


# ---------------------------------------------------------------------- runtime
def make_det():
    from oracle import synth
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    d = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    synth.fill_state_dict(d.state_dict(), seed=0)
    return d.cuda().train()


def targets(golden, tags=("g8", "g3")):
    a = golden("assigner")
    return ([torch.from_numpy(a[t + "_boxes"]) for t in tags], [torch.from_numpy(a[t + "_labels"]) for t in tags],
            [torch.from_numpy(a[t + "_p2g"].astype(np.int64)) for t in tags], [torch.from_numpy(a[t + "_w"]) for t in tags])


@pytest.fixture(scope="module")
def two_batches(golden):
    """batches A and B: different images, the two golden target sets in either order"""
    from oracle import synth
    return [dict(img=synth.synth_images(s, 2).cuda(), tg=targets(golden, tags)) for s, tags in ((0, ("g8", "g3")), (1, ("g3", "g8")))]


PARAMWISE = dict(norm_decay_mult=0.0, custom_keys={"backbone": dict(lr_mult=0.1, decay_mult=0.5)})


def test_sgd_train_step_with_groups_matches_autograd(two_batches):
    """runtime.train_step with SGD(momentum 0.9) + norm_decay_mult = 0 + a custom key on the backbone == the autograd path +
    torch.optim.SGD with the same groups on a clone; pattern and tolerances of
    test_gpu_model.py::test_native_train_step_matches_autograd"""
    from oracle import synth
    from radet_amd.apis import resolve_paramwise
    img, (gt_b, gt_l, p2g, pw) = two_batches[0]["img"], two_batches[0]["tg"]
    a, b = make_det(), make_det()
    lr, wd = 1e-3, 1e-4
    mult = resolve_paramwise(a, PARAMWISE)
    named = dict(a.named_parameters())
    opt = torch.optim.SGD([dict(params=[named[n]], lr=lr * lm, weight_decay=wd * dm) for n, (lm, dm) in mult.items()],
                          lr=lr, momentum=0.9, weight_decay=wd)
    rt = b.runtime()
    rt.init_optimizer(type="SGD", lr=lr, momentum=0.9, weight_decay=wd, max_norm=35.0, groups=resolve_paramwise(b, PARAMWISE))
    assert rt.opt_state["nruns"] == 18 and rt.opt_state["buf"] is not None and "m" not in rt.opt_state
    tg = rt.pack_targets(gt_b, gt_l, p2g, pw)
    for it in range(3):
        opt.zero_grad()
        losses = a(img=img, img_metas=synth.img_metas(2), return_loss=True, gt_bboxes=gt_b, gt_labels=gt_l,
                   points_to_gt_index=p2g, points_weight=pw)
        sum(losses.values()).backward()
        torch.nn.utils.clip_grad_norm_([p for p in a.parameters() if p.requires_grad], 35.0)
        opt.step()
        lb = rt.train_step(img, tg)
        assert np.allclose(lb.cpu().numpy(), [losses[k].item() for k in ("loss_cls", "loss_bbox", "loss_iou")],
                           rtol=1e-6 if it == 0 else 2e-3)
        if it == 0:
            pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
            for n in pa:
                d = (pa[n].detach() - pb[n].detach()).abs().max().item()
                assert d <= 1e-6, (n, d)
    assert rt.step_count == 3


def manual_micro(rt, batch):
    """forward / loss / backward of one batch, as train_step issues them; returns nothing: the gradients are in the arena"""
    rt.forward(batch["img"])
    rt.loss(batch["packed"], grad_scale=rt.loss_weights)
    rt.backward()


def state_of(rt):
    st = rt.opt_state
    torch.cuda.synchronize()
    return [rt.flat.params.clone(), st["grad_norm"].clone()] + [st[k].clone() for k in ("m", "v", "buf") if st.get(k) is not None]


def assert_same_state(a, b, what):
    for i, (x, y) in enumerate(zip(state_of(a), state_of(b))):
        assert torch.equal(x, y), (what, i, float((x - y).abs().max()))


def test_accumulated_steps_equal_the_manual_chain(two_batches):
    """k = 2 and k = 3 against forward / loss / backward per batch, the gradients summed by torch in the order
    (g0 + g1) + g2, and one optimizer_step(grad_div = k): parameters, AdamW moments and grad_norm bit-equal"""
    from radet_amd.apis import resolve_paramwise
    a, b = make_det(), make_det()
    ra, rb = a.runtime(), b.runtime()
    rb.tape_mode = "0"
    for rt, d in ((ra, a), (rb, b)):
        rt.init_optimizer(max_norm=35.0, groups=resolve_paramwise(d, dict(norm_decay_mult=0.0)))
        rt.set_loss_from_head(d.bbox_head)
    assert ra.opt_state["runs"] is not None
    bs = [dict(x, packed=ra.pack_targets(*x["tg"])) for x in two_batches]
    for k, order in ((2, (0, 1)), (3, (1, 0, 1))):
        for j, i in enumerate(order):
            ra.train_step(bs[i]["img"], bs[i]["packed"], lr=3e-4, accumulate=(j, k))
            assert ra.step_count == (1 if k == 2 else 2) - (j < k - 1)
        total = None
        for i in order:
            manual_micro(rb, bs[i])
            total = rb.flat.grads.clone() if total is None else total + rb.flat.grads
        rb.flat.grads.copy_(total)
        rb.optimizer_step(lr=3e-4, grad_div=float(k))
        assert_same_state(ra, rb, f"k={k}")
    assert float(ra.opt_state["grad_norm"]) > 0


def test_taped_accumulation_equals_eager(two_batches):
    """3 * (tape_after + 2) micro-steps at k = 3: every phase's tape is recorded and replayed, bit-identical to RADET_TAPE=0"""
    a, b = make_det(), make_det()
    ra, rb = a.runtime(), b.runtime()
    rb.tape_mode = "0"
    assert ra.tape_mode != "0"
    for rt, d in ((ra, a), (rb, b)):
        rt.init_optimizer(max_norm=35.0)
        rt.set_loss_from_head(d.bbox_head)
    bs = [dict(x, packed=ra.pack_targets(*x["tg"])) for x in two_batches]
    steps = 3 * (ra.tape_after + 2)
    for s in range(steps):
        x = bs[s % 2]
        la = ra.train_step(x["img"], x["packed"], lr=3e-4 * (1 + s), accumulate=(s % 3, 3)).clone()
        lb = rb.train_step(x["img"], x["packed"], lr=3e-4 * (1 + s), accumulate=(s % 3, 3)).clone()
        assert torch.equal(la, lb), s
    assert_same_state(ra, rb, "taped vs eager")
    assert ra.step_count == rb.step_count == steps // 3
    for phase in ("first", "middle", "last"):
        st = ra.tape_stats(phase)
        assert st is not None and st["replays"] >= 1, (phase, st, ra._slot(phase)["failed"])
        assert rb.tape_stats(phase) is None
    assert ra.tape_stats() is None                 # no plain step was taken


def test_default_step_issues_todays_optimizer_calls(two_batches):
    """no table, no accumulation: the recorded tape's optimizer calls are radet_sqnorm_partials + radet_adamw_step"""
    from radet_amd import _lib
    d = make_det()
    rt = d.runtime()
    with pytest.raises(NotImplementedError, match="Adam"):
        rt.init_optimizer(type="Adam")
    with pytest.raises(ValueError, match="Nesterov"):
        rt.init_optimizer(type="SGD", nesterov=True)
    rt.init_optimizer()
    assert rt.opt_state["runs"] is None and rt.opt_state["nruns"] == 0
    assert {"m", "v", "lr", "betas", "eps", "wd", "max_norm", "partials", "grad_norm"} <= set(rt.opt_state)
    tg = rt.pack_targets(*two_batches[0]["tg"])
    for _ in range(rt.tape_after + 2):             # (the first call builds the engine's plan: its key is another one)
        rt.train_step(two_batches[0]["img"], tg)
    tape = rt._tape["tape"]
    assert tape is not None, rt._tape["failed"]
    lib = _lib.load()
    index = {n: lib.radet_tape_fn_index(n.encode()) for n in ("radet_sqnorm_partials", "radet_adamw_step", "radet_adamw_step_runs",
                                                             "radet_sgd_step", "radet_grad_accumulate")}
    assert all(i >= 0 for i in index.values()), index
    name = {i: n for n, i in index.items()}
    assert [name[o[1]] for o in tape._ops if o[0] == 0 and o[1] in name] == ["radet_sqnorm_partials", "radet_adamw_step"]
    marks = {tag: [(tape._ops[i][1], j) for i, j, _ in sites] for tag, sites in tape._marks.items()}
    assert marks == {"lr": [(index["radet_adamw_step"], 5)], "step": [(index["radet_adamw_step"], 10)]}


# ---------------------------------------------------------------------- harness
def harness_cfg(max_iters):
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    cfg.merge_from_dict({
        "optimizer": dict(_delete_=True, type="SGD", lr=2e-3, momentum=0.9, weight_decay=1e-4, paramwise_cfg=PARAMWISE),
        "lr_config": dict(_delete_=True, policy="step", by_epoch=False, step=[4], gamma=0.5, warmup="linear", warmup_iters=3,
                          warmup_ratio=0.25),
        "optimizer_config": dict(type="GradientCumulativeOptimizerHook", cumulative_iters=2),
        "checkpoint_config.interval": 4, "log_config.interval": 1, "runner.max_iters": max_iters})
    return cfg


def harness_batches(two_batches, n):
    return [dict(img=two_batches[i % 2]["img"], gt_bboxes=two_batches[i % 2]["tg"][0], gt_labels=two_batches[i % 2]["tg"][1],
                 points_to_gt_index=two_batches[i % 2]["tg"][2], points_weight=two_batches[i % 2]["tg"][3]) for i in range(n)]


def test_harness_sgd_schedule_accumulation_and_exact_resume(two_batches, tmp_path):
    from radet_amd.apis import IterLR, train_detector
    cfg = harness_cfg(6)
    batches = harness_batches(two_batches, 6)
    path = str(tmp_path / "iter_{iter}.pth")
    full, lines = make_det(), []
    hist = train_detector(full, batches, cfg, log=lines.append, checkpoint_path=path)
    sched = IterLR("step", 2e-3, 6, step=[4], gamma=0.5, warmup="linear", warmup_iters=3, warmup_ratio=0.25)
    expect = [2e-3 * 0.25, 2e-3 * 0.5, 2e-3 * 0.75, 2e-3, 1e-3, 1e-3]                # by hand: warm-up 0..2, one decay at 4
    assert [sched.get_lr(i) for i in range(6)] == pytest.approx(expect)
    assert len(hist) == 6 and len(lines) == 6
    assert [re.search(r"lr: (\S+),", ln).group(1) for ln in lines] == [f"{v:.3e}" for v in expect]
    rt = full.runtime()
    assert rt.step_count == 3 and rt.opt_state["type"] == "SGD" and os.path.exists(path.format(iter=4))
    osd = torch.load(path.format(iter=4), map_location="cpu")["optimizer"]
    # one group per distinct (lr, weight_decay): base (the frozen parameters' too), the backbone's key, the norm layers
    assert [(round(g["lr"] / 2e-3, 6), round(g["weight_decay"] / 1e-4, 6)) for g in osd["param_groups"]] == \
        [(1.0, 1.0), (0.1, 0.5), (1.0, 0.0)] and osd["step_count"] == 2
    assert sum(len(g["params"]) for g in osd["param_groups"]) == len(list(full.parameters()))
    assert all(g["momentum"] == 0.9 and g["nesterov"] is False for g in osd["param_groups"])
    assert all("momentum_buffer" in s for s in osd["state"].values()) and len(osd["state"]) == len(rt.flat.train_names)
    resumed, lines2 = make_det(), []
    train_detector(resumed, batches[4:], cfg, log=lines2.append, resume_from=path.format(iter=4))
    assert [re.search(r"Iter \[(\d+)/6\]", ln).group(1) for ln in lines2] == ["5", "6"]
    assert_same_state(rt, resumed.runtime(), "resume at 4")
    assert resumed.runtime().step_count == 3
    for (k, x), y in zip(full.state_dict().items(), resumed.state_dict().values()):
        assert torch.equal(x, y), k


def test_harness_remainder_rule_equals_the_manual_chain(two_batches):
    """5 iterations at cumulative_iters = 2: two steps of two and one step of the single trailing iteration, divided by 1"""
    from radet_amd.apis import train_detector
    from radet_amd.apis.train import build_lr_schedule, optimizer_kwargs
    cfg = harness_cfg(5)
    batches = harness_batches(two_batches, 5)
    a, b = make_det(), make_det()
    train_detector(a, batches, cfg, log=lambda *_: None)
    rb = b.runtime()
    rb.tape_mode = "0"
    kw, groups = optimizer_kwargs(b, cfg)
    rb.init_optimizer(**kw)
    rb.set_loss_from_head(b.bbox_head)
    sched = build_lr_schedule(cfg.lr_config, kw["lr"], 5, scaled_lr=True)
    total = None
    for it, (last, count) in enumerate([(False, 2), (True, 2), (False, 2), (True, 2), (True, 1)]):
        x = batches[it]
        manual_micro(rb, dict(img=x["img"], packed=rb.pack_targets(x["gt_bboxes"], x["gt_labels"], x["points_to_gt_index"], x["points_weight"])))
        total = rb.flat.grads.clone() if total is None else total + rb.flat.grads
        if last:
            rb.flat.grads.copy_(total)
            rb.optimizer_step(lr=sched.get_lr(it), grad_div=float(count))
            total = None
    assert a.runtime().step_count == rb.step_count == 3
    assert_same_state(a.runtime(), rb, "remainder")
