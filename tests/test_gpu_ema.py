"""Weight EMA on the GPU: radet_ema_update against torch's CPU `mul_().add_(alpha=)` bit for bit (odd sizes, misaligned arena
views, guard elements), radet_ema_swap, and the harness paths built on them -- the hook beside the plain, the interval-2 and
the accumulated step (eager and taped), evaluation and checkpoints that leave the trajectory alone, an exact resume and
inference on an EMA checkpoint."""
import os

import numpy as np
import pytest
import torch

from _ema_ref import MOMENTA, bits, inputs, torch_ema

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
GUARD = 64
ITERS = 8


@pytest.fixture(scope="module")
def K():
    from radet_amd import kernels
    return kernels


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


# ---------------------------------------------------------------------- kernels
def guarded(values, off):
    """a device buffer [GUARD sentinels | off pad | values | GUARD sentinels] and the view of `values` inside it: the view
    starts 4 * off bytes past a 16-byte line (torch's allocations are 512-byte aligned, GUARD * 4 is a multiple of 16)"""
    n = values.numel()
    buf = torch.full((GUARD + off + n + GUARD,), 12345.678, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + off:GUARD + off + n]
    view.copy_(values)
    return buf, view


def guards_intact(buf, off, n):
    return bool((buf[:GUARD + off] == 12345.678).all() and (buf[GUARD + off + n:] == 12345.678).all())


# same offset inside a 16-byte line: a peeled head and 16-byte accesses; different offsets: the element path
OFFSETS = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (3, 2), (2, 0)]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1023, 4099, 65541])
def test_ema_update_equals_torch_cpu_bit_for_bit(K, n):
    ema0, p0 = inputs(n, seed=100 + n)
    want = {m: torch_ema(ema0, p0, m) for m in MOMENTA}
    for oe, op in OFFSETS:
        for m in MOMENTA:
            ebuf, ema = guarded(ema0, oe)
            pbuf, p = guarded(p0, op)
            assert ema.data_ptr() % 16 == 4 * oe and p.data_ptr() % 16 == 4 * op
            K.ema_update(ema, p, n, m)
            torch.cuda.synchronize()
            got = ema.cpu()
            bad = np.flatnonzero(bits(got) != bits(want[m]))
            assert bad.size == 0, (n, oe, op, m, bad[:5], got[bad[:5]], want[m][bad[:5]])
            assert same_bits(p.cpu(), p0), (n, oe, op, m)
            assert guards_intact(ebuf, oe, n) and guards_intact(pbuf, op, n), (n, oe, op, m)


@pytest.mark.parametrize("n", [1, 5, 4099, 65541])
def test_ema_swap_is_an_exact_exchange(K, n):
    a0, b0 = inputs(n, seed=7 + n)
    for oa, ob in OFFSETS:
        abuf, a = guarded(a0, oa)
        bbuf, b = guarded(b0, ob)
        K.ema_swap(a, b, n)
        torch.cuda.synchronize()
        assert same_bits(a.cpu(), b0) and same_bits(b.cpu(), a0), (n, oa, ob)
        K.ema_swap(a, b, n)
        torch.cuda.synchronize()
        assert same_bits(a.cpu(), a0) and same_bits(b.cpu(), b0), (n, oa, ob)         # twice is the identity
        assert guards_intact(abuf, oa, n) and guards_intact(bbuf, ob, n), (n, oa, ob)


def test_ema_argument_checks(K):
    """RADET_ERR_ARG (RadetHipError) before anything is launched; n = 0 launches nothing, whatever the pointers"""
    from radet_amd import _lib
    a, b = torch.ones(16, device=DEV), torch.full((16,), 2.0, device=DEV)
    K.ema_update(None, None, 0, 0.5)
    K.ema_swap(None, None, 0)
    K.ema_update(a, b, 0, 0.5)
    for bad in ((None, b, 16), (a, None, 16), (a, a, 16), (a[:12], a[4:], 8)):
        with pytest.raises(_lib.RadetHipError):
            K.ema_update(bad[0], bad[1], bad[2], 0.5)
        with pytest.raises(_lib.RadetHipError):
            K.ema_swap(*bad)
    K.ema_swap(a[:8], a[8:], 8)                                # neighbours that touch but do not overlap
    torch.cuda.synchronize()
    assert bool((a == 1).all() and (b == 2).all())


# ---------------------------------------------------------------------- training (detector and batches as in test_gpu_optim.py)
def make_det():
    from oracle import synth
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    d = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    synth.fill_state_dict(d.state_dict(), seed=0)
    return d.cuda().train()


def targets(golden, tags):
    a = golden("assigner")
    return ([torch.from_numpy(a[t + "_boxes"]) for t in tags], [torch.from_numpy(a[t + "_labels"]) for t in tags],
            [torch.from_numpy(a[t + "_p2g"].astype(np.int64)) for t in tags], [torch.from_numpy(a[t + "_w"]) for t in tags])


@pytest.fixture(scope="module")
def batches(golden):
    """ITERS harness batches that alternate between two: different images, the two golden target sets in either order"""
    from oracle import synth
    two = []
    for s, tags in ((0, ("g8", "g3")), (1, ("g3", "g8"))):
        tg = targets(golden, tags)
        two.append(dict(img=synth.synth_images(s, 2).cuda(), gt_bboxes=tg[0], gt_labels=tg[1], points_to_gt_index=tg[2],
                        points_weight=tg[3]))
    return [two[i % 2] for i in range(ITERS)]


class _ValDataset:
    """what evaluate_during_training needs of a dataset: evaluate(); it keeps the detections it was given"""

    def __init__(self):
        self.seen = []

    def __len__(self):
        return 2

    def evaluate(self, results, device=None, **kw):
        assert kw.get("metric") == "bbox"
        self.seen.append([(b.clone(), l.clone()) for b, l in results])
        return dict(bbox_mAP=0.0)


class _ValLoader:
    """one test batch of two images, in the test-mode loader's layout"""

    def __init__(self):
        from oracle import synth
        self.dataset = _ValDataset()
        self.img = synth.synth_images(5, 2)

    def __iter__(self):
        from oracle import synth
        yield dict(img=[self.img], img_metas=[synth.img_metas(2)])


HOOKS = dict(plain=dict(type="EMAHook", momentum=0.75, warm_up=2, interval=1),
             every2=dict(type="EMAHook", momentum=0.75, warm_up=2, interval=2, priority="NORMAL"))


def harness_cfg(hook, k, every):
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    over = {"log_config.interval": 1, "runner.max_iters": ITERS, "checkpoint_config.interval": every,
            "evaluation": dict(_delete_=True, interval=every, metric="bbox")}
    if k > 1:
        over["optimizer_config"] = dict(type="GradientCumulativeOptimizerHook", cumulative_iters=k,
                                        grad_clip=dict(max_norm=35, norm_type=2))
    if hook is not None:
        over["custom_hooks"] = [dict(HOOKS[hook])]
    cfg.merge_from_dict(over)
    return cfg


def run(batches, hook=None, k=1, taped=True, every=0, ckpt_dir=None, resume_from=None, start=0):
    """train_detector over the batches (from `start` on when resuming from the file `resume_from`).  The batch generator runs
    between the iterations: it snapshots the parameter arena and the EMA arena (device clones) after every iteration; the
    first snapshot, before iteration `start`, is the state training starts from."""
    from radet_amd.apis import train_detector
    det = make_det()
    rt = det.runtime()
    rt.tape_after = 1                                           # replays within the 8 iterations (4 per phase at k = 2)
    if not taped:
        rt.tape_mode = "0"
    snaps = dict(p=[], ema=[])

    def snapshot():
        snaps["p"].append(rt.flat.params.clone())
        snaps["ema"].append(None if rt.ema_state is None else rt.ema_state["ema"].clone())

    def feed():
        for b in batches[start:]:
            snapshot()
            yield b

    loader = _ValLoader() if every else None
    path = os.path.join(ckpt_dir, "iter_{iter}.pth") if ckpt_dir else None
    lines = []
    hist = train_detector(det, feed(), harness_cfg(hook, k, every), log=lines.append, checkpoint_path=path, val_loader=loader,
                          resume_from=resume_from)
    snapshot()
    torch.cuda.synchronize()
    return dict(det=det, rt=rt, hist=hist, p0=snaps["p"][0], ema0=snaps["ema"][0], p=snaps["p"][1:], ema=snaps["ema"][1:],
                loader=loader, lines=lines, path=path)


@pytest.fixture(scope="module")
def runs(batches, tmp_path_factory):
    """the training runs of this file, each made once: name -> run()'s result"""
    made = {}
    recipes = {
        "none": dict(), "none_k2": dict(k=2),
        "plain": dict(hook="plain"), "plain_eager": dict(hook="plain", taped=False),
        "every2": dict(hook="every2"), "every2_eager": dict(hook="every2", taped=False),
        "k2": dict(hook="plain", k=2), "k2_eager": dict(hook="plain", k=2, taped=False),
    }

    def get(name):
        if name not in made:
            if name == "saved":                                 # a checkpoint and an evaluation every 2 iterations
                made[name] = run(batches, hook="plain", every=2, ckpt_dir=str(tmp_path_factory.mktemp("ema_ckpt")))
            elif name == "resumed":
                made[name] = run(batches, hook="plain", resume_from=get("saved")["path"].format(iter=4), start=4)
            else:
                made[name] = run(batches, **recipes[name])
        return made[name]
    return get


def cpu_chain(r, momentum, warm_up, interval):
    """the hook's own line on CPU tensors over the parameter snapshots: one EMA per iteration (the rule is written out here,
    not taken from the package)"""
    ema = r["p0"].cpu()
    out = []
    for it, p in enumerate(r["p"]):
        if it % interval == 0:
            m = min(momentum ** interval, (1 + it) / (warm_up + it))
            ema = torch_ema(ema, p.cpu(), m)
        out.append(ema)
    return out


@pytest.mark.parametrize("name,base,interval,phases", [("plain", "none", 1, ("plain",)), ("every2", "none", 2, ("plain",)),
                                                       ("k2", "none_k2", 1, ("first", "last"))])
def test_hook_leaves_training_alone_and_tracks_the_cpu_chain(runs, name, base, interval, phases):
    r, ref, eager = runs(name), runs(base), runs(name + "_eager")
    assert len(r["p"]) == ITERS and len(r["hist"]) == ITERS and ref["ema0"] is None
    # (a) parameters after every iteration and the logged losses: the run without the hook
    assert same_bits(r["p0"], ref["p0"]) and r["hist"] == ref["hist"]
    for it in range(ITERS):
        assert same_bits(r["p"][it], ref["p"][it]), it
    if name == "k2":                                            # micro-iterations 0, 2, 4, 6 move nothing; the EMA still updates
        assert all(same_bits(r["p"][it], r["p0"] if it == 0 else r["p"][it - 1]) for it in range(0, ITERS, 2))
        assert not same_bits(r["p"][1], r["p"][0]) and r["rt"].step_count == ITERS // 2
    # (b) the EMA arena after every iteration: torch's CPU chain over the parameter snapshots
    assert same_bits(r["ema0"], r["p0"])
    chain = cpu_chain(r, 0.75, 2, interval)
    for it in range(ITERS):
        got = r["ema"][it].cpu()
        bad = np.flatnonzero(bits(got) != bits(chain[it]))
        assert bad.size == 0, (it, bad.size, bad[:5])
    assert not same_bits(r["ema"][-1], r["p"][-1]) and not same_bits(r["ema"][-1], r["ema0"])
    if interval == 2:
        assert all(same_bits(r["ema"][it], r["ema"][it - 1]) for it in range(1, ITERS, 2))
    # (c) eager and taped: the same parameter and EMA bits, and the taped run did replay
    for phase in phases:
        st = r["rt"].tape_stats(phase)
        assert st is not None and st["replays"] >= 1, (phase, st)
        assert eager["rt"].tape_stats(phase) is None
        base_st = ref["rt"].tape_stats(phase)
        assert base_st["calls"] == st["calls"]                  # the tapes hold what they hold without the hook
    assert eager["hist"] == r["hist"]
    for it in range(ITERS):
        assert same_bits(eager["p"][it], r["p"][it]) and same_bits(eager["ema"][it], r["ema"][it]), it


def test_evaluation_and_checkpoints_leave_the_trajectory_alone(runs):
    from radet_amd.runtime import ema_key
    r, ref = runs("saved"), runs("plain")
    assert r["hist"] == ref["hist"]
    for it in range(ITERS):
        assert same_bits(r["p"][it], ref["p"][it]) and same_bits(r["ema"][it], ref["ema"][it]), it
    assert r["rt"].ema_state["swapped"] is False
    assert len(r["loader"].dataset.seen) == ITERS // 2 and sum("Iter(val)" in ln for ln in r["lines"]) == ITERS // 2
    for it in (2, 4, 6, 8):
        ck = torch.load(r["path"].format(iter=it), map_location="cpu")
        assert ck["meta"]["ema_swapped"] is True and ck["meta"]["iter"] == it
        sd, flat = ck["state_dict"], r["rt"].flat
        raw, ema = r["p"][it - 1].cpu(), r["ema"][it - 1].cpu()
        for n, p in r["det"].named_parameters():
            if n in flat.offsets:                               # the file's parameters are the EMA arena, its ema_* the raw weights
                o, k = flat.offsets[n], p.numel()
                assert same_bits(sd[n].reshape(-1), ema[o:o + k]), (it, n)
                assert same_bits(sd[ema_key(n)].reshape(-1), raw[o:o + k]), (it, n)
            else:                                               # frozen: not averaged
                assert same_bits(sd[ema_key(n)], sd[n]) and same_bits(sd[n], p.detach().cpu()), (it, n)
        assert len([k for k in sd if k.startswith("ema_")]) == len(list(r["det"].parameters()))


def test_resume_with_the_hook_is_exact(runs):
    full, res = runs("saved"), runs("resumed")
    assert len(res["p"]) == ITERS - 4 and res["hist"] == full["hist"][4:]
    assert same_bits(res["p0"], full["p"][3]) and same_bits(res["ema0"], full["ema"][3])       # swapped back after the load
    for it in range(4, ITERS):
        assert same_bits(res["p"][it - 4], full["p"][it]) and same_bits(res["ema"][it - 4], full["ema"][it]), it
    a, b = full["rt"], res["rt"]
    assert a.step_count == b.step_count == ITERS
    assert same_bits(a.opt_state["m"], b.opt_state["m"]) and same_bits(a.opt_state["v"], b.opt_state["v"])
    for (k, x), y in zip(full["det"].state_dict().items(), res["det"].state_dict().values()):
        assert torch.equal(x, y), k


def test_resume_without_the_hook_continues_from_the_ema_weights(runs, batches):
    from radet_amd.apis import train_detector
    full = runs("saved")
    det, lines = make_det(), []
    train_detector(det, [], harness_cfg(None, 1, 0), log=lines.append, resume_from=full["path"].format(iter=4))
    rt = det.runtime()
    assert rt.ema_state is None and same_bits(rt.flat.params, full["ema"][3])
    assert sum("EMA weights" in ln for ln in lines) == 1


def test_plain_load_of_an_ema_checkpoint_detects_like_the_ema_weights(runs):
    from oracle import synth
    from radet_amd.apis import load_checkpoint
    full = runs("saved")
    det, rt = full["det"], full["rt"]
    img, metas = synth.synth_images(5, 2).cuda(), synth.img_metas(2)
    fresh = make_det().eval()
    load_checkpoint(fresh, full["path"].format(iter=ITERS))
    want = fresh.runtime().detect(img, metas, fresh.test_cfg)
    assert fresh.runtime().ema_state is None
    det.eval()
    with rt.ema_weights():
        assert rt.ema_state["swapped"] is True and same_bits(rt.flat.params, full["ema"][-1])
        got = rt.detect(img, metas, det.test_cfg)
    det.train()
    assert rt.ema_state["swapped"] is False
    assert same_bits(rt.flat.params, full["p"][-1]) and same_bits(rt.ema_state["ema"], full["ema"][-1])
    assert sum(int(b.shape[0]) for b, _ in want) > 0
    for (b0, l0), (b1, l1) in zip(want, got):
        assert same_bits(b0, b1) and torch.equal(l0, l1)
    # the last evaluation of the run saw the same weights: its detections on that batch are these (boxes are rescaled by 1)
    for (b0, l0), (b1, l1) in zip(full["loader"].dataset.seen[-1], got):
        assert same_bits(b0, b1) and torch.equal(l0, l1)
