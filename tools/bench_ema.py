"""Times the weight EMA and writes profiles/bench_ema.json.  Needs an MI355X.

  step_vs_parent  with --parent DIR (a built checkout of the parent commit): the headline step WITHOUT the hook, `bench.py
                  --gpus 1 --steps S --warmup W` without its extras, a fresh process per run, parent / this alternating --runs
                  times; medians, the parent's own spread, the taped-call counts and the loss bits of both.
  kernel          radet_ema_update beside radet_grad_accumulate mode 1 (the same 12 bytes per element) and radet_ema_swap on
                  the headline arena: tools/bench_optim.py's interleaved rounds; the floor of 12 bytes per element at the
                  rate the sibling reached in profiles/bench_optim.json and at the device's peak HBM rate.
  step_with_hook  the headline step in this process, plain / with the hook (train_step(..., ema_iter=)) alternating --runs
                  times, S steps each behind W warm-up steps.

The child processes run first, before this process opens the device.

    python tools/bench_ema.py [--parent DIR] [--runs 6] [--steps 100] [--warmup 10] [--out profiles/bench_ema.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

HBM_PEAK_TBS = 8.0          # MI355X, HBM3E


def bench_run(tree, steps, warmup):
    """one `bench.py` process in `tree`; its result line"""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline",
           "--no-kernel-events", "--no-mfma-line", "--no-clock-sampler", "--no-extras"]
    r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"bench.py in {tree} ended with {r.returncode}: {r.stderr[-400:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    if "error" in d:
        raise SystemExit(f"bench.py in {tree}: {d['error']}")
    return d


def spread(xs):
    return round(max(xs) - min(xs), 3)


def step_vs_parent(parent, runs, steps, warmup):
    rows = dict(parent=[], this=[])
    for _ in range(runs):
        for name, tree in (("parent", parent), ("this", ROOT)):
            rows[name].append(bench_run(tree, steps, warmup))
    out = dict(command=f"bench.py --gpus 1 --steps {steps} --warmup {warmup} (no extras), a fresh process per run, parent / this "
                       "alternating", runs=runs)
    for name, ds in rows.items():
        ms = [d["ms_per_step"] for d in ds]
        out[name] = dict(ms_per_step=ms, median_ms=round(float(np.median(ms)), 3), spread_ms=spread(ms),
                         taped_calls=sorted({d["config"]["launch_tape"]["calls"] for d in ds}),
                         losses_step1=ds[0]["config"]["losses_step1"], losses=ds[0]["config"]["losses"],
                         same_losses_every_run=all(d["config"]["losses_step1"] == ds[0]["config"]["losses_step1"]
                                                   and d["config"]["losses"] == ds[0]["config"]["losses"] for d in ds))
    p, t = out["parent"], out["this"]
    out["delta_ms"] = round(t["median_ms"] - p["median_ms"], 3)
    out["inside_parent_spread"] = bool(abs(out["delta_ms"]) <= p["spread_ms"])
    out["same_taped_calls"] = p["taped_calls"] == t["taped_calls"]
    out["same_loss_bits"] = p["losses_step1"] == t["losses_step1"] and p["losses"] == t["losses"]
    return out


def kernel_part(rounds, warmup):
    import bench_optim
    full = bench_optim.measure(argparse.Namespace(rounds=rounds, warmup=warmup))
    names = ("grad_accumulate_add", "ema_update", "ema_swap", "ema_swap_back")
    out = dict(n=full["n"], rounds=rounds, warmup=warmup, timing=full["timing"],
               variants={k: full["variants"][k] for k in names}, ema_vs_sibling=full["ema_vs_sibling"])
    nbytes = 12 * full["n"]
    try:
        with open(os.path.join(ROOT, "profiles", "bench_optim.json")) as fh:
            rate = json.load(fh)["variants"]["grad_accumulate_add"]["tb_per_s"]
    except (OSError, KeyError):
        rate = None
    out["floor_12_bytes_per_element"] = dict(
        bytes=nbytes, at_hbm_peak=dict(tb_per_s=HBM_PEAK_TBS, us=round(nbytes / HBM_PEAK_TBS / 1e6, 2)),
        at_sibling_rate_of_bench_optim_json=None if rate is None else dict(tb_per_s=rate, us=round(nbytes / rate / 1e6, 2)))
    return out


def step_with_hook(runs, steps, warmup):
    import torch
    import bench
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    dev = torch.device("cuda")
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(dev).train()
    rt = det.runtime()
    o = cfg.optimizer
    rt.init_optimizer(lr=o.lr, betas=tuple(o.betas), eps=o.eps, weight_decay=o.weight_decay,
                      max_norm=float(cfg.optimizer_config.grad_clip.max_norm))
    rt.set_loss_from_head(det.bbox_head)
    B = bench.PER_GPU_BATCH
    img, boxes, labels, p2g, pw = bench.make_batch(0, B, dev)
    tg = rt.pack_targets([torch.from_numpy(b) for b in boxes], [torch.from_numpy(x) for x in labels], list(p2g), list(pw))
    rt.init_ema()                                               # mmcv's defaults; a step without ema_iter issues no update
    it = 0

    def timed(hook):
        nonlocal it
        for k in range(warmup + steps):
            if k == warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            rt.train_step(img, tg, ema_iter=it if hook else None)
            it += 1
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) / steps * 1e3, 3)

    rows = dict(plain=[], hook=[])
    for _ in range(runs):
        rows["plain"].append(timed(False))
        rows["hook"].append(timed(True))
    return dict(how=f"one process, plain / hook alternating {runs} times, {steps} taped steps each behind {warmup} warm-up steps, "
                    "wall clock around the synchronised loop; the update is one eager launch behind the replayed tape",
                batch=B, taped_calls=rt.tape_stats()["calls"],
                plain=dict(ms_per_step=rows["plain"], median_ms=round(float(np.median(rows["plain"])), 3), spread_ms=spread(rows["plain"])),
                hook=dict(ms_per_step=rows["hook"], median_ms=round(float(np.median(rows["hook"])), 3), spread_ms=spread(rows["hook"])),
                delta_ms=round(float(np.median(rows["hook"]) - np.median(rows["plain"])), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit (step_vs_parent is skipped without it)")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_ema.json"))
    args = ap.parse_args()
    out = {}
    if args.parent:
        out["step_vs_parent"] = step_vs_parent(os.path.abspath(args.parent), args.runs, args.steps, args.warmup)
        print(json.dumps({k: v for k, v in out["step_vs_parent"].items() if k not in ("parent", "this")}), flush=True)
    out["kernel"] = kernel_part(args.rounds, 5)
    print(json.dumps(out["kernel"]["ema_vs_sibling"]), flush=True)
    out["step_with_hook"] = step_with_hook(args.runs, args.steps, args.warmup)
    print(json.dumps(out["step_with_hook"]), flush=True)
    import torch
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
