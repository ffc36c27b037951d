"""Times the optimizer kernels on the headline arena (the trainable parameters of configs/bop/r50_ycbv_pbr.py) and writes
profiles/bench_optim.json.  The variants -- radet_adamw_step (the yardstick), radet_adamw_step_runs with the table that
paramwise_cfg=dict(norm_decay_mult=0.) makes, radet_sgd_step with and without that table and with and without momentum,
radet_grad_accumulate in its three modes, radet_ema_update (beside the accumulate mode that moves the same 12 bytes per
element) and radet_ema_swap -- are launched interleaved, round after round, each between two HIP events; per
variant: median / min / max / 10th-90th percentile of the device time, the bytes the algorithm has to move and the rate
they give.  Needs an MI355X: there is no CPU path.

    python tools/bench_optim.py [--rounds 40] [--warmup 5] [--out profiles/bench_optim.json]
"""
import argparse
import json
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def measure(args):
    """the timed rounds; args: rounds, warmup.  Returns the dictionary main() writes."""
    if args.rounds < 20:
        raise SystemExit("at least 20 timed launches per variant")
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim needs an MI355X: the optimizer kernels have no CPU path")
    from radet_amd import kernels as K
    from radet_amd.apis import resolve_paramwise
    from radet_amd.models import build_detector
    from radet_amd.runtime import FlatParams, build_opt_runs
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    flat = FlatParams(det, "cpu")                                   # (the layout only; the timed arenas are the device ones below)
    table = build_opt_runs(flat, resolve_paramwise(det, dict(norm_decay_mult=0.0)))
    n, nruns = flat.n_train, len(table)
    dev = torch.device("cuda")
    runs = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=gen)
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    m, v, buf, acc = (torch.zeros(n, device=dev) for _ in range(4))
    ema = torch.zeros(n, device=dev)
    parts, gn = torch.zeros(1024, device=dev), torch.zeros(1, device=dev)
    K.sqnorm_partials(g, n, parts)
    lr, step = 1e-6, 7                                              # (small: thousands of launches must not move p far)
    adam = ((0.9, 0.999), 1e-8, 0.05, step, 35.0, 1.0, parts, gn)
    sgd = (1e-4, False, step, 35.0, 1.0, parts, gn)
    F = 4 * n
    variants = [
        ("adamw_step", 7 * F, lambda: K.adamw_step(p, g, m, v, n, lr, *adam)),
        ("adamw_step_runs", 7 * F + 16 * nruns, lambda: K.adamw_step_runs(p, g, m, v, n, lr, *adam, runs, nruns)),
        ("sgd_step_momentum", 5 * F, lambda: K.sgd_step(p, g, buf, n, lr, 0.9, 0.0, *sgd)),
        ("sgd_step_momentum_runs", 5 * F + 16 * nruns, lambda: K.sgd_step(p, g, buf, n, lr, 0.9, 0.0, *sgd, runs, nruns)),
        ("sgd_step_plain", 3 * F, lambda: K.sgd_step(p, g, None, n, lr, 0.0, 0.0, *sgd)),
        ("sgd_step_plain_runs", 3 * F + 16 * nruns, lambda: K.sgd_step(p, g, None, n, lr, 0.0, 0.0, *sgd, runs, nruns)),
        ("grad_accumulate_set", 2 * F, lambda: K.grad_accumulate(acc, g, n, K.GRAD_ACC_SET)),
        ("grad_accumulate_add", 3 * F, lambda: K.grad_accumulate(acc, g, n, K.GRAD_ACC_ADD)),
        ("grad_accumulate_restore", 3 * F, lambda: K.grad_accumulate(acc, g, n, K.GRAD_ACC_RESTORE)),
        # the EMA update on the arenas of the accumulate modes (mode 1 moves the same bytes: read two arenas, write one);
        # the swap twice, so that every round starts from the same arenas
        ("ema_update", 3 * F, lambda: K.ema_update(acc, g, n, 0.0002)),
        ("ema_swap", 4 * F, lambda: K.ema_swap(acc, ema, n)),
        ("ema_swap_back", 4 * F, lambda: K.ema_swap(acc, ema, n)),
    ]
    g0 = g.clone()
    times = {name: [] for name, _, _ in variants}
    for r in range(args.warmup + args.rounds):
        evs = []
        for name, _, launch in variants:
            if name == "grad_accumulate_restore":
                acc.zero_()                                         # (g = acc + g must not grow round after round)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            evs.append((name, a, b))
        torch.cuda.synchronize()
        if r >= args.warmup:
            for name, a, b in evs:
                times[name].append(a.elapsed_time(b) * 1e3)
    assert torch.isfinite(p).all() and torch.equal(g, g0)
    out = dict(device=torch.cuda.get_device_name(0), n=n, nruns=nruns, rounds=args.rounds, warmup=args.warmup,
               timing="HIP events around each launch, variants interleaved per round, default clocks", variants={})
    for name, nbytes, _ in variants:
        t = np.array(times[name])
        med = float(np.median(t))
        out["variants"][name] = dict(median_us=round(med, 2), min_us=round(float(t.min()), 2), max_us=round(float(t.max()), 2),
                                     p10_us=round(float(np.percentile(t, 10)), 2), p90_us=round(float(np.percentile(t, 90)), 2),
                                     bytes=int(nbytes), tb_per_s=round(nbytes / med / 1e6, 3))
    y, t = out["variants"]["adamw_step"], out["variants"]["adamw_step_runs"]
    out["runs_vs_yardstick"] = dict(delta_us=round(t["median_us"] - y["median_us"], 2),
                                    yardstick_spread_us=round(y["p90_us"] - y["p10_us"], 2),
                                    ratio=round(t["median_us"] / y["median_us"], 4))
    y, t = out["variants"]["grad_accumulate_add"], out["variants"]["ema_update"]
    out["ema_vs_sibling"] = dict(delta_us=round(t["median_us"] - y["median_us"], 2), sibling_p10_us=y["p10_us"],
                                 sibling_p90_us=y["p90_us"], inside_band=bool(y["p10_us"] <= t["median_us"] <= y["p90_us"]),
                                 ratio=round(t["median_us"] / y["median_us"], 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_optim.json"))
    args = ap.parse_args()
    out = measure(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out["runs_vs_yardstick"]))
    for name, d in out["variants"].items():
        print(f"{name:26s} median {d['median_us']:8.2f} us  [{d['p10_us']:.2f} .. {d['p90_us']:.2f}]  {d['tb_per_s']:.3f} TB/s")


if __name__ == "__main__":
    main()
