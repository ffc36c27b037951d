"""Time radet_nms / radet_soft_nms on synthetic candidates:
    python tools/bench_nms.py [N per image] [B] [vote | nms | soft_linear | soft_gaussian | all] [json path]
`vote` (the default) times radet_nms in vote mode as before.  `all` times the four in alternating rounds on the same
candidates and prints (and, given a path, writes) one JSON line with the medians."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from radet_amd import kernels as K
from radet_amd import ops

MODES = ("vote", "nms", "soft_linear", "soft_gaussian")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 4420
B = int(sys.argv[2]) if len(sys.argv) > 2 else 8
MODE = sys.argv[3] if len(sys.argv) > 3 else "vote"
if MODE not in MODES + ("all",):
    sys.exit(f"mode {MODE!r}: expected one of {MODES + ('all',)}")
g = torch.Generator().manual_seed(0)
c = torch.rand(B, N, 2, generator=g) * torch.tensor([600.0, 440.0])
wh = torch.rand(B, N, 2, generator=g) * 120 + 8
boxes = torch.cat([c - wh / 2, c + wh / 2], -1).cuda().contiguous()
sc = torch.rand(B, N, generator=g).cuda()
lab = torch.randint(0, 21, (B, N), generator=g).cuda()
cnt = torch.full((B,), N, dtype=torch.int32).cuda()
cap = N
ob = torch.empty(B, 100, 4).cuda(); osc = torch.empty(B, 100).cuda()
ol = torch.empty(B, 100, dtype=torch.long).cuda(); oc = torch.zeros(B, dtype=torch.int32).cuda()
aux = torch.empty(2, B * cap, dtype=torch.long).cuda()
ws = torch.empty(K.nms_ws_bytes(B, cap), dtype=torch.uint8).cuda()
sws = torch.empty(K.soft_nms_ws_bytes(B, cap), dtype=torch.uint8).cuda()
keep = torch.empty(B, 100, dtype=torch.long).cuda()


def run(mode="vote"):
    if mode == "vote":
        K.nms(boxes, sc, sc, lab, cnt, B, cap, 0, 0.65, False, 0.025, 100, ob, osc, ol, oc, aux[0], aux[1], ws)
    elif mode == "nms":
        K.nms(boxes, sc, sc, lab, cnt, B, cap, 3, 0.5, False, 0.0, 100, ob, osc, ol, oc, aux[0], aux[1], ws)
    else:
        K.soft_nms(boxes, sc, lab, cnt, B, cap, K.SOFT_NMS_METHODS[mode[5:]], 0.3, 0.5, 1e-3, False, 100, ob, osc, ol, keep,
                   oc, sws)


def timed(mode, iters=10):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        run(mode)
    e.record(); e.synchronize()
    return s.elapsed_time(e) / iters * 1e3


if MODE != "all":
    for _ in range(3):
        run(MODE)
    torch.cuda.synchronize()
    tag = "" if MODE == "vote" else MODE + " "
    print(f"N={N} B={B} {tag}{timed(MODE):.0f} us per launch, heads {oc.tolist()[:4]}")
else:
    heads = {}
    for m in MODES:
        for _ in range(3):
            run(m)
        torch.cuda.synchronize()
        heads[m] = oc.tolist()[:4]
    rounds = {m: [] for m in MODES}
    for _ in range(15):                      # alternating rounds: drift and other people's load hit every mode alike
        for m in MODES:
            rounds[m].append(timed(m, 20))
    med = {m: float(np.median(v)) for m, v in rounds.items()}
    res = dict(tool="bench_nms", N=N, B=B, max_out=100, rounds=15, iters=20, device=torch.cuda.get_device_name(0),
               clocks="default governor, not pinned; medians over alternating rounds",
               settings=dict(vote="mode 0, thr 0.65", nms="mode 3, thr 0.5", soft_linear="thr 0.3, min_score 1e-3",
                             soft_gaussian="sigma 0.5, min_score 1e-3"),
               median_us=med, min_us={m: float(min(v)) for m, v in rounds.items()},
               max_us={m: float(max(v)) for m, v in rounds.items()}, heads=heads,
               soft_over_nms={m: med[m] / med["nms"] for m in ("soft_linear", "soft_gaussian")})
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            f.write(line + "\n")
