"""Per-detector device runtime: flat parameter / gradient / optimiser-state arenas, the HIP Engine,
target packing, the native train step (forward + hand-written backward + RCCL all-reduce overlapped
with backward + fused clip/AdamW) and inference (decode + NMS).

Replaces what the reference obtains from torch autograd + mmcv's DDP wrapper / OptimizerHook
(radet/apis/train.py:73-126, radet/models/detectors/base.py:185-253).
"""
import contextlib
import os

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from . import kernels as K
from .engine import Engine


def _align(n, a=4):
    return (n + a - 1) // a * a


class FlatParams:
    """Re-points every floating-point parameter / buffer of `module` into flat fp32 arenas.

    Trainable parameters (module order: backbone -> neck -> head, which is also the order of the
    engine's conv table) form one arena with a same-layout gradient arena; the rest (frozen
    parameters, BN running statistics) a second one."""

    def __init__(self, module, device):
        named = [(n, p) for n, p in module.named_parameters()]
        train = [(n, p) for n, p in named if p.requires_grad]
        frozen = [(n, p) for n, p in named if not p.requires_grad]
        bufs = [(n, b) for n, b in module.named_buffers() if b.is_floating_point()]
        self.train_names = [n for n, _ in train]
        self.offsets = {}
        off = 0
        for n, p in train:
            if p.numel() >= 4:
                off = _align(off)
            self.offsets[n] = off
            off += p.numel()
        self.n_train = _align(off)
        self.params = torch.zeros(self.n_train, device=device)
        self.grads = torch.zeros(self.n_train, device=device)
        self.p, self.g = {}, {}
        # name -> the tensor objects through which torch code can write this parameter: the arena view and the module's
        # Parameter (same storage, separate version counters); Engine.fold() watches both
        self.watch = {}
        for n, p in train:
            o = self.offsets[n]
            v = self.params[o:o + p.numel()].view(p.shape)
            v.copy_(p.data)
            p.data = v
            self.p[n] = v
            self.watch[n] = (v, p)
            self.g[n] = self.grads[o:o + p.numel()].view(p.shape)
        off = 0
        foffs = {}
        for n, t in frozen + bufs:
            off = _align(off)
            foffs[n] = off
            off += t.numel()
        self.frozen = torch.zeros(_align(off), device=device)
        for n, p in frozen:
            v = self.frozen[foffs[n]:foffs[n] + p.numel()].view(p.shape)
            v.copy_(p.data)
            p.data = v
            self.p[n] = v
            self.watch[n] = (v, p)
        for n, b in bufs:
            v = self.frozen[foffs[n]:foffs[n] + b.numel()].view(b.shape)
            v.copy_(b)
            mod, _, leaf = n.rpartition(".")
            owner = module.get_submodule(mod) if mod else module
            owner._buffers[leaf] = v
            self.p[n] = v
        self._probe = train[0][1] if train else None

    def group_ranges(self, prefixes):
        """Contiguous [begin, end) ranges of the trainable arena per name-prefix group (in arena order)."""
        out = []
        for pf in prefixes:
            names = [n for n in self.train_names if n.startswith(pf)]
            if not names:
                continue
            b = self.offsets[names[0]]
            last = names[-1]
            e = self.offsets[last] + self.p[last].numel()
            out.append((pf, b, e))
        return out

    def still_bound(self):
        p = self._probe
        return p is None or (p.data_ptr() == self.p[self.train_names[0]].data_ptr())


def compute_buckets(flat, conv_names, conv_trainable, split=("backbone.layer4.",), min_bytes=15e6):
    """Gradient buckets in backward order: (prefix, conv-table range, gradient-arena range).
    Arena ranges are contiguous, disjoint and together cover every trainable parameter.
    A stage named in `split` is cut into one bucket per run of bottleneck blocks of >= min_bytes (fp32), last block first:
    layer4 holds 47 % of all gradient bytes (59.9 MB) and is the first backbone stage of the backward pass, so as ONE message
    its exchange could only start when the whole stage's weight gradients were reduced (3.97 ms into a 5.93-ms backward
    pass); per block (17.8 + 17.8 + 24.3 MB) the first message leaves a third of the way through the stage.  xGMI links
    want few large messages, hence the 15-MB floor (layer3's six blocks of 4.5 MB stay one 28-MB bucket)."""
    def rng(pf):
        idx = [i for i, n in enumerate(conv_names) if n.startswith(pf)]
        return (idx[0], idx[-1] + 1) if idx else None

    def bucket(pf, groups, r, blocks=None):
        arena = flat.group_ranges(groups)
        d = dict(prefix=pf, convs=r, arena=(min(a[1] for a in arena), max(a[2] for a in arena)))
        if blocks is not None:
            d["blocks"] = blocks                  # (stage index, first block, last block) of a per-block bucket
        return d

    buckets = []
    for pf in ("bbox_head.", "neck.", "backbone.layer4.", "backbone.layer3.", "backbone.layer2.", "backbone.layer1.",
               "backbone.conv1"):
        r = rng(pf)
        if r is None or not any(conv_trainable[r[0]:r[1]]):
            continue
        if pf in split and os.environ.get("RADET_SPLIT_BUCKETS", "1") != "0":
            nblk = 1 + max(int(n[len(pf):].split(".")[0]) for n in conv_names[r[0]:r[1]])
            runs, hi = [], nblk - 1
            while hi >= 0:                         # runs of blocks [lo, hi], last block first, each >= min_bytes
                lo, size = hi, 0
                while True:
                    size += 4 * sum(e - b for _, b, e in flat.group_ranges([f"{pf}{lo}."]))
                    if size >= min_bytes or lo == 0:
                        break
                    lo -= 1
                runs.append((lo, hi))
                hi = lo - 1
            if len(runs) > 1 and 4 * sum(e - b for _, b, e in flat.group_ranges([f"{pf}{k}." for k in range(runs[-1][0], runs[-1][1] + 1)])) < min_bytes:
                runs[-2] = (runs[-1][0], runs[-2][1])      # a short remainder joins the run before it
                runs.pop()
            if len(runs) > 1:
                li = int(pf[len("backbone.layer"):-1]) - 1
                for lo, hi in runs:
                    names = [f"{pf}{k}." for k in range(lo, hi + 1)]
                    cr = [rng(n) for n in names]
                    buckets.append(bucket(f"{pf}{lo}-{hi}." if lo != hi else names[0], names, (min(c[0] for c in cr), max(c[1] for c in cr)),
                                          blocks=(li, lo, hi)))
                continue
        buckets.append(bucket(pf, ["backbone.conv1", "backbone.bn1"] if pf == "backbone.conv1" else [pf], r))
    return buckets


OPT_RUN_DTYPE = np.dtype([("begin", "<u4"), ("end", "<u4"), ("lr_mult", "<f4"), ("decay_mult", "<f4")])   # RadetOptRun


def check_opt_runs(runs, n):
    """A run table the optimizer kernels accept (include/radet_hip.h, RadetOptRun): at most kernels.OPT_MAX_RUNS non-empty
    runs, sorted, disjoint, covering [0, n).  The kernels trust this; nothing else validates it."""
    if len(runs) > K.OPT_MAX_RUNS:
        raise NotImplementedError(f"{len(runs)} parameter-group runs: the optimizer kernels hold at most RADET_OPT_MAX_RUNS = "
                                  f"{K.OPT_MAX_RUNS} in LDS (merge groups, or give neighbouring parameters equal multipliers)")
    if len(runs) < 1 or n >= 2 ** 32:
        raise ValueError(f"a run table needs at least one run and an arena below 2^32 elements (got {len(runs)} runs, n = {n})")
    b, e = runs["begin"].astype(np.int64), runs["end"].astype(np.int64)
    if b[0] != 0 or e[-1] != n or (e <= b).any() or (b[1:] != e[:-1]).any():
        raise ValueError("run table is not sorted, disjoint and covering [0, n)")
    return runs


def build_opt_runs(flat, groups):
    """Per-parameter multipliers -> the run table of the optimizer kernels.  groups: {parameter name: (lr_mult, decay_mult)};
    a trainable parameter it does not name has (1, 1).  Tensors that follow each other in the arena with equal multipliers
    merge into one run; the arena's alignment gaps (zeros no kernel writes) join the run in front of them, the leading
    one and the arena's padded end likewise, so the table covers [0, n_train).  Returns None when every multiplier is 1
    (no table: the plain kernels), else a numpy record array of OPT_RUN_DTYPE."""
    groups = dict(groups or {})
    unknown = [k for k in groups if k not in flat.offsets]
    if unknown:
        raise KeyError(f"parameter groups name {unknown[:3]}{'...' if len(unknown) > 3 else ''}: not trainable parameters of this model")
    out = []                                            # [begin, end, lr_mult, decay_mult]
    for name in flat.train_names:
        lm, dm = (float(x) for x in groups.get(name, (1.0, 1.0)))
        b = flat.offsets[name]
        e = b + flat.p[name].numel()
        if out and (out[-1][2], out[-1][3]) == (lm, dm):
            out[-1][1] = e
        else:
            if out:
                out[-1][1] = b                          # (an alignment gap stays with the run before it)
            out.append([b if out else 0, e, lm, dm])
    if not out:
        return None
    out[-1][1] = flat.n_train
    if all((r[2], r[3]) == (1.0, 1.0) for r in out):
        return None
    runs = np.array([tuple(r) for r in out], dtype=OPT_RUN_DTYPE)
    return check_opt_runs(runs, flat.n_train)


def ema_momentum(it, momentum, interval=1, warm_up=100):
    """mmcv EMAHook's momentum for the update after iteration `it` (0-based, runner.iter): min(momentum ** interval,
    (1 + it) / (warm_up + it)), in Python doubles.  The hook fires only when it % interval == 0."""
    if warm_up + it == 0:                       # (warm_up = 0 at iteration 0 is 1 / 0 in mmcv; here the EMA restarts from the parameters)
        return 1.0
    return min(momentum ** interval, (1 + it) / (warm_up + it))


def ema_key(name):
    """mmcv EMAHook's buffer name of a parameter: 'ema_' + the name with every '.' replaced by '_'"""
    return "ema_" + name.replace(".", "_")


class _StreamWork:
    """What GradReducer needs of a c10d Work, for a collective issued synchronously on a stream of ours: an event behind it"""

    def __init__(self, timed, t0):
        self.t0 = t0
        self.done = torch.cuda.Event(enable_timing=timed)
        self.done.record()

    def wait(self):
        torch.cuda.current_stream().wait_event(self.done)

    def _get_duration(self):                                   # ms, valid once `done` has completed
        return self.t0.elapsed_time(self.done)


def sync_collectives_run_on_current_stream():
    """c10d issues `async_op=False` NCCL / RCCL collectives on the caller's current stream since torch 2.8 (before that
    every collective ran on the process group's internal stream and the caller's stream waited for it).  The gradient exchange
    relies on it to stay inside the four-stream budget (engine.py): on an older build the collectives would silently move
    to RCCL's own stream -- a fifth stream, measured +35 % step time."""
    try:
        major, minor = (int(x) for x in torch.__version__.split("+")[0].split(".")[:2])
    except ValueError:
        return True
    return (major, minor) >= (2, 8)


class GradReducer:
    """Sum-all-reduce of gradient-arena buckets as they become ready (RCCL over xGMI on the GPU box,
    gloo in the CPU tests).  `bucket_ready` is called on the stream that produced the bucket (the engine's side
    stream, right after the bucket's slab reduction); the collective runs behind an event of that stream on the
    communication stream (`comm_stream`: see __init__; without one, asynchronously on the process group's internal
    stream), so neither the side stream nor the main stream waits for it, and `finish()` makes the current stream wait
    for all of them.  The mean (1/world) is applied later, inside the fused clip+AdamW kernel."""

    def __init__(self, grads, device, bf16=False, comm_stream=None):
        """bf16=True: each bucket is exchanged as bf16 (half the bytes on xGMI; the reference's fp16 training also
        all-reduces half-precision gradients): fp32 -> bf16 staging buffer -> all-reduce -> back into the fp32 arena.
        comm_stream: a HIP stream of the caller on which the collectives run, as SYNCHRONOUS `all_reduce` calls (which
        c10d issues on the current stream) behind an event of the producing stream -- instead of asynchronous ones on the
        process group's internal stream.  The detector passes its tower-chain stream, idle from the end of the head's
        backward pass to the next step: a process may not USE more than four HIP streams on this device ("stream budget",
        engine.py), and main + side + second weight-gradient stream + chain are four already (with RCCL's own stream as the
        fifth the step took 13.8-14.1 instead of 10.2-10.3 ms, tools/bench_dp1.py)."""
        self.grads, self.device, self.bf16 = grads, device, bf16
        self.comm_stream = comm_stream if grads.is_cuda else None
        self.works = []
        self.staging = torch.empty(grads.numel(), dtype=torch.bfloat16, device=device) if bf16 else None
        # diagnostics (enable_trace()): per bucket an event on the producing stream when the bucket is handed over, an event
        # on the main stream right behind finish()'s wait for it ("done by": an upper bound of the completion, exact for the
        # bucket the optimizer really waits for) and -- with TORCH_NCCL_ENABLE_TIMING=1 -- RCCL's own start-to-end time of
        # the collective.  (Taking the completion on a stream of its own that only waits for the work was tried: that
        # stream's barrier packets stalled the main stream's hardware queue, +45 % step time under tracing.)
        self.trace = None

    def enable_trace(self, on=True):
        self.trace = [] if on else None

    def _convert(self, src, dst):
        if src.is_cuda:
            K.convert_rows(src.view(1, -1), dst.view(1, -1))
        else:
            dst.copy_(src)

    def bucket_ready(self, bucket):
        b, e = bucket["arena"]
        ready = None
        if self.trace is not None and self.grads.is_cuda:
            ready = torch.cuda.Event(enable_timing=True)
            ready.record()
        if self.comm_stream is not None:
            cs = self.comm_stream
            handed = torch.cuda.Event()
            handed.record()                                    # on the stream that produced the bucket
            timed = self.trace is not None
            with torch.cuda.stream(cs):
                cs.wait_event(handed)
                t0 = torch.cuda.Event(enable_timing=True) if timed else None
                if timed:
                    t0.record()
                if self.bf16:
                    st = self.staging[b:e]
                    self._convert(self.grads[b:e], st)
                    dist.all_reduce(st, op=dist.ReduceOp.SUM, async_op=False)
                else:
                    dist.all_reduce(self.grads[b:e], op=dist.ReduceOp.SUM, async_op=False)
                w = _StreamWork(timed, t0)
        elif self.bf16:
            st = self.staging[b:e]
            self._convert(self.grads[b:e], st)
            w = dist.all_reduce(st, op=dist.ReduceOp.SUM, async_op=True)
        else:
            w = dist.all_reduce(self.grads[b:e], op=dist.ReduceOp.SUM, async_op=True)
        self.works.append((w, b, e))
        if ready is not None:
            self.trace.append(dict(prefix=bucket["prefix"], bytes=(e - b) * (2 if self.bf16 else 4), ready=ready, done=None, work=w))

    def finish(self):
        for w, b, e in self.works:
            w.wait()
            if self.trace is not None and self.grads.is_cuda:
                for t in self.trace[-len(self.works):]:
                    if t["work"] is w and t["done"] is None:
                        t["done"] = torch.cuda.Event(enable_timing=True)
                        t["done"].record()
            if self.bf16:
                self._convert(self.staging[b:e], self.grads[b:e])
        self.works = []


class DetectorRuntime:
    def __init__(self, det, depth, num_classes, frozen_stages, strides, stacked_convs=4, math=None):
        dev = next(det.parameters()).device
        if dev.type != "cuda":
            raise _lib.RadetHipError(
                "radet_amd runs on MI355X only: move the detector to a HIP device (model.cuda()) first; "
                "there is no CPU / PyTorch fallback path.")
        _lib.load()
        self.dev = dev
        self.flat = FlatParams(det, dev)
        self.engine = Engine(self.flat.p, self.flat.g, depth=depth, num_classes=num_classes,
                             frozen_stages=frozen_stages, strides=strides, stacked_convs=stacked_convs, math=math,
                             watch=self.flat.watch)
        self.num_classes, self.strides = num_classes, tuple(strides)
        self.opt_state = None
        self.step_count = 0
        self.comm_stream = None
        self.buckets = compute_buckets(self.flat, [c.name for c in self.engine.convs],
                                       [c.trainable for c in self.engine.convs])
        self.reducer = None
        self._replicas_synced = False
        # (no collective here: a runtime may be built by a subset of the ranks -- rank-0 evaluation, checkpoint
        # conversion.  Data-parallel replicas are equalised by init_optimizer(), the entry point of every training run.)

    def caller_stream(self):
        """a HIP stream for the caller's own asynchronous work (next-batch upload) that stays off the main stream's pipe of the
        command processor (Engine.caller_stream; INTEGRATION.md, streams)"""
        return self.engine.caller_stream()

    def sync_replicas(self, src=0):
        """Broadcast the parameter arenas (trainable + frozen / BN statistics) and, once it exists, the optimizer
        state from rank `src`: what wrapping the model in MMDistributedDataParallel does at construction in the
        reference (radet/apis/train.py:73-81) and what a checkpoint loaded on one rank needs.  Collective: every rank
        of the default process group must call it.  No-op without an initialised group / with a single rank."""
        self._replicas_synced = True
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return False
        arenas = [self.flat.params, self.flat.frozen]
        if self.opt_state is not None:
            arenas += [self.opt_state[k] for k in ("m", "v", "buf") if self.opt_state.get(k) is not None]
        if self.ema_state is not None:
            arenas.append(self.ema_state["ema"])      # (every rank then computes the same EMA: no further communication)
        for t in arenas:
            dist.broadcast(t, src)
        step = torch.tensor([self.step_count], dtype=torch.int64, device=self.dev)
        dist.broadcast(step, src)
        self.step_count = int(step.item())
        return True

    # ------------------------------------------------------------------ inputs
    def pack_targets(self, gt_bboxes, gt_labels, points_to_gt_index, points_weight):
        """list-per-image tensors (the reference's DataContainer layout) -> flat device tensors."""
        dev = self.dev
        B = len(gt_bboxes)
        counts = [int(b.shape[0]) for b in gt_bboxes]
        off = np.zeros(B + 1, np.int32)
        off[1:] = np.cumsum(counts)
        boxes = torch.cat([b.reshape(-1, 4).float() for b in gt_bboxes]) if sum(counts) else torch.zeros(0, 4)
        labels = torch.cat([l.reshape(-1).long() for l in gt_labels]) if sum(counts) else torch.zeros(0, dtype=torch.long)
        boxes = boxes.to(dev).contiguous()
        labels = labels.to(dev).contiguous()
        if boxes.shape[0] == 0:   # keep valid device pointers
            boxes = torch.zeros(1, 4, device=dev)
            labels = torch.zeros(1, dtype=torch.long, device=dev)
        p2g = torch.stack([t.reshape(-1).long() for t in points_to_gt_index]).to(dev).contiguous()
        pw = torch.stack([t.reshape(-1).float() for t in points_weight]).to(dev).contiguous()
        return dict(boxes=boxes, labels=labels, off=torch.from_numpy(off).to(dev), p2g=p2g, pw=pw, B=B)

    # ------------------------------------------------------------------ forward / backward
    def forward(self, img, fold=True):
        """img: NCHW fp32 device tensor. Runs fold -> backbone -> neck -> head. Returns engine buffers."""
        assert img.is_cuda and img.dtype == torch.float32 and img.dim() == 4 and img.shape[1] == 3
        img = img.contiguous()
        e = self.engine
        e.prepare(img.shape[0], img.shape[2], img.shape[3])
        if fold:
            e.fold()
        feats = e.backbone_forward(img)
        P = e.neck_forward(feats)
        return e.head_forward(P)

    loss_hparams = None
    loss_weights = None      # device f32[3] = (loss_cls.loss_weight, 1, loss_iou.loss_weight) when either differs from 1

    def set_loss_from_head(self, head):
        """Take focal alpha / gamma, the box loss's kind and eps and the three loss weights from the head's loss modules
        (config values).  A `loss_bbox` the fused head loss has no kernel for raises NotImplementedError."""
        from .models.losses import fused_box_loss
        kind, eps = fused_box_loss(head.loss_bbox)
        self.loss_hparams = dict(alpha=float(head.loss_cls.alpha), gamma=float(head.loss_cls.gamma),
                                 lbw=float(head.loss_bbox.loss_weight), box_kind=kind, box_eps=eps)
        wc, wi = float(head.loss_cls.loss_weight), float(head.loss_iou.loss_weight)
        self.loss_weights = None if (wc == 1.0 and wi == 1.0) else torch.tensor([wc, 1.0, wi], device=self.dev)
        return self

    def loss(self, tg, grad_scale=None, labels_out=None, tgt_out=None):
        hp = self.loss_hparams or dict(alpha=0.25, gamma=2.0, lbw=2.0)
        return self.engine.loss(tg["boxes"], tg["labels"], tg["off"], tg["p2g"], tg["pw"], grad_scale=grad_scale,
                                labels_out=labels_out, tgt_out=tgt_out, **hp)

    def backward(self, bucket_hook=None, next_img=None):
        """Reverse program. After each parameter group's wgrads are done its slabs are reduced /
        un-folded into the gradient arena and `bucket_hook(bucket)` may start its all-reduce.  next_img: the NEXT step's
        batch, if the caller already has it -- its frozen prefix (stem, frozen stages) then runs next to this backward pass
        (Engine.prefetch_prefix)."""
        e = self.engine
        if not self._replicas_synced:
            # the reference's DDP wrap broadcasts rank 0's parameters at construction (apis/train.py:73-81); here that is
            # sync_replicas(), called by init_optimizer() / load_checkpoint().  A module-API training loop with its own
            # torch optimizer never passes through those: say so once instead of training diverging replicas silently
            self._replicas_synced = True
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                import warnings
                warnings.warn("radet_amd: backward pass under a process group of "
                              f"{dist.get_world_size()} ranks before DetectorRuntime.sync_replicas() / init_optimizer() was "
                              "called: the replicas still hold their own initial parameters (call "
                              "det.runtime().sync_replicas() on every rank once, see INTEGRATION.md)")

        def unfold(bucket):
            self._unfold_bucket(bucket, bucket_hook)

        bk = {b["prefix"]: b for b in self.buckets}
        per_block = {(b["blocks"][0], b["blocks"][1]): b for b in self.buckets if "blocks" in b}   # keyed by the run's FIRST block
        dP = e.head_backward()
        if next_img is not None and bucket_hook is None:
            e.prefetch_prefix(next_img)         # on the tower-chain stream, idle from here on (single-GPU runs)
        unfold(bk["bbox_head."])
        d_feats = e.neck_backward(dP)
        unfold(bk["neck."])

        def after(li, bi=None):
            if bi is not None:                  # a block's weight gradients are all issued: its run's bucket, if it ends one
                if (li, bi) in per_block:
                    unfold(per_block[(li, bi)])
                return
            pf = "backbone.conv1" if li == "stem" else f"backbone.layer{li + 1}."
            if pf in bk:                        # (a stage that is cut into per-block buckets has none of its own)
                unfold(bk[pf])
        e.backbone_backward(d_feats, after_stage=after, block_ends=set(per_block))
        e.join_side()                           # gradients complete on the current stream from here on
        if next_img is not None and bucket_hook is not None:
            # data-parallel runs: the tower-chain stream carries the gradient exchange during the backward pass, so the prefix
            # follows the last bucket there (next to the exposed end of the exchange, the clip and AdamW)
            e.prefetch_prefix(next_img)

    def _unfold_bucket(self, bucket, bucket_hook=None):
        """Reduce / un-fold the weight-gradient slabs of one bucket's convs into the gradient arena."""
        import ctypes as C
        e = self.engine
        desc_bytes = C.sizeof(_lib.RadetConvDesc)
        a, b = bucket["convs"]
        if e.use_streams:
            # the slab reduction follows the bucket's weight-gradient GEMMs on the side stream, off the
            # critical path of the dgrad chain; the all-reduce hook keys off the side stream too
            side = e._side()
            e.side_collect()
            e._fork(side)
            with torch.cuda.stream(side):
                K.unfold_grads(e.table[a * desc_bytes:], b - a, e.max_cout)
                if bucket_hook is not None:
                    self._hand_over(bucket_hook, bucket, side)
        else:
            K.unfold_grads(e.table[a * desc_bytes:], b - a, e.max_cout)
            if bucket_hook is not None:
                self._hand_over(bucket_hook, bucket, None)

    @staticmethod
    def _hand_over(bucket_hook, bucket, stream):
        """bucket_hook(bucket); `stream`: the stream the caller made current for it (None: it did not switch).  While a launch
        tape is recorded this is a cut: a replayed step hands the bucket over at the same point, on the same stream, and the
        hook itself -- its converts and events included -- is never recorded (Tape.run_cut)."""
        if _lib.TAPE is not None:
            _lib.TAPE.run_cut(lambda: bucket_hook(bucket), stream)
        else:
            bucket_hook(bucket)

    # ------------------------------------------------------------------ optimiser
    def init_optimizer(self, lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, max_norm=35.0, sync=True,
                       type="AdamW", momentum=0.0, dampening=0.0, nesterov=False, groups=None):
        """Optimizer state for the trainable arena: type "AdamW" (m, v) or "SGD" (buf, with momentum != 0).
        groups: {parameter name: (lr_mult, decay_mult)} -- mmcv's paramwise_cfg, resolved (apis/train.py:resolve_paramwise);
        it becomes a device run table (build_opt_runs) the fused kernels look each element up in.  None, or every
        multiplier 1, is no table and, for AdamW, the plain radet_adamw_step.
        COLLECTIVE when a process group is initialised (sync=True): every rank must call it; the replicas then start from
        rank 0's parameters -- the broadcast MMDistributedDataParallel does at construction in the reference
        (radet/apis/train.py:73-81)."""
        if type not in ("AdamW", "SGD"):
            raise NotImplementedError(f"optimizer type {type!r}: the fused step implements AdamW and SGD")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        n = self.flat.n_train
        table = build_opt_runs(self.flat, groups)
        st = dict(lr=lr, wd=weight_decay, max_norm=max_norm, partials=torch.zeros(1024, device=self.dev),
                  grad_norm=torch.zeros(1, device=self.dev), type=type, groups=dict(groups or {}), run_table=table,
                  runs=None if table is None else torch.from_numpy(table.view(np.uint8).copy()).to(self.dev),
                  nruns=0 if table is None else len(table))
        if type == "AdamW":
            st.update(m=torch.zeros(n, device=self.dev), v=torch.zeros(n, device=self.dev), betas=betas, eps=eps)
        else:
            st.update(buf=torch.zeros(n, device=self.dev) if momentum != 0 else None, momentum=float(momentum),
                      dampening=float(dampening), nesterov=bool(nesterov))
        self.opt_state = st
        self.step_count = 0
        self._acc = None
        if sync:
            self.sync_replicas()

    def optimizer_step(self, lr=None, grad_div=1.0):
        st = self.opt_state
        self.step_count += 1
        lr = st["lr"] if lr is None else lr
        f, n = self.flat, self.flat.n_train
        K.sqnorm_partials(f.grads, n, st["partials"])
        marks = (5, 10)                           # the two arguments that move from step to step: lr, step
        if st.get("type", "AdamW") == "SGD":
            K.sgd_step(f.params, f.grads, st["buf"], n, lr, st["momentum"], st["dampening"], st["wd"], st["nesterov"],
                       self.step_count, st["max_norm"], grad_div, st["partials"], st["grad_norm"], st["runs"], st["nruns"])
            marks = (4, 9)
        elif st.get("runs") is not None:
            K.adamw_step_runs(f.params, f.grads, st["m"], st["v"], n, lr, st["betas"], st["eps"], st["wd"], self.step_count,
                              st["max_norm"], grad_div, st["partials"], st["grad_norm"], st["runs"], st["nruns"])
        else:
            K.adamw_step(f.params, f.grads, st["m"], st["v"], n, lr, st["betas"], st["eps"], st["wd"], self.step_count,
                         st["max_norm"], grad_div, st["partials"], st["grad_norm"])
        if _lib.TAPE is not None:
            _lib.TAPE.mark("lr", marks[0])
            _lib.TAPE.mark("step", marks[1])
        self.engine.params_changed()              # the kernel wrote the arena behind torch's back: fold again next step

    _acc = None             # the accumulation arena (train_step(accumulate=...)): same layout as the gradient arena

    # ------------------------------------------------------------------ weight EMA (mmcv's EMAHook)
    ema_state = None        # dict(ema, momentum, interval, warm_up, swapped) once init_ema() was called

    def init_ema(self, momentum=0.0002, interval=1, warm_up=100):
        """Exponential moving average of the trainable arena, mmcv 1.3.18's EMAHook restated: the EMA arena has the layout of
        `flat.params` and starts as a copy of it; train_step(..., ema_iter=it) then runs, for every iteration with
        it % interval == 0, ema = ema * (1 - m) + m * param with m = ema_momentum(...).  Frozen parameters and buffers (BN
        running statistics) are not averaged.  Call it on every rank, once the parameters are what training starts from; a
        later apis.load_checkpoint(..., runtime=) takes the file's EMA, or restarts it from the loaded parameters, and
        sync_replicas() broadcasts the arena with the others."""
        if not 0.0 < momentum < 1.0:
            raise ValueError(f"EMA momentum must lie in (0, 1), got {momentum!r}")
        if not (isinstance(interval, int) and not isinstance(interval, bool) and interval > 0):
            raise ValueError(f"EMA interval must be a positive int, got {interval!r}")
        self.ema_state = dict(ema=self.flat.params.clone(), momentum=float(momentum), interval=interval,
                              warm_up=warm_up, swapped=False)
        return self.ema_state

    def swap_ema(self):
        """Exchange the parameter arena and the EMA arena (one launch): the model's parameters are then the averaged weights
        and `ema_state['ema']` holds the raw ones, until the next call puts both back bit for bit."""
        st = self.ema_state
        if st is None:
            raise RuntimeError("swap_ema() without init_ema(): this runtime keeps no EMA")
        K.ema_swap(self.flat.params, st["ema"], self.flat.n_train)
        st["swapped"] = not st["swapped"]
        self.engine.params_changed()              # the kernel wrote the arena behind torch's back: fold again next pass

    @contextlib.contextmanager
    def ema_weights(self):
        """`with rt.ema_weights():` -- the block sees the EMA weights as the parameters; the raw weights are back after it"""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def _ema_update(self, it):
        """The EMA update of iteration `it`, if it fires: one eager launch on the current stream behind the step (taped or
        not: it is never recorded, so both give the same bits and the tapes hold what they held without an EMA)."""
        st = self.ema_state
        if st is None or it is None or it % st["interval"]:
            return
        if st["swapped"]:
            raise RuntimeError("train_step with the EMA weights swapped in: call swap_ema() again first")
        K.ema_update(st["ema"], self.flat.params, self.flat.n_train, ema_momentum(it, st["momentum"], st["interval"], st["warm_up"]))

    def bf16_buckets(self):
        """Gradient buckets travel as bf16 (fp32 arena -> bf16 staging -> all-reduce -> back) by default in the bf16-STORAGE
        mode only: its step is half as long as the fp32 one while the fp32 exchange (127.7 MB per step, ~1.5 ms of per-link
        ring time on xGMI) stays the same, so the exchange is twice as exposed there; the mode's activation
        gradients are bf16 already, and the reference's fp16 training (apis/train.py:113-117) all-reduces half-precision
        gradients as well.  fp32 and the bf16-math mode (fp32 tensors) keep fp32 buckets.  RADET_BF16_BUCKETS=0 / 1 overrides."""
        env = os.environ.get("RADET_BF16_BUCKETS")
        if env is not None:
            return env == "1" and self.engine.math_name != "fp32"
        return self.engine.math_name == "bf16-storage"

    def comm_report(self):
        """Diagnostics of the traced steps since reducer.enable_trace() (averaged), times in ms after the start of the
        backward pass: per bucket `ready` (handed to RCCL: its slab reduction finished on the side stream), `allreduce_ms`
        (start-to-end time of the collective: HIP events around it on the communication stream, or RCCL's own timing with
        TORCH_NCCL_ENABLE_TIMING=1 when the process group's internal stream is used) and `done_by` (the main stream saw it complete in
        finish(): an upper bound, exact for the bucket that is waited for); `exposed_comm_ms` = how long the main stream
        waits for the exchange after its last backward kernel -- what clip + AdamW pays.  Host-synchronising: call it after
        the steps, not between them."""
        tr = self.reducer.trace if self.reducer is not None else None
        marks = self.__dict__.get("comm_marks")
        if not tr or not marks:
            return None
        torch.cuda.synchronize()
        n, lo = len(marks), 0
        acc = None
        fwd = bwd = exposed = 0.0
        for ev_b, ev0, ev1, hi in marks:
            step = tr[lo:hi]
            lo = hi
            def dur(w):                          # RCCL's own timing of the collective (TORCH_NCCL_ENABLE_TIMING=1), else -1
                try:
                    return float(w._get_duration())
                except Exception:
                    return -1.0
            rows = [(t["prefix"], t["bytes"], ev0.elapsed_time(t["ready"]), ev0.elapsed_time(t["done"]), dur(t["work"])) for t in step]
            b = ev0.elapsed_time(ev1)
            fwd += ev_b.elapsed_time(ev0); bwd += b
            exposed += max(0.0, max((r[3] for r in rows), default=0.0) - b)     # (a traced step may have handed over no bucket)
            acc = rows if acc is None else [(a[0], a[1], a[2] + r[2], a[3] + r[3], a[4] + r[4]) for a, r in zip(acc, rows)]
        rep = dict(steps=n, forward_loss_ms=round(fwd / n, 3), backward_ms=round(bwd / n, 3),
                   exposed_comm_ms=round(exposed / n, 3), bf16_buckets=bool(self.reducer.bf16),
                   buckets=[dict(bucket=a[0], mbytes=round(a[1] / 1e6, 2), ready_ms=round(a[2] / n, 3), done_by_ms=round(a[3] / n, 3),
                                 allreduce_ms=(round(a[4] / n, 3) if a[4] >= 0 else None)) for a in acc])
        self.reducer.trace.clear()
        self.comm_marks.clear()
        return rep

    # ------------------------------------------------------------------ data-parallel train step
    # ------------------------------------------------------------------ launch tape (radet_amd/tape.py)
    # RADET_TAPE=1 (default): once a train step has run `tape_after` times with the same geometry / mode, the next one is
    # recorded (every C-ABI call and cross-stream event operation it issues) and the steps after that are REPLAYED by one C
    # call per segment -- the same calls on the same streams, bit-identical results, ~5x less host time per step.
    # RADET_TAPE=0: always the eager step.  A step falls back to eager (and drops the tape) whenever something the tape baked
    # in has moved: another geometry plan, re-folded frozen weights, a changed optimizer hyper-parameter, tracing / per-kernel
    # timing switched on, a prefetch hand-over (next_img).
    tape_mode = os.environ.get("RADET_TAPE", "1")
    tape_after = int(os.environ.get("RADET_TAPE_AFTER", "2"))

    def _tape_key(self, img, tg, world, use_reducer, phase="plain", k=1):
        e, st = self.engine, self.opt_state
        opt = (st.get("type", "AdamW"), st.get("betas"), st.get("eps"), st.get("momentum"), st.get("dampening"), st.get("nesterov"),
               None if st.get("runs") is None else st["runs"].data_ptr(), st.get("nruns", 0))
        state = st["m"] if st.get("m") is not None else st.get("buf")
        return (e.geo_key, getattr(e, "plan_id", None), tuple(img.shape), img.dtype, tuple(tg["p2g"].shape), int(tg["off"].numel()),
                world, use_reducer, self.loss_weights is None or self.loss_weights.data_ptr(),
                opt, st["wd"], st["max_norm"], None if state is None else state.data_ptr(), e.wgrad_streams, e.use_streams,
                tuple(sorted(self.loss_hparams.items())) if self.loss_hparams else None,
                phase, k, None if self._acc is None else self._acc.data_ptr())

    # One tape slot per PHASE of an accumulated step -- "plain" (no accumulation; `_tape`), "first", "middle", "last": the
    # phases alternate, and a single slot would be reset by every call and never replay.
    _tape = None            # dict(key, count, tape, failed) of the plain step
    _acc_tapes = None       # phase -> the same, for the micro-steps of an accumulated step

    def _slot(self, phase):
        return self._tape if phase == "plain" else (self._acc_tapes or {}).get(phase)

    def _new_slot(self, phase, key):
        st = dict(key=key, count=0, tape=None, failed=None)
        if phase == "plain":
            self._tape = st
        else:
            if self._acc_tapes is None:
                self._acc_tapes = {}
            self._acc_tapes[phase] = st
        return st

    def drop_tape(self):
        self._tape = None
        self._acc_tapes = None

    def tape_stats(self, phase="plain"):
        t = (self._slot(phase) or {}).get("tape")
        return None if t is None else dict(t.stats(), replays=t.replays)

    @staticmethod
    def _phase(accumulate):
        """accumulate = (j, k): micro-step j of k -> (phase, k); None or k = 1 is the plain step"""
        if accumulate is None:
            return "plain", 1
        j, k = (int(x) for x in accumulate)
        if k < 1 or not 0 <= j < k:
            raise ValueError(f"accumulate=(j, k) needs 0 <= j < k, got {accumulate}")
        if k == 1:
            return "plain", 1
        return ("first" if j == 0 else "last" if j == k - 1 else "middle"), k

    def train_step(self, img, tg, lr=None, next_img=None, accumulate=None, ema_iter=None):
        """One optimisation step. With torch.distributed initialised (backend nccl = RCCL) gradients
        are summed across ranks per bucket on a side stream while the backward of earlier layers is
        still running; the mean (1/world) is folded into the fused clip+AdamW kernel.
        next_img: the batch of the NEXT call, if it is already on the device (a data loader one batch ahead): the frozen part
        of its forward pass (stem + frozen stages, `frozen_stages` of resnet.py:572-588) is then computed during this step's
        backward pass and picked up by the next call when it is given the same tensor; results are bit-identical to calls
        without it.
        accumulate=(j, k): micro-step j of a step accumulated over k batches (mmcv's GradientCumulativeOptimizerHook).  The
        gradient arena is overwritten by every backward pass, so the sum lives in a second arena: micro-step 0 copies the
        (exchanged) gradients there, the following ones add theirs, and the last one writes sum + its own back into the
        gradient arena and runs the optimizer with grad_div = world * k -- the mean over ranks and micro-batches, folded
        into the fused kernel.  Only the last micro-step moves the parameters and `step_count`; `lr` is used by it alone.
        None, or k = 1, is the plain step.
        ema_iter: the iteration number (0-based, counted like mmcv's runner.iter) when init_ema() was called: the EMA update
        of that iteration follows the step on the same stream -- behind the optimizer kernel, or at the end of a micro-step
        that moved nothing (mmcv's hook fires on every iteration), and in front of the next step's weight fold.  It is one
        eager launch outside the tape.  None, or no init_ema(): the step issues what it issued before.
        Steady-state calls are replayed from a launch tape (see above); results are bit-identical to the eager step."""
        phase, k = self._phase(accumulate)
        if phase != "plain" and self._acc is None:
            self._acc = torch.zeros_like(self.flat.grads)
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # a 1-rank process group still exercises the bucketed exchange when forced (single-GPU test of the RCCL path)
        use_reducer = world > 1 or (world == 1 and dist.is_available() and dist.is_initialized()
                                    and os.environ.get("RADET_FORCE_REDUCER") == "1")
        e = self.engine
        record = None
        tapeable = (self.tape_mode != "0" and next_img is None and K.EVENTS is None and e.tower_events is None
                    and not (self.reducer is not None and self.reducer.trace is not None) and e._pfx_ready is None
                    and img is not None and img.is_cuda and img.dtype == torch.float32 and img.is_contiguous()
                    and self.opt_state is not None and "partials" in self.opt_state
                    and all(tg[k].is_contiguous() for k in ("boxes", "labels", "off", "p2g", "pw")))
        if tapeable:
            if phase != "plain":
                # the key names the engine's plan: have it built before the key is taken, so that the phase that opens a
                # run ("first") counts from its first call like the phases behind it (forward() finds the plan prepared)
                e.prepare(img.shape[0], img.shape[2], img.shape[3])
            key = self._tape_key(img, tg, world, use_reducer, phase, k)
            st = self._slot(phase)
            if st is None or st["key"] != key:
                st = self._new_slot(phase, key)
            if st["tape"] is not None:
                if self._tape_still_valid(phase):
                    out = self._replay_step(st["tape"], img, tg, lr, world, phase)
                    self._ema_update(ema_iter)
                    return out
                st = self._new_slot(phase, key)                                       # something moved: start over
            st["count"] += 1
            if st["count"] > self.tape_after and st["failed"] is None and (not use_reducer or self.reducer is not None):
                from .tape import Tape
                record = Tape()
        if self.reducer is not None and self.reducer.trace is not None:
            self._ev_begin = torch.cuda.Event(enable_timing=True)
            self._ev_begin.record()
        if record is not None:
            torch.cuda.current_stream().synchronize()     # (recording compares allocator counters: nothing of ours in flight)
            record.begin(self.dev)
        try:
            self.forward(img)
            self.loss(tg, grad_scale=self.loss_weights)
            if use_reducer:
                if self.reducer is None:
                    on_chain = self.engine.use_streams and self.flat.grads.is_cuda
                    if on_chain and not sync_collectives_run_on_current_stream():
                        # the process group's internal stream will carry the exchange: keep the process at four streams by
                        # giving up the second weight-gradient stream (10.43 instead of 9.97 ms at one rank)
                        import warnings
                        warnings.warn(f"torch {torch.__version__} runs synchronous collectives on the process group's own stream: "
                                      "the gradient exchange uses that stream and the engine drops its second weight-gradient "
                                      "stream to stay inside the four-stream budget of this device")
                        on_chain = False
                        self.engine.wgrad_streams = 1
                    self.reducer = GradReducer(self.flat.grads, self.dev, bf16=self.bf16_buckets(),
                                               comm_stream=self.engine._chain_stream() if on_chain else None)
                tr = self.reducer.trace is not None
                if tr:
                    ev0 = torch.cuda.Event(enable_timing=True)
                    ev0.record()                     # (after forward + loss: the exchange can only overlap the backward pass)
                self.backward(self.reducer.bucket_ready, next_img=next_img)
                if tr:
                    ev1 = torch.cuda.Event(enable_timing=True)
                    ev1.record()                     # end of the backward pass on the main stream
                    self.__dict__.setdefault("comm_marks", []).append((self._ev_begin, ev0, ev1, len(self.reducer.trace)))
                if record is not None:
                    record.run_cut(self.reducer.finish, None)     # (un-recorded: the replayed step calls it at this cut)
                else:
                    self.reducer.finish()
            else:
                self.backward(next_img=next_img)
            if phase in ("first", "middle"):
                K.grad_accumulate(self._acc, self.flat.grads, self.flat.n_train,
                                  K.GRAD_ACC_SET if phase == "first" else K.GRAD_ACC_ADD)
            else:
                if phase == "last":
                    K.grad_accumulate(self._acc, self.flat.grads, self.flat.n_train, K.GRAD_ACC_RESTORE)
                self.optimizer_step(lr=lr, grad_div=float(world * k))
        except BaseException:
            if record is not None:
                record.abort()
            raise
        if record is not None:
            record.end()
            st = self._slot(phase)
            # steady state: the frozen weights are not folded; the trainable ones are folded by the steps that follow an
            # optimizer step (plain, first) and by no other (middle, last: the parameters have not moved since)
            if record.poisoned is None and (e._last_fold != (False, phase in ("plain", "first")) or e._pfx_ready is not None):
                record.poisoned = "the recorded step was not a steady-state step (its weight folds are not the phase's)"
            if record.poisoned is None:
                record.bind("img", img)
                for k in ("boxes", "labels", "off", "p2g", "pw"):
                    record.bind(k, tg[k])
                st["tape"] = record
                st["nf"] = e._frozen_conv_count()
            else:
                st["failed"] = record.poisoned
                if os.environ.get("RADET_TAPE_STRICT") == "1":
                    raise _lib.RadetHipError(f"launch tape could not be recorded: {record.poisoned}")
        self._ema_update(ema_iter)
        if self.loss_weights is not None:       # reported values carry the configured loss weights, like the reference's
            return self.engine.losses * self.loss_weights
        return self.engine.losses

    def _trainable_version(self, nf):
        e = self.engine
        return e._part_version(nf, len(e.convs)) + (e._param_epoch,)

    def _tape_still_valid(self, phase="plain"):
        """what a recorded step baked in beyond its key: the frozen convs' folded weights (folded outside the tape whenever
        their sources move), the arenas the module's parameters view and -- for the micro-steps that hold no fold of the
        trainable weights (middle, last) -- that those folded weights are still the parameters' """
        e, st = self.engine, self._slot(phase)
        nf = st["nf"]
        if nf > 0 and e._part_version(0, nf) != e._folded[0]:
            return False
        if phase in ("middle", "last") and self._trainable_version(nf) != e._folded[1]:
            return False
        return self.flat.still_bound() and _lib.TAPE is None

    def _replay_step(self, tape, img, tg, lr, world, phase="plain"):
        e, st = self.engine, self.opt_state
        tensors = dict(img=img, boxes=tg["boxes"], labels=tg["labels"], off=tg["off"], p2g=tg["p2g"], pw=tg["pw"])
        if phase in ("first", "middle"):          # no optimizer call on these tapes: nothing to patch, no parameter moves
            tape.replay(tensors=tensors)
            if phase == "first":                  # (the tape folded the trainable weights: they are current now)
                e._folded = (e._folded[0], self._trainable_version(self._slot(phase)["nf"]))
            return e.losses * self.loss_weights if self.loss_weights is not None else e.losses
        self.step_count += 1
        tape.replay(tensors=tensors, values=dict(lr=st["lr"] if lr is None else lr, step=self.step_count))
        e.params_changed()
        if self.loss_weights is not None:
            return e.losses * self.loss_weights
        return e.losses


# ---------------------------------------------------------------------- autograd bridge (drop-in API)
class _DetectorLossFn(torch.autograd.Function):
    """losses = f(img, params): forward = engine forward + fused loss; backward = the engine's reverse
    program. Gradients come back as clones of the gradient-arena views (autograd accumulates them)."""

    @staticmethod
    def forward(ctx, rt, img, tg, weights, *params):
        rt.forward(img)
        losses = rt.loss(tg)
        ctx.rt, ctx.tg, ctx.weights = rt, tg, weights
        out = losses * weights
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g0, g1, g2):
        rt = ctx.rt
        gs = (torch.stack([g0.reshape(()), g1.reshape(()), g2.reshape(())]).float() * ctx.weights).contiguous()
        rt.loss(ctx.tg, grad_scale=gs)       # head-output gradients scaled by the upstream gradients
        rt.backward()
        grads = tuple(rt.flat.g[n].clone() for n in rt.flat.train_names)
        return (None, None, None, None) + grads


def _losses_autograd(self, img, gt_bboxes, gt_labels, points_to_gt_index, points_weight):
    det = self.owner()
    head = det.bbox_head
    tg = self.pack_targets(gt_bboxes, gt_labels, points_to_gt_index, points_weight)
    self.set_loss_from_head(head)
    weights = torch.tensor([head.loss_cls.loss_weight, 1.0, head.loss_iou.loss_weight], device=self.dev)
    named = dict(det.named_parameters())
    plist = [named[n] for n in self.flat.train_names]
    l0, l1, l2 = _DetectorLossFn.apply(self, img.to(self.dev), tg, weights, *plist)
    return dict(loss_cls=l0, loss_bbox=l1, loss_iou=l2)


DetectorRuntime.losses_autograd = _losses_autograd


def owner_runtime(module):
    ref = getattr(module, "_owner_ref", None)
    det = ref() if ref is not None else None
    if det is None:
        raise RuntimeError(f"{type(module).__name__} executes through its detector's MI355X runtime: build the "
                           "detector with build_detector(cfg).cuda() and call it (or detector.extract_feat)")
    return det.runtime()


def standalone_forward(module, part, x):
    rt = owner_runtime(module)
    if part == "backbone":
        return rt.backbone_api(x)
    return rt.neck_api(x)


def _neck_api(self, inputs):
    """inputs: NCHW C2..C5 (as returned by the backbone module). Returns NCHW P3..P7."""
    with torch.no_grad():
        e = self.engine
        B = inputs[0].shape[0]
        feats = [None]
        for i, x in enumerate(inputs[1:]):
            blk = e.stages[i + 1][-1]
            rows = e.buf[f"l{i + 2}.{len(e.stages[i + 1]) - 1}.out"]
            K.nchw_to_nhwc(x.to(self.dev).contiguous(), rows, B, x.shape[1], x.shape[2], x.shape[3])
            feats.append(rows)
            del blk
        P = e.neck_forward(feats)
        return tuple(_rows_to_nchw(self, P, e.plv, e.feat))


DetectorRuntime.neck_api = _neck_api


# ---------------------------------------------------------------------- inference + module-level API
def _detect(self, img, img_metas, test_cfg, rescale=False, crops=None):
    """simple_test: forward -> per-level threshold/top-k/decode -> NMS, all on the GPU, batched over
    images; returns [(dets f32[K,5], labels i64[K])] per image on the device.  crops = (CropSpec, frame descriptor table):
    the RoI crops of the detections are cut from the batch's frames behind NMS (two more launches, the same stream, their
    counters in the counts' own device-to-host copy); returns (that list, ops.crops.Crops of the batch, ends i32 [B] on the
    host: frame b's crops are [ends[b - 1], ends[b]) of the batch's -- ops.crops.split_crops)."""
    with torch.no_grad():
        self.forward(img.to(self.dev))
        hw, sf = _meta_tensors(self, img_metas, rescale)
        B = len(img_metas)
        outs, counts, job = _launch_with_crops(self, B, crops, lambda c: _post_launch(self, hw, sf, test_cfg, counts_out=c))
        return _finish(self, outs, job, B, counts.cpu().numpy())


def _launch_with_crops(self, B, crops, launch):
    """launch(counts_out) -> the NMS outputs of a batch of B images, and with crops = (CropSpec, descriptor table) the two crop
    launches behind it on the current stream.  -> (outs, counts, job): counts is what the host needs of the batch in ONE
    device-to-host copy -- the detection counts [B], with crops followed by the crop plan's counters: n_out | n_total | where
    each frame's rows end [B]; job: the crops' (images, rows), or None"""
    if crops is None:
        outs = launch(None)
        return outs, outs[3], None
    from .ops.crops import launch_crops
    spec, desc = crops
    counts = torch.zeros(B + 2 + B, dtype=torch.int32, device=self.dev)
    outs = launch(counts)
    ob, osc, _, oc = outs
    k = int(ob.shape[1])
    cap = spec.max_crops if spec.max_crops is not None else B * k
    if cap > K.CROP_MAX_SLOTS:
        raise ValueError(f"crops: {B} x {k} detection slots exceed the kernel's {K.CROP_MAX_SLOTS}; pass max_crops")
    return outs, counts, launch_crops(spec, ob, osc, oc, desc, cap, counts[B:])


def _finish(self, outs, job, B, host):
    """what a batch returns, from _launch_with_crops' outs and job and its counts on the host: the detections, or with crops
    (detections, Crops of the batch, ends [B])"""
    dets = _post_collect(self, *outs, counts=host)
    if job is None:
        return dets
    from .ops.crops import collect_crops
    return dets, collect_crops(job[0], job[1], host[B], host[B + 1]), host[B + 2:B + 2 + B].copy()


def _uploader(self, pinned):
    """ndarray -> device tensor: a blocking copy, or (pinned) through pinned memory without one, for the streams"""
    if pinned:
        return lambda a: torch.from_numpy(a).pin_memory().to(self.dev, non_blocking=True)
    return lambda a: torch.from_numpy(a).to(self.dev)


def _one_behind(self, batches, enqueue):
    """The loop of the three streams, the host one batch behind the device: enqueue(batch, fetch) puts a batch's whole device
    program on its streams and calls fetch(counts) where the counts are made -- the counts into pinned memory and the
    "arrived" event, on the current stream -- and returns (outs, job, B, pinned, done, whatever has to stay alive until the
    host has waited for the batch).  Batch k is handed out (_finish) once batch k + 1 is enqueued; the host waits for that
    batch's event only."""
    def fetch(counts):
        pinned = torch.empty(counts.shape, dtype=counts.dtype).pin_memory()
        pinned.copy_(counts, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        return pinned, done

    def collect(rec):
        outs, job, B, pinned, done = rec[:5]
        done.synchronize()                                      # the host waits for THIS batch only
        return _finish(self, outs, job, B, pinned.numpy())

    prev = None
    with torch.no_grad():
        for batch in batches:
            rec = enqueue(batch, fetch)
            if prev is not None:
                yield collect(prev)
            prev = rec
        if prev is not None:
            yield collect(prev)


def _detect_stream(self, batches, test_cfg, rescale=False, crops=None):
    """`detect` over an iterable of (img, img_metas) batches with the host one batch behind the device: batch k + 1's
    device program (forward, decode, NMS) is enqueued BEFORE the host waits for batch k's detection counts, so the GPU
    never idles on the per-batch hand-over (what the reference's `single_gpu_test` loop -- apis/test.py -- pays per batch
    as a device synchronisation).  Yields exactly what `detect` returns, in order.  The small per-batch uploads (image
    sizes, scale factors) go through pinned memory and the counts come back behind an event on the stream that produced
    them: nothing in the loop synchronises the main stream.  Decode + NMS of batch k (a dozen launches of a few workgroups each, ~0.3 ms at
    batch 8) run on a stream of their own NEXT TO the forward pass of batch k + 1: the head outputs alternate between two
    sets of buffers, and the forward pass that reuses a set first waits for the post-processing that read it.
    crops (an ops.crops.CropSpec): every batch is (img, img_metas, (descriptor table, frames)) and its RoI crops are cut behind
    its NMS on the same stream; yields (that list, Crops of the batch, ends) as `detect` returns them -- the plan's counters
    come with the counts in the pinned copy, so handing the crops out per frame reads nothing more from the device.  The
    batch's record holds the table (a view of the upload buffer) and the frames until the host has waited for the batch: the
    launches that read them run a batch behind."""
    # (no stream of its own: a process should not create more than four HIP streams on this device -- engine.py, "stream
    # budget" -- and the training step's tower-chain stream is idle here: the inference pass runs its reg chain on `side`)
    post = self.engine._chain_stream()
    overlap = os.environ.get("RADET_POST_OVERLAP", "1") != "0"
    HEAD_OUT = ("cls", "reg_u", "iou")
    alts = {}                    # id(plan) -> (plan, the other set of head-output buffers)
    post_ev = [None, None]       # events "decode / NMS done" of the batch before last and of the last batch

    def post_launch(hw, sf, src):       # decode + NMS, and the batch's crops behind them: -> (outs, what fetch copies, job)
        return _launch_with_crops(self, hw.shape[0], None if crops is None else (crops, src[0]),
                                  lambda c: _post_launch(self, hw, sf, test_cfg, counts_out=c))

    swapped = {}                 # id(plan) -> the plan currently holds its second set

    def enqueue(batch, fetch):
        img, img_metas = batch[:2]
        src = batch[2] if crops is not None else None
        hw, sf = _meta_tensors(self, img_metas, rescale, _uploader(self, True))
        img = img.to(self.dev, non_blocking=True)
        if overlap:
            e = self.engine
            e.prepare(img.shape[0], img.shape[2], img.shape[3])
            plan = e.buf
            if id(plan) not in alts or alts[id(plan)][0] is not plan:
                alts[id(plan)] = (plan, {k: torch.empty_like(plan[k]) for k in HEAD_OUT})
            other = alts[id(plan)][1]
            for k in HEAD_OUT:                               # this batch writes the set the batch before last wrote
                plan[k], other[k] = other[k], plan[k]
            swapped[id(plan)] = not swapped.get(id(plan), False)
            if post_ev[0] is not None:
                torch.cuda.current_stream().wait_event(post_ev[0])   # ... once that batch's decode / NMS have read it
            self.forward(img)
            fwd = torch.cuda.Event()
            fwd.record()
            with torch.cuda.stream(post):
                post.wait_event(fwd)
                outs, counts, job = post_launch(hw, sf, src)
                ev = torch.cuda.Event()
                ev.record()
                pinned, done = fetch(counts)
            if job is not None:                             # (the crops and their rows are read on the caller's
                for t in job:                               # stream next: their memory returns to this one's pool)
                    t.record_stream(torch.cuda.current_stream())
            post_ev[0], post_ev[1] = post_ev[1], ev
        else:
            self.forward(img)
            outs, counts, job = post_launch(hw, sf, src)
            ev = torch.cuda.Event()
            ev.record()
            with torch.cuda.stream(post):                   # (the copy must not queue behind the next batch's forward pass)
                post.wait_event(ev)
                pinned, done = fetch(counts)
        # (the size / scale tensors stay alive until the batch's decode has run, the frames and their table until its crops have)
        return outs, job, hw.shape[0], pinned, done, (hw, sf), src

    try:
        yield from _one_behind(self, batches, enqueue)
    finally:
        # leave every plan with its own set (captured graphs and the training step hold pointers to it).  After a complete
        # run collect() has host-synchronised the last batch; an abandoned generator (break / exception mid-iteration) can
        # still have a batch's decode / NMS reading the head outputs and the shared post-processing workspaces on the chain
        # stream: whatever the caller enqueues next on this stream waits for it
        for ev in post_ev:
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
        for pid, odd in swapped.items():
            if odd and pid in alts:
                plan, other = alts[pid]
                for k in HEAD_OUT:
                    plan[k], other[k] = other[k], plan[k]


def _rows_hw_sf(metas, with_sf=True):
    """the metas of a list of rows on the host: img_shape's (h, w) f32 [R, 2] and, asked for, scale_factor f32 [R, 4]"""
    hw = np.empty((len(metas), 2), np.float32)
    sf = np.empty((len(metas), 4), np.float32) if with_sf else None
    for r, m in enumerate(metas):
        hw[r] = m["img_shape"][:2]
        if with_sf:
            sf[r] = np.asarray(m["scale_factor"], np.float32).reshape(4)
    return hw, sf


def _meta_tensors(self, img_metas, rescale, upload=None):
    upload = upload or _uploader(self, False)
    hw, sf = _rows_hw_sf(img_metas, rescale)
    return upload(hw), (upload(sf) if rescale else None)


def _post_launch(self, hw, sf, test_cfg, head_out=None, counts_out=None):
    """Device part of the post-processing (no host synchronisation, no host->device copies: capturable in a hipGraph):
    decode + NMS launches on the engine's head outputs (or on `head_out` = dict(cls, reg, iou, scales, ldesc, nlvl, B,
    level_hw) row buffers handed in through the module API).  Returns the output tensors (boxes, scores, labels, counts);
    counts_out: a zeroed i32 tensor whose first B entries become `counts` (a caller that copies more words with them)."""
    ho = _head_out(self, head_out)
    B, nlvl = ho["B"], ho["nlvl"]
    nms_pre = _nms_pre(self, test_cfg, ho["level_hw"])
    cap = nlvl * nms_pre
    if cap > 65536:
        raise NotImplementedError(f"nms_pre={nms_pre}: more than 65536 candidates per image exceed the NMS kernel's 16-bit positions")
    soft = dict(test_cfg["nms"]).get("type") == "soft_nms"
    p = _post_ws(self, ("post", B, nlvl, nms_pre) + (("soft",) if soft else ()), B, cap, soft, K.decode_ws_bytes(B, nlvl, nms_pre),
                 f"batch {B} with nms_pre={nms_pre}")
    K.decode_candidates(ho["cls"], ho["reg"], ho["iou"], ho["scales"], ho["ldesc"], nlvl, B, self.num_classes,
                        float(test_cfg["score_thr"]), nms_pre, hw, sf, p["boxes"], p["scores"], p["ctr"], p["labels"],
                        p["count"], p["dws"])
    return _nms_launch(self, p, B, cap, test_cfg, counts_out)


def _head_out(self, head_out=None):
    e = self.engine
    if head_out is None:
        head_out = dict(cls=e.buf["cls"], reg=e.buf["reg_u"], iou=e.buf["iou"], scales=e.scales_tensor(), ldesc=e.ldesc,
                        nlvl=e.nlvl, B=e.B, level_hw=e.plv.hw)
    return head_out


def _nms_pre(self, test_cfg, level_hw):
    nms_pre = int(test_cfg.get("nms_pre", -1))
    if nms_pre <= 0:
        nms_pre = max(h * w for h, w in level_hw) * self.num_classes
    return nms_pre


def _post_ws(self, key, B, cap, soft, extra_bytes, what, pool=0, counters=None):
    """The cached buffers of one post-processing geometry: the candidate lists [B, cap] the NMS reads, its workspace, and
    `extra_bytes` of decode workspace (dws); pool > 0 (test-time augmentation, tiles): the rows' candidate pool of that many
    entries in front of them, with the zeroed i32 buffers of `counters` (name -> length: the per-row counts, the merge's
    own).  The limit (RADET_POST_WS_LIMIT_GB) is checked on cap, the capacity the NMS sees."""
    posts = self.__dict__.setdefault("_posts", {})
    if key not in posts:
        # the NMS workspace holds a dense cap x cap / 64 x 8 B suppression mask per image (+ sort keys): 7 MiB per image at
        # the BOP configs' nms_pre = 1000, ~310 MB at nms_pre = 10000, 512 MiB at the 65536-candidate limit
        need = (K.soft_nms_ws_bytes if soft else K.nms_ws_bytes)(B, cap) + extra_bytes + 32 * pool
        limit = int(float(os.environ.get("RADET_POST_WS_LIMIT_GB", "16")) * 2 ** 30)
        if need > limit:
            raise MemoryError(f"decode + NMS workspaces for {what} ({cap} candidates per image) need "
                              f"{need / 2 ** 30:.1f} GiB (dense suppression mask: cap^2 / 8 bytes per image); lower nms_pre or the "
                              f"batch, or raise RADET_POST_WS_LIMIT_GB (now {limit / 2 ** 30:.0f})")
        while posts and (len(posts) >= 8 or sum(v["nws"].numel() for v in posts.values()) + need > limit):
            posts.pop(next(iter(posts)))
        dev = self.dev
        posts[key] = dict(
            boxes=torch.empty(B, cap, 4, device=dev), scores=torch.empty(B, cap, device=dev),
            ctr=torch.empty(B, cap, device=dev), labels=torch.empty(B, cap, dtype=torch.long, device=dev),
            count=torch.zeros(B, dtype=torch.int32, device=dev), cscore=torch.empty(B, cap, device=dev),
            dws=torch.empty(extra_bytes, dtype=torch.uint8, device=dev),
            nws=torch.empty((K.soft_nms_ws_bytes if soft else K.nms_ws_bytes)(B, cap), dtype=torch.uint8, device=dev))
        if not soft:
            posts[key].update(aux0=torch.zeros(B, cap, dtype=torch.long, device=dev),
                              aux1=torch.zeros(B, cap, dtype=torch.long, device=dev))
        if pool:
            posts[key].update(pool_boxes=torch.empty(pool, 4, device=dev), pool_scores=torch.empty(pool, device=dev),
                              pool_ctr=torch.empty(pool, device=dev), pool_labels=torch.empty(pool, dtype=torch.long, device=dev))
        for name, n in (counters or {}).items():
            posts[key][name] = torch.zeros(n, dtype=torch.int32, device=dev)
    return posts[key]


def _nms_launch(self, p, B, cap, test_cfg, counts_out=None):
    """The NMS half of the post-processing, shared by the single-view path and test-time augmentation: the config's NMS
    (vote / global_vote / nms / soft_nms) over the candidate lists p[boxes, scores, ctr, labels, count] of capacity cap, and
    max_per_img.  Returns (boxes, scores, labels, counts)."""
    ncfg = dict(test_cfg["nms"])
    typ = ncfg.get("type")
    soft = typ == "soft_nms"          # Soft-NMS has a workspace of its own (24 B per candidate): no dense mask, no aux rows
    max_per_img = int(test_cfg.get("max_per_img", 100))
    k = max_per_img if max_per_img > 0 else cap
    ob = torch.zeros(B, k, 4, device=self.dev)
    osc = torch.zeros(B, k, device=self.dev)
    ol = torch.zeros(B, k, dtype=torch.long, device=self.dev)
    oc = torch.zeros(B, dtype=torch.int32, device=self.dev) if counts_out is None else counts_out[:B]
    if typ in ("vote", "global_vote"):
        ctype, vtype = ncfg.get("cluster_score", "cls"), ncfg.get("vote_score", "iou")
        prod = None

        def pick(t):
            nonlocal prod
            if isinstance(t, (list, tuple)):
                if prod is None:
                    prod = p["cscore"]
                    torch.mul(p["scores"], p["ctr"], out=prod)   # elementwise product of two sigmoid outputs (plumbing)
                return prod
            return p["scores"] if t == "cls" else p["ctr"]
        K.nms(p["boxes"], pick(ctype), pick(vtype), p["labels"], p["count"], B, cap, K.NMS_MODES[typ],
              float(ncfg.get("iou_threshold", 0.6)), bool(ncfg.get("iou_enable", False)), float(ncfg.get("sigma", 0.025)),
              max_per_img, ob, osc, ol, oc, p["aux0"], p["aux1"], p["nws"])
    elif soft:
        from .ops import _soft_args
        method = _soft_args(ncfg.get("iou_threshold", 0.3), ncfg.get("sigma", 0.5), ncfg.get("min_score", 1e-3),
                            ncfg.get("method", "linear"), ncfg.get("offset", 0))
        torch.mul(p["scores"], p["ctr"], out=p["cscore"])
        keep = torch.zeros(B, k, dtype=torch.long, device=self.dev)
        K.soft_nms(p["boxes"], p["cscore"], p["labels"], p["count"], B, cap, method, float(ncfg.get("iou_threshold", 0.3)),
                   float(ncfg.get("sigma", 0.5)), float(ncfg.get("min_score", 1e-3)), bool(ncfg.get("class_agnostic", False)),
                   k, ob, osc, ol, keep, oc, p["nws"])
    else:
        torch.mul(p["scores"], p["ctr"], out=p["cscore"])
        K.nms(p["boxes"], p["cscore"], p["cscore"], p["labels"], p["count"], B, cap, 3,
              float(ncfg.get("iou_threshold", 0.5)), False, 0.0, k, ob, osc, ol, oc, p["aux0"], p["aux1"], p["nws"])
    return ob, osc, ol, oc


def _post_collect(self, ob, osc, ol, oc, counts=None):
    """counts: the first B words are oc's, already on the host"""
    counts = oc.cpu().numpy() if counts is None else counts
    out = []
    for i in range(ob.shape[0]):
        kk = int(counts[i])
        out.append((torch.cat([ob[i, :kk], osc[i, :kk, None]], -1), ol[i, :kk]))
    return out


def _detect_graph(self, img, img_metas, test_cfg, rescale=False, crops=None):
    """`detect` with the whole device program (weight folding, ~110 conv / GroupNorm launches on two streams, decode,
    the NMS pipeline) captured once per (batch, image size, test_cfg) in a hipGraph and replayed: single-image
    serving is otherwise bound by the host's launch rate (3.2 ms of Python + ctypes enqueue for ~1.7 ms of GPU work
    at batch 1).  Inputs are copied into the graph's static buffers; results are read back like `detect`.  crops= is refused:
    the frames' addresses change from call to call and a captured launch holds the ones it was captured with."""
    if isinstance(img_metas, dict) and "row_start" in img_metas:
        raise NotImplementedError("detect_graph with a tile plan: tiled inference is not captured in a graph (the rows, their "
                                  "number and the frames' addresses are per call); use detect_tiles / detect_tiles_stream")
    if isinstance(img, (list, tuple)):
        if len(img) != 1:
            raise NotImplementedError(f"detect_graph with {len(img)} views: test-time augmentation is not captured in a graph; "
                                      "use detect_aug")
        img, img_metas = img[0], img_metas[0]
    if crops is not None:
        raise NotImplementedError("detect_graph(crops=...): RoI crops are not captured in the graph (the frames' addresses are "
                                  "per call); use detect / detect_stream, or ops.crop_detections on the graph's detections")
    with torch.no_grad():
        img = img.to(self.dev)
        key = (tuple(img.shape), bool(rescale), repr(sorted(dict(test_cfg).items(), key=str)))
        cache = self.__dict__.setdefault("_graphs", {})
        self.engine.prepare(img.shape[0], img.shape[2], img.shape[3])
        g = cache.get(key)
        if g is not None and g["plan"] is not self.engine.buf:    # the geometry plan was evicted and rebuilt: stale pointers
            g = None
        if g is None:
            hw, sf = _meta_tensors(self, img_metas, rescale)
            static_img = img.clone()
            for _ in range(2):                                  # warm-up: prepare(), autotune, lazy workspaces
                self.forward(static_img)
                _post_launch(self, hw, sf, test_cfg)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            cap_stream = self.engine._chain_stream()            # (an existing stream: see engine.py, "stream budget")
            K.splitk_ws_for(cap_stream)                         # allocate the stream's split-K workspace outside capture
            self.engine.invalidate_fold()                       # the weight fold is part of the graph: replays see
            with torch.cuda.graph(graph, stream=cap_stream):    # the parameters of the moment, like the eager path
                self.forward(static_img)
                outs = _post_launch(self, hw, sf, test_cfg)
            # the captured launches hold raw pointers into the decode / NMS workspaces: the record keeps them alive when
            # the `_posts` cache drops its reference
            # (... as do the head-output buffers: detect_stream alternates the plan's entries between two sets)
            g = cache[key] = dict(graph=graph, img=static_img, hw=hw, sf=sf, outs=outs, plan=self.engine.buf,
                                  keep=list(self.__dict__.get("_posts", {}).values())
                                  + [self.engine.buf[k] for k in ("cls", "reg_u", "iou")])
        else:
            hw, sf = _meta_tensors(self, img_metas, rescale)
            g["hw"].copy_(hw)
            if sf is not None:
                g["sf"].copy_(sf)
        g["img"].copy_(img)
        g["graph"].replay()
        return _post_collect(self, *g["outs"])


# ---------------------------------------------------------------------- test-time augmentation
def _level_hw(H, W):
    """the head's level sizes for an H x W input (the engine's own chain: stem 7/2/3, pool 3/2/1, three stride-2 stages,
    two stride-2 extra levels) -- known before any launch, for the capacity checks of detect_aug"""
    from .engine import conv_out_hw
    hw = conv_out_hw(*conv_out_hw(H, W, 7, 2, 3), 3, 2, 1)
    out = []
    for _ in range(5):
        hw = conv_out_hw(*hw, 3, 2, 1)
        out.append(hw)
    return out


def _view_groups(imgs):
    """consecutive views of one tensor shape: [(first view, one past the last)] -- each runs as one forward batch"""
    groups, v0 = [], 0
    for v in range(1, len(imgs) + 1):
        if v == len(imgs) or tuple(imgs[v].shape) != tuple(imgs[v0].shape):
            groups.append((v0, v))
            v0 = v
    return groups


def _stack_views(ts):
    """the views of a group as one batch: no copy when they are consecutive slices of one tensor (ImagePipeline writes a
    scale's views that way), else a concatenation"""
    if len(ts) == 1:
        return ts[0]
    t0 = ts[0]
    if all(t.is_contiguous() and t.untyped_storage().data_ptr() == t0.untyped_storage().data_ptr()
           and t.storage_offset() == t0.storage_offset() + i * t0.numel() for i, t in enumerate(ts)):
        return torch.empty(0, dtype=t0.dtype, device=t0.device).set_(t0.untyped_storage(), t0.storage_offset(),
                                                                     (len(ts) * t0.shape[0],) + tuple(t0.shape[1:]))
    return torch.cat(ts)


# _aug_plan and _tile_plan return one shape of record, a batch of B images as rows (views or tiles) for _rows_launch:
#   name, B, nlvl, hw [R, 2] (the rows' img_shape), groups [(first row, rows, nms_pre, cap, pool offset)]: the forward batches,
#   each decoded into its block of the candidate pool; cap_out: the merged list's capacity per image; pool: the pool's entries;
#   key, what, counters: the workspace's (_post_ws), counters its i32 buffers beside the pool; tables: the host arrays the
#   merge reads on the device; merge(p, tables on the device): the ONE merge launch; check_nms_pre: nms_pre follows from
#   test_cfg and the level sizes; split(imgs) -> the groups' tensors
def _check_pool(mode, cap_out, pool, rows, how=""):
    """the capacity rules of a merged batch: the NMS kernel's 16-bit positions, the pool's 31-bit offsets; rows() -> how the
    refusals describe the batch (the merged list's rows, the pool's)"""
    if cap_out > 65536:
        raise NotImplementedError(f"{mode} with {rows()[0]}: the merged list of {cap_out} candidates per image exceeds the NMS "
                                  f"kernel's 65536 (16-bit positions); lower nms_pre{how}")
    if pool >= 2 ** 31:
        raise NotImplementedError(f"{mode}: a candidate pool of {pool} entries ({rows()[1]}); lower nms_pre or the batch")


def _pool_args(p):
    return p["pool_boxes"], p["pool_scores"], p["pool_ctr"], p["pool_labels"], p["row_count"]


def _list_args(p):
    return p["boxes"], p["scores"], p["ctr"], p["labels"], p["count"]


def _aug_plan(self, imgs, img_metas, test_cfg):
    """Host part of detect_aug, before any launch: the checks, the groups of views, the pool layout and the merge descriptor.
    -> the row plan (above _check_pool; rows view-major, row v * B + b) with V and sf0 beside it"""
    V = len(imgs)
    if V != len(img_metas) or not 1 <= V <= K.TTA_MAX_VIEWS:
        raise ValueError(f"detect_aug: {V} views with {len(img_metas)} lists of metas (1..{K.TTA_MAX_VIEWS} views, one list each)")
    B = int(imgs[0].shape[0])
    for v in range(V):
        if int(imgs[v].shape[0]) != B or len(img_metas[v]) != B:
            raise ValueError(f"detect_aug: view {v} holds {int(imgs[v].shape[0])} images and {len(img_metas[v])} metas, view 0 "
                             f"{B}: every view is a view of the same batch")
    for b in range(B):
        shapes = {tuple(m[b]["ori_shape"]) for m in img_metas if "ori_shape" in m[b]}
        if len(shapes) > 1:
            raise ValueError(f"detect_aug: the views of image {b} disagree in ori_shape ({sorted(shapes)})")
    nlvl = len(self.engine.strides)
    views = _view_groups(imgs)
    groups, pool, cap_out = [], 0, 0
    hw, sf = _rows_hw_sf([m for metas in img_metas for m in metas])
    flips, starts, caps = (np.zeros(V * B, np.int32) for _ in range(3))
    for v0, v1 in views:
        nms_pre = _nms_pre(self, test_cfg, _level_hw(int(imgs[v0].shape[2]), int(imgs[v0].shape[3])))
        cap = nlvl * nms_pre
        groups.append((v0 * B, (v1 - v0) * B, nms_pre, cap, pool))
        for v in range(v0, v1):
            for b, m in enumerate(img_metas[v]):
                r = v * B + b
                direction = m.get("flip_direction") if m.get("flip") else None
                if direction not in K.FLIP_CODES:
                    raise ValueError(f"detect_aug: view {v} has flip_direction {direction!r}")
                flips[r], starts[r], caps[r] = K.FLIP_CODES[direction], pool + ((v - v0) * B + b) * cap, cap
        pool += (v1 - v0) * B * cap
        cap_out += (v1 - v0) * cap
    pres = sorted({g[2] for g in groups})
    _check_pool("test-time augmentation", cap_out, pool,
                lambda: (f"V={V} views, nlvl={nlvl} levels and nms_pre={pres}", f"batch {B}"))
    desc = K.merge_desc_rows(hw, sf, flips, starts, caps)

    def merge(p, tables):
        K.merge_views(desc, tables["desc"], V, B, *_pool_args(p), cap_out, *_list_args(p))

    def split(imgs):                    # a group's views as one forward batch
        return (_stack_views([t.to(self.dev) for t in imgs[v0:v1]]) for v0, v1 in views)
    return dict(name="detect_aug", B=B, nlvl=nlvl, hw=hw, groups=groups, cap_out=cap_out, pool=pool,
                key=("aug", B, tuple(g[:4] for g in groups)), what=f"batch {B} with {V} views, nlvl={nlvl}, nms_pre={pres}",
                counters=dict(row_count=V * B), tables=dict(desc=desc), merge=merge, check_nms_pre=True, split=split,
                V=V, sf0=sf[:B].copy())


def _rows_launch(self, batches, plan, test_cfg, upload, counts_out=None):
    """Device part of detect_aug and detect_tiles on the current stream: per forward group (batches yields their tensors) one
    forward pass and, behind it, one radet_decode_candidates into the group's block of the pool (row coordinates, clamped to
    the row's own img_shape -- a box that reaches past a tile lands exactly on its edge); the plan's ONE merge launch
    (radet_merge_views / radet_merge_tiles: map-back, stable compaction per image); the config's NMS over the merged lists
    (_nms_launch).  upload: ndarray -> device tensor.  Returns the NMS outputs, boxes in the frames' coordinates."""
    B, nlvl, cap_out = plan["B"], plan["nlvl"], plan["cap_out"]
    soft = dict(test_cfg["nms"]).get("type") == "soft_nms"
    dbytes = max(K.decode_ws_bytes(n, nlvl, pre) for _, n, pre, _, _ in plan["groups"])
    p = _post_ws(self, plan["key"] + (("soft",) if soft else ()), B, cap_out, soft, dbytes, plan["what"], pool=plan["pool"],
                 counters=plan["counters"])
    hw = upload(plan["hw"])
    tables = {k: upload(a) for k, a in plan["tables"].items()}
    for img, (r0, n, nms_pre, cap, off) in zip(batches, plan["groups"]):
        self.forward(img)
        ho = _head_out(self)
        if ho["B"] != n or ho["nlvl"] != nlvl or (plan["check_nms_pre"] and _nms_pre(self, test_cfg, ho["level_hw"]) != nms_pre):
            raise RuntimeError(f"{plan['name']}: the engine's level geometry differs from the planned one")
        K.decode_candidates(ho["cls"], ho["reg"], ho["iou"], ho["scales"], ho["ldesc"], nlvl, n, self.num_classes,
                            float(test_cfg["score_thr"]), nms_pre, hw[r0:r0 + n], None,
                            *(t[off:off + n * cap] for t in _pool_args(p)[:4]), p["row_count"][r0:r0 + n], p["dws"])
    plan["merge"](p, tables)
    return _nms_launch(self, p, B, cap_out, test_cfg, counts_out)


def _rows_batch(self, imgs, plan, test_cfg, pinned, crops):
    """a planned batch's whole device program: _rows_launch and, with crops, the crop launches -> _launch_with_crops' triple"""
    return _launch_with_crops(self, plan["B"], crops, lambda c: _rows_launch(self, plan["split"](imgs), plan, test_cfg,
                                                                             _uploader(self, pinned), c))


def _detect_aug(self, imgs, img_metas, test_cfg, rescale=False, crops=None):
    """aug_test: `detect` over several views of one batch (test-time augmentation; imgs, img_metas: lists over views, as
    MultiScaleFlipAug's collated batch).  Views of one tensor shape run as ONE forward batch -- a scale's unflipped and
    flipped views at batch F * B.  The union handed to the NMS holds exactly the candidates the single-view path would
    hand its NMS for each view (score_thr on the class score, the top nms_pre per level and view), mapped back to the
    frame (bbox_mapping_back) and concatenated in view order; then the config's own NMS and max_per_img, once.  This
    composition rule is this project's: the reference's aug_test cannot run with this head.  rescale=False: the kept
    boxes times view 0's scale factor (aug_test_bboxes).  crops: as in `detect`, cut from the frames with the merged
    detections (the descriptor table's first B rows).  Returns what `detect` returns."""
    with torch.no_grad():
        plan = _aug_plan(self, imgs, img_metas, test_cfg)
        if plan["V"] == 1:
            return _detect(self, imgs[0], img_metas[0], test_cfg, rescale, crops)
        outs, counts, job = _rows_batch(self, imgs, plan, test_cfg, False, crops)
        if not rescale:
            outs = (outs[0] * _uploader(self, False)(plan["sf0"])[:, None, :],) + tuple(outs[1:])
        return _finish(self, outs, job, plan["B"], counts.cpu().numpy())


def _detect_aug_stream(self, batches, test_cfg, crops=None):
    """`detect_aug(rescale=True)` over an iterable of multi-view batches (imgs [V], img_metas [V], (descriptor table, frames))
    with the host one batch behind the device: batch k + 1's device program is enqueued before the host waits for batch k's
    counts, which arrive through a pinned copy behind an event, as in detect_stream.  Everything runs on the caller's stream:
    the decode / NMS overlap of detect_stream on a second stream is absent here.  crops: an ops.crops.CropSpec; the crops are
    cut from the batch's frames (the table's first B rows) behind its NMS.  Yields what detect_aug returns, in order."""
    def enqueue(batch, fetch):
        imgs, metas, source = batch
        plan = _aug_plan(self, imgs, metas, test_cfg)
        outs, counts, job = _rows_batch(self, imgs, plan, test_cfg, True, None if crops is None else (crops, source[0]))
        return (outs, job, plan["B"]) + fetch(counts) + (batch,)   # (the batch's views, table and frames stay alive with it)
    return _one_behind(self, batches, enqueue)


DetectorRuntime.detect_aug = _detect_aug
DetectorRuntime.detect_aug_stream = _detect_aug_stream


# ---------------------------------------------------------------------- tiled inference
def _tile_plan(self, imgs, plan, test_cfg):
    """Host part of detect_tiles, before any launch: the checks, the forward batches, the pool layout and the merge
    descriptor.  plan: what ImagePipeline.run_tile_rows returns (img_metas [R], rects [R, 4], edges [R], row_start [B + 1])
    with edge_margin, batch and nms_pre beside them (apis.set_tiling's).
    -> the row plan (above _check_pool; rows image-major, as the plan has them) with R and nms_pre beside it"""
    R = int(imgs.shape[0])
    row_start = np.ascontiguousarray(plan["row_start"], dtype=np.int32)
    B = len(row_start) - 1
    metas = plan["img_metas"]
    if B < 1 or R < 1 or int(row_start[0]) != 0 or int(row_start[-1]) != R or len(metas) != R or len(plan["rects"]) != R \
            or len(plan["edges"]) != R:
        raise ValueError(f"detect_tiles: {R} rows with row_start {row_start.tolist()}, {len(metas)} metas, {len(plan['rects'])} "
                         f"rectangles and {len(plan['edges'])} edge masks")
    rows_b = np.diff(row_start)
    if rows_b.min() < 1 or rows_b.max() > K.TILE_MAX_ROWS:
        raise NotImplementedError(f"detect_tiles: {int(rows_b.max())} rows for one frame (1..{K.TILE_MAX_ROWS}): enlarge the tile")
    batch = int(plan.get("batch") or 16)
    margin = float(plan.get("edge_margin") or 0.0)
    if batch < 1 or not np.isfinite(margin) or margin < 0:
        raise ValueError(f"detect_tiles: batch={batch}, edge_margin={margin}")
    nlvl = len(self.engine.strides)
    own_pre = plan.get("nms_pre")
    nms_pre = int(own_pre) if own_pre else _nms_pre(self, test_cfg, _level_hw(int(imgs.shape[2]), int(imgs.shape[3])))
    cap = nlvl * nms_pre
    cap_out = int(rows_b.max()) * cap
    _check_pool("tiled inference", cap_out, R * cap,
                lambda: (f"{int(rows_b.max())} rows for a frame, nlvl={nlvl} levels and nms_pre={nms_pre}", f"{R} rows"),
                " (set_tiling(..., nms_pre=...)) or enlarge the tile")
    hw, sf = _rows_hw_sf(metas)
    rects = np.asarray(plan["rects"], np.int64).reshape(R, 4)
    desc = K.tile_desc_rows(hw, sf, rects[:, 0:2], np.asarray(plan["edges"], np.int32), np.arange(R, dtype=np.int64) * cap,
                            np.full(R, cap, np.int32))

    def merge(p, tables):               # (the edge rule, map-back, stable compaction per image)
        K.merge_tiles(desc, tables["desc"], row_start, tables["row_start"], B, *_pool_args(p), margin, cap_out, *_list_args(p),
                      p["dropped"])

    def split(imgs):                    # the R rows as consecutive forward batches of at most `batch` rows
        imgs = imgs.to(self.dev)
        return (imgs[i0:i0 + batch] for i0 in range(0, R, batch))
    return dict(name="detect_tiles", B=B, nlvl=nlvl, hw=hw, cap_out=cap_out, pool=R * cap,
                groups=[(i0, min(batch, R - i0), nms_pre, cap, i0 * cap) for i0 in range(0, R, batch)],
                key=("tiles", B, R, cap_out, nms_pre, batch), what=f"{B} frames as {R} tiled rows, nlvl={nlvl}, nms_pre={nms_pre}",
                counters=dict(row_count=R, dropped=B), tables=dict(desc=desc, row_start=row_start), merge=merge,
                check_nms_pre=not own_pre, split=split, R=R, nms_pre=nms_pre)


def _detect_tiles(self, imgs, plan, test_cfg, crops=None):
    """`detect` over the rows of a tiled batch (imgs f32 [R, 3, Hp, Wp] and plan: ImagePipeline.run_tile_rows' tensor and
    record, with edge_margin, batch and nms_pre from apis.set_tiling).  Every row -- a frame's full-frame view, then its
    overlapping tiles -- runs at the network's resolution; the union handed to the NMS holds the candidates the single-view
    path would hand its NMS for each row (score_thr, the top nms_pre per level and row), minus those that touch a side of
    their tile that cuts through the frame (radet_merge_tiles' edge rule: the object continues beyond the tile, and a
    neighbouring tile or the full-frame row sees it whole), mapped back to the frame and concatenated in row order; then the
    config's own NMS (vote / global_vote / nms / soft_nms) and max_per_img, once per frame.  This composition is this
    project's rule: the reference has no tiled inference.  Results are in the frames' coordinates (there is no
    rescale=False).  crops = (CropSpec, descriptor table whose first B rows are the source frames), as in `detect_aug`.
    Returns what `detect` returns, one entry per FRAME."""
    with torch.no_grad():
        tp = _tile_plan(self, imgs, plan, test_cfg)
        outs, counts, job = _rows_batch(self, imgs, tp, test_cfg, False, crops)
        return _finish(self, outs, job, tp["B"], counts.cpu().numpy())


def _detect_tiles_stream(self, batches, test_cfg, crops=None):
    """`detect_tiles` over an iterable of tiled batches (imgs, plan) with the host one batch behind the device: batch k + 1's
    device program is enqueued before the host waits for batch k's counts, which arrive through a pinned copy behind an
    event, as in detect_aug_stream; everything runs on the caller's stream.  crops: an ops.crops.CropSpec; the crops are cut
    from the batch's frames (plan['table'], whose first B rows are the source frames) behind its NMS.  Yields what
    detect_tiles returns, in order."""
    def enqueue(batch, fetch):
        imgs, plan = batch
        tp = _tile_plan(self, imgs, plan, test_cfg)
        outs, counts, job = _rows_batch(self, imgs, tp, test_cfg, True, None if crops is None else (crops, plan["table"]))
        return (outs, job, tp["B"]) + fetch(counts) + (batch,)   # (the batch's rows, table and frames stay alive with it)
    return _one_behind(self, batches, enqueue)


DetectorRuntime.detect_tiles = _detect_tiles
DetectorRuntime.detect_tiles_stream = _detect_tiles_stream


def _rows_to_nchw(self, rows, levels, ch):
    """Row-major NHWC level slices -> list of NCHW tensors (module-API outputs)."""
    outs = []
    for i, (h, w) in enumerate(levels.hw):
        r0, r1 = levels.level_rows(i)
        t = torch.empty(levels.B, ch, h, w, device=self.dev)
        K.nhwc_to_nchw(rows[r0:r1], t, levels.B, ch, h, w)
        outs.append(t)
    return outs


def _extract_feat_api(self, img):
    with torch.no_grad():
        img = img.to(self.dev).contiguous()
        e = self.engine
        e.prepare(img.shape[0], img.shape[2], img.shape[3])
        e.fold()
        P = e.neck_forward(e.backbone_forward(img))
        return tuple(_rows_to_nchw(self, P, e.plv, e.feat))


def _backbone_api(self, img):
    with torch.no_grad():
        img = img.to(self.dev).contiguous()
        e = self.engine
        e.prepare(img.shape[0], img.shape[2], img.shape[3])
        e.fold()
        feats = e.backbone_forward(img)
        outs = []
        for li, f in enumerate(feats):
            lv = e.stages[li][-1]["lout"]
            outs.append(_rows_to_nchw(self, f, lv, f.shape[1])[0])
        return tuple(outs)


def _head_forward_api(self, feats):
    """feats: tuple of NCHW P3..P7 (as produced by extract_feat). Returns (cls_scores, bbox_preds, iou_preds)
    lists of NCHW tensors, bbox_preds already Scale'd + ReLU'd like RADetHead.forward_single."""
    with torch.no_grad():
        e = self.engine
        B = feats[0].shape[0]
        P = e.buf["P"]
        for i, f in enumerate(feats):
            r0, r1 = e.plv.level_rows(i)
            K.nchw_to_nhwc(f.to(self.dev).contiguous(), P[r0:r1], B, e.feat, f.shape[2], f.shape[3])
        cls, reg_u, iou = e.head_forward(P)
        reg = torch.empty_like(reg_u)
        K.scale_relu(reg_u, e.scales_tensor(), reg, e.ldesc, e.nlvl, B)
        return (_rows_to_nchw(self, cls, e.plv, self.num_classes), _rows_to_nchw(self, reg, e.plv, 4),
                _rows_to_nchw(self, iou, e.plv, 1))


DetectorRuntime.detect = _detect
DetectorRuntime.detect_stream = _detect_stream
DetectorRuntime.detect_graph = _detect_graph


def _postprocess(self, img_metas, test_cfg, rescale):
    hw, sf = _meta_tensors(self, img_metas, rescale)
    return _post_collect(self, *_post_launch(self, hw, sf, test_cfg))


DetectorRuntime._postprocess = _postprocess
DetectorRuntime.extract_feat_api = _extract_feat_api
DetectorRuntime.backbone_api = _backbone_api
DetectorRuntime.head_forward_api = _head_forward_api


# ---------------------------------------------------------------------- RADetHead module API (loss / get_bboxes / forward_train)
def _lists_to_rows(self, tensors, ch):
    """list of NCHW level tensors -> (Levels, [R, ch] fp32 row buffer in the head's level-major order)"""
    B = int(tensors[0].shape[0])
    lv = K.Levels([(int(t.shape[2]), int(t.shape[3])) for t in tensors], B)
    rows = torch.empty(lv.rows, ch, device=self.dev)
    for i, t in enumerate(tensors):
        assert t.shape[0] == B and t.shape[1] == ch, (tuple(t.shape), B, ch)
        r0, r1 = lv.level_rows(i)
        K.nchw_to_nhwc(t.detach().to(self.dev, torch.float32).contiguous(), rows[r0:r1], B, ch, t.shape[2], t.shape[3])
    return lv, rows


class _HeadLossFn(torch.autograd.Function):
    """RADetHead.loss on NCHW head outputs (bbox_preds AFTER Scale + ReLU, as the reference passes them):
    fused targets + focal + box loss (the head's `loss_bbox` kind) + IoU-BCE kernel; backward = the same kernel with the upstream gradients folded in,
    gradients returned in the inputs' NCHW layout."""

    @staticmethod
    def forward(ctx, rt, tg, weights, nlv, *tensors):
        cls, reg, iou = tensors[:nlv], tensors[nlv:2 * nlv], tensors[2 * nlv:]
        lv, rc = _lists_to_rows(rt, cls, rt.num_classes)
        _, rr = _lists_to_rows(rt, reg, 4)
        _, ri = _lists_to_rows(rt, iou, 1)
        ctx.rt, ctx.tg, ctx.weights, ctx.lv = rt, tg, weights, lv
        ctx.rows = (rc, rr, ri)
        ctx.srcs = [t.device for t in tensors]
        losses = _HeadLossFn.run(ctx, None)[0]
        out = losses * weights
        return out[0], out[1], out[2]

    @staticmethod
    def run(ctx, grad_scale):
        rt, tg, lv = ctx.rt, ctx.tg, ctx.lv
        rc, rr, ri = ctx.rows
        R, C = lv.rows, rt.num_classes
        ldesc, nlvl = K.level_desc(lv, rt.strides)
        dev = rt.dev
        hp = {"box_kind": "giou", "box_eps": 1e-6, **(rt.loss_hparams or dict(alpha=0.25, gamma=2.0, lbw=2.0))}
        losses = torch.zeros(3, device=dev)
        dcls, dreg, diou = torch.empty(R, C, device=dev), torch.empty(R, 4, device=dev), torch.empty(R, 1, device=dev)
        ws = torch.zeros(K.head_loss_ws_ints(R), dtype=torch.int32, device=dev)
        K.head_loss(rc, rr, ri, torch.ones(nlvl, device=dev), tg["boxes"], tg["labels"], tg["off"], tg["p2g"], tg["pw"], ldesc,
                    nlvl, lv.B, C, hp["alpha"], hp["gamma"], hp["lbw"], hp["box_eps"], grad_scale, losses, dcls, C, dreg, 4, diou, 1,
                    torch.zeros(nlvl, device=dev), ws, flags=K.head_loss_flags(hp["box_kind"], postact=True))
        return losses, dcls, dreg, diou

    @staticmethod
    def backward(ctx, g0, g1, g2):
        rt, lv = ctx.rt, ctx.lv
        gs = (torch.stack([g0.reshape(()), g1.reshape(()), g2.reshape(())]).to(rt.dev, torch.float32) * ctx.weights).contiguous()
        _, dcls, dreg, diou = _HeadLossFn.run(ctx, gs)
        grads = []
        for rows, ch in ((dcls, rt.num_classes), (dreg, 4), (diou, 1)):
            grads += _rows_to_nchw(rt, rows, lv, ch)
        return (None, None, None, None) + tuple(g.to(d) for g, d in zip(grads, ctx.srcs))


def _head_loss_api(self, cls_scores, bbox_preds, iou_preds, gt_bboxes, gt_labels, points_to_gt_index, points_weight):
    """RADetHead.loss (radet/models/dense_heads/radet_head.py:173-288): lists of NCHW tensors per level in,
    dict(loss_cls, loss_bbox, loss_iou) out, differentiable w.r.t. the three input lists."""
    head = self.owner().bbox_head
    assert len(cls_scores) == len(bbox_preds) == len(iou_preds)
    self.set_loss_from_head(head)
    tg = self.pack_targets(gt_bboxes, gt_labels, points_to_gt_index, points_weight)
    weights = torch.tensor([head.loss_cls.loss_weight, 1.0, head.loss_iou.loss_weight], device=self.dev)
    l0, l1, l2 = _HeadLossFn.apply(self, tg, weights, len(cls_scores), *cls_scores, *bbox_preds, *iou_preds)
    return dict(loss_cls=l0, loss_bbox=l1, loss_iou=l2)


def _get_bboxes_api(self, cls_scores, bbox_preds, centernesses, img_metas, cfg, rescale=False, with_nms=True):
    """ATSSHead.get_bboxes / RADetHead._get_bboxes_single (atss_head.py:325-387, radet_head.py:55-170): NCHW lists
    -> [(det_bboxes [k, 5], det_labels [k])] per image (device tensors)."""
    if not with_nms:
        raise NotImplementedError("get_bboxes(with_nms=False) only feeds the reference's aug_test; test-time augmentation "
                                  "runs through detect_aug (RADet.aug_test), which merges the views' candidates on the GPU")
    assert len(cls_scores) == len(bbox_preds) == len(centernesses)
    with torch.no_grad():
        lv, rc = _lists_to_rows(self, cls_scores, self.num_classes)
        _, rr = _lists_to_rows(self, bbox_preds, 4)
        _, ri = _lists_to_rows(self, centernesses, 1)
        ldesc, nlvl = K.level_desc(lv, self.strides)
        # bbox_preds already carry Scale + ReLU: decode with unit scales (relu is idempotent on them)
        ho = dict(cls=rc, reg=rr, iou=ri, scales=torch.ones(nlvl, device=self.dev), ldesc=ldesc, nlvl=nlvl, B=lv.B,
                  level_hw=lv.hw)
        hw, sf = _meta_tensors(self, img_metas, rescale)
        return _post_collect(self, *_post_launch(self, hw, sf, cfg, head_out=ho))


class _HeadTrainFn(torch.autograd.Function):
    """RADetHead.forward_train on NCHW pyramid features: head forward + fused loss through the engine; backward =
    the engine's head reverse program (gradients for the head parameters and for the input features)."""

    @staticmethod
    def forward(ctx, rt, tg, weights, nfeat, *args):
        feats = args[:nfeat]
        e = rt.engine
        B = int(feats[0].shape[0])
        for i, f in enumerate(feats):
            r0, r1 = e.plv.level_rows(i)
            K.nchw_to_nhwc(f.detach().to(rt.dev, torch.float32).contiguous(), e.buf["P"][r0:r1], B, e.feat, f.shape[2], f.shape[3])
        e.head_forward(e.buf["P"])
        losses = rt.loss(tg)
        ctx.rt, ctx.tg, ctx.weights, ctx.nfeat = rt, tg, weights, nfeat
        ctx.srcs = [f.device for f in feats]
        ctx.pnames = [n for n in rt.flat.train_names if n.startswith("bbox_head.")]
        out = losses * weights
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g0, g1, g2):
        rt = ctx.rt
        e = rt.engine
        gs = (torch.stack([g0.reshape(()), g1.reshape(()), g2.reshape(())]).to(rt.dev, torch.float32) * ctx.weights).contiguous()
        rt.loss(ctx.tg, grad_scale=gs)
        dP = e.head_backward()
        rt._unfold_bucket({b["prefix"]: b for b in rt.buckets}["bbox_head."])
        e.join_side()
        dfe = [g.to(d) for g, d in zip(_rows_to_nchw(rt, dP, e.plv, e.feat), ctx.srcs)]
        return (None, None, None, None) + tuple(dfe) + tuple(rt.flat.g[n].clone() for n in ctx.pnames)


def _head_forward_train_api(self, x, img_metas, gt_bboxes, gt_labels, points_to_gt_index, points_weight, proposal_cfg=None):
    """RADetHead.forward_train (radet_head.py:32-52): x = NCHW P3..P7 -> losses (and proposals with proposal_cfg)."""
    if gt_labels is None:
        raise NotImplementedError("RADetHead.forward_train without gt_labels (RPN use) is not on the RADet path")
    det = self.owner()
    head = det.bbox_head
    e = self.engine
    B = int(x[0].shape[0])
    hw = [(int(f.shape[2]), int(f.shape[3])) for f in x]
    shape = (img_metas[0].get("batch_input_shape") or img_metas[0].get("pad_shape")) if img_metas else None
    H, W = (int(shape[0]), int(shape[1])) if shape is not None else (hw[0][0] * self.strides[0], hw[0][1] * self.strides[0])
    e.prepare(B, H, W)
    if list(e.plv.hw) != hw:
        raise ValueError(f"feature sizes {hw} do not belong to a {H}x{W} input (expected {list(e.plv.hw)})")
    e.fold()
    e._await_fold()
    self.set_loss_from_head(head)
    tg = self.pack_targets(gt_bboxes, gt_labels, points_to_gt_index, points_weight)
    weights = torch.tensor([head.loss_cls.loss_weight, 1.0, head.loss_iou.loss_weight], device=self.dev)
    named = dict(det.named_parameters())
    plist = [named[n] for n in self.flat.train_names if n.startswith("bbox_head.")]
    l0, l1, l2 = _HeadTrainFn.apply(self, tg, weights, len(x), *x, *plist)
    losses = dict(loss_cls=l0, loss_bbox=l1, loss_iou=l2)
    if proposal_cfg is None:
        return losses
    with torch.no_grad():
        hwt, sf = _meta_tensors(self, img_metas, False)
        return losses, _post_collect(self, *_post_launch(self, hwt, sf, proposal_cfg))


DetectorRuntime.head_loss_api = _head_loss_api
DetectorRuntime.get_bboxes_api = _get_bboxes_api
DetectorRuntime.head_forward_train_api = _head_forward_train_api
