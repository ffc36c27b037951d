"""Iteration-based training harness around the native train step.

Reproduces what the reference delegates to mmcv (radet/apis/train.py:87-169, configs/base/default_runtime.py:1-26):
IterBasedRunner loop, AdamW or SGD + grad-clip (fused on the GPU) with mmcv's `paramwise_cfg` parameter groups, the
OneCycle learning rate with mmcv's defaults (div_factor 25, final_div_factor 1e4, linear anneal, two phases) or the
iteration-based fixed / step / CosineAnnealing / poly policies with warm-up, gradient accumulation
(GradientCumulativeOptimizerHook), text log every `interval` iterations (one 3-float device->host read instead of the
reference's four blocking all-reduces per iteration) and checkpoints whose `state_dict` uses the reference's parameter
names."""
import contextlib
import math
import time

import torch
import torch.distributed as dist


class OneCycleLR:
    """mmcv OneCycleLrUpdaterHook (policy='OneCycle', anneal_strategy='linear', three_phase=False)."""

    def __init__(self, max_lr, total_steps, pct_start=0.3, anneal_strategy="linear", div_factor=25.0,
                 final_div_factor=1e4, three_phase=False):
        if anneal_strategy not in ("linear", "cos"):
            raise ValueError("anneal_strategy must be 'cos' or 'linear'")
        if three_phase:
            raise NotImplementedError("three_phase=True is not used by the RADet configs")
        self.max_lr, self.total_steps, self.anneal = float(max_lr), int(total_steps), anneal_strategy
        self.initial_lr = self.max_lr / div_factor
        self.min_lr = self.initial_lr / final_div_factor
        self.up_end = float(pct_start * total_steps) - 1
        self.down_end = float(total_steps) - 1

    def _anneal(self, start, end, pct):
        if self.anneal == "linear":
            return (end - start) * pct + start
        import math
        return end + (start - end) / 2.0 * (math.cos(math.pi * pct) + 1)

    def get_lr(self, step):
        """Learning rate used for iteration `step` (0-based), exactly torch.optim.lr_scheduler.OneCycleLR's value."""
        if step > self.down_end:
            raise ValueError(f"step {step} exceeds total_steps {self.total_steps}")
        if step <= self.up_end:
            return self._anneal(self.initial_lr, self.max_lr, step / self.up_end)
        return self._anneal(self.max_lr, self.min_lr, (step - self.up_end) / (self.down_end - self.up_end))


class IterLR:
    """mmcv's LrUpdaterHook family with by_epoch=False: policy 'fixed', 'step' (step: int or list, gamma, min_lr),
    'CosineAnnealing' (min_lr or min_lr_ratio) and 'poly' (power, min_lr) over `max_iters` iterations, with
    warmup=None | 'constant' | 'linear' | 'exp' over the first `warmup_iters` iterations (warmup_ratio).  The formulas are
    mmcv's (mmcv/runner/hooks/lr_updater.py), restated; mmcv is not a dependency, so parity is by formula and against
    torch.optim.lr_scheduler (tests/test_optim_cpu.py), not against an installed mmcv."""

    POLICIES = ("fixed", "step", "CosineAnnealing", "poly")

    def __init__(self, policy, base_lr, max_iters, warmup=None, warmup_iters=0, warmup_ratio=0.1, step=None, gamma=0.1,
                 min_lr=None, min_lr_ratio=None, power=1.0):
        if policy not in self.POLICIES:
            raise NotImplementedError(f"lr_config policy {policy!r}: implemented are OneCycle, " + ", ".join(self.POLICIES))
        if warmup is not None:
            if warmup not in ("constant", "linear", "exp"):
                raise ValueError(f'"{warmup}" is not a supported type for warming up, valid types are "constant", "linear" and "exp"')
            if not warmup_iters > 0 or not 0 < warmup_ratio <= 1.0:
                raise ValueError('"warmup_iters" must be a positive integer and "warmup_ratio" must be in range (0,1]')
        if policy == "step":
            if isinstance(step, int):
                if step <= 0:
                    raise ValueError('"step" must be a positive integer or a list of them')
            elif not (isinstance(step, (list, tuple)) and step and all(isinstance(x, int) and x > 0 for x in step)):
                raise TypeError('"step" must be a list or integer')
        if policy == "CosineAnnealing" and (min_lr is None) == (min_lr_ratio is None):
            raise ValueError("CosineAnnealing takes exactly one of min_lr and min_lr_ratio")
        self.policy, self.base_lr, self.max_iters = policy, float(base_lr), int(max_iters)
        self.warmup, self.warmup_iters, self.warmup_ratio = warmup, int(warmup_iters), float(warmup_ratio)
        self.step = step if isinstance(step, int) or step is None else list(step)
        self.gamma, self.power, self.min_lr, self.min_lr_ratio = float(gamma), float(power), min_lr, min_lr_ratio

    @property
    def absolute_floor(self):
        """an absolute min_lr is in force: the rate is then no multiple of base_lr (parameter groups cannot scale it)"""
        return self.policy != "fixed" and self.min_lr is not None and self.min_lr != 0

    def regular_lr(self, it):
        base = self.base_lr
        if self.policy == "fixed":
            return base
        if self.policy == "step":
            if isinstance(self.step, int):
                exp = it // self.step
            else:
                exp = len(self.step)
                for i, s in enumerate(self.step):
                    if it < s:
                        exp = i
                        break
            lr = base * self.gamma ** exp
            return lr if self.min_lr is None else max(lr, self.min_lr)
        if self.policy == "CosineAnnealing":
            target = base * self.min_lr_ratio if self.min_lr_ratio is not None else self.min_lr
            return target + 0.5 * (base - target) * (math.cos(math.pi * it / self.max_iters) + 1)
        floor = 0.0 if self.min_lr is None else self.min_lr                      # poly
        return (base - floor) * (1 - it / self.max_iters) ** self.power + floor

    def get_lr(self, it):
        """Learning rate of iteration `it` (0-based)."""
        lr = self.regular_lr(it)
        if self.warmup is None or it >= self.warmup_iters:
            return lr
        if self.warmup == "constant":
            return lr * self.warmup_ratio
        if self.warmup == "linear":
            return lr * (1 - (1 - it / self.warmup_iters) * (1 - self.warmup_ratio))
        return lr * self.warmup_ratio ** (1 - it / self.warmup_iters)


def build_lr_schedule(lr_config, base_lr, max_iters, scaled_lr=False):
    """cfg.lr_config -> an object with get_lr(iteration).  scaled_lr: some parameter group has lr_mult != 1.  One scalar
    rate per step goes to the kernel and the groups scale it, which is what mmcv does for every proportional policy; where
    mmcv would do something else the config is refused: OneCycle (its hook overwrites every group's rate with the scalar
    max_lr) and an absolute min_lr (mmcv clamps each group to the same floor; use min_lr_ratio)."""
    lc = dict(lr_config)
    policy = lc.pop("policy")
    if policy == "OneCycle":
        if scaled_lr:
            raise NotImplementedError("policy='OneCycle' with a paramwise lr_mult != 1: mmcv's OneCycle hook sets every group "
                                      "to the scalar max_lr, which the group-scaled fused step would not reproduce")
        return OneCycleLR(lc["max_lr"], lc["total_steps"], pct_start=lc.get("pct_start", 0.3),
                          anneal_strategy=lc.get("anneal_strategy", "cos"))
    if policy not in IterLR.POLICIES:
        raise NotImplementedError(f"lr_config policy {policy!r}: implemented are OneCycle, " + ", ".join(IterLR.POLICIES))
    if lc.pop("by_epoch", True) or lc.pop("warmup_by_epoch", False):
        raise NotImplementedError(f"lr_config policy {policy!r} by epoch: this harness counts iterations "
                                  "(IterBasedRunner); set by_epoch=False (and leave warmup_by_epoch unset)")
    try:
        sched = IterLR(policy, base_lr, max_iters, **lc)
    except TypeError as e:
        if "unexpected keyword" in str(e):
            raise KeyError(f"lr_config of policy {policy!r}: {e}") from None
        raise
    if scaled_lr and sched.absolute_floor:
        raise NotImplementedError(f"policy {policy!r} with an absolute min_lr and a paramwise lr_mult != 1: mmcv clamps every "
                                  "group to the same floor; use min_lr_ratio (or min_lr=0)")
    return sched


_PARAMWISE_KEYS = ("custom_keys", "bias_lr_mult", "bias_decay_mult", "norm_decay_mult", "dwconv_decay_mult",
                   "dcn_offset_lr_mult", "bypass_duplicate")


def resolve_paramwise(model, paramwise_cfg):
    """mmcv's DefaultOptimizerConstructor.add_params, restated (mmcv is not a dependency: parity with it is by these rules,
    unpinned by a test against mmcv itself).  Returns {parameter name: (lr_mult, decay_mult)} for every TRAINABLE
    parameter of `model`, in named_parameters() order:
      * custom_keys = {key: dict(lr_mult=, decay_mult=)}: a key matches when it is a substring of the full parameter name;
        keys are tried longest first, ties alphabetically, and the first match sets both multipliers (a missing one is 1)
        and wins over every rule below;
      * otherwise bias_lr_mult / bias_decay_mult apply to parameters named `bias` of modules that are not norm layers;
      * norm_decay_mult applies to `weight` and `bias` of norm layers (BNShell, GNShell);
      * dwconv_decay_mult / dcn_offset_lr_mult: this model has no depth-wise or deformable conv, accepted only at 1;
      * frozen parameters (requires_grad = False) have no optimizer state here and are skipped;
      * an unknown key raises KeyError."""
    from ..models.shells import BNShell, GNShell
    cfg = dict(paramwise_cfg or {})
    for k in cfg:
        if k not in _PARAMWISE_KEYS:
            raise KeyError(f"paramwise_cfg key {k!r} is not one of {_PARAMWISE_KEYS}")
    for k in ("dwconv_decay_mult", "dcn_offset_lr_mult"):
        if float(cfg.get(k, 1.0)) != 1.0:
            raise NotImplementedError(f"paramwise_cfg {k} = {cfg[k]}: this detector has nothing it would act on")
    custom = cfg.get("custom_keys", {}) or {}
    if not isinstance(custom, dict):
        raise TypeError(f"If specified, custom_keys must be a dict, but got {type(custom)}")
    for key, d in custom.items():
        extra = set(d) - {"lr_mult", "decay_mult"}
        if extra:
            raise KeyError(f"custom_keys[{key!r}] has {sorted(extra)}: expected lr_mult and / or decay_mult")
    keys = sorted(sorted(custom), key=len, reverse=True)
    bias_lr, bias_decay = float(cfg.get("bias_lr_mult", 1.0)), float(cfg.get("bias_decay_mult", 1.0))
    norm_decay = float(cfg.get("norm_decay_mult", 1.0))
    out = {}
    for prefix, module in model.named_modules():
        is_norm = isinstance(module, (BNShell, GNShell))
        for leaf, p in module.named_parameters(recurse=False):
            if not p.requires_grad:
                continue
            name = f"{prefix}.{leaf}" if prefix else leaf
            for key in keys:
                if key in name:
                    out[name] = (float(custom[key].get("lr_mult", 1.0)), float(custom[key].get("decay_mult", 1.0)))
                    break
            else:
                lm = bias_lr if leaf == "bias" and not is_norm else 1.0
                dm = norm_decay if is_norm else bias_decay if leaf == "bias" else 1.0
                out[name] = (lm, dm)
    order = {n: i for i, (n, _) in enumerate(model.named_parameters())}
    return dict(sorted(out.items(), key=lambda kv: order[kv[0]]))


def _param_groups(model, runtime):
    """(multipliers, [parameter names]) per distinct (lr_mult, decay_mult), in order of first appearance over
    model.named_parameters(); frozen parameters carry the base values, as they do in mmcv's groups"""
    mult = runtime.opt_state.get("groups") or {}
    groups = {}
    for n, _ in model.named_parameters():
        groups.setdefault(tuple(mult.get(n, (1.0, 1.0))), []).append(n)
    return list(groups.items())


def optimizer_state_dict(model, runtime):
    """The fused optimizer's state in `torch.optim.AdamW.state_dict()` / `torch.optim.SGD.state_dict()` format ({state,
    param_groups}), so checkpoints written here resume under the reference's runner and vice versa.  Without parameter
    groups there is one group and a parameter's index is its position in `model.parameters()` (what mmcv's
    `build_optimizer` hands to the optimizer).  With them there is one group per distinct (lr, weight_decay), numbered group
    after group as torch does, each with torch's optional `param_names`.  `step_count` (an extra top-level key torch ignores)
    carries the step counter, which torch's SGD state does not hold."""
    st = runtime.opt_state
    flat = runtime.flat
    sgd = st.get("type", "AdamW") == "SGD"
    groups = _param_groups(model, runtime)
    state, param_groups, idx = {}, [], 0
    for (lm, dm), names in groups:
        for i, n in enumerate(names, idx):
            if n not in flat.offsets:
                continue
            o, k = flat.offsets[n], flat.p[n].numel()
            def view(a):
                return a[o:o + k].view(flat.p[n].shape).cpu().clone()
            if not sgd:
                state[i] = dict(step=torch.tensor(float(runtime.step_count)), exp_avg=view(st["m"]), exp_avg_sq=view(st["v"]))
            elif st["buf"] is not None and runtime.step_count > 0:
                state[i] = dict(momentum_buffer=view(st["buf"]))
        if sgd:
            g = dict(lr=st["lr"] * lm, momentum=st["momentum"], dampening=st["dampening"], weight_decay=st["wd"] * dm,
                     nesterov=st["nesterov"])
        else:
            g = dict(lr=st["lr"] * lm, betas=tuple(st["betas"]), eps=st["eps"], weight_decay=st["wd"] * dm, amsgrad=False)
        g["params"] = list(range(idx, idx + len(names)))
        if len(groups) > 1:
            g["param_names"] = list(names)
        param_groups.append(g)
        idx += len(names)
    out = dict(state=state, param_groups=param_groups)
    if sgd or len(groups) > 1:
        out["step_count"] = int(runtime.step_count)
    return out


def load_optimizer_state_dict(model, runtime, osd):
    """Accepts the torch / mmcv format above (AdamW or SGD, one group or several) and the flat-arena format of earlier
    checkpoints of this package."""
    st = runtime.opt_state
    sgd = st.get("type", "AdamW") == "SGD"
    if "state" in osd and "param_groups" in osd:
        flat = runtime.flat
        names = [n for n, _ in model.named_parameters()]
        pg = osd["param_groups"]
        order = [i for g in pg for i in g["params"]]
        if len(order) != len(names):
            raise ValueError(f"optimizer state has {len(order)} parameters, the model {len(names)}")
        if all("param_names" in g for g in pg):
            by_pos = [n for g in pg for n in g["param_names"]]
        elif len(pg) == 1:
            by_pos = names
        else:           # several groups, no names: they must be this run's groups (same config), which fixes the numbering
            mine = _param_groups(model, runtime)
            if [len(g["params"]) for g in pg] != [len(ns) for _, ns in mine]:
                raise ValueError("optimizer state has several parameter groups without param_names and they are not the "
                                 "groups this run's paramwise_cfg makes: the parameters cannot be told apart")
            by_pos = [n for _, ns in mine for n in ns]
        if sorted(by_pos) != sorted(names):
            raise ValueError("optimizer state names parameters this model does not have")
        step = 0
        for pos, key in enumerate(order):
            entry = osd["state"].get(key)
            n = by_pos[pos]
            if entry is None or n not in flat.offsets:
                continue
            o, k = flat.offsets[n], flat.p[n].numel()
            if sgd:
                if "momentum_buffer" not in entry:
                    raise KeyError("optimizer state is not torch.optim.SGD's (no momentum_buffer) but the optimizer is SGD")
                if st["buf"] is not None and entry["momentum_buffer"] is not None:
                    st["buf"][o:o + k].copy_(entry["momentum_buffer"].reshape(-1))
                    step = max(step, 2)               # (a filled buffer: not the first step; the counter itself is below)
            else:
                if "exp_avg" not in entry:
                    raise KeyError("optimizer state is not torch.optim.AdamW's (no exp_avg) but the optimizer is AdamW")
                st["m"][o:o + k].copy_(entry["exp_avg"].reshape(-1))
                st["v"][o:o + k].copy_(entry["exp_avg_sq"].reshape(-1))
                step = max(step, int(float(entry["step"])))
        runtime.step_count = int(osd.get("step_count", step))
    elif "step" in osd:                                   # flat arenas (round-1 checkpoints of this package)
        if sgd or osd["exp_avg"].numel() != st["m"].numel():
            raise ValueError("flat optimizer state does not match this model's parameter arena")
        runtime.step_count = int(osd["step"])
        st["m"].copy_(osd["exp_avg"])
        st["v"].copy_(osd["exp_avg_sq"])
    else:
        raise KeyError("unrecognised optimizer state: expected torch's {state, param_groups} or {step, exp_avg, exp_avg_sq}")


_EMA_HOOK_KEYS = ("type", "momentum", "interval", "warm_up", "resume_from", "priority")


def parse_custom_hooks(cfg):
    """cfg.custom_hooks -> the keyword arguments of DetectorRuntime.init_ema, or None without a hook.  The reference builds
    every entry from mmcv's HOOKS (radet/apis/train.py:151-163); the one implemented here is
    dict(type='EMAHook', momentum=0.0002, interval=1, warm_up=100) with mmcv 1.3.18's defaults (`priority` is accepted and
    ignored: the update's place behind the optimizer is fixed).  Its own `resume_from` and every other hook type raise
    NotImplementedError instead of being dropped."""
    hooks = cfg.get("custom_hooks", None) or []
    if not isinstance(hooks, (list, tuple)):
        raise TypeError(f"custom_hooks should be a list, but got {type(hooks)}")
    ema = None
    for h in hooks:
        if not isinstance(h, dict) or "type" not in h:
            raise TypeError(f"each item of custom_hooks is a dict with a 'type', but got {h!r}")
        if h["type"] != "EMAHook":
            raise NotImplementedError(f"custom_hooks type {h['type']!r}: the only hook this harness implements is EMAHook "
                                      "(an entry is never dropped silently)")
        for k in h:
            if k not in _EMA_HOOK_KEYS:
                raise KeyError(f"EMAHook key {k!r} is not one of {_EMA_HOOK_KEYS}")
        if h.get("resume_from") is not None:
            raise NotImplementedError("EMAHook resume_from is not implemented: resume with train_detector(resume_from=), "
                                      "whose checkpoints carry the EMA")
        if ema is not None:
            raise ValueError("custom_hooks holds more than one EMAHook")
        momentum, interval = h.get("momentum", 0.0002), h.get("interval", 1)
        if not (isinstance(momentum, float) and 0.0 < momentum < 1.0):
            raise ValueError(f"EMAHook momentum must lie in (0, 1), got {momentum!r}")
        if not (isinstance(interval, int) and not isinstance(interval, bool) and interval > 0):
            raise ValueError(f"EMAHook interval must be a positive int, got {interval!r}")
        ema = dict(momentum=momentum, interval=interval, warm_up=h.get("warm_up", 100))
    return ema


def ema_state_dict(model, runtime):
    """The EMA arena under mmcv EMAHook's buffer names (`ema_` + the parameter's name with '.' replaced by '_').  Only the
    trainable arena is averaged: a frozen parameter's entry is a copy of the parameter."""
    from ..runtime import ema_key
    flat, ema = runtime.flat, runtime.ema_state["ema"]
    out = {}
    for n, p in model.named_parameters():
        if n in flat.offsets:
            o = flat.offsets[n]
            out[ema_key(n)] = ema[o:o + p.numel()].view(p.shape).cpu().clone()
        else:
            out[ema_key(n)] = p.detach().cpu().clone()
    return out


def load_ema_state_dict(model, runtime, sd):
    """Fill the EMA arena from the `ema_*` entries of a checkpoint's state_dict.  A file that holds none of them restarts
    the EMA from the parameters as they are now (just loaded); one that holds only some of them is refused."""
    from ..runtime import ema_key
    flat, ema = runtime.flat, runtime.ema_state["ema"]
    have = [n for n in flat.train_names if ema_key(n) in sd]
    if not have:
        ema.copy_(flat.params)
        return False
    if len(have) != len(flat.train_names):
        lost = [n for n in flat.train_names if ema_key(n) not in sd]
        raise KeyError(f"checkpoint holds EMA entries but not those of {lost[:3]}{'...' if len(lost) > 3 else ''}")
    for n in flat.train_names:
        o, k = flat.offsets[n], flat.p[n].numel()
        ema[o:o + k].copy_(sd[ema_key(n)].reshape(-1))
    return True


def save_checkpoint(model, path, meta=None, runtime=None):
    """mmcv-style checkpoint: dict(meta=..., state_dict=..., optimizer=...) with reference parameter names; the
    optimizer entry is `torch.optim.AdamW.state_dict()`-compatible.  A runtime with an EMA (init_ema) adds the EMA arena to
    the state_dict under mmcv's `ema_*` names and meta['ema_swapped']: True when written inside `runtime.ema_weights()`, as
    train_detector does -- the parameters of the file are then the EMA weights and its `ema_*` entries the raw ones."""
    ckpt = dict(meta=dict(meta or {}), state_dict={k: v.detach().cpu() for k, v in model.state_dict().items()})
    if runtime is not None and runtime.opt_state is not None:
        ckpt["optimizer"] = optimizer_state_dict(model, runtime)
    if runtime is not None and runtime.ema_state is not None:
        ckpt["state_dict"].update(ema_state_dict(model, runtime))
        ckpt["meta"]["ema_swapped"] = bool(runtime.ema_state["swapped"])
    torch.save(ckpt, path)
    return path


def load_checkpoint(model, path, strict=False, runtime=None, sync=True):
    """Load a reference-format checkpoint.  With `runtime` and an initialised process group this is COLLECTIVE (sync=True):
    every rank must call it, and all continue from rank 0's parameters / optimizer state / step counter -- so a file that
    only rank 0 can read reaches every replica.  Pass sync=False for rank-local use (rank-0 evaluation, conversion).
    A runtime with an EMA (init_ema) takes the file's `ema_*` entries into its EMA arena -- without them the EMA restarts
    from the loaded parameters -- and, where meta['ema_swapped'] says the file holds the EMA weights as the parameters,
    swaps the two back: training continues exactly.  Without an EMA the entries are ignored and the model is the file's
    parameters, the EMA weights of a swapped file."""
    ckpt = torch.load(path, map_location="cpu")
    sd = ckpt.get("state_dict", ckpt)
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    missing = model.load_state_dict(sd, strict=strict)      # copies in place: parameters stay in the flat arena
    if runtime is not None and "optimizer" in ckpt and runtime.opt_state is not None:
        load_optimizer_state_dict(model, runtime, ckpt["optimizer"])
    if runtime is not None and runtime.ema_state is not None:
        st = runtime.ema_state
        st["swapped"] = load_ema_state_dict(model, runtime, sd) and bool(ckpt.get("meta", {}).get("ema_swapped"))
        if st["swapped"]:
            runtime.swap_ema()                               # the file's parameters were the EMA weights: back to the raw ones
    if runtime is not None and sync:
        runtime.sync_replicas()                              # data-parallel: every rank continues from rank 0's state
    return ckpt.get("meta", {}), missing


def wrap_fp16_model(model, mode="bf16-storage"):
    """Mixed-precision switch with mmcv's name (the reference: `wrap_fp16_model` + `Fp16OptimizerHook`,
    apis/train.py:113-117, which keep half-precision activations and fp32 master weights).  Marks the detector so that
    its HIP runtime is built in `mode`:
      "bf16-storage" (default): bf16 activations / folded weights / activation gradients in HBM, bf16 matrix cores,
                                fp32 accumulate, GroupNorm statistics, loss, weight gradients, master weights, AdamW;
      "bf16":                   fp32 tensors, operands rounded to bf16 on their way into the matrix cores.
    No loss scaling is needed with bf16's fp32-sized exponent."""
    assert mode in ("bf16-storage", "bf16")
    model.fp16_enabled = True
    model.fp16_mode = mode
    return model


_EVAL_HOOK_KEYS = ("interval", "start", "by_epoch", "save_best", "rule", "gpu_collect", "tmpdir", "broadcast_bn_buffer")


def evaluate_during_training(model, rt, val_loader, cfg, it, log=print, eval_log=None):
    """What the reference's EvalHook / DistEvalHook do after iteration `it` (radet/apis/train.py:131-149): the model goes to
    eval(), the validation loader is tested (every rank its share when a process group is initialised), rank 0 evaluates
    with `cfg.evaluation`'s metric and options on the device, logs one line and appends (it, metrics) to `eval_log`.
    The training state is put back explicitly: train mode (the weights are folded again by the next step), the launch tape is
    dropped (it is recorded again from the next steady-state step; a replay is bit-identical to the eager step), the engine
    switches back to the training batch's plan on the next forward pass, and detect_stream has already handed the head-output
    buffers back to their plans when its loop ended."""
    from .test import multi_gpu_test, single_gpu_test
    ev = dict(cfg.get("evaluation", None) or {})
    kw = {k: v for k, v in ev.items() if k not in _EVAL_HOOK_KEYS}
    kw.setdefault("logger", "silent")
    distributed = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank() if distributed else 0
    was_training = model.training
    model.eval()
    try:
        if distributed:
            results = multi_gpu_test(model, val_loader, tmpdir=ev.get("tmpdir"), gpu_collect=ev.get("gpu_collect", True))
        else:
            results = single_gpu_test(model, val_loader, on_device=True)[1]
        metrics = None
        if rank == 0:
            metrics = val_loader.dataset.evaluate(results, device=rt.dev, **kw)
            log(f"Iter(val) [{it}] " + ", ".join(f"{k}: {v:.4f}" if isinstance(v, float) else f"{k}: {v}"
                                                for k, v in metrics.items() if k != "classwise"))
            if eval_log is not None:
                eval_log.append((it, metrics))
    finally:
        if was_training:
            model.train()
        rt.drop_tape()
    return metrics


_OPTIMIZER_KEYS = dict(AdamW=("type", "lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "paramwise_cfg"),
                       SGD=("type", "lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize", "foreach", "paramwise_cfg"))


def optimizer_kwargs(model, cfg):
    """cfg.optimizer (+ paramwise_cfg, inside it as mmdetection writes it or beside it as cfg.paramwise_cfg) and the clip of
    cfg.optimizer_config -> (keyword arguments of DetectorRuntime.init_optimizer, the resolved groups or None).  The plain
    recipe -- AdamW, no group multiplier other than 1 -- yields exactly the keywords lr, betas, eps, weight_decay, max_norm."""
    o = dict(cfg.optimizer)
    kind = o.get("type")
    if kind not in _OPTIMIZER_KEYS:
        raise NotImplementedError(f"optimizer type {kind!r}: the fused step implements AdamW and SGD")
    for k in o:
        if k not in _OPTIMIZER_KEYS[kind]:
            raise KeyError(f"optimizer key {k!r} is not one of {kind}'s {_OPTIMIZER_KEYS[kind]}")
    for k in ("amsgrad", "maximize", "foreach"):
        if o.get(k):
            raise NotImplementedError(f"optimizer {k}={o[k]!r} is not implemented by the fused step")
    clip = (cfg.get("optimizer_config", None) or {}).get("grad_clip") or {}
    if float(clip.get("norm_type", 2)) != 2.0:
        raise NotImplementedError(f"grad_clip norm_type={clip['norm_type']}: the fused clip is the global L2 norm")
    pw = o.get("paramwise_cfg", None) or cfg.get("paramwise_cfg", None)
    groups = resolve_paramwise(model, pw) if pw else None
    if groups is not None and all(v == (1.0, 1.0) for v in groups.values()):
        groups = None
    if kind == "AdamW":
        kw = dict(lr=o["lr"], betas=tuple(o.get("betas", (0.9, 0.999))), eps=o.get("eps", 1e-8),
                  weight_decay=o.get("weight_decay", 0.01), max_norm=float(clip.get("max_norm", 0.0)))
    else:
        kw = dict(lr=o["lr"], weight_decay=o.get("weight_decay", 0.0), max_norm=float(clip.get("max_norm", 0.0)), type="SGD",
                  momentum=o.get("momentum", 0.0), dampening=o.get("dampening", 0.0), nesterov=bool(o.get("nesterov", False)))
    if groups is not None:
        kw["groups"] = groups
    return kw, groups


def accumulation_plan(cfg, max_iters, checkpoints=True, evaluations=True):
    """cfg.optimizer_config -> k = cumulative_iters of a GradientCumulativeOptimizerHook (1: OptimizerHook, the plain step).
    mmcv's remainder rule: the trailing max_iters % k iterations form one step of their own, divided by their count.  A
    checkpoint or an evaluation never falls inside an accumulation: their intervals must be multiples of k."""
    oc = dict(cfg.get("optimizer_config", None) or {})
    kind = oc.get("type", "OptimizerHook")
    if kind == "OptimizerHook":
        return 1
    if kind != "GradientCumulativeOptimizerHook":
        raise NotImplementedError(f"optimizer_config type {kind!r}: implemented are OptimizerHook and "
                                  "GradientCumulativeOptimizerHook")
    k = oc.get("cumulative_iters", 1)
    if not (isinstance(k, int) and k > 0):
        raise ValueError(f"cumulative_iters only accepts positive int, but got {k!r}")
    for name, on in (("checkpoint_config", checkpoints), ("evaluation", evaluations)):
        every = int((cfg.get(name, None) or {}).get("interval", 0) or 0)
        if on and every % k:
            raise ValueError(f"{name}.interval = {every} is no multiple of cumulative_iters = {k}: it would fall inside an "
                             "accumulated step")
    return k


def micro_step(it, max_iters, k, start=0):
    """(j, count) of iteration `it`: micro-step j of an optimizer step accumulated over `count` iterations.  mmcv's rule
    (GradientCumulativeOptimizerHook._init): of the max_iters - start iterations of this run the first whole multiples of
    k accumulate k each, the remainder forms one last step."""
    whole = start + (max_iters - start) // k * k
    if it < whole:
        return (it - start) % k, k
    return it - whole, max_iters - whole


def train_detector(model, batches, cfg, max_iters=None, log=print, checkpoint_path=None, val_loader=None, eval_log=None,
                   resume_from=None):
    """`batches`: iterable of dict(img=f32[B,3,H,W], gt_bboxes, gt_labels, points_to_gt_index, points_weight)
    (device or host tensors; lists per image).  One process per GPU; gradients are averaged over the
    `torch.distributed` group if one is initialised.  Returns the list of logged loss triples.
    val_loader: a test-mode `build_dataloader`; with it and `cfg.evaluation.interval = n` the detector is evaluated after
    every n-th iteration (evaluate_during_training; the training trajectory is the same with and without it).
    cfg.optimizer.type: AdamW or SGD, with mmcv's paramwise_cfg (resolve_paramwise); cfg.lr_config.policy: OneCycle, fixed,
    step, CosineAnnealing, poly (build_lr_schedule); cfg.optimizer_config type GradientCumulativeOptimizerHook accumulates
    `cumulative_iters` batches per optimizer step (the learning rate follows the micro-iteration, as mmcv's hooks do).
    resume_from: a checkpoint of this harness; training continues at its meta['iter'] (a multiple of cumulative_iters) and
    `batches` supplies the batches from that iteration on.
    cfg.custom_hooks: one dict(type='EMAHook', ...) keeps an exponential moving average of the trainable parameters
    (parse_custom_hooks, DetectorRuntime.init_ema).  The update follows every iteration, micro-iterations of an accumulated
    step included; every evaluation and every checkpoint is bracketed by a swap, so both see the EMA weights: a
    checkpoint's parameters are the EMA weights, its `ema_*` entries the raw ones, and a resume with the hook is exact."""
    ema_cfg = parse_custom_hooks(cfg)
    if cfg.get("fp16", None) is not None:        # reference: Fp16OptimizerHook + wrap_fp16_model (apis/train.py:113-117)
        wrap_fp16_model(model)                   # here: bf16 operands, fp32 accumulate / master weights, no loss scaling
    rt = model.train().runtime()
    max_iters = max_iters or cfg.runner.max_iters
    kw, groups = optimizer_kwargs(model, cfg)
    eval_every = int((cfg.get("evaluation", None) or {}).get("interval", 0)) if val_loader is not None else 0
    ckpt_every = cfg.get("checkpoint_config", {}).get("interval", 0)
    k = accumulation_plan(cfg, max_iters, checkpoints=bool(checkpoint_path), evaluations=val_loader is not None)
    sched = build_lr_schedule(cfg.lr_config, kw["lr"], max_iters,
                              scaled_lr=groups is not None and any(lm != 1.0 for lm, _ in groups.values()))
    rt.init_optimizer(**kw)
    rt.set_loss_from_head(model.bbox_head)
    start = 0
    if ema_cfg is not None:
        rt.init_ema(**ema_cfg)                   # a copy of the parameters; a resumed run takes its EMA from the file below
    if resume_from:
        meta, _ = load_checkpoint(model, resume_from, runtime=rt)
        start = int(meta.get("iter", 0))
        if meta.get("ema_swapped") and ema_cfg is None:
            log(f"{resume_from} holds EMA weights as its parameters and no EMAHook is configured: training continues from "
                "the EMA weights")
        if start % k:
            raise ValueError(f"{resume_from} was written at iteration {start}, inside an accumulated step of {k} iterations")
    interval = cfg.get("log_config", {}).get("interval", 50)
    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    history, t0 = [], time.time()
    ema_in = rt.ema_weights if ema_cfg is not None else contextlib.nullcontext     # swap in, evaluate or save, swap out
    for it, batch in enumerate(batches, start):
        if it >= max_iters:
            break
        lr = sched.get_lr(it)
        tg = rt.pack_targets(batch["gt_bboxes"], batch["gt_labels"], batch["points_to_gt_index"], batch["points_weight"])
        if k == 1:
            losses = rt.train_step(batch["img"].to(rt.dev), tg, lr=lr, ema_iter=it)
        else:
            losses = rt.train_step(batch["img"].to(rt.dev), tg, lr=lr, accumulate=micro_step(it, max_iters, k, start), ema_iter=it)
        if (it + 1) % interval == 0 or it + 1 == max_iters:
            vals = torch.cat([losses, rt.opt_state["grad_norm"]]).cpu().tolist()     # the only host sync
            history.append(vals[:3])
            if rank == 0:
                log(f"Iter [{it + 1}/{max_iters}] lr: {lr:.3e}, loss_cls: {vals[0]:.4f}, loss_bbox: {vals[1]:.4f}, "
                    f"loss_iou: {vals[2]:.4f}, loss: {sum(vals[:3]):.4f}, grad_norm: {vals[3]:.4f}, "
                    f"time: {(time.time() - t0) / (it + 1 - start):.4f} s/iter")
        if checkpoint_path and ckpt_every and (it + 1) % ckpt_every == 0 and rank == 0:
            with ema_in():
                save_checkpoint(model, checkpoint_path.format(iter=it + 1), meta=dict(iter=it + 1), runtime=rt)
        if eval_every > 0 and (it + 1) % eval_every == 0:
            with ema_in():
                evaluate_during_training(model, rt, val_loader, cfg, it + 1, log=log, eval_log=eval_log)
    return history
