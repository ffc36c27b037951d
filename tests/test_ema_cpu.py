"""CPU side of the weight EMA (no kernel is launched): mmcv EMAHook's momentum schedule, the arithmetic the kernel is
pinned to (torch's CPU mul_ / add_ against its NumPy restatement, bit for bit), the `ema_*` checkpoint entries, the
`custom_hooks` configurations the harness accepts and refuses, and the declaration of the two entry points."""
import os
import re
import types

import numpy as np
import pytest
import torch

from _ema_ref import MOMENTA, bits, inputs, numpy_ema, torch_ema

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py")


def load_cfg(path=CFG, **override):
    from radet_amd.utils import Config
    cfg = Config.fromfile(path)
    cfg.model["pretrained"] = None
    return Config({**dict(cfg._cfg_dict), **override}) if override else cfg


# ---------------------------------------------------------------------- schedule
@pytest.mark.parametrize("momentum", [0.0002, 0.5])
@pytest.mark.parametrize("warm_up,interval", [(100, 1), (100, 3), (0, 1)])
def test_momentum_schedule(monkeypatch, warm_up, interval, momentum):
    """it = 0..300 through DetectorRuntime._ema_update with the launch replaced by a recorder: which iterations fire and with
    which momentum.  Expected values are written out here from the hook's rule, not taken from the code under test."""
    from radet_amd import runtime as R
    fired = {}
    monkeypatch.setattr(R.K, "ema_update", lambda ema, p, n, m: fired.setdefault(ema, m))
    rt = types.SimpleNamespace(flat=types.SimpleNamespace(params=None, n_train=0))
    for it in range(301):
        rt.ema_state = dict(ema=it, momentum=momentum, interval=interval, warm_up=warm_up, swapped=False)
        R.DetectorRuntime._ema_update(rt, it)
    R.DetectorRuntime._ema_update(rt, None)                    # no iteration number: no update
    assert sorted(fired) == [it for it in range(301) if it % interval == 0]
    M = momentum ** interval
    for it, m in fired.items():
        if warm_up == 0 and it == 0:
            assert m == 1.0                                    # the EMA restarts from the parameters
        elif warm_up == 0:
            assert m == M                                      # (1 + it) / it > 1 > M
        else:
            ramp = (1 + it) / (100 + it)
            assert m == (ramp if ramp < M else M)
    if warm_up == 100:
        assert fired[0] == min(M, 0.01)
        if momentum == 0.5 and interval == 1:                  # the ramp crosses 1/2 between it = 97 (98/197) and 98 (99/198)
            assert fired[97] == 98 / 197 and fired[98] == 0.5 and fired[300] == 0.5
        if momentum == 0.0002:
            assert set(fired.values()) == {M}                  # 1/100 is above it from the start


def test_swapped_arena_refuses_the_update():
    from radet_amd import runtime as R
    rt = types.SimpleNamespace(ema_state=dict(ema=None, momentum=0.1, interval=1, warm_up=1, swapped=True))
    with pytest.raises(RuntimeError, match="swap"):
        R.DetectorRuntime._ema_update(rt, 0)


# ---------------------------------------------------------------------- arithmetic
@pytest.mark.parametrize("m", MOMENTA)
def test_numpy_restatement_equals_torch_cpu(m):
    ema, p = inputs(4099, seed=11)
    assert (bits(ema) == 0x80000000).any() and (bits(p) == 0x80000000).any() and (bits(ema) == 0).any() and (bits(p) == 0).any()
    want = torch_ema(ema, p, m)
    got = numpy_ema(ema.numpy(), p.numpy(), m)
    assert np.array_equal(bits(got), bits(want))
    # the form with two separately rounded products is NOT the yardstick (it would hide a kernel that contracts nothing)
    two = (ema.numpy() * np.float32(1 - m)).astype(np.float32) + (p.numpy() * np.float32(m)).astype(np.float32)
    if m in (1 / 100, 38 / 137):
        assert (bits(two) != bits(want)).any()
    chained = want
    for _ in range(3):                                         # a short chain, as the hook runs it
        chained = torch_ema(chained, p, m)
        got = numpy_ema(got, p.numpy(), m)
    assert np.array_equal(bits(got), bits(chained))


# ---------------------------------------------------------------------- checkpoint entries
@pytest.fixture(scope="module")
def det():
    from radet_amd.models import build_detector
    cfg = load_cfg()
    torch.manual_seed(0)
    return build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)


def test_ema_key_naming_and_state_dict_entries(det):
    from radet_amd.apis.train import ema_state_dict, load_ema_state_dict
    from radet_amd.runtime import FlatParams, ema_key
    assert ema_key("backbone.layer1.0.conv1.weight") == "ema_backbone_layer1_0_conv1_weight"
    assert ema_key("bbox_head.scales.0.scale") == "ema_bbox_head_scales_0_scale" and ema_key("w") == "ema_w"
    flat = FlatParams(det, "cpu")
    ema = torch.arange(flat.n_train, dtype=torch.float32)
    rt = types.SimpleNamespace(flat=flat, ema_state=dict(ema=ema))
    sd = ema_state_dict(det, rt)
    names = [n for n, _ in det.named_parameters()]
    assert sorted(sd) == sorted(ema_key(n) for n in names) and len(sd) == len(names)
    frozen = [n for n, p in det.named_parameters() if not p.requires_grad]
    assert frozen and set(names) - set(frozen) == set(flat.train_names)
    for n, p in det.named_parameters():
        e = sd[ema_key(n)]
        assert e.shape == p.shape
        if n in frozen:                                        # not averaged: a copy of the parameter
            assert torch.equal(e, p.detach())
        else:
            o = flat.offsets[n]
            assert torch.equal(e.reshape(-1), ema[o:o + p.numel()])
    # back into an arena: the same bits; a file without entries restarts the EMA from the parameters; half a set is refused
    rt2 = types.SimpleNamespace(flat=flat, ema_state=dict(ema=torch.zeros(flat.n_train)))
    assert load_ema_state_dict(det, rt2, sd) is True
    for n in flat.train_names:
        o, k = flat.offsets[n], flat.p[n].numel()
        assert torch.equal(rt2.ema_state["ema"][o:o + k], ema[o:o + k])
    assert load_ema_state_dict(det, rt2, {}) is False and torch.equal(rt2.ema_state["ema"], flat.params)
    part = dict(sd)
    del part[ema_key(flat.train_names[-1])]
    with pytest.raises(KeyError, match=re.escape(flat.train_names[-1])):
        load_ema_state_dict(det, rt2, part)


# ---------------------------------------------------------------------- configuration
def test_custom_hooks_parsing():
    from radet_amd.apis.train import parse_custom_hooks
    assert parse_custom_hooks(load_cfg()) is None and parse_custom_hooks(load_cfg(custom_hooks=[])) is None
    shipped = load_cfg(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr_ema.py"))
    assert parse_custom_hooks(shipped) == dict(momentum=0.0002, interval=1, warm_up=100)          # mmcv's defaults
    assert parse_custom_hooks(load_cfg(custom_hooks=[dict(type="EMAHook")])) == dict(momentum=0.0002, interval=1, warm_up=100)
    hook = dict(type="EMAHook", momentum=0.01, interval=3, warm_up=7, priority="NORMAL", resume_from=None)
    assert parse_custom_hooks(load_cfg(custom_hooks=[hook])) == dict(momentum=0.01, interval=3, warm_up=7)
    base = {k: v for k, v in dict(load_cfg()._cfg_dict).items()}
    rest = {k: v for k, v in dict(shipped._cfg_dict).items() if k != "custom_hooks"}
    assert rest == base                                        # the shipped file is the base file plus the hook


@pytest.mark.parametrize("hook,err,match", [
    (dict(type="EMAHook", momentum=0.0), ValueError, "momentum"),
    (dict(type="EMAHook", momentum=1.0), ValueError, "momentum"),
    (dict(type="EMAHook", momentum=-0.1), ValueError, "momentum"),
    (dict(type="EMAHook", interval=0), ValueError, "interval"),
    (dict(type="EMAHook", interval=1.5), ValueError, "interval"),
    (dict(type="EMAHook", resume_from="work_dirs/latest.pth"), NotImplementedError, "resume_from"),
    (dict(type="NumClassCheckHook"), NotImplementedError, "NumClassCheckHook"),
    (dict(type="EMAHook", decay=0.99), KeyError, "decay"),
])
def test_custom_hooks_refusals(hook, err, match):
    from radet_amd.apis.train import parse_custom_hooks
    with pytest.raises(err, match=match):
        parse_custom_hooks(load_cfg(custom_hooks=[hook]))


def test_unknown_hook_is_refused_beside_an_ema_hook_and_by_train_detector():
    """the refusal comes before anything touches the model: train_detector on an object that is no model at all"""
    from radet_amd.apis import train_detector
    from radet_amd.apis.train import parse_custom_hooks
    hooks = [dict(type="EMAHook"), dict(type="SyncNormHook", priority=48)]
    with pytest.raises(NotImplementedError, match="SyncNormHook"):
        parse_custom_hooks(load_cfg(custom_hooks=hooks))
    with pytest.raises(NotImplementedError, match="SyncNormHook"):
        train_detector(object(), [], load_cfg(custom_hooks=hooks))
    with pytest.raises(ValueError, match="more than one"):
        parse_custom_hooks(load_cfg(custom_hooks=[dict(type="EMAHook"), dict(type="EMAHook", momentum=0.1)]))


def test_init_ema_validates_without_a_device():
    from radet_amd.runtime import DetectorRuntime
    rt = types.SimpleNamespace()
    for kw in (dict(momentum=0.0), dict(momentum=1.0), dict(interval=0), dict(interval=True), dict(interval=2.0)):
        with pytest.raises(ValueError):
            DetectorRuntime.init_ema(rt, **kw)
    with pytest.raises(RuntimeError, match="init_ema"):
        DetectorRuntime.swap_ema(types.SimpleNamespace(ema_state=None))


def test_sync_replicas_broadcasts_the_ema_arena(monkeypatch):
    """data-parallel start-up: the EMA arena travels with the parameter arenas (the collective replaced by a recorder)"""
    from radet_amd import runtime as R
    sent = []
    monkeypatch.setattr(R.dist, "is_available", lambda: True)
    monkeypatch.setattr(R.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(R.dist, "get_world_size", lambda: 2)
    monkeypatch.setattr(R.dist, "broadcast", lambda t, src: sent.append((t, src)))
    params, frozen, ema = torch.zeros(8), torch.zeros(4), torch.ones(8)
    rt = types.SimpleNamespace(flat=types.SimpleNamespace(params=params, frozen=frozen), opt_state=None, step_count=3, dev="cpu",
                               ema_state=None)
    assert R.DetectorRuntime.sync_replicas(rt, src=1) is True
    assert len(sent) == 3 and sent[0][0] is params and sent[1][0] is frozen               # no EMA: what it sent before
    sent.clear()
    rt.ema_state = dict(ema=ema)
    assert R.DetectorRuntime.sync_replicas(rt, src=1) is True
    assert len(sent) == 4 and sent[2][0] is ema and all(src == 1 for _, src in sent)      # params, frozen, EMA, step counter


# ---------------------------------------------------------------------- C ABI
def test_entry_points_are_declared():
    import ctypes as C
    from radet_amd import _lib
    hdr = open(os.path.join(REPO, "include", "radet_hip.h")).read()
    assert "int radet_ema_update(float* ema, const float* p, size_t n, float momentum, float one_minus, void* stream);" in hdr
    assert "int radet_ema_swap(float* a, float* b, size_t n, void* stream);" in hdr
    p, f, z = C.c_void_p, C.c_float, C.c_size_t
    assert _lib.SIGNATURES["radet_ema_update"] == (C.c_int, [p, p, z, f, f, p])
    assert _lib.SIGNATURES["radet_ema_swap"] == (C.c_int, [p, p, z, p])
    thunks = open(os.path.join(REPO, "radet_amd", "csrc", "tape_thunks.c")).read()
    for name in ("radet_ema_update", "radet_ema_swap"):
        assert f'{{"{name}", t_{name}, {len(_lib.SIGNATURES[name][1])}}}' in thunks
