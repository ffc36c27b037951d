"""Soft-NMS without a GPU: the NumPy restatements agree with each other (mmcv's literal loops, the vectorised step, the
per-class decomposition), and the host-side layers (header defines, refusals, config) are in place."""
import os
import re

import numpy as np
import pytest

from _softnms_ref import (METHODS, batched_soft_nms, per_class_soft_nms, soft_nms_fast, soft_nms_literal)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_case(rng, n, classes=4, zero_area=True, low=True):
    """n boxes in a 100 x 100 window, heavy overlaps, distinct scores; some zero-area boxes, some scores below 1e-3"""
    c = rng.uniform(10, 90, (n, 2))
    wh = rng.uniform(4, 40, (n, 2))
    if zero_area and n:
        wh[rng.random(n) < 0.1] = 0
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    scores = rng.permutation(np.linspace(0.02, 0.99, n)).astype(np.float32)          # tie-free
    if low and n:
        mode = rng.integers(0, 3)
        if mode == 1:
            scores[rng.random(n) < 0.3] *= np.float32(1e-2)
        elif mode == 2:
            scores *= np.float32(5e-4)                                               # wholly below min_score
    labels = rng.integers(0, classes, n)
    return boxes, scores, labels


@pytest.mark.parametrize("method", sorted(METHODS))
def test_literal_equals_fast(method):
    rng = np.random.default_rng(METHODS[method])
    for _ in range(40):
        n = int(rng.integers(1, 61))
        boxes, scores, _ = random_case(rng, n)
        thr, sigma = float(rng.choice([0.1, 0.3, 0.5])), float(rng.choice([0.1, 0.5, 2.0]))
        kl, sl = soft_nms_literal(boxes, scores, METHODS[method], thr, sigma, 1e-3)
        kf, sf = soft_nms_fast(boxes, scores, METHODS[method], thr, sigma, 1e-3)
        if len(np.unique(sf)) != len(sf):
            continue                                        # a tie among decayed scores: mmcv's order is its swap history
        assert np.array_equal(kl, kf)
        assert np.array_equal(sl.view(np.uint32), sf.view(np.uint32))
        assert np.all(np.diff(sf) <= 0)


@pytest.mark.parametrize("method", sorted(METHODS))
def test_global_loop_equals_per_class_decomposition(method):
    rng = np.random.default_rng(10 + METHODS[method])
    seen_cut = False
    for _ in range(60):
        n = int(rng.integers(1, 61))
        boxes, scores, labels = random_case(rng, n)
        args = (METHODS[method], 0.3, 0.5, 1e-3)
        kg, sg = batched_soft_nms(boxes, scores, labels, *args)
        kl, sl = batched_soft_nms(boxes, scores, labels, *args, loop=soft_nms_literal)
        kc, sc = per_class_soft_nms(boxes, scores, labels, *args)
        assert np.array_equal(kg, kc) and np.array_equal(sg.view(np.uint32), sc.view(np.uint32))
        if len(np.unique(sg)) == len(sg):
            assert np.array_equal(kg, kl) and np.array_equal(sg.view(np.uint32), sl.view(np.uint32))
        assert np.all(np.diff(sg) <= 0)
        assert len(sg) >= 1 and np.all(sg[1:] >= np.float32(1e-3))
        seen_cut |= bool(sg[0] < np.float32(1e-3)) or len(kg) < len(np.unique(labels))
    assert seen_cut                                         # the min_score cut of the decomposition was exercised


def test_small_fixtures():
    m = METHODS
    # the case the hard-NMS dispatch gets wrong: IoU 0.6, linear, thr 0.3 -> both stay, the second decayed
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 6]], np.float32)
    k, s = soft_nms_fast(boxes, [0.9, 0.8], m["linear"], 0.3, 0.5, 1e-3)
    ovr = np.float32(60) / (np.float32(100) + np.float32(60) - np.float32(60))
    assert k.tolist() == [0, 1] and s[1] == np.float32(0.8) * (np.float32(1) - ovr)
    # IoU exactly at the threshold decays (>=)
    k, s = soft_nms_fast([[0, 0, 2, 2], [0, 0, 2, 1]], [0.9, 0.8], m["linear"], 0.5, 0.5, 1e-3)
    assert s[1] == np.float32(0.8) * np.float32(0.5)
    k, s = soft_nms_fast([[0, 0, 2, 2], [0, 0, 2, 1]], [0.9, 0.8], m["naive"], 0.5, 0.5, 1e-3)
    assert k.tolist() == [0]
    # equal scores: lower index first
    k, _ = soft_nms_fast([[0, 0, 1, 1], [5, 5, 6, 6], [9, 9, 10, 10]], [0.5, 0.7, 0.7], m["linear"], 0.3, 0.5, 1e-3)
    assert k.tolist() == [1, 2, 0]
    # the first pick survives below min_score, nothing else does
    k, _ = soft_nms_fast([[0, 0, 1, 1], [5, 5, 6, 6]], [5e-4, 4e-4], m["gaussian"], 0.3, 0.5, 1e-3)
    assert k.tolist() == [0]
    # two zero-area boxes: NaN IoU -> weight 1
    k, s = soft_nms_fast([[3, 3, 3, 3], [3, 3, 3, 3]], [0.9, 0.8], m["gaussian"], 0.3, 0.5, 1e-3)
    assert k.tolist() == [0, 1] and s[1] == np.float32(0.8)


def test_header_defines_match_kernels():
    from radet_amd import kernels as K
    header = open(os.path.join(REPO, "include", "radet_hip.h")).read()
    defs = {n.lower(): int(v) for n, v in re.findall(r"#define RADET_SOFT_NMS_(\w+) (\d+)", header)}
    assert defs == K.SOFT_NMS_METHODS == METHODS


def test_refusals_need_no_device():
    import torch

    from radet_amd import ops
    boxes, scores, labels = torch.zeros(3, 4), torch.ones(3), torch.zeros(3, dtype=torch.long)
    with pytest.raises(NotImplementedError):
        ops.soft_nms(boxes, scores, offset=1)
    with pytest.raises(ValueError):
        ops.soft_nms(boxes, scores, method="quadratic")
    with pytest.raises(ValueError):
        ops.soft_nms(boxes, scores, method="gaussian", sigma=0.0)
    with pytest.raises(ValueError):
        ops.batched_nms(boxes, scores, labels, dict(type="soft_nms", method="gaussian", sigma=-1.0))
    with pytest.raises(ValueError):
        ops.batched_nms(boxes, scores, labels, dict(type="soft_nms", method="none"))
    with pytest.raises(NotImplementedError):
        ops.batched_nms(boxes, scores, labels, dict(type="soft_nms", offset=1))
    with pytest.raises(NotImplementedError):
        ops.batched_nms(boxes, scores, labels, dict(type="soft_nms", split_thr=3))
    big = 10000
    with pytest.raises(NotImplementedError):
        ops.batched_nms(torch.zeros(big, 4), torch.ones(big), torch.zeros(big, dtype=torch.long), dict(type="soft_nms"))


def test_softnms_config_loads():
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr_softnms.py"))
    base = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    assert dict(cfg.test_cfg["nms"]) == dict(type="soft_nms", iou_threshold=0.3, sigma=0.5, min_score=1e-3, method="linear")
    for k in ("nms_pre", "min_bbox_size", "score_thr", "max_per_img"):
        assert cfg.test_cfg[k] == base.test_cfg[k]
    assert cfg.model == base.model
