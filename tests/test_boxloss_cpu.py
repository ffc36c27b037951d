"""Box regression losses beside GIoU (IoULoss, DIoULoss, CIoULoss), the parts that need no GPU: the registry, the
`*_ciou` config, the fixture's edge cases and how DetectorRuntime.set_loss_from_head maps a `loss_bbox` module to the
fused head loss's kind and eps."""
import os
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("iou", "iou_linear", "diou", "ciou")
REDS = ("mean", "avg_w", "none_w", "sum")


def test_classes_build_with_the_reference_defaults():
    from radet_amd import models
    from radet_amd.models import build_loss
    for name, kind in (("IoULoss", "iou"), ("DIoULoss", "diou"), ("CIoULoss", "ciou")):
        m = build_loss(dict(type=name))
        assert type(m) is getattr(models, name) and name in models.__all__
        assert (m.eps, m.reduction, m.loss_weight) == (1e-6, "mean", 1.0) and m.box_loss_kind() == kind
    m = build_loss(dict(type="IoULoss"))
    assert m.linear is False
    m = build_loss(dict(type="IoULoss", linear=True, eps=1e-3, reduction="sum", loss_weight=0.5))
    assert (m.linear, m.eps, m.reduction, m.loss_weight, m.box_loss_kind()) == (True, 1e-3, "sum", 0.5, "iou_linear")
    assert build_loss(dict(type="GIoULoss", loss_weight=2.0)).box_loss_kind() == "giou"


def test_bounded_iou_loss_still_fails_to_build():
    from radet_amd.models import LOSSES, build_loss
    assert "BoundedIoULoss" not in LOSSES.module_dict
    with pytest.raises(KeyError, match="BoundedIoULoss"):
        build_loss(dict(type="BoundedIoULoss"))


def test_kind_numbers_match_the_header():
    from radet_amd import kernels as K
    hdr = open(os.path.join(REPO, "include", "radet_hip.h")).read()
    names = dict(giou="GIOU", iou="IOU", iou_linear="IOU_LINEAR", diou="DIOU", ciou="CIOU")
    for kind, word in names.items():
        assert f"#define RADET_BOX_LOSS_{word} {K.BOX_LOSS_KINDS[kind]}\n" in hdr
    assert f"#define RADET_BOX_LOSS_KINDS {len(names)}\n" in hdr and len(K.BOX_LOSS_KINDS) == len(names)
    assert f"#define RADET_HEAD_LOSS_POSTACT {K.HEAD_LOSS_POSTACT}\n" in hdr
    assert f"#define RADET_HEAD_LOSS_KIND_SHIFT {K.HEAD_LOSS_KIND_SHIFT}\n" in hdr
    assert K.head_loss_flags() == 0 and K.head_loss_flags(postact=True) == 1          # every earlier caller's flags
    assert K.head_loss_flags("ciou") == 8 and K.head_loss_flags("iou", postact=True) == 3


def test_fixture_holds_the_edge_cases(golden):
    g = golden("box_losses")
    p, t, w = g["pred"], g["tgt"], g["w"]
    n0 = int(g["n_ops2"])
    g2 = golden("ops2")
    assert n0 == 90 and p.shape == (120, 4) and t.shape == (120, 4) and w.shape == (120,) and len(g["edge_notes"]) == 30
    assert np.array_equal(p[:n0], g2["g_pred"]) and np.array_equal(t[:n0], g2["g_tgt"]) and np.array_equal(w[:n0], g2["g_w"])
    # what torch's autograd did at the ties when the fixture was written: max, min split, clamp passes at equality
    assert g["ties"].tolist() == [0.5, 0.5, 1.0, 1.0]
    iw = np.minimum(p[:, 2], t[:, 2]) - np.maximum(p[:, 0], t[:, 0])
    ih = np.minimum(p[:, 3], t[:, 3]) - np.maximum(p[:, 1], t[:, 1])
    inter = np.clip(iw, 0, None).astype(np.float64) * np.clip(ih, 0, None)
    area = lambda b: (b[:, 2] - b[:, 0]).astype(np.float64) * (b[:, 3] - b[:, 1])   # noqa: E731
    iou = inter / np.maximum(area(p) + area(t) - inter, 1e-6)
    ident = (p == t).all(1)
    assert ident[:5].all() and ident.sum() == 6                                      # ops2's five + the zero-size one
    assert ((iw < 0) | (ih < 0)).sum() >= 5                                          # disjoint
    touching = ((iw == 0) | (ih == 0)) & (iw >= 0) & (ih >= 0) & (area(p) > 0) & (area(t) > 0)
    assert touching.sum() >= 3                                                       # clamp(min=0) at exactly 0
    nested = ((p[:, 0] >= t[:, 0]) & (p[:, 1] >= t[:, 1]) & (p[:, 2] <= t[:, 2]) & (p[:, 3] <= t[:, 3]) & ~ident) | \
             ((t[:, 0] >= p[:, 0]) & (t[:, 1] >= p[:, 1]) & (t[:, 2] <= p[:, 2]) & (t[:, 3] <= p[:, 3]) & ~ident)
    assert nested.sum() >= 5
    ties = (p == t) & ~ident[:, None]                                                # single max / min ties
    assert ties.any(0).all() and ties.sum() >= 8
    assert ((p[:, 2] == p[:, 0]) & (p[:, 3] > p[:, 1])).sum() >= 2                   # zero width
    assert ((p[:, 3] == p[:, 1]) & (p[:, 2] > p[:, 0])).sum() >= 2                   # zero height
    assert ((t[:, 2] == t[:, 0]) & (t[:, 3] == t[:, 1])).sum() >= 2                  # zero-size target
    same_wh = ((p[:, 2] - p[:, 0]) == (t[:, 2] - t[:, 0])) & ((p[:, 3] - p[:, 1]) == (t[:, 3] - t[:, 1])) & ~ident
    assert same_wh.sum() >= 3                                                        # v == 0 exactly
    below = (iou > 0) & (iou < 1e-6)
    assert below.sum() >= 2                                                          # IoULoss' clamp holds the gradient
    assert np.allclose(g["iou_none_w"][below], 2.0 * w[below] * -np.log(1e-6), rtol=1e-6)
    assert (g["iou_none_w_g"][below] == 0).all() and (g["iou_linear_none_w_g"][below] == 0).all()
    assert (np.abs(g["diou_none_w_g"][below]).sum(1) > 0).all()
    # equality with the clamp: IoU == eps == 0.25 and the gradient passes
    assert float(g["eq_eps"]) == 0.25 and np.abs(g["iou_eq_g"]).sum() > 0 and np.abs(g["iou_linear_eq_g"]).sum() > 0
    assert np.isclose(float(g["iou_eq"]), -np.log(0.25)) and float(g["iou_linear_eq"]) == 0.75
    # CIoU runs on pred_ciou: the reference's own fp32 result on an identical pair is NaN (0 / 0 in the penalty)
    pc = g["pred_ciou"]
    assert np.isnan(g["ciou_ident"]).all() and np.array_equal(pc[5:], p[5:]) and np.array_equal(pc[:5, 2], p[:5, 2] + 0.5)
    assert np.array_equal(pc[:5, [0, 1, 3]], t[:5, [0, 1, 3]])
    for kind in KINDS:
        for red in REDS:
            tag = f"{kind}_{red}"
            for k, shape in ((tag, (120,) if red == "none_w" else ()), (tag + "_g", (120, 4))):
                assert g[k].dtype == np.float32 and g[k + "_64"].dtype == np.float64 and g[k + "_m"].dtype == np.bool_
                assert g[k].shape == shape == g[k + "_64"].shape == g[k + "_m"].shape and np.isfinite(g[k]).all()
                assert g[k + "_m"].mean() <= 0.02                                    # the cap on fp64-judged elements
        for k in ("loss_cls", "loss_bbox", "loss_iou", "g_reg_pos", "g_iou_pos", "g_cls_pos"):
            assert np.isfinite(g[f"h_{kind}_{k}"]).all()
    h = golden("head_loss")
    assert g["h_ciou_g_reg_pos"].shape == h["g_reg_pos"].shape
    assert len({float(g[f"h_{k}_loss_bbox"]) for k in KINDS} | {float(h["loss_bbox"])}) == 5     # five different losses
    for kind in KINDS:                                                               # the other branches do not see the kind
        assert np.array_equal(g[f"h_{kind}_loss_cls"], h["loss_cls"]) and np.array_equal(g[f"h_{kind}_loss_iou"], h["loss_iou"])
        assert np.array_equal(g[f"h_{kind}_g_iou_pos"], h["g_iou_pos"]) and np.array_equal(g[f"h_{kind}_g_cls_pos"], h["g_cls_pos"])


def test_ciou_config_loads():
    from radet_amd.models import build_loss
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr_ciou.py"))
    base = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    assert dict(cfg.model["bbox_head"]["loss_bbox"]) == dict(type="CIoULoss", loss_weight=2.0)
    m = build_loss(cfg.model["bbox_head"]["loss_bbox"])
    assert type(m).__name__ == "CIoULoss" and m.loss_weight == 2.0 and m.eps == 1e-6
    strip = lambda c: {k: v for k, v in dict(c.model["bbox_head"]).items() if k != "loss_bbox"}   # noqa: E731
    assert strip(cfg) == strip(base) and dict(cfg.model["backbone"]) == dict(base.model["backbone"])
    assert dict(cfg.train_cfg) == dict(base.train_cfg) and dict(cfg.data) == dict(base.data)


def _stub_head(loss_bbox):
    from radet_amd.models import build_loss
    cls = build_loss(dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0))
    iou = build_loss(dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0))
    return types.SimpleNamespace(loss_cls=cls, loss_bbox=loss_bbox, loss_iou=iou)


def test_set_loss_from_head_maps_class_to_kind_and_eps():
    """on a stub runtime: DetectorRuntime needs a GPU to construct, set_loss_from_head only its `dev` for the weights"""
    from radet_amd.models import build_loss
    from radet_amd.models.losses import CIoULoss
    from radet_amd.runtime import DetectorRuntime
    rt = types.SimpleNamespace(dev="cpu")
    for cfg, kind, eps in ((dict(type="GIoULoss", loss_weight=2.0), "giou", 1e-6),
                           (dict(type="IoULoss", loss_weight=1.5), "iou", 1e-6),
                           (dict(type="IoULoss", linear=True, eps=1e-4), "iou_linear", 1e-4),
                           (dict(type="DIoULoss", eps=1e-7), "diou", 1e-7),
                           (dict(type="CIoULoss", loss_weight=2.0), "ciou", 1e-6)):
        DetectorRuntime.set_loss_from_head(rt, _stub_head(build_loss(cfg)))
        hp = rt.loss_hparams
        assert (hp["box_kind"], hp["box_eps"], hp["lbw"]) == (kind, eps, float(cfg.get("loss_weight", 1.0))), cfg
        assert (hp["alpha"], hp["gamma"]) == (0.25, 2.0) and rt.loss_weights is None

    class MyCIoU(CIoULoss):                     # a subclass may compute anything
        pass

    class BoundedIoULoss:                       # someone's own module under the reference's name
        eps, reduction, loss_weight = 1e-3, "mean", 1.0

    for bad in (MyCIoU(), BoundedIoULoss()):
        rt.loss_hparams = None
        with pytest.raises(NotImplementedError, match=type(bad).__name__):
            DetectorRuntime.set_loss_from_head(rt, _stub_head(bad))
        assert rt.loss_hparams is None          # nothing set: no silent GIoU
    with pytest.raises(NotImplementedError, match="reduction"):
        DetectorRuntime.set_loss_from_head(rt, _stub_head(build_loss(dict(type="DIoULoss", reduction="sum"))))
