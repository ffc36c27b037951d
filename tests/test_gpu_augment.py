"""Image side of the BOP data pipeline on the GPU: the augmentation kernels (csrc/augment.hip) against the NumPy
restatement (tests/_augment_ref.py, itself pinned to Pillow by tests/test_augment_cpu.py), the loader against a host
restatement of the reference's stage order fed the same per-sample seeds, and training / detection fed by the loader."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _augment_ref as R  # noqa: E402
from oracle import masks as om  # noqa: E402

pytestmark = pytest.mark.gpu

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
COSY = [dict(type="PillowBlur", p=1., factor_interval=(1, 3)),
        dict(type="PillowSharpness", p=0.3, factor_interval=(0., 50.)),
        dict(type="PillowContrast", p=0.3, factor_interval=(0.2, 50.)),
        dict(type="PillowBrightness", p=0.5, factor_interval=(0.1, 6.0)),
        dict(type="PillowColor", p=0.3, factor_interval=(0., 20.))]
ASSIGNER = dict(type="LabelAssignment",
                anchor_generator_cfg=dict(type="AnchorGenerator", ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                          strides=[8, 16, 32, 64, 128]),
                neg_threshold=0.2, positive_num=10, adapt_positive_num=False, balance_sample=True)


def train_pipeline(background_dir, bg_prob=0.3, cosy_p=0.8):
    return [
        dict(type="LoadImageFromFile"),
        dict(type="LoadAnnotations", with_bbox=True, with_bop_mask=True),
        dict(type="Resize", img_scale=(640, 480), keep_ratio=True),
        dict(type="RandomBackground", background_dir=background_dir, prob=bg_prob),
        dict(type="CosyPoseAug", p=cosy_p, pipelines=COSY),
        dict(type="RandomFlip", flip_ratio=0.5),
        dict(type="GenerateDistanceMap"),
        ASSIGNER,
        dict(type="Normalize", **NORM),
        dict(type="Pad", size_divisor=16),
        dict(type="DefaultFormatBundle"),
        dict(type="Collect", keys=["img", "gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight"]),
    ]


TEST_PIPELINE = [
    dict(type="LoadImageFromFile"),
    dict(type="MultiScaleFlipAug", img_scale=(640, 480), flip=False, transforms=[
        dict(type="Resize", keep_ratio=True),
        dict(type="RandomFlip"),
        dict(type="Normalize", **NORM),
        dict(type="Pad", size_divisor=32),
        dict(type="ImageToTensor", keys=["img"]),
        dict(type="Collect", keys=["img"])]),
]


def restate_image(img_bgr, resize_hw, background=None, masks=None, blur=None, sharp=None, contr=None, bright=None, col=None,
                  flip=False, pad_hw=None):
    """the reference's image path, restated on the host: Resize -> RandomBackground -> CosyPoseAug -> RandomFlip ->
    Normalize -> Pad; returns (f32 [3, Hp, Wp], resized masks after the flip)"""
    h, w = resize_hw
    x = R.resize_linear_u8(img_bgr, w, h)
    m = None if masks is None else om.transform(masks, resized_hw=(h, w), norm=True)
    if background is not None:
        x = R.merge_background(x, R.resize_linear_u8(background, w, h), m if m is not None else np.zeros((0, h, w), np.uint8))
    x = np.ascontiguousarray(R.cosypose(x[..., ::-1], blur, sharp, contr, bright, col)[..., ::-1])
    if flip:
        x = x[:, ::-1]
        m = None if m is None else om.flip(m)
    y = R.normalize(x, NORM["mean"], NORM["std"])
    Hp, Wp = pad_hw or (h, w)
    out = np.zeros((3, Hp, Wp), np.float32)
    out[:, :h, :w] = y
    return out, m


def test_augment_kernels_mixed_batch():
    """one batch, ragged sizes (widths not multiples of 4 / 16, 1-3 px sides), every image with its own set of stages"""
    from radet_amd.datasets.loading import Collect, ImagePipeline
    rng = np.random.RandomState(0)
    pipe = ImagePipeline([dict(type="LoadImageFromFile"), dict(type="Normalize", **NORM), dict(type="Pad", size_divisor=16),
                          dict(type="Collect", keys=["img"])])
    norm_cfg = dict(mean=np.array(NORM["mean"], np.float32), std=np.array(NORM["std"], np.float32), to_rgb=True)
    cases = [  # (src hw, resized hw, stages)
        ((48, 61), (48, 61), dict()),
        ((40, 50), (67, 83), dict(background=True)),
        ((33, 45), (33, 45), dict(blur=1)),
        ((29, 77), (29, 77), dict(blur=2, flip=True)),
        ((52, 37), (41, 29), dict(blur=3, background=True)),
        ((31, 53), (31, 53), dict(sharp=12.5)),
        ((3, 3), (3, 3), dict(sharp=0.0, contr=1.0)),
        ((2, 9), (2, 9), dict(blur=3, sharp=50.0, bright=6.0)),
        ((1, 1), (1, 1), dict(contr=0.2, col=20.0)),
        ((1, 3), (3, 1), dict(blur=2, col=0.0, flip=True)),
        ((45, 59), (45, 59), dict(contr=50.0)),
        ((26, 35), (26, 35), dict(bright=float(np.nextafter(np.float32(1), np.float32(2))))),
        ((37, 47), (37, 47), dict(col=0.37, flip=True)),
        ((50, 66), (57, 71), dict(background=True, blur=1, sharp=3.3, contr=0.6, bright=1.7, col=2.5, flip=True)),
    ]
    planned, expected = [], []
    for (sh, sw), (h, w), st in cases:
        img = rng.randint(0, 256, (sh, sw, 3)).astype(np.uint8)
        s = dict(img=img, resize_hw=(h, w), img_norm_cfg=norm_cfg, flip=st.get("flip", False), _collect=Collect(["img"]),
                 _nprnd=None, pad_shape=(-(-h // 16) * 16, -(-w // 16) * 16, 3))
        masks = None
        if st.get("background"):
            s["background"] = rng.randint(0, 256, (rng.randint(5, 70), rng.randint(5, 90), 3)).astype(np.uint8)
            masks = ((rng.rand(rng.randint(0, 4), sh, sw) < 0.4) * rng.choice([1, 255])).astype(np.uint8)
            s["gt_masks"] = masks
        for key, name in (("blur", "aug_blur"), ("sharp", "aug_sharpness"), ("contr", "aug_contrast"),
                          ("bright", "aug_brightness"), ("col", "aug_color")):
            if key in st:
                s[name] = st[key]
        planned.append(s)
        expected.append((img, (h, w), s.get("background"), masks, st))
    out = pipe.run(planned, collate=True)["img"].cpu().numpy()
    Hp, Wp = out.shape[2:]
    for i, (img, hw, bg, masks, st) in enumerate(expected):
        ref, _ = restate_image(img, hw, bg, masks, st.get("blur"), st.get("sharp"), st.get("contr"), st.get("bright"),
                               st.get("col"), st.get("flip", False), (Hp, Wp))
        np.testing.assert_array_equal(out[i], ref, err_msg=f"image {i}: {st}")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL decodes the generated JPEG / PNG files")
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=8, objects=(3, 6), n_backgrounds=3, seed=11)


def _dataset(tree, test_mode=False, **kw):
    from radet_amd.datasets import build_dataset
    pipe = TEST_PIPELINE if test_mode else train_pipeline(tree["background_dir"], **kw)
    return build_dataset(dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"],
                              seg_prefix=tree["seg_prefix"], pipeline=pipe, test_mode=test_mode))


def restate_sample(ds, idx, seed, epoch, background_dir):
    """the reference's train pipeline for sample idx on the sample's generators, restated on the host"""
    from PIL import Image
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.utils import build_from_cfg
    from radet_amd.datasets import PIPELINES
    rnd, nprnd = sample_generators(seed, epoch, idx)
    info, ann = ds.data_infos[idx], ds.get_ann_info(idx)
    img = np.asarray(Image.open(os.path.join(ds.img_prefix, info["filename"])).convert("RGB"))[..., ::-1]
    masks = np.stack([np.asarray(Image.open(os.path.join(ds.seg_prefix, p))) for p in ann["masks"]])
    h0, w0 = img.shape[:2]
    f = min(640 / max(h0, w0), 480 / min(h0, w0))
    w, h = int(w0 * f + 0.5), int(h0 * f + 0.5)
    sf = np.array([w / w0, h / h0, w / w0, h / h0], np.float32)
    boxes = ann["bboxes"] * sf
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, w)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, h)
    bg = None
    if not rnd.random() > 0.3:
        bgs = sorted(os.path.join(background_dir, n) for n in os.listdir(background_dir))
        bg = np.asarray(Image.open(rnd.choice(bgs)).convert("RGB"))[..., ::-1]
    aug = {}
    if not rnd.random() > 0.8:
        aug["blur"] = rnd.randint(1, 3)
        for key, (p, iv) in zip(("sharp", "contr", "bright", "col"),
                                ((0.3, (0., 50.)), (0.3, (0.2, 50.)), (0.5, (0.1, 6.0)), (0.3, (0., 20.)))):
            if rnd.random() <= p:
                aug[key] = rnd.uniform(*iv)
    flip = nprnd.choice(["horizontal", None], p=[0.5, 0.5]) is not None
    if flip:
        boxes = np.stack([w - boxes[:, 2], boxes[:, 1], w - boxes[:, 0], boxes[:, 3]], axis=1)
    x, m = restate_image(img, (h, w), bg, masks, flip=flip, pad_hw=(-(-h // 16) * 16, -(-w // 16) * 16), **aug)
    assigner = build_from_cfg(ASSIGNER, PIPELINES)
    p2g, pw = assigner.assign_batch([boxes], [np.ascontiguousarray(m)], (h, w), rngs=[nprnd])
    return dict(img=x, gt_bboxes=boxes, gt_labels=ann["labels"], p2g=p2g[0].cpu().numpy(), pw=pw[0].cpu().numpy(), flip=flip,
                aug=aug, bg=bg is not None, img_shape=(h, w, 3), scale_factor=sf)


def test_loader_equals_host_restatement(tree):
    from radet_amd.datasets import build_dataloader
    ds = _dataset(tree, bg_prob=0.3, cosy_p=0.8)
    loader = build_dataloader(ds, samples_per_gpu=4, workers=4, seed=5)
    n, stages = 0, set()
    for batch, idxs in zip(loader, loader.batches()):
        assert batch["img"].shape == (4, 3, 480, 640) and batch["img"].is_cuda
        img = batch["img"].cpu().numpy()
        for j, idx in enumerate(idxs):
            ref = restate_sample(ds, idx, 5, 0, tree["background_dir"])
            np.testing.assert_array_equal(img[j], ref["img"], err_msg=f"sample {idx}: {ref['aug']}, bg {ref['bg']}")
            np.testing.assert_array_equal(batch["gt_bboxes"][j].numpy(), ref["gt_bboxes"])
            np.testing.assert_array_equal(batch["gt_labels"][j].numpy(), ref["gt_labels"])
            np.testing.assert_array_equal(batch["points_to_gt_index"][j].cpu().numpy(), ref["p2g"])
            np.testing.assert_array_equal(batch["points_weight"][j].cpu().numpy(), ref["pw"])
            meta = batch["img_metas"][j]
            assert meta["flip"] == ref["flip"] and tuple(meta["img_shape"]) == ref["img_shape"]
            assert meta["pad_shape"] == (480, 640, 3) and np.array_equal(meta["scale_factor"], ref["scale_factor"])
            stages |= set(ref["aug"]) | ({"bg"} if ref["bg"] else set()) | ({"flip"} if ref["flip"] else set())
            n += 1
    assert n == 8 and {"blur", "flip"} <= stages
    # a single sample (global generators) is the same path with B = 1
    import random
    random.seed(3)
    np.random.seed(3)
    one = ds[2]
    assert one["img"].shape == (3, 480, 640) and one["points_to_gt_index"].shape == one["points_weight"].shape


@pytest.fixture(scope="module")
def cfg_det():
    from oracle import synth
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    d = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    synth.fill_state_dict(d.state_dict(), seed=0)
    return cfg, d.cuda()


def test_train_detector_from_loader(tree, cfg_det):
    from radet_amd.apis import train_detector
    from radet_amd.datasets import build_dataloader
    cfg, det = cfg_det
    cfg.merge_from_dict({"lr_config.total_steps": 40, "log_config.interval": 1})
    ds = _dataset(tree)
    loader = build_dataloader(ds, samples_per_gpu=4, workers=4, seed=0)

    def batches():
        epoch = 0
        while True:
            loader.set_epoch(epoch)
            yield from loader
            epoch += 1
    hist = train_detector(det, batches(), cfg, max_iters=6, log=lambda *_: None)
    assert len(hist) == 6 and all(np.isfinite(h).all() for h in hist)
    assert det.runtime().tape_stats()["replays"] > 0


def test_test_loader_feeds_simple_test(tree, cfg_det):
    from PIL import Image
    from radet_amd.datasets import build_dataloader
    _, det = cfg_det
    det.eval()
    ds = _dataset(tree, test_mode=True)
    loader = build_dataloader(ds, samples_per_gpu=2, workers=2, seed=0, shuffle=False)
    batch = next(iter(loader))
    assert isinstance(batch["img"], list) and batch["img"][0].shape == (2, 3, 480, 640)
    metas = batch["img_metas"][0]
    host = []
    for i in range(2):
        img = np.asarray(Image.open(os.path.join(ds.img_prefix, ds.data_infos[i]["filename"])).convert("RGB"))[..., ::-1]
        host.append(restate_image(img, (480, 640), pad_hw=(480, 640))[0])
    ref_in = torch.from_numpy(np.stack(host)).cuda()
    assert torch.equal(batch["img"][0], ref_in)
    with torch.no_grad():
        a = det(img=batch["img"], img_metas=batch["img_metas"], return_loss=False, rescale=True)
        b = det(img=[ref_in], img_metas=[metas], return_loss=False, rescale=True)
    assert len(a) == 2
    for ra, rb in zip(a, b):
        for ca, cb in zip(ra, rb):
            np.testing.assert_array_equal(ca, cb)
    det.train()
