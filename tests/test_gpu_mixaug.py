"""The mixpbr stages on the GPU: aug_hsv_noise / aug_box (csrc/augment.hip) against the NumPy restatement
(tests/_mixaug_ref.py, itself checked by tests/test_mixaug_cpu.py), a MixDataset loader batch against a host restatement
of the whole stage chain fed the same per-sample seeds, and training fed by a MixDataset loader."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _augment_ref as R  # noqa: E402
import _mixaug_ref as M  # noqa: E402
from oracle import masks as om  # noqa: E402

pytestmark = pytest.mark.gpu

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
ASSIGNER = dict(type="LabelAssignment",
                anchor_generator_cfg=dict(type="AnchorGenerator", ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                          strides=[8, 16, 32, 64, 128]),
                neg_threshold=0.2, positive_num=10, adapt_positive_num=False, balance_sample=True)


def mix_pipeline(background_dir):
    return [
        dict(type="LoadImageFromFile"),
        dict(type="LoadAnnotations", with_bbox=True, with_bop_mask=True),
        dict(type="Resize", img_scale=(640, 480), keep_ratio=True),
        dict(type="RandomBackground", background_dir=background_dir, prob=0.3),
        dict(type="RandomHSV", h_ratio=0.2, s_ratio=0.5, v_ratio=0.5, prob=1.0),
        dict(type="RandomNoise", noise_ratio=0.1, prob=1.0),
        dict(type="RandomSmooth", max_kernel_size=7, prob=1.0),
        dict(type="RandomFlip", flip_ratio=0.5),
        dict(type="GenerateDistanceMap"),
        ASSIGNER,
        dict(type="Normalize", **NORM),
        dict(type="Pad", size_divisor=16),
        dict(type="DefaultFormatBundle"),
        dict(type="Collect", keys=["img", "gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight"]),
    ]


def _run_mix(images, stages, align=1):
    """images (u8 HWC) packed at multiples of `align` pixels -> aug_hsv_noise then aug_box with the given per-image stage
    dicts (aug_hsv / aug_noise / aug_smooth); returns (after hsv_noise, after box) per image"""
    from radet_amd import kernels as K
    from radet_amd.datasets.loading import ImagePipeline
    offs, o = [], 0
    for im in images:
        offs.append(o)
        o += -(-im.shape[0] * im.shape[1] // align) * align
    host = np.zeros(o * 3, np.uint8)
    for im, off in zip(images, offs):
        host[off * 3:off * 3 + im.size] = im.reshape(-1)
    hw = [im.shape[:2] for im in images]
    dev = torch.device("cuda", torch.cuda.current_device())
    src = torch.from_numpy(host).to(dev)
    mid = torch.full_like(src, 77)
    out = torch.full_like(src, 77)
    p2 = torch.from_numpy(ImagePipeline._params2(stages, offs, hw)).to(dev)
    n = len(images)
    K.augment_hsv_noise(src, p2, mid, n, max(h * w for h, w in hw))
    K.augment_box(mid, p2, out, n, max(h for h, _ in hw), max(w for _, w in hw))
    a, b = mid.cpu().numpy(), out.cpu().numpy()
    # bytes between images (alignment gaps) are never written
    gaps = np.ones(o * 3, bool)
    for im, off in zip(images, offs):
        gaps[off * 3:off * 3 + im.size] = False
    assert (a[gaps] == 77).all() and (b[gaps] == 77).all()
    return ([a[off * 3:off * 3 + im.size].reshape(im.shape) for im, off in zip(images, offs)],
            [b[off * 3:off * 3 + im.size].reshape(im.shape) for im, off in zip(images, offs)])


def test_hsv_kernel_all_colours_bit_exact():
    c = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([c & 255, (c >> 8) & 255, c >> 16], axis=1).astype(np.uint8).reshape(4096, 4096, 3)
    triples = [(0.8, 0.5, 0.5), (1.2, 1.5, 1.5), (0.93, 1.27, 0.61), (1.0, 1.0, 1.0),
               (float(np.nextafter(1.0, 0.0)), 1.0000001, 0.9999999)]
    for t in triples:
        got, _ = _run_mix([img], [dict(aug_hsv=t)])
        np.testing.assert_array_equal(got[0], M.random_hsv(img, *t), err_msg=str(t))


def _noise_ok(got, img, sigma, key):
    """equal except where the restated img + x lies within 1e-9 of an integer (ocml's fp64 log / sin / cos and the
    host's may differ in the last ulp); returns the number of such bytes that differ"""
    x = M.noise_sum(img, sigma, key)
    want = np.clip(x, 0, 255).astype(np.uint8)
    bad = got != want
    if bad.any():
        edge = np.abs(x - np.rint(x)) < 1e-9
        assert (bad <= edge).all(), f"{int((bad & ~edge).sum())} bytes differ away from an integer"
        assert (np.abs(got.astype(int) - want.astype(int))[bad] <= 1).all()
    return int(bad.sum())


def test_noise_kernel_mixed_sizes():
    rng = np.random.RandomState(3)
    sizes = [(1, 1), (1, 3), (2, 5), (7, 3), (4, 4), (33, 47), (64, 101), (480, 640)]
    keys = [rng.randint(0, 2 ** 64, size=2, dtype=np.uint64) for _ in sizes]
    sigmas = [0.1, 0.0, 0.05, 0.1, 1e-3, 0.0999, 0.037, 0.1]
    images = [rng.randint(0, 256, (*hw, 3)).astype(np.uint8) for hw in sizes]
    images[-1][:40] = 0
    images[-1][40:80] = 255
    stages = [dict(aug_noise=(s, k)) for s, k in zip(sigmas, keys)]
    for align in (1, 4):
        got, _ = _run_mix(images, stages, align=align)
        edge = sum(_noise_ok(g, im, s, k) for g, im, s, k in zip(got, images, sigmas, keys))
        assert edge <= 8
    # sigma 0 and no noise stage leave the image as it was
    np.testing.assert_array_equal(got[1], images[1])


def test_hsv_then_noise_in_one_pass():
    rng = np.random.RandomState(5)
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (16, 16), (5, 9))]
    keys = [rng.randint(0, 2 ** 64, size=2, dtype=np.uint64) for _ in images]
    stages = [dict(aug_hsv=(1.1, 0.7, 1.4), aug_noise=(0.08, keys[0])), dict(aug_hsv=(0.85, 1.3, 0.6)),
              dict(aug_noise=(0.02, keys[2]))]
    got, _ = _run_mix(images, stages)
    _noise_ok(got[0], M.random_hsv(images[0], 1.1, 0.7, 1.4), 0.08, keys[0])
    np.testing.assert_array_equal(got[1], M.random_hsv(images[1], 0.85, 1.3, 0.6))
    _noise_ok(got[2], images[2], 0.02, keys[2])


def test_box_kernel_mixed_sizes():
    rng = np.random.RandomState(7)
    sizes = [(4, 4), (5, 7), (8, 5), (6, 8), (7, 6), (1, 1), (2, 3), (16, 64), (17, 65), (31, 129), (100, 131), (480, 640)]
    for align in (1, 4):
        for k in (1, 3, 5, 7):
            images = [rng.randint(0, 256, (*hw, 3)).astype(np.uint8) for hw in sizes]
            _, got = _run_mix(images, [dict(aug_smooth=k) for _ in sizes], align=align)
            for g, im in zip(got, images):
                np.testing.assert_array_equal(g, M.box_filter(im, k), err_msg=f"k {k}, {im.shape}, align {align}")
    # every image with its own k, and the box off for one
    images = [rng.randint(0, 256, (*hw, 3)).astype(np.uint8) for hw in sizes[:5]]
    ks = [7, None, 3, 5, 1]
    _, got = _run_mix(images, [dict(aug_smooth=k) if k else {} for k in ks])
    for g, im, k in zip(got, images, ks):
        np.testing.assert_array_equal(g, M.box_filter(im, k or 1))


# ------------------------------------------------------------------------------------------------ the loader
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL decodes the generated JPEG / PNG files")
    from tools.synth_bop import write_tree
    pbr = write_tree(str(tmp_path_factory.mktemp("pbr")), n_frames=6, objects=(3, 6), n_backgrounds=3, seed=31)
    real = write_tree(str(tmp_path_factory.mktemp("real")), n_frames=2, objects=(2, 4), n_backgrounds=1, seed=32)
    return pbr, real


def _mix_dataset(trees):
    from radet.datasets import build_dataset
    pbr, real = trees
    pipe = mix_pipeline(pbr["background_dir"])
    return build_dataset(dict(
        type="MixDataset",
        dataset_0=dict(type="BOPDataset", ann_file=pbr["ann_file"], img_prefix=pbr["img_prefix"], seg_prefix=pbr["seg_prefix"],
                       pipeline=pipe, ratio=2),
        dataset_1=dict(type="BOPDataset", ann_file=real["ann_file"], img_prefix=real["img_prefix"],
                       seg_prefix=real["seg_prefix"], pipeline=pipe, ratio=1)))


def restate_mix_sample(ds, idx, seed, epoch, background_dir):
    """the reference's mix train pipeline for wrapper index idx on the sample's generators, restated on the host;
    returns the normalised image, targets, and the restated img + x of the noise stage (for the ulp rule)"""
    from PIL import Image
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.datasets import PIPELINES
    from radet_amd.utils import build_from_cfg
    d, j = ds._locate(idx)
    sub = ds.datasets[d].dataset
    j %= len(sub)                                        # (index into the RepeatDataset -> the frame)
    rnd, nprnd = sample_generators(seed, epoch, idx)
    info, ann = sub.data_infos[j], sub.get_ann_info(j)
    img = np.asarray(Image.open(os.path.join(sub.img_prefix, info["filename"])).convert("RGB"))[..., ::-1]
    masks = np.stack([np.asarray(Image.open(os.path.join(sub.seg_prefix, p))) for p in ann["masks"]])
    h0, w0 = img.shape[:2]
    f = min(640 / max(h0, w0), 480 / min(h0, w0))
    w, h = int(w0 * f + 0.5), int(h0 * f + 0.5)
    sf = np.array([w / w0, h / h0, w / w0, h / h0], np.float32)
    boxes = ann["bboxes"] * sf
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, w)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, h)
    x = R.resize_linear_u8(img, w, h)
    m = om.transform(masks, resized_hw=(h, w), norm=True)
    bg = None
    if not rnd.random() > 0.3:
        bgs = sorted(os.path.join(background_dir, n) for n in os.listdir(background_dir))
        bg = np.asarray(Image.open(rnd.choice(bgs)).convert("RGB"))[..., ::-1]
        x = R.merge_background(x, R.resize_linear_u8(bg, w, h), m)
    rnd.random()
    hsv = tuple(rnd.uniform(-1, 1) * r + 1 for r in (0.2, 0.5, 0.5))
    x = M.random_hsv(x, *hsv)
    rnd.random()
    sigma = rnd.uniform(0, 0.1)
    key = nprnd.randint(0, 2 ** 64, size=2, dtype=np.uint64)
    xs = M.noise_sum(x, sigma, key)
    x = np.clip(xs, 0, 255).astype(np.uint8)
    rnd.random()
    k = rnd.choice([1, 3, 5, 7])
    x = M.box_filter(x, k)
    flip = nprnd.choice(["horizontal", None], p=[0.5, 0.5]) is not None
    if flip:
        boxes = np.stack([w - boxes[:, 2], boxes[:, 1], w - boxes[:, 0], boxes[:, 3]], axis=1)
        x = x[:, ::-1]
        m = om.flip(m)
    Hp, Wp = -(-h // 16) * 16, -(-w // 16) * 16
    out = np.zeros((3, Hp, Wp), np.float32)
    out[:, :h, :w] = R.normalize(np.ascontiguousarray(x), NORM["mean"], NORM["std"])
    assigner = build_from_cfg(ASSIGNER, PIPELINES)
    p2g, pw = assigner.assign_batch([boxes], [np.ascontiguousarray(m)], (h, w), rngs=[nprnd])
    return dict(img=out, gt_bboxes=boxes, gt_labels=ann["labels"], p2g=p2g[0].cpu().numpy(), pw=pw[0].cpu().numpy(),
                flip=flip, k=k, bg=bg is not None, noise_sum=xs)


def test_mix_loader_equals_host_restatement(trees):
    from radet_amd.datasets import build_dataloader
    ds = _mix_dataset(trees)
    assert len(ds) == 14
    loader = build_dataloader(ds, samples_per_gpu=4, workers=4, seed=6)
    stdinv = 1.0 / np.asarray(NORM["std"], np.float32).min()
    n, seen, edge = 0, set(), 0
    for batch, idxs in zip(loader, loader.batches()):
        assert batch["img"].shape == (4, 3, 480, 640) and batch["img"].is_cuda
        img = batch["img"].cpu().numpy()
        for j, idx in enumerate(idxs):
            ref = restate_mix_sample(ds, idx, 6, 0, trees[0]["background_dir"])
            diff = img[j] != ref["img"]
            if diff.any():
                # only next to bytes whose img + x lies on an integer (one LSB before the box, <= 1 after it)
                xs = ref["noise_sum"]
                near = (np.abs(xs - np.rint(xs)) < 1e-9).sum()
                assert near and diff.sum() <= 3 * ref["k"] ** 2 * near, (idx, int(diff.sum()), int(near))
                assert np.abs(img[j] - ref["img"]).max() <= 1.01 * stdinv
                edge += 1
            np.testing.assert_array_equal(batch["gt_bboxes"][j].numpy(), ref["gt_bboxes"])
            np.testing.assert_array_equal(batch["gt_labels"][j].numpy(), ref["gt_labels"])
            np.testing.assert_array_equal(batch["points_to_gt_index"][j].cpu().numpy(), ref["p2g"])
            np.testing.assert_array_equal(batch["points_weight"][j].cpu().numpy(), ref["pw"])
            assert batch["img_metas"][j]["flip"] == ref["flip"]
            seen |= {("k", ref["k"]), ("flip", ref["flip"]), ("bg", ref["bg"])}
            n += 1
        if n >= 8:
            break
    assert n == 8 and edge <= 2
    assert len({s for s in seen if s[0] == "k"}) >= 2 and ("flip", True) in seen


def test_mix_launch_count_does_not_depend_on_batch_size(trees, monkeypatch):
    from radet_amd import _lib
    from radet_amd.datasets.loader import sample_generators
    ds = _mix_dataset(trees)
    planned = []
    for idx in range(6):
        s = ds.plan_sample(idx, *sample_generators(2, 0, idx))
        s.pop("background", None)
        s["flip"] = True
        planned.append(s)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name) or real(name, *a))
    counts = []
    for b in (1, 4, 6):
        calls.clear()
        ds.pipeline.run(planned[:b], collate=True)
        torch.cuda.synchronize()
        counts.append(sorted(calls))
    assert counts[0] == counts[1] == counts[2]
    assert counts[0].count("radet_augment_hsv_noise") == 1 and counts[0].count("radet_augment_box") == 1
    assert "radet_augment_vblur" not in counts[0] and "radet_augment_sharp" not in counts[0]


def test_train_detector_from_mix_loader(trees):
    from oracle import synth
    from radet_amd.apis import train_detector
    from radet_amd.datasets import build_dataloader
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    synth.fill_state_dict(det.state_dict(), seed=0)
    det = det.cuda()
    cfg.merge_from_dict({"lr_config.total_steps": 40, "log_config.interval": 1})
    loader = build_dataloader(_mix_dataset(trees), samples_per_gpu=4, workers=4, seed=0)

    def batches():
        epoch = 0
        while True:
            loader.set_epoch(epoch)
            yield from loader
            epoch += 1
    hist = train_detector(det, batches(), cfg, max_iters=5, log=lambda *_: None)
    assert len(hist) == 5 and all(np.isfinite(h).all() for h in hist)
