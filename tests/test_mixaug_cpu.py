"""The mixpbr stages on the host: the NumPy restatement of RandomHSV / RandomNoise / RandomSmooth (tests/_mixaug_ref.py)
against colorsys, scipy.ndimage and numpy.random.Philox, the stages' random draws against a line-by-line restatement of
the reference's __call__ order, and MixDataset / build_dataset for a mixpbr-shaped config."""
import colorsys
import copy
import os
import random
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _mixaug_ref as M  # noqa: E402

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


# ------------------------------------------------------------------------------------------------ HSV
def _all_colours():
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([c & 255, (c >> 8) & 255, c >> 16], axis=1).astype(np.uint8)       # BGR


def _rgb_to_hsv(r, g, b):
    """colorsys.rgb_to_hsv, vectorised in float64"""
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    rng = maxc - minc
    safe = np.where(rng == 0, 1.0, rng)
    s = np.where(maxc == 0, 0.0, rng / np.where(maxc == 0, 1.0, maxc))
    rc, gc, bc = (maxc - r) / safe, (maxc - g) / safe, (maxc - b) / safe
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc))
    h = np.where(rng == 0, 0.0, (h / 6.0) % 1.0)
    return h, np.where(rng == 0, 0.0, s), maxc


def _hsv_to_rgb(h, s, v):
    """colorsys.hsv_to_rgb, vectorised in float64"""
    i = np.floor(h * 6.0).astype(np.int64)
    f = h * 6.0 - i
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    i = i % 6
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    zero = s == 0.0
    return np.where(zero, v, r), np.where(zero, v, g), np.where(zero, v, b)


def test_vectorised_colorsys_equals_colorsys():
    rng = np.random.RandomState(0)
    rgb = rng.randint(0, 256, (4000, 3)).astype(np.float64) / 255
    rgb[:64] = np.repeat(rng.randint(0, 256, (64, 1)), 3, axis=1) / 255           # greys
    got = np.stack(_rgb_to_hsv(rgb[:, 0], rgb[:, 1], rgb[:, 2]), axis=1)
    np.testing.assert_allclose(got, [colorsys.rgb_to_hsv(*p) for p in rgb], rtol=0, atol=1e-12)
    hsv = rng.rand(4000, 3)
    hsv[:64, 1] = 0.0
    got = np.stack(_hsv_to_rgb(hsv[:, 0], hsv[:, 1], hsv[:, 2]), axis=1)
    np.testing.assert_allclose(got, [colorsys.hsv_to_rgb(*p) for p in hsv], rtol=0, atol=1e-12)


def test_bgr2hsv_against_colorsys_all_colours():
    bgr = _all_colours()
    for lo in range(0, len(bgr), 1 << 21):
        x = bgr[lo:lo + (1 << 21)]
        hsv = M.bgr2hsv(x[None])[0].astype(np.int64)
        f = x.astype(np.float64) / 255
        h, s, v = _rgb_to_hsv(f[:, 2], f[:, 1], f[:, 0])
        dh = np.abs(hsv[:, 0] - h * 180) % 180
        assert np.minimum(dh, 180 - dh).max() <= 1
        assert hsv[:, 0].max() <= 179
        assert np.abs(hsv[:, 1] - s * 255).max() <= 1
        assert np.abs(hsv[:, 2] - v * 255).max() <= 1


def test_hsv2bgr_against_colorsys_all_inputs():
    c = np.arange(180 * 256 * 256, dtype=np.int64)
    hsv = np.stack([c // 65536, (c // 256) % 256, c % 256], axis=1).astype(np.uint8)
    bgr = M.hsv2bgr(hsv[None])[0].astype(np.int64)
    f = hsv.astype(np.float64)
    r, g, b = _hsv_to_rgb(f[:, 0] / 180, f[:, 1] / 255, f[:, 2] / 255)
    assert np.abs(bgr - np.stack([b, g, r], axis=1) * 255).max() <= 1


def test_hsv_scale_clips_like_the_reference():
    hsv = np.array([[[179, 255, 255], [100, 200, 10]]], np.uint8)
    np.testing.assert_array_equal(M.hsv_scale(hsv, 1.2, 1.5, 1.0), [[[179, 255, 255], [120, 255, 10]]])
    np.testing.assert_array_equal(M.hsv_scale(hsv, 0.9, 0.5, 0.999), [[[161, 127, 254], [90, 100, 9]]])


# ------------------------------------------------------------------------------------------------ box filter
@pytest.mark.parametrize("hw", [(4, 4), (5, 7), (8, 5), (6, 8), (13, 17), (31, 64), (37, 129)])
def test_box_filter_against_scipy(hw):
    from scipy import ndimage
    img = np.random.RandomState(hw[0] * 100 + hw[1]).randint(0, 256, (*hw, 3)).astype(np.uint8)
    for k in (1, 3, 5, 7):
        s = ndimage.correlate(img.astype(np.int64), np.ones((k, k, 1), np.int64), mode="mirror")
        np.testing.assert_array_equal(M.box_sums(img, k), s)
        np.testing.assert_array_equal(M.box_filter(img, k), ((s + (k * k - 1) // 2) // (k * k)).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ noise
def test_philox_words_equal_numpy_philox():
    for key in ([0, 0], [1, 2], [2 ** 64 - 1, 2 ** 63 + 12345], [0x0123456789ABCDEF, 0xFEDCBA9876543210]):
        key = np.array(key, np.uint64)
        np.testing.assert_array_equal(M.philox_words(key, 4099), np.random.Philox(key=key).random_raw(4099))
        # block b is the counter b + 1
        for b in (0, 1, 517):
            want = np.random.Philox(key=key, counter=np.array([b, 0, 0, 0], np.uint64)).random_raw(4)
            np.testing.assert_array_equal(M.philox_words(key, 4 * b + 4)[4 * b:], want)


def test_box_muller_is_standard_normal():
    from scipy import stats
    z = M.normals(np.array([7, 11], np.uint64), 10 ** 6)
    assert abs(z.mean()) < 5e-3 and abs(z.std() - 1) < 5e-3
    assert stats.kstest(z, "norm").pvalue > 1e-3
    assert np.isfinite(z).all()


def test_noise_stage_arithmetic():
    img = np.random.RandomState(1).randint(0, 256, (5, 7, 3)).astype(np.uint8)
    key = np.array([3, 4], np.uint64)
    z = M.normals(key, img.size).reshape(img.shape)
    want = img + (0.07 * z) * 255
    want[want > 255] = 255
    want[want < 0] = 0
    np.testing.assert_array_equal(M.random_noise(img, 0.07, key), want.astype(np.uint8))


# ------------------------------------------------------------------------------------------------ draw order
def _reference_draws(rnd, nprnd, backgrounds):
    """the reference's RandomBackground / RandomHSV / RandomNoise / RandomSmooth / RandomFlip __call__ draws, line by line
    (np.random.normal replaced by the Philox key draw)"""
    out = {}
    if not rnd.random() > 0.3:
        out["background"] = rnd.choice(backgrounds)
    if not rnd.random() > 1.0:
        a = rnd.uniform(-1, 1) * 0.2 + 1
        b = rnd.uniform(-1, 1) * 0.5 + 1
        c = rnd.uniform(-1, 1) * 0.5 + 1
        out["aug_hsv"] = (a, b, c)
    if not rnd.random() > 1.0:
        sigma = rnd.uniform(0, 0.1)
        out["aug_noise"] = (sigma, nprnd.randint(0, 2 ** 64, size=2, dtype=np.uint64))
    if not rnd.random() > 1.0:
        out["aug_smooth"] = rnd.choice([1, 3, 5, 7])
    out["flip"] = nprnd.choice(["horizontal", None], p=[0.5, 0.5]) is not None
    return out


def test_draw_plan_consumes_generators_like_the_reference(tmp_path, monkeypatch):
    from radet_amd.datasets import loading
    from radet_amd.datasets.pipelines import PIPELINES
    from radet_amd.utils import build_from_cfg
    open(tmp_path / "b0.png", "wb").close()
    open(tmp_path / "b1.jpg", "wb").close()
    monkeypatch.setattr(loading, "decode_bgr", lambda p: p)
    cfgs = [c for c in mix_pipeline(str(tmp_path)) if c["type"] in ("RandomBackground", "RandomHSV", "RandomNoise",
                                                                        "RandomSmooth", "RandomFlip")]
    stages = [build_from_cfg(c, PIPELINES) for c in cfgs]
    bgs = stages[0].background_images
    a, b = random.Random(9), random.Random(9)
    na, nb = np.random.RandomState(9), np.random.RandomState(9)
    seen = set()
    for _ in range(200):
        s = dict(img_shape=(4, 5, 3), bbox_fields=[])
        for st in stages:
            st.plan(s, a, na)
        ref = _reference_draws(b, nb, bgs)
        assert s.get("background") == ref.get("background")
        assert s["aug_hsv"] == ref["aug_hsv"] and s["aug_smooth"] == ref["aug_smooth"] and s["flip"] == ref["flip"]
        assert s["aug_noise"][0] == ref["aug_noise"][0]
        np.testing.assert_array_equal(s["aug_noise"][1], ref["aug_noise"][1])
        seen.add(s["aug_smooth"])
        assert a.getstate() == b.getstate()
        sa, sb = na.get_state(), nb.get_state()
        assert sa[2] == sb[2] and np.array_equal(sa[1], sb[1])
    assert seen == {1, 3, 5, 7}


# ------------------------------------------------------------------------------------------------ MixDataset
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL writes the synthetic JPEG / PNG files")
    from tools.synth_bop import write_tree
    pbr = write_tree(str(tmp_path_factory.mktemp("pbr")), n_frames=5, seed=21)
    real = write_tree(str(tmp_path_factory.mktemp("real")), n_frames=3, size=(480, 640), n_backgrounds=1, seed=22)
    return pbr, real


def mix_config(trees, pipeline=None, pipeline_1=None):
    pbr, real = trees
    pipe = pipeline or mix_pipeline(pbr["background_dir"])
    return dict(type="MixDataset",
                dataset_0=dict(type="BOPDataset", ann_file=pbr["ann_file"], img_prefix=pbr["img_prefix"],
                               seg_prefix=pbr["seg_prefix"], pipeline=pipe, ratio=2),
                dataset_1=dict(type="BOPDataset", ann_file=real["ann_file"], img_prefix=real["img_prefix"],
                               seg_prefix=real["seg_prefix"], pipeline=pipeline_1 or pipe, ratio=1))


def test_mix_dataset_from_config(trees):
    import radet.datasets as RD
    from radet_amd.datasets import build_dataloader
    from radet_amd.datasets.loader import sample_generators
    from radet_amd.datasets.loading import ImagePipeline
    cfg = mix_config(trees)
    before = copy.deepcopy(cfg)
    ds = RD.build_dataset(cfg)
    assert cfg == before                                                   # the caller's config is left as it was
    assert isinstance(ds, RD.MixDataset) and isinstance(ds, RD.ConcatDataset)
    assert RD.DATASETS.get("MixDataset") is RD.MixDataset and RD.DATASETS.get("RepeatDataset") is RD.RepeatDataset
    pbr, real = ds.datasets
    assert isinstance(pbr, RD.RepeatDataset) and pbr.times == 2 and real.times == 1
    assert len(ds) == 2 * 5 + 3 and ds.CLASSES == pbr.dataset.CLASSES
    np.testing.assert_array_equal(ds.flag, np.concatenate([np.tile(pbr.dataset.flag, 2), real.dataset.flag]))
    assert ds.flag.tolist() == [1] * 10 + [0] * 3
    assert isinstance(ds.pipeline, ImagePipeline) and ds.pipeline.mix
    assert pbr.dataset.pipeline is ds.pipeline and real.dataset.pipeline is ds.pipeline
    # index mapping: 0..4 and 5..9 are the pbr frames, 10..12 the real ones
    for idx, (d, j) in {0: (pbr, 0), 4: (pbr, 4), 5: (pbr, 0), 9: (pbr, 4), 10: (real, 0), 12: (real, 2)}.items():
        s = ds.plan_sample(idx, *sample_generators(1, 0, idx))
        assert s["filename"] == os.path.join(d.dataset.img_prefix, d.dataset.data_infos[j]["filename"])
        assert set(s) >= {"aug_hsv", "aug_noise", "aug_smooth", "flip"}
    assert ds.get_cat_ids(11) == real.dataset.get_cat_ids(1)
    with pytest.raises(IndexError):
        ds.plan_sample(13, random, np.random)
    # repeated copies of a frame are planned from their own seeds
    s0, s5 = (ds.plan_sample(i, *sample_generators(1, 0, i)) for i in (0, 5))
    np.testing.assert_array_equal(s0["img"], s5["img"])
    assert s0["aug_hsv"] != s5["aug_hsv"]
    # loader batches: aspect groups never mix, every index is covered
    loader = build_dataloader(ds, samples_per_gpu=2, workers=2, seed=3)
    batches = loader.batches()
    assert sorted(set(i for b in batches for i in b)) == list(range(13))
    assert all(len(set(ds.flag[b])) == 1 for b in batches)
    # a plain BOPDataset config builds exactly as before, a list is a ConcatDataset, RepeatDataset works on its own
    plain = RD.build_dataset({k: v for k, v in before["dataset_1"].items() if k != "ratio"})
    assert type(plain) is RD.BOPDataset and len(plain) == 3
    cat = RD.build_dataset([{k: v for k, v in before[key].items() if k != "ratio"} for key in ("dataset_0", "dataset_1")])
    assert type(cat) is RD.ConcatDataset and len(cat) == 8
    rep = RD.build_dataset(dict(type="RepeatDataset", times=3, dataset={k: v for k, v in before["dataset_1"].items()
                                                                       if k != "ratio"}))
    assert len(rep) == 9 and rep.flag.tolist() == [0] * 9


def test_mix_refusals(trees):
    from radet_amd.datasets import build_dataset
    pbr, _ = trees
    cosy = mix_pipeline(pbr["background_dir"])
    cosy.insert(4, dict(type="CosyPoseAug", p=0.8, pipelines=[dict(type="PillowBlur", p=1., factor_interval=(1, 3))]))
    with pytest.raises(NotImplementedError):
        build_dataset(mix_config(trees, pipeline=cosy))
    other = mix_pipeline(pbr["background_dir"])
    other[5] = dict(type="RandomNoise", noise_ratio=0.2, prob=1.0)
    with pytest.raises(NotImplementedError):
        build_dataset(mix_config(trees, pipeline_1=other))
    with pytest.raises(NotImplementedError):
        build_dataset(dict(type="ClassBalancedDataset", oversample_thr=1e-3, dataset=mix_config(trees)["dataset_1"]))
    twice = mix_pipeline(pbr["background_dir"])
    twice.insert(5, dict(type="RandomHSV", h_ratio=0.2, s_ratio=0.5, v_ratio=0.5))
    with pytest.raises(NotImplementedError):
        build_dataset(mix_config(trees, pipeline=twice))
