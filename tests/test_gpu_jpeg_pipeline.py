"""image_decode='device' end to end: the pbr, the mix and a mask-free pipeline fed from files decoded on the GPU against
the same pipelines with Pillow on the loader threads (every collected tensor and both generators' positions equal), two
train_detector steps with bit-equal losses, and the test pipeline / inference_detector on file names."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _maskfree_pipelines import NORM, train_pipeline  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 5
KEYS = ("img", "gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """six frames of two sizes, frame 4 without objects, three backgrounds"""
    pytest.importorskip("PIL", reason="PIL writes and decodes the generated files")
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=6, objects=(3, 6), n_backgrounds=3, seed=17,
                      sizes=[(640, 480), (600, 480)], empty_frames=(4,))


def _dataset(tree, decode, mix=False, dm="mask", **kw):
    from radet_amd.datasets import build_dataset
    from tools.synth_bop import YCBV_NAMES
    cfg = dict(type="BOPDataset", img_prefix=tree["img_prefix"], filter_empty_gt=False, classes=YCBV_NAMES,
               ann_file=tree["ann_file"], seg_prefix=tree["seg_prefix"],
               pipeline=train_pipeline(tree["background_dir"], dm, mix=mix, bg_prob=0.5), **kw)
    if decode is not None:
        cfg["image_decode"] = decode
    return build_dataset(cfg)


def _run(ds):
    from radet_amd import _lib
    from radet_amd.datasets.loader import sample_generators
    gens = [sample_generators(SEED, 0, i) for i in range(len(ds))]
    planned = [ds.plan_sample(i, *gens[i]) for i in range(len(ds))]
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        out = ds.pipeline.run(planned)
    finally:
        _lib.call = call
    ds.pipeline.check_decode_errors(wait=True)
    return out, gens, planned, seen


def _compare(tree, mix, dm):
    from radet_amd.core import jpeg
    ref, ref_gens, ref_planned, ref_seen = _run(_dataset(tree, None, mix, dm))
    ds = _dataset(tree, "device", mix, dm)
    out, gens, planned, seen = _run(ds)
    assert all(isinstance(s["img"], np.ndarray) for s in ref_planned) and "radet_jpeg_decode" not in ref_seen
    assert all(isinstance(s["img"], jpeg.DeviceJpeg) for s in planned)
    assert all(isinstance(s["background"], jpeg.DeviceJpeg) for s in planned if "background" in s)
    # one more call (the decode's three launches) in front of the launches of the host path
    assert seen == ["radet_jpeg_decode"] + ref_seen
    n_bg = sum("background" in s for s in planned)
    assert ds.pipeline.decode_stats == dict(device=6 + n_bg, fallback=0)
    for i in range(6):
        for k in KEYS:
            assert torch.equal(out[i][k], ref[i][k]), f"sample {i}: {k}"
        assert out[i]["img_metas"].keys() == ref[i]["img_metas"].keys()
        assert gens[i][0].getstate() == ref_gens[i][0].getstate(), f"sample {i}: random.Random position"
        for a, b in zip(gens[i][1].get_state(), ref_gens[i][1].get_state()):
            assert np.array_equal(a, b), f"sample {i}: RandomState position"
    return planned


@pytest.mark.parametrize("mix", [False, True], ids=["pbr", "mix"])
def test_pipeline_equals_host_decode(tree, mix):
    planned = _compare(tree, mix, "mask")
    # the batch covers: two source sizes, flipped and not, backgrounds on at least two samples, a sample without objects
    assert len({s["img"].shape for s in planned}) == 2 and {bool(s["flip"]) for s in planned} == {True, False}
    assert sum("background" in s for s in planned) >= 2
    assert [len(s["gt_bboxes"]) for s in planned].count(0) == 1


def test_mask_free_pipeline_equals_host_decode(tree):
    _compare(tree, False, "mbd")


def test_default_pipeline_issues_no_decode(tree):
    ds = _dataset(tree, None)
    _, _, planned, seen = _run(ds)
    assert "radet_jpeg_decode" not in seen and ds.pipeline.decode_stats == dict(device=0, fallback=0)
    assert seen[0] == "radet_resize_linear_u8"


def test_index_cache_directory(tree, tmp_path):
    """index_cache=<directory> through build_dataset: filled by the first pass, read by a second dataset without a walk"""
    from radet_amd.core import jpeg
    d = str(tmp_path / "idx")
    a = _dataset(tree, "device", index_cache=d)
    ref = _run(a)[0]
    n = len(os.listdir(d))
    assert n >= 6
    b = _dataset(tree, "device", index_cache=d)
    walk, seen = jpeg.scan_index, []
    jpeg.scan_index = lambda *x, **k: seen.append(1) or walk(*x, **k)
    try:
        out = _run(b)[0]
    finally:
        jpeg.scan_index = walk
    assert not seen and len(os.listdir(d)) == n
    for i in range(6):
        assert torch.equal(out[i]["img"], ref[i]["img"])


def test_train_steps_equal_host_decode(tmp_path_factory):
    """two steps of train_detector from the loader with device decoding: the losses of host decoding, bit for bit"""
    from radet_amd.apis import train_detector
    from radet_amd.datasets import build_dataloader
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill
    from tools.synth_bop import write_tree
    tiny = write_tree(str(tmp_path_factory.mktemp("tiny")), n_frames=4, objects=(2, 4), n_backgrounds=1, seed=23)

    def run(decode):
        cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
        cfg.model["pretrained"] = None
        cfg.merge_from_dict({"lr_config.total_steps": 40, "log_config.interval": 1})
        torch.manual_seed(0)
        det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda()
        synth_fill(det, seed=0)
        loader = build_dataloader(_dataset(tiny, decode), samples_per_gpu=4, workers=4, seed=0)

        def batches():
            epoch = 0
            while True:
                loader.set_epoch(epoch)
                yield from loader
                epoch += 1
        try:
            return train_detector(det, batches(), cfg, max_iters=2, log=lambda *_: None)
        finally:
            loader.close()
    a, b = run(None), run("device")
    assert len(a) == len(b) == 2 and np.isfinite(a).all() and a == b


def test_test_pipeline_and_inference_on_file_names(tree):
    from radet_amd.apis import inference_detector
    from radet_amd.datasets.loading import ImagePipeline
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill

    def pipe(decode):
        return [dict(type="LoadImageFromFile", **({} if decode is None else dict(decode=decode))),
                dict(type="MultiScaleFlipAug", img_scale=(640, 480), flip=False,
                     transforms=[dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), dict(type="Normalize", **NORM),
                                 dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]),
                                 dict(type="Collect", keys=["img"])])]
    import random
    names = [os.path.join(tree["img_prefix"], "000000", "rgb", f"{f:06d}.jpg") for f in (0, 1)]
    data = {}
    for decode in (None, "device"):
        p = ImagePipeline(pipe(decode))
        planned = [p.plan(dict(img_info=dict(filename=n), img_prefix=None, bbox_fields=[], mask_fields=[], seg_fields=[]),
                          random, np.random) for n in names]
        data[decode] = p.run(planned, collate=True)
    assert torch.equal(data[None]["img"][0], data["device"]["img"][0])
    for ma, mb in zip(data[None]["img_metas"][0], data["device"]["img_metas"][0]):
        assert ma.keys() == mb.keys() and ma["ori_shape"] == mb["ori_shape"] and ma["img_shape"] == mb["img_shape"]
        assert np.array_equal(ma["scale_factor"], mb["scale_factor"])
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().eval()
    synth_fill(det, seed=0)
    res = {}
    for decode in (None, "device"):
        det.cfg = Config(dict(data=dict(test=dict(pipeline=pipe(decode)))))
        res[decode] = inference_detector(det, names)
    for ra, rb in zip(res[None], res["device"]):
        assert len(ra) == len(rb)
        for ca, cb in zip(ra, rb):
            np.testing.assert_array_equal(ca, cb)
