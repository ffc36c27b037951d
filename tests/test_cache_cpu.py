"""The sample cache without a device: option handling of the dataset configs and ImagePipeline, the arena's bookkeeping
with an injected host allocator, invalidation by size / mtime, the once-converted mask run lists against the NumPy
restatement of normalise-by-own-maximum, and the placeholder that plan() returns for a cached file without opening it."""
import os
import random
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytest.importorskip("PIL", reason="PIL writes the generated files")
from _maskfree_pipelines import NORM, train_pipeline  # noqa: E402


def host_alloc(nbytes):
    """a 256-byte aligned u8 host tensor standing in for a device chunk"""
    t = torch.empty(nbytes + 256, dtype=torch.uint8)
    off = -t.data_ptr() % 256
    return t[off:off + nbytes]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=4, objects=(2, 3), n_backgrounds=2, seed=3,
                      sizes=[(64, 48), (50, 37)])


def _cfg(tree, kind="BOPDataset", **kw):
    from tools.synth_bop import YCBV_NAMES
    return dict(type=kind, img_prefix=tree["img_prefix"], filter_empty_gt=False, classes=YCBV_NAMES, ann_file=tree["ann_file"],
                seg_prefix=tree["seg_prefix"], pipeline=train_pipeline(tree["background_dir"], "mask"), **kw)


# ------------------------------------------------------------------------------------------------ options
@pytest.mark.parametrize("kind", ["BOPDataset", "CocoDataset"])
def test_options_of_the_dataset_configs(tree, kind):
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.sample_cache import SampleCache
    with pytest.raises(ValueError, match="cache_bytes"):
        build_dataset(_cfg(tree, kind, sample_cache="device"))
    for bad in (0, -1, None, 1.5):
        with pytest.raises(ValueError, match="cache_bytes"):
            build_dataset(_cfg(tree, kind, sample_cache="device", cache_bytes=bad))
    with pytest.raises(ValueError, match="sample_cache"):
        build_dataset(_cfg(tree, kind, sample_cache="host", cache_bytes=1 << 20))
    ds = build_dataset(_cfg(tree, kind, sample_cache="device", cache_bytes=3 << 20))
    assert isinstance(ds.pipeline.sample_cache, SampleCache) and ds.pipeline.sample_cache.cache_bytes == 3 << 20
    assert not ds.pipeline.sample_cache.chunks                            # (nothing is allocated before the first insertion)
    off = build_dataset(_cfg(tree, kind))
    assert off.pipeline.sample_cache is None and set(off.pipeline.cache_stats.values()) == {0}
    assert {"hits", "misses", "inserted", "bytes", "rejected_full", "invalidated", "mask_hits"} <= set(off.pipeline.cache_stats)


def test_options_of_the_pipeline():
    from radet_amd.datasets.loading import ImagePipeline
    stages = [dict(type="LoadImageFromFile"), dict(type="Normalize", **NORM), dict(type="Collect", keys=["img"])]
    with pytest.raises(ValueError):
        ImagePipeline(stages, sample_cache="device")
    with pytest.raises(ValueError):
        ImagePipeline(stages, sample_cache="device", cache_bytes=0)
    with pytest.raises(ValueError):
        ImagePipeline(stages, sample_cache="pinned", cache_bytes=1 << 20)
    with pytest.raises(ValueError):
        ImagePipeline(stages, cache_bytes=1 << 20)                        # (a budget without a cache)
    p = ImagePipeline(stages, sample_cache="device", cache_bytes=1 << 20)
    assert p.transforms[0].sample_cache is p.sample_cache
    assert p.cache_stats["hits"] == p.cache_stats["bytes"] == 0


def test_wrapper_configs_pass_the_options_down(tree):
    from radet_amd.datasets import build_dataset
    rep = build_dataset(dict(type="RepeatDataset", times=2, dataset=_cfg(tree), sample_cache="device", cache_bytes=1 << 20))
    assert rep.pipeline.sample_cache is not None and rep.pipeline.sample_cache.cache_bytes == 1 << 20
    mix = build_dataset(dict(type="MixDataset", pbr_dataset=dict(_cfg(tree), ratio=1), real_dataset=dict(_cfg(tree), ratio=2),
                             sample_cache="device", cache_bytes=2 << 20))
    caches = {id(r.dataset.pipeline.sample_cache) for r in mix.datasets}
    assert len(caches) == 1 and mix.pipeline.sample_cache.cache_bytes == 2 << 20      # one pipeline, one cache
    with pytest.raises(ValueError, match="cache_bytes"):
        build_dataset(dict(type="RepeatDataset", times=2, dataset=_cfg(tree), sample_cache="device"))


# ------------------------------------------------------------------------------------------------ arena
def _key(i, size=1):
    return (f"/nowhere/{i}", size, 0)


def test_arena_alignment_chunks_and_budget():
    from radet_amd.datasets.sample_cache import SampleCache
    chunk, budget = 4096, 10000                        # two whole chunks and one of 1808 bytes
    c = SampleCache(budget, chunk_bytes=chunk, alloc=host_alloc)
    shapes = [(10, 10, 3), (7, 5, 3), (30, 30, 3), (1, 1, 3), (20, 20, 3), (25, 17, 3), (36, 36, 3), (9, 9, 3), (31, 14, 3),
              (2, 3, 3), (16, 16, 3), (24, 21, 3), (2, 2, 3)]
    taken = c.reserve([(_key(i), s) for i, s in enumerate(shapes)])
    c.commit(taken)
    assert c.allocated <= budget and [t.numel() for t in c.chunks] == [4096, 4096, 1808]
    spans = [(t.data_ptr(), t.data_ptr() + t.numel()) for t in c.chunks]
    used = []
    for key, shape, addr, nbytes in taken:
        assert addr % 256 == 0 and nbytes == int(np.prod(shape))
        assert sum(lo <= addr and addr + nbytes <= hi for lo, hi in spans) == 1          # inside one chunk
        used.append((addr, addr + nbytes))
    used.sort()
    assert all(a[1] <= b[0] for a, b in zip(used, used[1:]))                             # no two entries overlap
    st = c.stats
    assert st["inserted"] == len(taken) < len(shapes) and st["rejected_full"] == len(shapes) - len(taken) > 0
    assert st["bytes"] == sum(t[3] for t in taken) <= budget
    # the rejected ones are those that did not fit when their turn came; later smaller ones were still taken
    names = {t[0][0] for t in taken}
    assert _key(6)[0] not in names and _key(12)[0] in names
    # an entry larger than a chunk is rejected even by an empty cache with budget to spare
    big = SampleCache(1 << 20, chunk_bytes=chunk, alloc=host_alloc)
    assert big.reserve([(_key(0), (40, 40, 3))]) == [] and big.stats["rejected_full"] == 1 and not big.chunks
    assert len(big.reserve([(_key(1), (36, 37, 3))])) == 1                               # 3996 bytes fit
    # a file that is in the table already, or twice in one batch, is reserved once
    again = c.reserve([(taken[0][0], taken[0][1])]) + big.reserve([(_key(2), (2, 2, 3)), (_key(2), (2, 2, 3))])
    assert len(again) == 1


def test_changed_size_or_mtime_invalidates(tmp_path):
    from radet_amd.datasets.sample_cache import CachedImage, SampleCache, file_key
    c = SampleCache(1 << 16, chunk_bytes=1 << 14, alloc=host_alloc)
    p = str(tmp_path / "a.bin")
    open(p, "wb").write(b"x" * 100)
    hit, key = c.lookup(p)
    assert hit is None and key == file_key(p) and key[0] == os.path.realpath(p)
    taken = c.reserve([(key, (4, 5, 3))])
    c.commit(taken)
    hit, _ = c.lookup(p)
    assert isinstance(hit, CachedImage) and hit.shape == (4, 5, 3) and hit.addr == taken[0][2] and hit.nbytes == 60
    link = str(tmp_path / "link.bin")
    os.symlink(p, link)
    assert c.lookup(link)[0] is not None                                    # (keys are real paths)
    st = os.stat(p)
    os.utime(p, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))        # same bytes, another mtime
    hit, key2 = c.lookup(p)
    assert hit is None and c.stats["invalidated"] == 1 and key2 != key
    assert c.lookup(p)[0] is None and c.stats["invalidated"] == 1           # (dropped once)
    fill = c.fill
    c.commit(c.reserve([(key2, (4, 5, 3))]))
    assert c.fill > fill and c.lookup(p)[0].addr != taken[0][2]             # the old bytes are not reused
    open(p, "wb").write(b"y" * 101)                                         # another size
    os.utime(p, ns=(st.st_atime_ns, key2[2]))
    assert c.lookup(p)[0] is None and c.stats["invalidated"] == 2
    assert c.stats["hits"] == 3 and c.stats["misses"] == 4


# ------------------------------------------------------------------------------------------------ masks
def _normalise(m):
    """(mask / mask.max()).astype(u8) as the loader's PNG path does it; 0 / 0 = NaN -> 0"""
    with np.errstate(all="ignore"):
        q = m.astype(np.float64) / np.float64(m.max())
    return np.nan_to_num(q, nan=0.0).astype(np.uint8)


def _four_masks(h, w):
    rs = np.random.RandomState(4)
    binary = np.zeros((h, w), np.uint8)
    binary[5:20, 7:30] = 255
    grey = rs.randint(0, 201, (h, w)).astype(np.uint8)
    grey[rs.rand(h, w) < 0.2] = 200                      # the maximum on a fifth of the pixels, values of every size below it
    one = np.zeros((h, w), np.uint8)
    one[h - 1, w - 1] = 7
    return dict(binary=binary, grey=grey, one_pixel=one, zero=np.zeros((h, w), np.uint8))


def test_mask_run_lists_equal_the_normalised_bitmaps(tmp_path):
    from PIL import Image
    from radet_amd.core import rle
    from radet_amd.datasets.loading import LoadAnnotations
    from radet_amd.datasets.sample_cache import SampleCache, normalised_runs
    h, w = 37, 50
    masks = _four_masks(h, w)
    assert masks["grey"].max() == 200 and 0 < (masks["grey"] == 200).sum() < h * w
    for name, m in masks.items():
        ref = _normalise(m)
        assert set(np.unique(ref)) <= {0, 1} and ref.sum() == ((m == m.max()).sum() if m.max() else 0)
        assert np.array_equal(rle.mask_from_rle(normalised_runs(m), h, w), ref), name
        Image.fromarray(m).save(str(tmp_path / f"{name}.png"))
    # through the stage: the first visit carries the bitmaps and converts them once, the second carries the run lists
    stage = LoadAnnotations(with_bbox=True, with_bop_mask=True)
    stage.sample_cache = SampleCache(1 << 20, alloc=host_alloc)

    def sample():
        return dict(img_info=dict(height=h, width=w), seg_prefix=str(tmp_path), bbox_fields=[], mask_fields=[],
                    ann_info=dict(bboxes=np.zeros((4, 4), np.float32), labels=np.arange(4), masks=[f"{n}.png" for n in masks]))
    first, second = sample(), sample()
    stage.plan(first, random.Random(0), np.random.RandomState(0))
    assert "gt_masks_rle" not in first and np.array_equal(first["gt_masks"], np.stack(list(masks.values())))
    from radet_amd.datasets import loading
    decode, loading.decode_unchanged = loading.decode_unchanged, None       # (the second visit decodes nothing)
    try:
        stage.plan(second, random.Random(0), np.random.RandomState(0))
    finally:
        loading.decode_unchanged = decode
    assert "gt_masks" not in second and second["mask_fields"] == ["gt_masks"]
    parts, hw = second["gt_masks_rle"]
    assert hw == (h, w) and len(parts) == 4 and all(len(p) == 1 for p in parts)
    for p, m in zip(parts, first["gt_masks"]):
        assert np.array_equal(rle.mask_from_parts(p, h, w), _normalise(m))
    st = stage.sample_cache.stats
    assert st["mask_hits"] == 4 and st["mask_bytes"] == sum(p[0].nbytes for p in parts) > 0 and st["bytes"] == 0
    # a rewritten mask file is converted again
    Image.fromarray(masks["binary"][::-1].copy()).save(str(tmp_path / "binary.png"))
    st0 = os.stat(str(tmp_path / "binary.png"))
    os.utime(str(tmp_path / "binary.png"), ns=(st0.st_atime_ns, st0.st_mtime_ns + 1_000_000_000))
    third = sample()
    stage.plan(third, random.Random(0), np.random.RandomState(0))
    assert "gt_masks" in third and stage.sample_cache.stats["invalidated"] == 1


# ------------------------------------------------------------------------------------------------ the placeholder
@pytest.mark.parametrize("decode", ["host", "device"])
def test_a_planned_hit_is_a_placeholder_and_opens_no_file(tree, decode, monkeypatch):
    from radet_amd.core import jpeg
    from radet_amd.datasets import loading
    from radet_amd.datasets.sample_cache import CachedImage
    pipe = loading.ImagePipeline([dict(type="LoadImageFromFile"), dict(type="Resize", img_scale=(96, 72), keep_ratio=True),
                                  dict(type="RandomBackground", background_dir=tree["background_dir"], prob=1.0),
                                  dict(type="Normalize", **NORM), dict(type="Collect", keys=["img"])],
                                 image_decode=decode, sample_cache="device", cache_bytes=4 << 20)
    pipe.sample_cache.alloc = host_alloc
    name = os.path.join(tree["img_prefix"], "000000", "rgb", "000001.jpg")

    def plan():
        return pipe.plan(dict(img_info=dict(filename=name), img_prefix=None, bbox_fields=[], mask_fields=[], seg_fields=[]),
                         random.Random(1), np.random.RandomState(1))
    cold = plan()
    assert isinstance(cold["img"], np.ndarray if decode == "host" else jpeg.DeviceJpeg) and cold["img"].shape == (37, 50, 3)
    assert set(cold["_cache_keys"]) == {"img", "background"} and cold["_cache_keys"]["img"][0] == os.path.realpath(name)
    assert pipe.cache_stats["misses"] == 2 and pipe.cache_stats["hits"] == 0
    # what run() does after the copy into the arena has been enqueued
    cache = pipe.sample_cache
    cache.commit(cache.reserve([(cold["_cache_keys"][f], cold[f].shape) for f in ("img", "background")]))

    def refuse(*a, **k):
        raise AssertionError("a cached file was opened")
    monkeypatch.setattr(loading, "decode_bgr", refuse)
    monkeypatch.setattr(jpeg, "plan_file", refuse)
    warm = plan()
    for f in ("img", "background"):
        assert isinstance(warm[f], CachedImage) and warm[f].shape == cold[f].shape and warm[f].addr % 256 == 0
        assert warm[f].nbytes == int(np.prod(cold[f].shape))
    assert "_cache_keys" not in warm and pipe.cache_stats["hits"] == 2
    for k in ("img_shape", "ori_shape", "pad_shape", "resize_hw"):
        assert warm[k] == cold[k]
    assert np.array_equal(warm["scale_factor"], cold["scale_factor"])
