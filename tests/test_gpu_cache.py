"""sample_cache='device' on the GPU: radet_copy_segments against a NumPy copy (every source / destination alignment, guard
bytes, very unequal rows), and the cached pipelines against the uncached ones -- two epochs of the pbr and mix pipelines
under host / device decoding and PNG / run-list annotations, a budget that holds part of the files, a rewritten frame, a
fill on one stream read on another, two epochs of train_detector and a repeated single_gpu_test.  Every comparison is
array_equal / torch.equal: the cache moves bytes and may not change one.

The cached stages of run() -- the packed source buffer (gather, decode, insert) and the masks -- run with synchronising
calls made an error in the second epoch.  (run() as a whole cannot: the assigner reads its sampling codes back, cache or
not.)"""
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytest.importorskip("PIL", reason="PIL writes and decodes the generated files")
from _maskfree_pipelines import NORM, train_pipeline  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 11
KEYS = ("img", "gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight")
SCALE = (96, 72)


# ------------------------------------------------------------------------------------------------ radet_copy_segments
def _copy_case(sizes_and_alignments, seed):
    """rows laid out with >= 32 guard bytes around every destination; returns (src, dst0, rows of (s, d, n) offsets)"""
    rs = np.random.RandomState(seed)
    rows, so, do = [], 0, 64
    for n, sa, da in sizes_and_alignments:
        s = -(-so // 16) * 16 + sa
        d = -(-do // 16) * 16 + da
        rows.append((s, d, n))
        so, do = s + n + 1, d + n + 32
    src = rs.randint(0, 256, so + 64).astype(np.uint8)
    dst0 = rs.randint(0, 256, do + 64).astype(np.uint8)
    return src, dst0, rows


def _run_copy(src, dst0, rows):
    from radet_amd import _lib, kernels as K
    dev = torch.device("cuda", torch.cuda.current_device())
    s, d = torch.from_numpy(src).to(dev), torch.from_numpy(dst0).to(dev)
    assert s.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
    table, tiles = K.copy_segments_table([(s.data_ptr() + a, d.data_ptr() + b, n) for a, b, n in rows])
    assert table.shape == (len(rows), K.COPY_DESC_INTS)
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        K.copy_segments(torch.from_numpy(table).to(dev), len(rows), tiles)
    finally:
        _lib.call = call
    assert seen == ["radet_copy_segments"]
    want = dst0.copy()
    for a, b, n in rows:
        want[b:b + n] = src[a:a + n]
    got = d.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[:5]}"      # the copies and every guard byte


def test_copy_segments_every_alignment_pair():
    sizes = (0, 1, 15, 16, 17, 63, 64, 65, 4099)
    case = [(n, sa, da) for sa in range(16) for da in range(16) for n in sizes] + [(3 * 1024 * 1024 + 5, 7, 9)]
    src, dst0, rows = _copy_case(case, 0)
    assert len(rows) == 16 * 16 * 9 + 1 and {(a % 16, b % 16) for a, b, _ in rows} == {(i, j) for i in range(16) for j in range(16)}
    _run_copy(src, dst0, rows)


def test_copy_segments_very_unequal_rows():
    """rows from nothing to megabytes in one table (a tile is 16 KiB: the large rows span hundreds of workgroups, rows
    without bytes own none, also at the table's two ends)"""
    case = [(0, 3, 5), (5 * 1024 * 1024 + 3, 1, 14), (1, 15, 0), (100_000, 8, 8), (0, 0, 0), (33, 5, 2), (2 * 1024 * 1024 + 1, 0, 3),
            (16384, 0, 0), (16385, 4, 15), (7, 9, 13), (0, 1, 1)]
    _run_copy(*_copy_case(case, 1))


def test_copy_segments_arguments():
    from radet_amd import _lib
    fn = _lib.load().radet_copy_segments
    assert fn(None, -1, 0, None) == -1 and fn(None, 3, 1, None) == -1 and fn(None, 2, -1, None) == -1
    assert fn(None, 0, 0, None) == 0


# ------------------------------------------------------------------------------------------------ the pipelines
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """six frames of 64 x 48 and 50 x 37 (odd: the packed offsets are unaligned), three backgrounds of other sizes; the
    annotations once more with run lists"""
    from radet_amd.datasets.bop_convert import add_segmentation
    from tools.synth_bop import write_tree
    root = str(tmp_path_factory.mktemp("bop"))
    t = write_tree(root, n_frames=6, objects=(2, 4), n_backgrounds=3, seed=21, sizes=[(64, 48), (50, 37)])
    t["rle"] = os.path.join(root, "train_pbr_rle.json")
    json.dump(add_segmentation(json.load(open(t["ann_file"])), t["seg_prefix"], "rle"), open(t["rle"], "w"))
    return t


def _dataset(tree, mix=False, decode="host", ann="png", **kw):
    from radet_amd.datasets import build_dataset
    from tools.synth_bop import YCBV_NAMES
    pipe = train_pipeline(tree["background_dir"], "mask", mix=mix, bg_prob=0.7)
    assert pipe[2]["type"] == "Resize" and pipe[1]["type"] == "LoadAnnotations"
    pipe[2] = dict(type="Resize", img_scale=SCALE, keep_ratio=True)
    cfg = dict(type="BOPDataset", img_prefix=tree["img_prefix"], filter_empty_gt=False, classes=YCBV_NAMES, image_decode=decode, **kw)
    if ann == "png":
        return build_dataset(dict(cfg, ann_file=tree["ann_file"], seg_prefix=tree["seg_prefix"], pipeline=pipe))
    pipe[1] = dict(type="LoadAnnotations", with_bbox=True, with_mask=True)
    return build_dataset(dict(cfg, ann_file=tree["rle"], mask_source="annotation", pipeline=pipe))


def _plan(ds, epoch, idx):
    from radet_amd.datasets.loader import sample_generators
    gens = [sample_generators(SEED, epoch, i) for i in idx]
    return [ds.plan_sample(i, *g) for i, g in zip(idx, gens)], gens


def _no_sync(fn):
    def wrapped(*a, **k):
        torch.cuda.set_sync_debug_mode("error")
        try:
            return fn(*a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return wrapped


def _run(ds, planned, no_sync=False):
    """run() of a planned batch; no_sync: the cached stages with synchronising calls made an error; also the C ABI calls"""
    from radet_amd import _lib
    pipe = ds.pipeline
    if no_sync:
        pipe._cached_packed, pipe._masks = _no_sync(pipe._cached_packed), _no_sync(pipe._masks)
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        return pipe.run(planned), seen
    finally:
        _lib.call = call
        if no_sync:
            del pipe._cached_packed, pipe._masks


def _assert_equal(out, ref, gens, ref_gens, what):
    assert len(out) == len(ref)
    for i in range(len(out)):
        for k in KEYS:
            assert torch.equal(out[i][k], ref[i][k]), f"{what}, sample {i}: {k}"
        assert gens[i][0].getstate() == ref_gens[i][0].getstate(), f"{what}, sample {i}: random.Random position"
        for a, b in zip(gens[i][1].get_state(), ref_gens[i][1].get_state()):
            assert np.array_equal(a, b), f"{what}, sample {i}: RandomState position"


BATCHES = ([0, 1, 2], [3, 4, 5])


@pytest.mark.parametrize("ann", ["png", "rle"])
@pytest.mark.parametrize("decode", ["host", "device"])
@pytest.mark.parametrize("mix", [False, True], ids=["pbr", "mix"])
def test_two_epochs_equal_the_uncached_pipeline(tree, mix, decode, ann):
    from radet_amd.datasets.sample_cache import CachedImage
    ref_ds = _dataset(tree, mix, decode, ann)
    ds = _dataset(tree, mix, decode, ann, sample_cache="device", cache_bytes=64 << 20)
    pipe = ds.pipeline
    n_masks = 0
    for epoch in (0, 1):
        # (a loader plans ahead of run(); here a whole epoch, so that every file of epoch 0 is a miss)
        plans = [_plan(ds, epoch, idx) for idx in BATCHES]
        ref_plans = [_plan(ref_ds, epoch, idx) for idx in BATCHES]
        before = dict(pipe.decode_stats)
        for b, ((planned, gens), (ref_planned, ref_gens)) in enumerate(zip(plans, ref_plans)):
            sources = [s["img"] for s in planned] + [s["background"] for s in planned if "background" in s]
            assert all(isinstance(a, CachedImage) for a in sources) if epoch else not any(isinstance(a, CachedImage) for a in sources)
            ref, ref_seen = _run(ref_ds, ref_planned)
            out, seen = _run(ds, planned, no_sync=bool(epoch))
            _assert_equal(out, ref, gens, ref_gens, f"epoch {epoch}, batch {b}")
            copies = seen.count("radet_copy_segments")
            if epoch:
                # one gather whatever the number of hits, no decode, no insert; then the launches of the uncached path
                assert copies == 1 and "radet_jpeg_decode" not in seen
                if ann == "png":
                    assert all("gt_masks_rle" in s and "gt_masks" not in s for s in planned)
                    assert "radet_mask_max" not in seen and "radet_rle_masks" in seen
                else:
                    assert [n for n in seen if n != "radet_copy_segments"] == [n for n in ref_seen if n != "radet_jpeg_decode"]
            else:
                assert copies == (1 if decode == "device" else 2)        # (host arrays are placed by the gather launch)
                n_masks += sum(len(s["gt_bboxes"]) for s in planned)
        st = pipe.cache_stats
        n_files = 6 + sum("background" in s for planned, _ in plans for s in planned)
        if epoch == 0:
            first = dict(st)
            assert st["hits"] == 0 and st["misses"] == n_files and st["mask_hits"] == 0
            assert 6 < st["inserted"] <= 6 + 3 and st["rejected_full"] == st["invalidated"] == 0
            assert (pipe.decode_stats["device"] > 0) == (decode == "device")
        else:
            assert st["misses"] == first["misses"] and st["hits"] == n_files
            assert st["inserted"] == first["inserted"] and st["bytes"] == first["bytes"]
            assert pipe.decode_stats == before                                  # nothing was decoded in the second epoch
            assert st["mask_hits"] == (n_masks if ann == "png" else 0)
        # the batches cover: both frame sizes in one batch, merged (and, in the first epoch, not), flipped and not
        flat = [s for planned, _ in plans for s in planned]
        assert any("background" in s for s in flat) and (epoch or any("background" not in s for s in flat))
        assert {bool(s["flip"]) for s in flat} == {True, False} and len({s["img"].shape for s in plans[0][0]}) == 2
    pipe.check_decode_errors(wait=True)


def _epochs(ds, ref_ds, epochs, what):
    for epoch in epochs:
        for idx in BATCHES:
            planned, gens = _plan(ds, epoch, idx)
            ref_planned, ref_gens = _plan(ref_ds, epoch, idx)
            out, _ = _run(ds, planned)
            ref, _ = _run(ref_ds, ref_planned)
            _assert_equal(out, ref, gens, ref_gens, f"{what}: epoch {epoch}, batch {idx}")
            yield planned


def test_budget_for_part_of_the_files(tree):
    """a budget that takes the frames and the smallest background: later batches hold hits and misses together"""
    from radet_amd.datasets.sample_cache import CachedImage
    budget = 300_000                              # frames 9216 / 5550 bytes, backgrounds 230400 / 1050000 / 921600 bytes
    ds = _dataset(tree, sample_cache="device", cache_bytes=budget)
    mixed = 0
    for planned in _epochs(ds, _dataset(tree), (0, 1, 2), "budget"):
        kinds = {isinstance(a, CachedImage) for s in planned for a in [s["img"]] + ([s["background"]] if "background" in s else [])}
        mixed += kinds == {True, False}
    st = ds.pipeline.cache_stats
    assert mixed >= 1 and st["rejected_full"] > 0 and 0 < st["bytes"] <= budget
    assert ds.pipeline.sample_cache.allocated <= budget and st["inserted"] >= 6


def test_rewritten_frame_is_decoded_again(tree, tmp_path):
    import shutil
    from PIL import Image
    root = str(tmp_path / "copy")
    shutil.copytree(os.path.dirname(tree["img_prefix"]), root)
    t = {k: v.replace(os.path.dirname(tree["img_prefix"]), root) for k, v in tree.items()}
    ds, ref_ds = _dataset(t, sample_cache="device", cache_bytes=64 << 20), _dataset(t)
    list(_epochs(ds, ref_ds, (0,), "before"))
    name = os.path.join(t["img_prefix"], "000000", "rgb", "000001.jpg")
    st = os.stat(name)
    old = np.asarray(Image.open(name))
    Image.fromarray(np.ascontiguousarray(255 - old[::-1])).save(name, quality=90)
    os.utime(name, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    list(_epochs(ds, ref_ds, (1,), "after"))
    c = ds.pipeline.cache_stats
    assert c["invalidated"] == 1 and c["misses"] >= 7 and c["hits"] >= 5
    list(_epochs(ds, ref_ds, (2,), "again"))                       # the new pixels are cached now
    assert ds.pipeline.cache_stats["invalidated"] == 1 and ds.pipeline.sample_cache.lookup(name)[0] is not None


def test_fill_on_one_stream_read_on_another(tree):
    """The insertions of a batch on stream A behind queued work, then the same files as hits on stream B with no host
    synchronisation in between: B waits for the cache's event, or it would gather arena bytes that are not written yet."""
    from radet_amd.datasets.loading import decode_bgr
    from radet_amd.datasets.sample_cache import CachedImage
    ds = _dataset(tree, sample_cache="device", cache_bytes=64 << 20)
    pipe = ds.pipeline
    dev = torch.device("cuda", torch.cuda.current_device())
    cold, _ = _plan(ds, 0, [0, 1, 2, 3])
    with_bg = [i for i, s in enumerate(cold) if "background" in s]
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    ballast = torch.zeros(64 << 20, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(a):
            for _ in range(20):
                ballast.add_(1.0)                                  # a few ms of work in front of the insertions
            pipe._cached_packed(cold, with_bg, [s["img"] for s in cold] + [cold[i]["background"] for i in with_bg], dev)
        warm, _ = _plan(ds, 1, [0, 1, 2, 3])
        warm_bg = [i for i, s in enumerate(warm) if "background" in s]
        sources = [s["img"] for s in warm] + [warm[i]["background"] for i in warm_bg]
        with torch.cuda.stream(b):
            src, offs = pipe._cached_packed(warm, warm_bg, sources, dev)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert pipe.cache_stats["hits"] >= 4 and all(isinstance(s, CachedImage) for s in sources[:4])
    b.synchronize()
    host = src.cpu().numpy()
    for s, o in zip(sources, offs):
        want = decode_bgr(s.path) if isinstance(s, CachedImage) else s          # (a background that epoch 0 did not draw)
        assert s.shape == want.shape and np.array_equal(host[o * 3:o * 3 + want.size].reshape(want.shape), want)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ training and testing
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("tiny")), n_frames=4, objects=(2, 4), n_backgrounds=1, seed=23)


def _detector():
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    cfg.merge_from_dict({"lr_config.total_steps": 40, "log_config.interval": 1})
    torch.manual_seed(0)
    det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda()
    synth_fill(det, seed=0)
    return cfg, det


def test_two_training_epochs_equal_uncached(tiny):
    from radet_amd.apis import train_detector
    from radet_amd.datasets import build_dataloader, build_dataset
    from tools.synth_bop import YCBV_NAMES, pipelines
    stats = {}

    def run(**kw):
        cfg, det = _detector()
        ds = build_dataset(dict(type="BOPDataset", ann_file=tiny["ann_file"], img_prefix=tiny["img_prefix"], seg_prefix=tiny["seg_prefix"],
                                classes=YCBV_NAMES, filter_empty_gt=False, pipeline=pipelines(tiny["background_dir"])[0], **kw))
        loader = build_dataloader(ds, samples_per_gpu=2, workers=2, seed=0)

        def batches():
            epoch = 0
            while True:
                loader.set_epoch(epoch)
                yield from loader
                epoch += 1
        try:
            return train_detector(det, batches(), cfg, max_iters=4, log=lambda *_: None)
        finally:
            loader.close()
            stats.update(ds.pipeline.cache_stats)
    ref = run()
    got = run(sample_cache="device", cache_bytes=64 << 20)
    assert len(ref) == len(got) == 4 and np.isfinite(ref).all() and ref == got        # two epochs of two batches
    assert stats["inserted"] >= 4 and stats["hits"] >= 4 and stats["mask_hits"] > 0


def test_single_gpu_test_twice_over_a_cached_pipeline(tiny):
    from radet_amd.apis import single_gpu_test
    from radet_amd.datasets import build_dataloader, build_dataset
    from tools.synth_bop import YCBV_NAMES, pipelines
    _, det = _detector()
    det.eval()

    def dataset(**kw):
        return build_dataset(dict(type="BOPDataset", ann_file=tiny["ann_file"], img_prefix=tiny["img_prefix"], classes=YCBV_NAMES,
                                  test_mode=True, pipeline=pipelines(tiny["background_dir"])[1], **kw))
    ref = single_gpu_test(det, build_dataloader(dataset(), samples_per_gpu=2, workers=2, seed=0, shuffle=False))
    ds = dataset(sample_cache="device", cache_bytes=64 << 20)
    loader = build_dataloader(ds, samples_per_gpu=2, workers=2, seed=0, shuffle=False)
    passes = [single_gpu_test(det, loader), single_gpu_test(det, loader)]
    loader.close()
    assert ds.pipeline.cache_stats["inserted"] == 4 and ds.pipeline.cache_stats["hits"] == 4
    for res in passes:
        assert len(res) == len(ref) == 4
        for ra, rb in zip(res, ref):
            assert len(ra) == len(rb)
            for ca, cb in zip(ra, rb):
                np.testing.assert_array_equal(ca, cb)
