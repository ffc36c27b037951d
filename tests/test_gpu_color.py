"""AutoAugment's colour stages on the GPU: radet_color_stats_u8 against np.bincount and radet_color_apply_u8 against the
NumPy restatement of the pixel rules (tests/_color_ref.py, checked by hand-worked cases in tests/test_color_cpu.py) on one
packed batch of awkward sizes and alignments; the bad-argument cases; radet_amd.ops' four functions; a block that mixes
colour, warp and CutOut entries through ImagePipeline._warp_packed against the staged host restatement; the colour config's
pipeline; launch parity.  Every comparison is array_equal / torch.equal."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _affine_ref as A  # noqa: E402
import _color_ref as C  # noqa: E402
import _cutout_ref as CUTREF  # noqa: E402
from _jitter_cfg import jitter_train_cfg  # noqa: E402

pytestmark = pytest.mark.gpu
# the factors of levels 3, 7 and 6 (the colour config's), as the stages compute them
FACTOR = dict(brightness=(3 / 10) * 1.8 + 0.1, contrast=(7 / 10) * 1.8 + 0.1, color=(6 / 10) * 1.8 + 0.1, equalize=1.0)
SKIP = C.SKIP_ROW


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _log_calls(fn):
    """the entry-point names fn() called, and its result"""
    from radet_amd import _lib
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        return seen, fn()
    finally:
        _lib.call = call


@pytest.fixture(scope="module")
def batch():
    """the packed batch of tests/_color_ref.py (tests/test_color_cpu.py shows that it holds the cases), computed once"""
    from radet_amd import kernels as K
    frames = C.kernel_frames(K.COLOR_CHUNK_PX)
    offs, packed = C.pack(frames)
    return frames, offs, packed


def _desc(K, frames, offs, kinds):
    D = np.zeros((len(frames), K.COLOR_DESC_INTS), np.int32)
    for i, (d, f, off, kind) in enumerate(zip(D, frames, offs, kinds)):
        K.color_desc_row(d, off, f.shape[0], f.shape[1], kind or "equalize", FACTOR[kind or "equalize"], skip=kind is None)
    return torch.from_numpy(D).to(_dev())


def _max_px(frames):
    return max(f.shape[0] * f.shape[1] for f in frames)


# ------------------------------------------------------------------------------------------------ radet_color_stats_u8
def test_stats_equal_bincount(batch):
    from radet_amd import kernels as K
    frames, offs, packed = batch
    kinds = ["equalize", "contrast", "equalize", "contrast", "brightness", "equalize", "contrast", "equalize", None]
    kinds2 = ["contrast", "equalize", "color", "equalize", "contrast", "contrast", "equalize", "contrast", None]
    buf = torch.from_numpy(packed).to(_dev())
    for ks in (kinds, kinds2):
        desc, runs = _desc(K, frames, offs, ks), []
        for _ in range(2):
            hist = torch.zeros((len(frames), 4, 256), dtype=torch.int32, device=_dev())
            seen, _ = _log_calls(lambda: K.color_stats_u8(buf, desc, hist, len(frames), _max_px(frames)))
            assert seen == ["radet_color_stats_u8"]
            runs.append(hist.cpu().numpy())
        for i, (f, kind) in enumerate(zip(frames, ks)):
            want = C.histograms(f) if kind in K.COLOR_STATS_KINDS else np.zeros((4, 256), np.int64)
            np.testing.assert_array_equal(runs[0][i], want, err_msg=f"image {i} {f.shape} {kind}")
        assert np.array_equal(runs[0], runs[1])
    assert np.array_equal(buf.cpu().numpy(), packed)                                            # the images are only read
    # the histogram is added to: a second launch doubles it
    hist = torch.zeros((len(frames), 4, 256), dtype=torch.int32, device=_dev())
    for _ in range(2):
        K.color_stats_u8(buf, desc, hist, len(frames), _max_px(frames))
    assert np.array_equal(hist.cpu().numpy(), 2 * runs[0])


# ------------------------------------------------------------------------------------------------ radet_color_apply_u8
def _run(K, frames, offs, packed, kinds):
    dev = _dev()
    buf, desc = torch.from_numpy(packed).to(dev), _desc(K, frames, offs, kinds)
    hist = torch.zeros((len(frames), 4, 256), dtype=torch.int32, device=dev)
    if any(k in K.COLOR_STATS_KINDS for k in kinds):
        K.color_stats_u8(buf, desc, hist, len(frames), _max_px(frames))
    seen, _ = _log_calls(lambda: K.color_apply_u8(buf, desc, hist, len(frames), _max_px(frames)))
    assert seen == ["radet_color_apply_u8"]
    return buf.cpu().numpy()


def _assert_buffer(got, want, frames, offs, what):
    for i, (f, off) in enumerate(zip(frames, offs)):
        np.testing.assert_array_equal(got[off * 3:off * 3 + f.size].reshape(f.shape), want[off * 3:off * 3 + f.size].reshape(f.shape),
                                      err_msg=f"{what}: image {i} {f.shape}")
    assert np.array_equal(got, want), what                                                      # guard bytes and the skip row


@pytest.mark.parametrize("kind", C.KINDS)
def test_apply_equals_the_restatement(batch, kind):
    from radet_amd import kernels as K
    frames, offs, packed = batch
    kinds = [kind] * len(frames)
    kinds[SKIP] = None
    want = C.expected(frames, offs, packed, kinds, FACTOR)
    assert not np.array_equal(want, packed)
    first = _run(K, frames, offs, packed, kinds)
    _assert_buffer(first, want, frames, offs, kind)
    assert np.array_equal(_run(K, frames, offs, packed, kinds), first)                          # run to run


def test_apply_mixed_kinds_in_one_launch(batch):
    from radet_amd import kernels as K
    frames, offs, packed = batch
    for shift in range(4):
        kinds = [C.KINDS[(i + shift) % 4] for i in range(len(frames))]
        kinds[SKIP] = None
        want = C.expected(frames, offs, packed, kinds, FACTOR)
        _assert_buffer(_run(K, frames, offs, packed, kinds), want, frames, offs, f"shift {shift}")


def test_other_factors_and_the_identity(batch):
    """factor 1.0 leaves every image as it is; the factors of levels 0 and 10 (0.1, 1.9) clip at both ends"""
    from radet_amd import kernels as K
    frames, offs, packed = batch
    dev = _dev()
    for factor in (1.0, 0.1, 1.9):
        for kind in ("brightness", "contrast", "color"):
            D = np.zeros((len(frames), K.COLOR_DESC_INTS), np.int32)
            for d, f, off in zip(D, frames, offs):
                K.color_desc_row(d, off, f.shape[0], f.shape[1], kind, factor)
            buf, desc = torch.from_numpy(packed).to(dev), torch.from_numpy(D).to(dev)
            hist = torch.zeros((len(frames), 4, 256), dtype=torch.int32, device=dev)
            K.color_stats_u8(buf, desc, hist, len(frames), _max_px(frames))
            K.color_apply_u8(buf, desc, hist, len(frames), _max_px(frames))
            want = C.expected(frames, offs, packed, [kind] * len(frames), {kind: factor})
            assert factor != 1.0 or np.array_equal(want, packed)
            _assert_buffer(buf.cpu().numpy(), want, frames, offs, f"{kind} {factor}")


def test_bad_arguments_leave_the_buffer_untouched(batch):
    from radet_amd import _lib, kernels as K
    frames, offs, packed = batch
    dev = _dev()
    f = frames[5]                                                                               # 48 x 64
    src = torch.from_numpy(np.concatenate([f.reshape(-1), np.full(30, C.GUARD, np.uint8)])).to(dev)
    buf = src.clone()
    hist = torch.zeros((3, 4, 256), dtype=torch.int32, device=dev)
    D = np.zeros((3, K.COLOR_DESC_INTS), np.int32)
    K.color_desc_row(D[0], 0, 48, 64, "brightness", 0.5)
    desc = torch.from_numpy(D).to(dev)
    for fn in (K.color_stats_u8, K.color_apply_u8):
        for args in ((buf, desc, hist, -1, 48 * 64), (buf, desc, hist, 1, -5), (buf, desc, hist, 1, 48 * 64, 1),
                     (buf, desc, hist, 70000, 48 * 64)):
            with pytest.raises((_lib.RadetHipError, AssertionError)):
                fn(*args)
        with pytest.raises(_lib.RadetHipError):                                                 # a null table
            _lib.call(f"radet_{fn.__name__}", buf.data_ptr(), buf.numel() // 3, None, 1, 48 * 64, hist.data_ptr(), 3, None)
    with pytest.raises(_lib.RadetHipError):                                                     # statistics without a histogram
        _lib.call("radet_color_stats_u8", buf.data_ptr(), buf.numel() // 3, desc.data_ptr(), 1, 48 * 64, None, 3, None)
    torch.cuda.synchronize()
    assert torch.equal(buf, src) and not hist.any()
    # rows that leave the buffer (offset 11: the last rows would pass the end; a negative offset; h * w beyond the buffer), a
    # row without pixels, a row of no kind, an Equalize row without a histogram: nothing is read or written
    for kind in ("brightness", "equalize"):
        K.color_desc_row(D[0], 11, 48, 64, kind, 0.5)
        K.color_desc_row(D[1], -1, 48, 64, kind, 0.5)
        K.color_desc_row(D[2], 0, 480, 640, kind, 0.5)
        K.color_stats_u8(buf, torch.from_numpy(D).to(dev), hist, 3, 480 * 640)
        K.color_apply_u8(buf, torch.from_numpy(D).to(dev), hist, 3, 480 * 640)
        K.color_desc_row(D[0], 0, 0, 64, kind, 0.5)
        K.color_desc_row(D[1], 0, 48, 64, None, 0.5)
        K.color_desc_row(D[2], 0, 48, 64, "equalize", 0.5)
        K.color_apply_u8(buf, torch.from_numpy(D).to(dev), None, 3, 48 * 64)
        assert torch.equal(buf, src) and not hist.any()
    # and the same launch with a row that fits maps that row only, inside its image
    K.color_desc_row(D[2], 10, 48, 64, "brightness", 0.5)
    K.color_apply_u8(buf, torch.from_numpy(D).to(dev), None, 3, 48 * 64)
    got, before = buf.cpu().numpy(), src.cpu().numpy()
    assert np.array_equal(got[30:30 + f.size], before[30:30 + f.size] // 2)
    assert np.array_equal(got[:30], before[:30])


# ------------------------------------------------------------------------------------------------ radet_amd.ops
def test_ops_functions(batch):
    from radet_amd import ops
    frames, _, _ = batch
    calls = dict(brightness=lambda x: ops.adjust_brightness(x, FACTOR["brightness"]), contrast=lambda x: ops.adjust_contrast(x, FACTOR["contrast"]),
                 color=lambda x: ops.adjust_color(x, FACTOR["color"]), equalize=ops.imequalize)
    some = [frames[1], frames[4], frames[7]]
    for kind, fn in calls.items():
        want = [C.apply(f, kind, FACTOR[kind]) for f in some]
        got = fn(some[1])                                                                       # an ndarray
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want[1])
        t = torch.from_numpy(some[2]).to(_dev())
        keep = t.clone()
        seen, got = _log_calls(lambda: fn(t))                                                   # a device tensor, out of place
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and got.data_ptr() != t.data_ptr()
        assert np.array_equal(got.cpu().numpy(), want[2]) and torch.equal(t, keep)
        stats = kind in ("contrast", "equalize")
        assert seen == (["radet_fill_zero", "radet_color_stats_u8"] if stats else []) + ["radet_color_apply_u8"]
        mixed = [some[0], torch.from_numpy(some[1]).to(_dev()), some[2]]                        # a list: one launch pair
        seen, got = _log_calls(lambda: fn(mixed))
        assert seen.count("radet_color_apply_u8") == 1 and seen.count("radet_color_stats_u8") == int(stats)
        assert isinstance(got, list) and [isinstance(g, np.ndarray) for g in got] == [True, False, True]
        for g, w in zip(got, want):
            assert np.array_equal(g if isinstance(g, np.ndarray) else g.cpu().numpy(), w)
    assert ops.imequalize([]) == []
    for bad in (np.zeros((4, 5), np.uint8), np.zeros((4, 5, 3), np.float32), np.zeros((4, 5, 4), np.uint8)):
        with pytest.raises(ValueError, match="H x W x 3 uint8"):
            ops.adjust_color(bad, 0.5)
    with pytest.raises(ValueError, match="finite number"):
        ops.adjust_brightness(frames[1], float("nan"))
    with pytest.raises(TypeError):
        ops.adjust_color(frames[1], 0.5, 0.5)                                                   # beta / gamma are not offered


# ------------------------------------------------------------------------------------------------ the order of a block's entries
def test_rank_order_of_colour_warp_and_holes():
    """colour, warp and CutOut entries of four frames in both orders, in one batch: per rank a warp launch, a CutOut launch, a
    statistics launch and an apply launch, each only where some frame has such an entry; an Equalize behind a Rotate counts the
    warp's fill pixels"""
    from radet_amd.datasets.loading import ColorOp, CutHoles, ImagePipeline
    dev = _dev()
    frame = np.random.RandomState(3).randint(0, 256, (48, 64, 3)).astype(np.uint8)
    frame[:, :32] //= 3
    rot, wfill = A.rotation_matrix((31.5, 23.5), -30, 1), (128, 128, 128)
    holes, fill = np.array([[10, 8, 40, 30], [50, 40, 70, 60]], np.int32), (0, 37, 255)
    cut_e, warp_e = CutHoles(holes, fill), (rot, wfill)
    col_e, eq_e = ColorOp("color", FACTOR["color"]), ColorOp("equalize", 1.0)
    con_e, bri_e = ColorOp("contrast", FACTOR["contrast"]), ColorOp("brightness", FACTOR["brightness"])
    ops = [[col_e, warp_e, cut_e], [cut_e, warp_e, eq_e], [warp_e, con_e], [eq_e, bri_e, warp_e], []]
    n = len(ops)
    offs = [k * (48 * 64 + 3) + 1 for k in range(n)]
    packed = np.full(offs[-1] * 3 + frame.size + 12, C.GUARD, np.uint8)
    for o in offs:
        packed[o * 3:o * 3 + frame.size] = frame.reshape(-1)
    seen, out = _log_calls(lambda: ImagePipeline._warp_packed(torch.from_numpy(packed).to(dev), ops, offs, [(48, 64)] * n, dev))
    assert seen == ["radet_fill_zero",
                    "radet_warp_affine_u8", "radet_cutout_u8", "radet_color_stats_u8", "radet_color_apply_u8",
                    "radet_warp_affine_u8", "radet_color_stats_u8", "radet_color_apply_u8",
                    "radet_warp_affine_u8", "radet_cutout_u8", "radet_color_stats_u8", "radet_color_apply_u8"]
    got = out.cpu().numpy()
    cut = lambda x: CUTREF.apply_holes(x, holes, np.array(fill, np.uint8))      # noqa: E731
    warp = lambda x: A.warp_affine_u8(x, rot, wfill)                            # noqa: E731
    col = lambda x, e: C.apply(x, e.kind, e.factor)                             # noqa: E731
    want = [cut(warp(col(frame, col_e))), col(warp(cut(frame)), eq_e), col(warp(frame), con_e), warp(col(col(frame, eq_e), bri_e)), frame]
    for i, (o, w) in enumerate(zip(offs, want)):
        np.testing.assert_array_equal(got[o * 3:o * 3 + frame.size].reshape(frame.shape), w, err_msg=f"frame {i}")
    # (the bytes between the frames are not compared: the warp launches ping-pong into a buffer that holds the frames only)
    # the order counts: Equalize in front of the Rotate gives another image than behind it
    assert not np.array_equal(col(warp(frame), eq_e), warp(col(frame, eq_e)))
    # a batch without statistics kinds zeroes and counts nothing
    seen, _ = _log_calls(lambda: ImagePipeline._warp_packed(torch.from_numpy(packed).to(dev), [[col_e], [bri_e, col_e]] + [[]] * 3, offs,
                                                            [(48, 64)] * n, dev))
    assert seen == ["radet_color_apply_u8", "radet_color_apply_u8"]


# ------------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL decodes the generated JPEG / PNG files")
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=4, objects=(3, 5), n_backgrounds=2, seed=11)


def _strip_colour(s):
    """the planned sample without its colour entries"""
    s = dict(s)
    if "color" in s:
        del s["color"]
        ops = [op for op in s["block_ops"] if op[0] != "color"]
        if any(kind == "cutout" for kind, _ in ops):
            s["block_ops"] = ops
        else:
            del s["block_ops"]
    return s


def test_color_config_pipeline_runs(tree):
    """the colour config's pipeline on the synthetic BOP sample: a batch that holds every policy; a sample whose colour entries
    are taken out of its plan gives another image, a sample without any gives the same one"""
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loader import sample_generators
    cfg, train = jitter_train_cfg(tree, name="r50_ycbv_pbr_color.py")
    ds = build_dataset(train)
    plans, kinds = [], set()
    for epoch in range(40):                                          # four samples that cover the colour kinds and a plain one
        for i in range(4):
            s = ds.plan_sample(i, *sample_generators(0, epoch, i))
            new = {op.kind for op in s.get("color", ())} - kinds
            if (new or ("plain" not in kinds and "color" not in s)) and len(plans) < 6:
                kinds |= new | ({"plain"} if "color" not in s else set())
                plans.append(s)
    assert kinds >= {"color", "equalize", "brightness", "contrast", "plain"}, kinds
    without = [_strip_colour(copy.deepcopy(s)) for s in plans]
    seen, batch = _log_calls(lambda: ds.pipeline.run(plans, collate=True))
    assert tuple(batch["img"].shape) == (len(plans), 3, 480, 640) and bool(torch.isfinite(batch["img"]).all())
    assert all(len(b) == len(l) for b, l in zip(batch["gt_bboxes"], batch["gt_labels"]))
    ranks = max(len(s.get("block_ops", ())) for s in plans)
    assert seen.count("radet_fill_zero") == 1 and 1 <= seen.count("radet_color_apply_u8") <= ranks
    assert 1 <= seen.count("radet_color_stats_u8") <= seen.count("radet_color_apply_u8")
    assert max(i for i, n in enumerate(seen) if "color" in n) < seen.index("radet_augment_merge_hblur")
    second, plain = _log_calls(lambda: ds.pipeline.run(without, collate=True))
    assert not any("color" in n for n in second) and "radet_fill_zero" not in second
    assert [n for n in seen if "color" not in n and n != "radet_fill_zero"] == second
    changed = 0
    for j, s in enumerate(plans):
        same = torch.equal(batch["img"][j], plain["img"][j])
        assert same or "color" in s, j
        changed += not same
        assert torch.equal(batch["gt_bboxes"][j], plain["gt_bboxes"][j])                          # boxes never move
    assert changed >= 3


def test_launch_parity(tree):
    """a batch in which no colour stage fired issues the launches, and gives the output, of the pipeline built without the
    stages (a stage at prob=0 draws once from the NumPy generator, so the later draws are set equal by hand); the default
    pipeline issues no colour launch"""
    import test_gpu_cutout as TC
    never = TC._dataset(tree, (dict(type="ColorTransform", level=6, prob=0), TC.ROTATE, dict(type="EqualizeTransform", prob=0)))
    without = TC._dataset(tree, (TC.ROTATE,))
    a, b = TC._plans(never), TC._plans(without)
    assert not any(key in s for s in a for key in ("block_ops", "color")) and all("affine" in s for s in a)
    keep = [{key: copy.deepcopy(t[key]) for key in TC.HANDED} for t in b]      # (before a run advances the RandomStates)
    for s, t, k in zip(a, b, keep):
        assert set(s) == set(t)
        s.update(copy.deepcopy(k))
    first, got = _log_calls(lambda: never.pipeline.run(a, collate=True))
    second, want = _log_calls(lambda: without.pipeline.run(b, collate=True))
    assert first == second and not any("color" in n for n in first) and "radet_fill_zero" not in first
    assert "radet_warp_affine_u8" in first
    assert torch.equal(got["img"], want["img"])
    for key in ("gt_bboxes", "gt_labels", "points_to_gt_index", "points_weight"):
        assert all(torch.equal(x, y) for x, y in zip(got[key], want[key]))
    # and colour entries add exactly their launches: one zero fill, then per rank a statistics and an apply launch
    fired = TC._dataset(tree, (dict(type="ContrastTransform", level=7, prob=1), TC.ROTATE, dict(type="ColorTransform", level=6, prob=1)))
    d = TC._plans(fired)
    assert all(s["block_ops"] == [("color", 0), ("warp", 0), ("color", 1)] for s in d)
    for s, k in zip(d, keep):
        s.update(copy.deepcopy(k))
    third, _ = _log_calls(lambda: fired.pipeline.run(d, collate=True))
    assert [n for n in third if "color" not in n and n != "radet_fill_zero"] == second
    assert [n for n in third if "color" in n or n == "radet_fill_zero"] == [
        "radet_fill_zero", "radet_color_stats_u8", "radet_color_apply_u8", "radet_color_apply_u8"]
    # the frames' warp launch (the first; the masks' follow behind the block) stands between the two ranks' apply launches
    applies = [i for i, n in enumerate(third) if n == "radet_color_apply_u8"]
    assert applies[0] < third.index("radet_warp_affine_u8") < applies[1] < third.index("radet_augment_merge_hblur")
    # the default pipeline (the pbr stages, no block): the call list holds no colour launch and no histogram fill
    plain = TC._dataset(tree)
    calls, _ = _log_calls(lambda: plain.pipeline.run(TC._plans(plain), collate=True))
    assert calls and not any("color" in n or "cutout" in n or "warp" in n for n in calls) and "radet_fill_zero" not in calls
