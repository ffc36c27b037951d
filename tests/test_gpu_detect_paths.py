"""The inference paths behind inference_detector and detect_frames, side by side: single view, test-time augmentation (one
scale + a flip; two scales) and tiling, each with and without crops=.  Per path the stream issues the launches of the
one-shot call and yields its results bit for bit, crops= adds no synchronising call to any stream, and an abandoned tiling
stream leaves the runtime usable.  Public entry points only."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_crops import _log_calls, _same_crops, _sync_warnings  # noqa: E402
from test_gpu_tta import SCALE_A, SCALE_B, _pipe  # noqa: E402

pytestmark = pytest.mark.gpu

CROPS = dict(size=(16, 12), scale=1.3)
# the tiny detector and frames of tests/test_gpu_tta.py; every forward batch is 1, 2 or 4 rows padded to 480 x 640 (pinned
# picks), but for the second scale's 240 x 320.
# tiling: a 64 x 48 tile without overlap cuts the 60 x 80 and 75 x 100 frames into 2 x 2 tiles (5 rows with the full frame)
# and leaves the smaller frames whole (2 rows); 2 rows per forward pass: frames[:2] run as 2 forward batches, frames[2:4] as 4
MODES = dict(
    single=None,
    tta_flip=("tta", dict(img_scale=[SCALE_A], flip=True, flip_direction="horizontal")),
    tta_scales=("tta", dict(img_scale=[SCALE_A, SCALE_B], flip=False)),
    tiles=("tiling", dict(tile=(64, 48), overlap=(0, 0), batch=2, nms_pre=200)),
)
# of frames[:2]: the forward groups of a batch, the merge launch behind them, the preparation launches in front (one per scale)
GROUPS = dict(single=(1, None, 1), tta_flip=(1, "radet_merge_views", 1), tta_scales=(2, "radet_merge_views", 2),
              tiles=(2, "radet_merge_tiles", 1))
POST = ("radet_preprocess_frames", "radet_decode_candidates", "radet_merge_views", "radet_merge_tiles", "radet_nms", "radet_soft_nms",
        "radet_crop_plan", "radet_crop_frames")


@pytest.fixture(scope="module")
def det():
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(0)
    d = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().eval()
    synth_fill(d, seed=0)
    with torch.no_grad():
        d.bbox_head.atss_cls.bias += 2.0                       # (scores above the threshold: the comparisons are not vacuous)
    d.cfg = Config(dict(data=dict(test=dict(pipeline=_pipe("LoadImageFromFile", img_scale=SCALE_A)))))
    return d


@pytest.fixture(scope="module")
def frames():
    rng = np.random.RandomState(11)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (48, 64), (60, 80), (30, 40), (75, 100))]


@contextlib.contextmanager
def _mode(det, name):
    """the mode on the (module-wide) detector for the length of a block"""
    from radet_amd.apis import set_tiling, set_tta
    setters = dict(tta=set_tta, tiling=set_tiling)
    if MODES[name] is not None:
        setters[MODES[name][0]](det, MODES[name][1])
    try:
        yield det
    finally:
        set_tta(det, None)
        set_tiling(det, None)


def _kw(crops):
    return dict(crops=CROPS) if crops else {}


def test_tiling_case_has_tiles_and_two_forward_batches(frames):
    from radet_amd.ops.tiles import tile_rows
    _, _, row_start = tile_rows([f.shape[:2] for f in frames], MODES["tiles"][1])
    assert np.diff(row_start).tolist() == [2, 2, 5, 2, 5]       # the 75 x 100 frame: its full-frame row + 4 tiles
    assert all(int(row_start[lo + n] - row_start[lo]) > MODES["tiles"][1]["batch"] for lo, n in ((0, 2), (2, 2), (4, 1)))


# ------------------------------------------------------------------------------------------- (a) the launches
@pytest.mark.parametrize("crops", [False, True], ids=["plain", "crops"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_stream_issues_the_one_shot_launches(det, frames, mode, crops):
    from radet_amd.apis import detect_frames, inference_detector
    groups, merge, preps = GROUPS[mode]
    with _mode(det, mode):
        def stream():
            return list(detect_frames(det, frames[:2], batch_size=2, on_device=True, **_kw(crops)))

        def one_shot():
            return inference_detector(det, frames[:2], **_kw(crops))
        stream(), one_shot()                                     # (weight fold, plans, tuned picks: not part of the logs)
        stream_log, got = _log_calls(stream)
        shot_log, _ = _log_calls(one_shot)
    assert len(got) == 2
    assert stream_log == shot_log
    log = shot_log
    assert log[:preps] == ["radet_preprocess_frames"] * preps and log.count("radet_preprocess_frames") == preps
    at = [i for i, n in enumerate(log) if n == "radet_decode_candidates"]
    assert len(at) == groups
    # every group: a forward pass, then its decode
    for a, b in zip([preps - 1] + at[:-1], at):
        assert b > a + 1 and not [n for n in log[a + 1:b] if n in POST], log[a + 1:b]
    # behind the last decode: the one merge, the one NMS launch, the two crop launches -- and nothing else
    want = ([merge] if merge else []) + ["radet_nms"] + (["radet_crop_plan", "radet_crop_frames"] if crops else [])
    assert log[at[-1] + 1:] == want


# ------------------------------------------------------------------------------------------- (b) the results
@pytest.mark.parametrize("crops", [False, True], ids=["plain", "crops"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_stream_yields_the_one_shot_results(det, frames, mode, crops):
    from radet_amd.apis import detect_frames, inference_detector
    from radet_amd.core.bbox import bbox2result
    from radet_amd.ops.crops import Crops
    num_classes = det.bbox_head.num_classes
    with _mode(det, mode):
        got = list(detect_frames(det, iter(frames), batch_size=2, on_device=True, **_kw(crops)))
        want = [inference_detector(det, frames[lo:lo + 2], **_kw(crops)) for lo in (0, 2, 4)]
    assert len(got) == 5
    n_dets = 0
    for k, lo in enumerate((0, 2, 4)):
        batch = got[lo:lo + 2]
        res, batch_crops = want[k] if crops else (want[k], None)
        assert len(res) == len(batch)
        for item, per_class in zip(batch, res):
            boxes, labels = item[0] if crops else item
            assert boxes.is_cuda and boxes.dtype == torch.float32 and labels.dtype == torch.int64
            n_dets += int(boxes.shape[0])
            mine = bbox2result(boxes, labels, num_classes)
            assert len(mine) == len(per_class) == num_classes
            for x, y in zip(mine, per_class):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(torch.from_numpy(x), torch.from_numpy(y))
        if crops:
            parts = [c for _, c in batch]
            assert all(c.n_total == batch_crops.n_total for c in parts)
            whole = Crops(*(torch.cat([c[i] for c in parts]) for i in range(3)), parts[0].n_total)
            _same_crops(whole, batch_crops)
            assert whole.images.shape[0] > 0
    assert n_dets > 0


# ------------------------------------------------------------------------------------------- (c) synchronising calls
@pytest.mark.parametrize("mode", sorted(MODES))
def test_crops_add_no_synchronising_call_to_the_stream(det, frames, mode):
    from radet_amd.apis import detect_frames
    got = []
    with _mode(det, mode):
        list(detect_frames(det, frames, batch_size=2, on_device=True, crops=CROPS))          # (plans, allocator pools)
        assert _sync_warnings(lambda: torch.zeros(3, device="cuda").cpu()) >= 1              # (the count sees a blocking copy)
        plain = _sync_warnings(lambda: list(detect_frames(det, frames, batch_size=2, on_device=True)))
        with_crops = _sync_warnings(lambda: got.extend(detect_frames(det, frames, batch_size=2, on_device=True, crops=CROPS)))
    print(f"{mode}: synchronising calls: {plain} without crops=, {with_crops} with")
    assert with_crops == plain
    assert len(got) == 5 and sum(int(c.images.shape[0]) for _, c in got) > 0


# ------------------------------------------------------------------------------------------- (d) an abandoned stream
def test_abandoned_tiling_stream_leaves_the_runtime_usable(det, frames):
    from radet_amd.apis import detect_frames, inference_detector
    before = inference_detector(det, frames[:2])
    assert sum(len(c) for r in before for c in r) > 0
    with _mode(det, "tiles"):
        want = inference_detector(det, frames[:2])
        it = detect_frames(det, frames, batch_size=2)
        first = next(it)                                         # (the second batch is in flight)
        it.close()
        assert all(np.array_equal(x, y) for x, y in zip(first, want[0]))
    after = inference_detector(det, frames[:2])
    assert len(after) == len(before) == 2
    for ra, rb in zip(after, before):
        assert len(ra) == len(rb) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(ra, rb))
