"""init_detector / inference_detector with the reference's signatures (radet/apis/inference.py), for inputs that are
already normalised NCHW tensors, for image files, and for frames in memory (ndarray or device tensor HxWx3 uint8 BGR), which
go through the config's test pipeline as in the reference; detect_frames streams an iterable of frames through it."""
from collections import namedtuple

import numpy as np
import torch

from ..core.bbox import bbox2result
from ..models import build_detector
from ..utils import Config
from .train import load_checkpoint


def init_detector(config, checkpoint=None, device="cuda:0", cfg_options=None):
    if isinstance(config, str):
        config = Config.fromfile(config)
    if cfg_options:
        config.merge_from_dict(cfg_options)
    config.model["pretrained"] = None
    model = build_detector(config.model, train_cfg=config.get("train_cfg"), test_cfg=config.get("test_cfg"))
    if checkpoint is not None:
        meta, _ = load_checkpoint(model, checkpoint)
        model.CLASSES = meta.get("CLASSES")
    model.cfg = config
    return model.to(device).eval()


def _inference_files(model, names):
    """file names through model.cfg.data.test.pipeline (LoadImageFromFile ... MultiScaleFlipAug with one view), one image
    per device pass: the files may differ in size"""
    import random
    from ..datasets.loading import ImagePipeline
    cfg = getattr(model, "cfg", None)
    if cfg is None:
        raise ValueError("inference_detector on file names needs model.cfg (init_detector sets it)")
    pipeline = ImagePipeline(cfg.data.test.pipeline)
    out = []
    with torch.no_grad():
        for name in names:
            sample = dict(img_info=dict(filename=name), img_prefix=None, bbox_fields=[], mask_fields=[], seg_fields=[])
            data = pipeline.run([pipeline.plan(sample, random, np.random)], collate=True)
            out += model(return_loss=False, rescale=True, **data)
    return out


def _is_frame(x):
    """a loaded image: an ndarray, or a uint8 tensor whose last dimension is 3 (a float tensor means normalised NCHW)"""
    return isinstance(x, np.ndarray) or (isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and x.dim() >= 1 and x.shape[-1] == 3)


_FILE_LOADER_ARGS = ("decode", "index_cache", "seg_mcus")        # LoadImageFromFile's own; LoadImageFromWebcam has no file


_TTA_KEYS = ("img_scale", "flip", "flip_direction")


def _tta_stages(stages, tta):
    """the test pipeline with the three view arguments of its MultiScaleFlipAug stage replaced by tta's; its transforms stay"""
    if not isinstance(tta, dict) or not tta or set(tta) - set(_TTA_KEYS):
        raise ValueError(f"tta={tta!r}: expected dict([{', '.join(_TTA_KEYS)}])")
    at = [i for i, t in enumerate(stages) if dict(t).get("type") == "MultiScaleFlipAug"]
    if len(at) != 1:
        raise ValueError("tta=: the test pipeline has no single MultiScaleFlipAug stage to override")
    stages = list(stages)
    stages[at[0]] = {**dict(stages[at[0]]), **tta}
    return stages


def set_tta(model, tta=None):
    """Test-time augmentation for this model's inference on loaded frames (inference_detector, detect_frames), set on the model
    beside its cfg: tta=dict(img_scale=[...], flip=True, flip_direction='horizontal' | 'vertical' | 'diagonal' | a list)
    overrides those three arguments of the MultiScaleFlipAug stage of model.cfg.data.test.pipeline; its transforms stay.
    None clears the override (the config's own stage, which may itself make several views, holds again).  The two entry
    points keep the reference's signatures, so the override is a property of the model, not an argument of theirs.
    With an override set, file names and normalised tensors are refused by inference_detector.  Returns the model."""
    if tta is not None:
        tta = dict(tta)
        if not tta or set(tta) - set(_TTA_KEYS):
            raise ValueError(f"tta={tta!r}: expected dict([{', '.join(_TTA_KEYS)}])")
    object.__setattr__(model, "tta", tta)
    return model


def set_tiling(model, tiling=None):
    """Tiled inference for this model's calls on loaded frames (inference_detector, detect_frames), set on the model beside
    its cfg, like set_tta: tiling=dict(tile=(tw, th), overlap=0.25, full_frame=True, edge_margin=0.0, batch=16, nms_pre=None).
    Every frame is cut into overlapping tiles of tw x th frame pixels (ops.plan_tiles; overlap in pixels (ow, oh) or one
    float ratio of the tile); the frame itself (full_frame) and every tile go through the config's test pipeline at its
    img_scale as rows of one batch, `batch` rows per forward pass; candidates that touch a cut side of their tile within
    edge_margin pixels are dropped, the others are mapped back to the frame and the config's NMS runs once per frame
    (DetectorRuntime.detect_tiles).  nms_pre replaces test_cfg's for these calls: a tile holds fewer objects than a frame, and
    the merged list of a frame is limited to 65536 candidates.  None clears it.  With tiling set, file names, normalised
    tensors, a set_tta override and a multi-view config are refused.  The plan, the edge rule and the defaults are this
    project's own starting points; nobody has evaluated them on BOP data.  Returns the model."""
    from ..ops.tiles import tiling_spec
    object.__setattr__(model, "tiling", None if tiling is None else tiling_spec(dict(tiling) if isinstance(tiling, dict) else tiling))
    return model


def _tile_pipeline(model):
    """the frame pipeline a tiled call runs its rows through; refuses what tiling does not compose with"""
    if getattr(model, "tta", None) is not None:
        raise NotImplementedError("set_tiling together with a set_tta override: tiles and test-time-augmentation views are not "
                                  "combined; clear one of them (set_tta(model, None) or set_tiling(model, None))")
    pipeline = _frame_pipeline(model)
    if pipeline.views > 1:
        raise NotImplementedError(f"set_tiling with a config whose MultiScaleFlipAug makes {pipeline.views} views: tiles and "
                                  "test-time-augmentation views are not combined; use one img_scale and flip=False, or clear the "
                                  "tiling (set_tiling(model, None))")
    return pipeline


# with set_tiling or set_tta, inference_detector takes loaded frames only: what the mode is called, and how anything that is
# neither a frame nor a file name is refused
_FRAMES_ONLY = dict(
    set_tiling=("tiled inference", NotImplementedError,
                "inference_detector on a normalised NCHW tensor with set_tiling(model, ...): tiles are cut from loaded frames "
                "(ndarray or uint8 tensor HxWx3 BGR) in front of the test pipeline; pass the frames, or clear the tiling "
                "(set_tiling(model, None))"),
    set_tta=("test-time augmentation", ValueError,
             "inference_detector with set_tta(model, ...) takes loaded frames (ndarray or uint8 tensor HxWx3 BGR)"))


def _loaded_frames_only(imgs, setter):
    what, error, message = _FRAMES_ONLY[setter]
    listed = isinstance(imgs, (list, tuple))
    if isinstance(imgs, str) or (listed and any(isinstance(i, str) for i in imgs)):
        raise NotImplementedError(f"inference_detector on file names with {setter}(model, ...): {what} is built for frames in "
                                  "memory; load the images (mmcv.imread order: HxWx3 uint8 BGR) and pass them")
    if not (_is_frame(imgs) or (listed and all(_is_frame(i) for i in imgs))):
        raise error(message)


def _frame_pipeline(model, tta=None):
    """model.cfg.data.test.pipeline with its first stage replaced by LoadImageFromWebcam (radet/apis/inference.py:97-102), built
    once per model, test pipeline and tta= override (the few last ones are kept)"""
    from ..datasets.loading import ImagePipeline
    cfg = getattr(model, "cfg", None)
    if cfg is None:
        raise ValueError("inference on frames needs model.cfg (init_detector sets it)")
    stages = list(cfg.data.test.pipeline)
    key = (repr(stages), None if tta is None else repr(sorted(dict(tta).items())))
    # model._frame_pipeline: (key, pipeline) of the config's own pipeline; model._tta_pipelines: the last few tta= overrides
    if tta is None:
        cached = getattr(model, "_frame_pipeline", None)
        if cached is not None and cached[0] == key:
            return cached[1]
    else:
        cache = getattr(model, "_tta_pipelines", None)
        if cache is None:
            cache = {}
            object.__setattr__(model, "_tta_pipelines", cache)
        if key in cache:
            return cache[key]
        stages = _tta_stages(stages, tta)
    first = {k: v for k, v in dict(stages[0]).items() if k not in _FILE_LOADER_ARGS}
    first["type"] = "LoadImageFromWebcam"
    pipeline = ImagePipeline([first] + stages[1:])
    if tta is None:
        object.__setattr__(model, "_frame_pipeline", (key, pipeline))
    else:
        while len(cache) >= 4:
            cache.pop(next(iter(cache)))
        cache[key] = pipeline
    return pipeline


def _prepare_frames(pipeline, frames, with_source=False):
    """one batch of frames, of any sizes, through the pipeline: the collated test batch (one upload, one launch); with_source:
    (that batch, (descriptor table, frames)) for the crops that are cut from the frames behind NMS"""
    import random
    planned = [pipeline.plan(dict(img=f, bbox_fields=[], mask_fields=[], seg_fields=[]), random, np.random) for f in frames]
    return pipeline.run_frames(planned) if with_source else pipeline.run(planned, collate=True)


_CROP_KEYS = ("size", "scale", "score_thr", "max_crops", "fill", "normalize")


def _crop_request(model, crops):
    """crops=dict(size=..., scale=1.2, score_thr=0.0, max_crops=None, fill=(0, 0, 0), normalize=...) -> ops.crops.CropSpec.
    normalize defaults to the test pipeline's img_norm_cfg (None asks for u8 NHWC BGR crops), max_crops to every detection
    slot of the batch (B * max_per_img)."""
    from ..ops.crops import crop_spec
    if not isinstance(crops, dict) or "size" not in crops or set(crops) - set(_CROP_KEYS):
        raise ValueError(f"crops={crops!r}: expected dict(size=..., [{', '.join(_CROP_KEYS[1:])}])")
    kw = dict(crops)
    if "normalize" not in kw:
        stages = list(model.cfg.data.test.pipeline)
        stages += [t for s in stages for t in (s.get("transforms") or ())]
        norm = [s for s in stages if s.get("type") == "Normalize"]
        if len(norm) != 1:
            raise ValueError("crops: the test pipeline has no single Normalize stage; pass normalize=dict(mean, std, to_rgb)")
        kw["normalize"] = dict(mean=norm[0]["mean"], std=norm[0]["std"], to_rgb=norm[0].get("to_rgb", True))
    return crop_spec(**kw)


def _single_view(data):
    imgs, metas = data["img"], data["img_metas"]
    if isinstance(imgs, (list, tuple)):                      # (a MultiScaleFlipAug pipeline: the single test view)
        imgs, metas = imgs[0], metas[0]
    return imgs, metas


_Mode = namedtuple("_Mode", "prepare table one_shot stream module_call")


def _frame_mode(model):
    """How this model's calls on loaded frames run -- tiles (set_tiling), views (a set_tta override, or a config whose
    MultiScaleFlipAug makes several) or a single view -- chosen once per call; refuses what does not compose.
    -> prepare(group of frames, with_source) -> the batch as the runtime's stream takes it (with_source: the descriptor table
    and the frames ride along for the crops; views and tiles always carry them), table(batch) -> that table (its first B rows:
    the source frames), one_shot(runtime, batch, crops) -> what DetectorRuntime.detect returns (crops: None or (CropSpec,
    table)), stream(runtime, batches, spec) -> the runtime's generator (spec: None or the CropSpec), module_call: without
    crops the one-shot is the module's own forward call (simple_test / aug_test), as for a normalised tensor."""
    tiling = getattr(model, "tiling", None)
    if tiling is not None:
        pipeline = _tile_pipeline(model)

        def prepare(group, with_source):
            plan = pipeline.run_tile_rows(group, tiling)
            return plan["img"], plan
        return _Mode(prepare, lambda b: b[1]["table"], lambda rt, b, crops: rt.detect_tiles(b[0], b[1], model.test_cfg, crops=crops),
                     lambda rt, batches, spec: rt.detect_tiles_stream(batches, model.test_cfg, crops=spec), False)
    pipeline = _frame_pipeline(model, getattr(model, "tta", None))
    if pipeline.views > 1:
        def prepare(group, with_source):
            data, source = _prepare_frames(pipeline, group, True)
            return data["img"], data["img_metas"], source
        return _Mode(prepare, lambda b: b[2][0], lambda rt, b, crops: rt.detect_aug(b[0], b[1], model.test_cfg, True, crops=crops),
                     lambda rt, batches, spec: rt.detect_aug_stream(batches, model.test_cfg, crops=spec), True)

    def prepare(group, with_source):
        if not with_source:
            return _single_view(_prepare_frames(pipeline, group))
        data, source = _prepare_frames(pipeline, group, True)
        return _single_view(data) + (source,)
    return _Mode(prepare, lambda b: b[2][0], lambda rt, b, crops: rt.detect(b[0], b[1], model.test_cfg, True, crops=crops),
                 lambda rt, batches, spec: rt.detect_stream(batches, model.test_cfg, rescale=True,
                                                            **({} if spec is None else dict(crops=spec))), True)


def _inference_frames(model, frames, crops=None):
    """one batch of loaded frames -> their results, or with crops= (results, Crops of the batch)"""
    spec = None
    if crops is not None:
        from ..ops.crops import check_frames
        check_frames(frames)
        spec = _crop_request(model, crops)
    mode = _frame_mode(model)
    if spec is None and not frames:
        return []
    batch = mode.prepare(frames, spec is not None)
    if spec is None and mode.module_call:
        imgs, metas = batch[:2]
        if not isinstance(imgs, (list, tuple)):
            imgs, metas = [imgs], [metas]
        with torch.no_grad():
            return model(img=imgs, img_metas=metas, return_loss=False, rescale=True)
    if model.training:
        model.eval()
    out = mode.one_shot(model.runtime(), batch, None if spec is None else (spec, mode.table(batch)))
    results = [bbox2result(b, l, model.bbox_head.num_classes) for b, l in (out if spec is None else out[0])]
    return results if spec is None else (results, out[1])


def detect_frames(model, frames, batch_size=8, on_device=False, crops=None):
    """Generator over an iterable of frames (ndarray or device tensor HxWx3 uint8 BGR, sizes may differ): batches of
    `batch_size` frames (the last one smaller) go through the frame pipeline and `DetectorRuntime.detect_stream`, so the host
    is one batch behind the device.  Yields one result per frame, in order: the per-class list of ndarray[k, 5] (boxes in the
    frame's own coordinates), or with on_device=True the (dets f32[k, 5], labels i64[k]) device tensors.  Leaving the loop
    early closes the stream underneath, which leaves the runtime ready for the next call.
    crops=dict(size=..., ...) as for inference_detector: yields (result, Crops of that frame) -- the crops of a batch are cut
    from its frames on the device behind its NMS; a frame's record holds views of the batch's tensors and the batch's n_total.
    Test-time augmentation -- set_tta(model, dict(img_scale=[...], flip=True, flip_direction=...)), or a config whose
    MultiScaleFlipAug makes several views: every batch runs DetectorRuntime.detect_aug's program -- the forward batch is F * batch_size per
    scale (F: that scale's unflipped + flipped views) -- still one batch behind the device, on the caller's stream.
    Tiled inference -- set_tiling(model, dict(tile=(tw, th), ...)): every batch runs DetectorRuntime.detect_tiles' program over
    the rows of its batch_size frames (full-frame views and tiles), likewise one batch behind the device."""
    from ..ops.crops import check_frames, split_crops
    if batch_size < 1:
        raise ValueError(f"batch_size={batch_size}")
    mode = _frame_mode(model)
    spec = None if crops is None else _crop_request(model, crops)
    if model.training:
        model.eval()
    num_classes = model.bbox_head.num_classes

    def batches():
        group = []
        for f in frames:
            group.append(f)
            if len(group) == batch_size:
                yield group
                group = []
        if group:
            yield group

    def prepared():
        for group in batches():
            if spec is not None:
                check_frames(group)
            yield mode.prepare(group, spec is not None)      # (the stream carries the table and the frames with the batch)

    stream = mode.stream(model.runtime(), prepared(), spec)
    try:
        for dets in stream:
            per_frame = None
            if spec is not None:
                dets, batch_crops, ends = dets
                per_frame = split_crops(batch_crops, ends)  # (ends came with the counts: nothing is read from the device)
            for i, (boxes, labels) in enumerate(dets):
                res = (boxes, labels) if on_device else bbox2result(boxes, labels, num_classes)
                yield res if per_frame is None else (res, per_frame[i])
    finally:
        stream.close()


def inference_detector(model, imgs, scale_factor=None, crops=None):
    """imgs: f32[B,3,H,W] (normalised) -> list[B] of list[num_classes] of ndarray[k,5]; or a file name -> the result of that
    image; or a list of file names -> the list of their results; or a loaded image (ndarray, or uint8 device tensor, HxWx3
    BGR) -> its result; or a list of those, of any sizes -> the list of their results, computed as one batch
    (radet/apis/inference.py:86-140).
    crops=dict(size=(Ho, Wo) or int, scale=1.2, score_thr=0.0, max_crops=None, fill=(0, 0, 0), normalize=...), with loaded
    frames only: returns (results, ops.Crops) -- one crop per detection, cut from its frame on the device behind NMS, resized to
    `size` and normalised like the test pipeline (normalize=None: u8 NHWC BGR); see radet_amd.ops.crop_detections.  An empty
    list of frames is refused with crops= (without it the result is []): there is no batch to cut crops from.
    Memory: the crops' tensor is allocated before the number of detections is known, max_crops slots of 3 * Ho * Wo values
    (f32: 12 * Ho * Wo bytes each), and the returned views keep all of it alive.  The default max_crops is every detection
    slot of the batch, B * max_per_img -- 629 MB for 8 frames x 100 slots of 256 x 256 f32, twice that in flight in
    detect_frames -- so pass the max_crops the pose stage can take.
    Test-time augmentation, with loaded frames only: a MultiScaleFlipAug with several views (flip=True, several img_scale) in
    cfg.data.test.pipeline is honoured as in the reference, and set_tta(model, dict(img_scale=[...], flip=True,
    flip_direction='horizontal' | 'vertical' | 'diagonal' | a list)) overrides those three arguments of the config's stage
    (its transforms stay) for this model's calls.  The frames go through DetectorRuntime.detect_aug: the forward batch is F * batch_size per scale (F = that
    scale's unflipped + flipped views), the views' candidates are mapped back and merged on the GPU and the config's NMS
    runs once.  How the views compose is this project's rule (detect_aug); with an override set, file names are refused.
    Tiled inference, with loaded frames only: after set_tiling(model, dict(tile=(tw, th), ...)) every frame runs as its
    full-frame view plus overlapping tiles at the network's resolution, merged by one NMS per frame
    (DetectorRuntime.detect_tiles); results and crops= stay in the frames' coordinates."""
    tiling, tta = getattr(model, "tiling", None), getattr(model, "tta", None)
    if tiling is not None and tta is not None:
        _tile_pipeline(model)                                    # (refuses: tiling together with a set_tta override)
    if tiling is not None or tta is not None:
        _loaded_frames_only(imgs, "set_tiling" if tiling is not None else "set_tta")
    if crops is not None or tiling is not None:
        if _is_frame(imgs):
            res = _inference_frames(model, [imgs], crops)
            return res[0] if crops is None else (res[0][0], res[1])
        return _inference_frames(model, list(imgs) if isinstance(imgs, (list, tuple)) else imgs, crops)
    if isinstance(imgs, str):
        return _inference_files(model, [imgs])[0]
    if isinstance(imgs, (list, tuple)) and all(isinstance(i, str) for i in imgs):
        return _inference_files(model, list(imgs))
    if _is_frame(imgs):
        return _inference_frames(model, [imgs])[0]
    if isinstance(imgs, (list, tuple)) and imgs and all(_is_frame(i) for i in imgs):
        return _inference_frames(model, list(imgs))
    if imgs.dim() == 3:
        imgs = imgs[None]
    B, _, H, W = imgs.shape
    sf = np.ones(4, np.float32) if scale_factor is None else np.asarray(scale_factor, np.float32)
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=sf, flip=False) for _ in range(B)]
    with torch.no_grad():
        return model(img=[imgs], img_metas=[metas], return_loss=False, rescale=True)


class _DrawGroup:
    """One batch of draw_frames: its host frames go up ONCE, in one pinned non-blocking copy, as device views -- what
    detect_frames reads and what the overlay is drawn into --, followed in the same allocation by the destinations of the
    caller's device frames (unless inplace).  sources[i]: what the detector reads; dests[i]: where frame i's overlay lands."""

    def __init__(self, frames, dev, inplace):
        sizes = [int(f.shape[0]) * int(f.shape[1]) * 3 for f in frames]
        host = [isinstance(f, np.ndarray) for f in frames]
        n_up = sum(s for s, h in zip(sizes, host) if h)
        n_out = 0 if inplace else sum(s for s, h in zip(sizes, host) if not h)
        self.buf = torch.empty(max(n_up + n_out, 1), dtype=torch.uint8, device=dev)
        self.sources, self.dests, self.slices = [], [], []
        stage = torch.empty(max(n_up, 1), dtype=torch.uint8, pin_memory=True)
        arr, up, out = stage.numpy(), 0, n_up
        for f, n, h in zip(frames, sizes, host):
            shape = (int(f.shape[0]), int(f.shape[1]), 3)
            if h:
                np.copyto(arr[up:up + n].reshape(shape), f)
                view = self.buf[up:up + n].view(shape)
                self.sources.append(view)
                self.dests.append(view)
                self.slices.append((up, n))
                up += n
            else:
                self.sources.append(f)
                self.dests.append(f if inplace else self.buf[out:out + n].view(shape))
                self.slices.append(None if inplace else (out, n))
                out += 0 if inplace else n
        if n_up:
            self.buf[:n_up].copy_(stage[:n_up], non_blocking=True)

    def to_host(self):
        """the annotated frames as host arrays: ONE copy of the batch's allocation (frames drawn in place in the caller's
        own tensors come back one by one)"""
        stage = torch.empty(self.buf.numel(), dtype=torch.uint8, pin_memory=True)
        stage.copy_(self.buf, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        arr = stage.numpy()
        return [d.cpu().numpy() if s is None else arr[s[0]:s[0] + s[1]].reshape(tuple(d.shape)) for d, s in zip(self.dests, self.slices)]


def draw_frames(model, frames, batch_size=8, on_device=False, inplace=False, **style):
    """Generator over an iterable of frames, as detect_frames: yields (result, annotated frame) per frame, in order -- the
    frame's detections drawn on it (box outlines, "name|score" labels) by ONE HIP launch per batch on the caller's stream,
    enqueued when the batch's detections are handed out.  result is what detect_frames yields (on_device=True: the (dets,
    labels) device tensors and the annotated frame as a device u8 [H,W,3] tensor; False: the per-class list and an ndarray,
    a batch's annotated frames brought back in one copy).
    Host frames of a batch go up once, in one pinned copy, as device views: detect_frames(on_device=True) reads those views
    and the overlay is drawn into them, so nothing is uploaded twice and the caller's arrays stay as they are.  Device frames
    from the caller are copied by the same launch, or with inplace=True drawn on where they are (device tensors only).
    **style: draw_detections' keyword arguments (class_names -- default: the model's CLASSES --, score_thr, bbox_color,
    text_color, thickness, font_size, label_alpha, max_dets, atlas).  set_tta / set_tiling work unchanged underneath."""
    from collections import deque
    from ..ops.crops import check_frames, frame_table
    from .. import kernels as K
    from ..ops.draw import Painter, check_device_frames, pad_detections
    if batch_size < 1:
        raise ValueError(f"batch_size={batch_size}")
    unknown = set(style) - {"class_names", "score_thr", "bbox_color", "text_color", "thickness", "font_size", "label_alpha",
                            "max_dets", "atlas"}
    if unknown:
        raise TypeError(f"draw_frames: unknown style arguments {sorted(unknown)}")
    if "class_names" not in style and getattr(model, "CLASSES", None) is not None:
        style["class_names"] = [str(c) for c in model.CLASSES]
    dev = torch.device("cuda", torch.cuda.current_device())
    painter = Painter(dev, **style)
    num_classes = model.bbox_head.num_classes
    groups = deque()

    def staged():
        def stage(group):
            check_frames(group)
            if inplace:
                check_device_frames(group, "inplace=True")
            groups.append(_DrawGroup(group, dev, inplace))
            return groups[-1].sources
        group = []
        for f in frames:
            group.append(f)
            if len(group) == batch_size:
                yield from stage(group)
                group = []
        if group:
            yield from stage(group)

    stream = detect_frames(model, staged(), batch_size=batch_size, on_device=True)
    try:
        dets = []
        for res in stream:
            dets.append(res)
            g = groups[0]
            if len(dets) < len(g.sources):
                continue
            groups.popleft()
            B = len(dets)
            boxes, scores, labels, counts = pad_detections(dets, dev)
            table, keep = frame_table(g.sources + g.dests, dev)          # (device views only: the table is the upload)
            n = B * K.PREP_DESC_INTS
            painter.launch(table[:n], table[n:], B, max(int(f.shape[0]) for f in g.sources),
                           max(int(f.shape[1]) for f in g.sources), boxes, scores, labels, counts, False)
            del keep
            shown = g.dests if on_device else g.to_host()
            for (b, l), img in zip(dets, shown):
                yield ((b, l) if on_device else bbox2result(b, l, num_classes)), img
            dets = []
    finally:
        stream.close()


_TRACK_KEYS = ("iou_thr", "track_thr", "new_thr", "max_age", "max_tracks", "motion", "class_aware")


def track_frames(model, frames, batch_size=8, on_device=False, tracker=None, crops=None, **params):
    """Generator over an iterable of frames of ONE camera, as detect_frames: yields (result, ids) per frame, in order -- ids[i]
    is the track of the frame's i-th detection (0: none), the same number for the same object instance from frame to frame.
    When a batch's detections are handed out its frames go through `ops.Tracker.update` in ONE HIP launch on the caller's
    stream (include/radet_hip.h, radet_track_update: greedy IoU association in rank order against a constant-velocity
    prediction; this project's own rules, parity unpinned, the defaults not evaluated on any data).
    on_device=True: result is the (dets f32 [k,5], labels i64 [k]) device tensors and ids an i32 device view of length k;
    nothing is read back.  on_device=False: result is the per-class list of ndarray [k,5] and ids a list of one i32 ndarray
    per class, regrouped exactly as bbox2result regroups the boxes; the ids of a whole batch come back in one copy.
    tracker: an ops.Tracker of one sequence to continue (its numbering goes on across calls; tracker.tracks() reads the live
    tracks, coasting ones included); otherwise one is made from **params (ops.track.track_params: iou_thr, track_thr, new_thr,
    max_age, max_tracks, motion, class_aware).  crops=dict(size=..., ...) as for detect_frames: yields (result, ids, Crops of
    that frame); the track of crop j is ids[crops.index[:, 1]][j].  set_tta / set_tiling work unchanged underneath.
    Refused: a tracker of several sequences (one generator is one camera), a tracker together with **params, unknown
    keyword arguments (TypeError)."""
    from collections import deque
    from ..ops.draw import pad_detections
    from ..ops.track import Tracker
    if batch_size < 1:
        raise ValueError(f"batch_size={batch_size}")
    unknown = set(params) - set(_TRACK_KEYS)
    if unknown:
        raise TypeError(f"track_frames: unknown tracker arguments {sorted(unknown)}")
    if tracker is None:
        tracker = Tracker(**params)
    elif params:
        raise TypeError(f"track_frames: a tracker was passed in together with {sorted(params)}; its parameters are its own")
    elif not isinstance(tracker, Tracker) or tracker.sequences != 1:
        raise ValueError("track_frames: tracker= takes an ops.Tracker of one sequence (one generator is one camera)")
    num_classes = model.bbox_head.num_classes
    sizes = deque()

    def counted():
        n = 0
        for f in frames:
            n += 1
            if n == batch_size:                                      # (noted before the frame that completes its group is taken)
                sizes.append(n)
                n = 0
            yield f
        if n:
            sizes.append(n)

    stream = detect_frames(model, counted(), batch_size=batch_size, on_device=True, crops=crops)
    try:
        got = []
        for res in stream:
            got.append(res)
            if len(got) < sizes[0]:
                continue
            sizes.popleft()
            dets = got if crops is None else [r[0] for r in got]
            ids, _ = tracker.update(pad_detections(dets, tracker.dev))
            host = None if on_device else ids.cpu().numpy()          # (the batch's ids: one copy)
            for i, (b, l) in enumerate(dets):
                k = int(b.shape[0])
                if on_device:
                    out = ((b, l), ids[i, :k])
                else:
                    b, l = b.detach().cpu().numpy(), l.detach().cpu().numpy()
                    out = (bbox2result(b, l, num_classes), [host[i, :k][l == c] for c in range(num_classes)])
                yield out if crops is None else out + (got[i][1],)
            got = []
    finally:
        stream.close()


def show_result_pyplot(model, img, result, score_thr=0.3, fig_size=(15, 10), title="result", block=True, wait_time=0):
    """radet/apis/inference.py:163: the result drawn over img (model.show_result) and shown with matplotlib; `block` is
    ignored as in the reference"""
    if hasattr(model, "module"):
        model = model.module
    return model.show_result(img, result, score_thr=score_thr, show=True, wait_time=wait_time, fig_size=fig_size, win_name=title,
                             bbox_color=(72, 101, 241), text_color=(72, 101, 241))
