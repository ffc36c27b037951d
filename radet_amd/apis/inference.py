"""init_detector / inference_detector with the reference's signatures (radet/apis/inference.py), for inputs that are
already normalised NCHW tensors, for image files, and for frames in memory (ndarray or device tensor HxWx3 uint8 BGR), which
go through the config's test pipeline as in the reference; detect_frames streams an iterable of frames through it."""
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


def _frame_pipeline(model):
    """model.cfg.data.test.pipeline with its first stage replaced by LoadImageFromWebcam (radet/apis/inference.py:97-102), built
    once per model and test pipeline"""
    from ..datasets.loading import ImagePipeline
    cfg = getattr(model, "cfg", None)
    if cfg is None:
        raise ValueError("inference on frames needs model.cfg (init_detector sets it)")
    stages = list(cfg.data.test.pipeline)
    key = repr(stages)
    cached = getattr(model, "_frame_pipeline", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    first = {k: v for k, v in dict(stages[0]).items() if k not in _FILE_LOADER_ARGS}
    first["type"] = "LoadImageFromWebcam"
    pipeline = ImagePipeline([first] + stages[1:])
    object.__setattr__(model, "_frame_pipeline", (key, pipeline))
    return pipeline


def _prepare_frames(pipeline, frames):
    """one batch of frames, of any sizes, through the pipeline: the collated test batch (one upload, one launch)"""
    import random
    planned = [pipeline.plan(dict(img=f, bbox_fields=[], mask_fields=[], seg_fields=[]), random, np.random) for f in frames]
    return pipeline.run(planned, collate=True)


def _inference_frames(model, frames):
    if not frames:
        return []
    with torch.no_grad():
        return model(return_loss=False, rescale=True, **_prepare_frames(_frame_pipeline(model), frames))


def detect_frames(model, frames, batch_size=8, on_device=False):
    """Generator over an iterable of frames (ndarray or device tensor HxWx3 uint8 BGR, sizes may differ): batches of
    `batch_size` frames (the last one smaller) go through the frame pipeline and `DetectorRuntime.detect_stream`, so the host
    is one batch behind the device.  Yields one result per frame, in order: the per-class list of ndarray[k, 5] (boxes in the
    frame's own coordinates), or with on_device=True the (dets f32[k, 5], labels i64[k]) device tensors.  Leaving the loop
    early closes the stream underneath, which leaves the runtime ready for the next call."""
    if batch_size < 1:
        raise ValueError(f"batch_size={batch_size}")
    pipeline = _frame_pipeline(model)
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
            data = _prepare_frames(pipeline, group)
            imgs, metas = data["img"], data["img_metas"]
            if isinstance(imgs, (list, tuple)):              # (a MultiScaleFlipAug pipeline: the single test view)
                imgs, metas = imgs[0], metas[0]
            yield imgs, metas

    stream = model.runtime().detect_stream(prepared(), model.test_cfg, rescale=True)
    try:
        for dets in stream:
            for boxes, labels in dets:
                yield (boxes, labels) if on_device else bbox2result(boxes, labels, num_classes)
    finally:
        stream.close()


def inference_detector(model, imgs, scale_factor=None):
    """imgs: f32[B,3,H,W] (normalised) -> list[B] of list[num_classes] of ndarray[k,5]; or a file name -> the result of that
    image; or a list of file names -> the list of their results; or a loaded image (ndarray, or uint8 device tensor, HxWx3
    BGR) -> its result; or a list of those, of any sizes -> the list of their results, computed as one batch
    (radet/apis/inference.py:86-140)."""
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
