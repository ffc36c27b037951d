"""init_detector / inference_detector with the reference's signatures (radet/apis/inference.py), for inputs that are
already normalised NCHW tensors, or for image files, which go through the config's test pipeline as in the reference."""
import numpy as np
import torch

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


def inference_detector(model, imgs, scale_factor=None):
    """imgs: f32[B,3,H,W] (normalised) -> list[B] of list[num_classes] of ndarray[k,5]; or a file name -> the result of that
    image; or a list of file names -> the list of their results (radet/apis/inference.py:86-140)."""
    if isinstance(imgs, str):
        return _inference_files(model, [imgs])[0]
    if isinstance(imgs, (list, tuple)) and all(isinstance(i, str) for i in imgs):
        return _inference_files(model, list(imgs))
    if imgs.dim() == 3:
        imgs = imgs[None]
    B, _, H, W = imgs.shape
    sf = np.ones(4, np.float32) if scale_factor is None else np.asarray(scale_factor, np.float32)
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=sf, flip=False) for _ in range(B)]
    with torch.no_grad():
        return model(img=[imgs], img_metas=[metas], return_loss=False, rescale=True)
