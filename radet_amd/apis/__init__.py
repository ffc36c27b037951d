from .train import (IterLR, OneCycleLR, build_lr_schedule, load_checkpoint, resolve_paramwise, save_checkpoint, train_detector,
                    wrap_fp16_model)
from .inference import (detect_frames, draw_frames, inference_detector, init_detector, set_tiling, set_tta,
                        show_result_pyplot, track_frames)
from .test import multi_gpu_test, single_gpu_test

__all__ = ["OneCycleLR", "IterLR", "build_lr_schedule", "resolve_paramwise", "train_detector", "wrap_fp16_model", "save_checkpoint",
           "load_checkpoint", "init_detector", "inference_detector", "detect_frames", "draw_frames", "track_frames", "show_result_pyplot", "set_tta", "set_tiling", "single_gpu_test", "multi_gpu_test"]
