"""The reference's visualisation names (radet/core/visualization/image.py) on top of the HIP overlay kernel
(radet_amd/ops/draw.py).  The reference renders through matplotlib; here the boxes and labels are drawn by
radet_draw_detections with this project's own pixel rules (parity unpinned) and files are written with Pillow."""
import os

import numpy as np

from ..ops.draw import color_val


def color_val_matplotlib(color):
    """a colour (one of mmcv's eight names, or three ints BGR) as matplotlib's RGB floats in [0, 1] (image.py:11-23)"""
    return tuple(c / 255 for c in color_val(color)[::-1])


def imread_bgr(img):
    """a file name -> its BGR uint8 pixels; an array is taken as it is"""
    if isinstance(img, (str, bytes)) or hasattr(img, "__fspath__"):
        from ..datasets.loading import decode_bgr
        return decode_bgr(img)
    return np.asarray(img)


def imwrite_bgr(img, out_file):
    from PIL import Image
    d = os.path.dirname(os.path.abspath(out_file))
    os.makedirs(d, exist_ok=True)
    Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(out_file)


def imshow_det_bboxes(img, bboxes, labels, segms=None, class_names=None, score_thr=0, bbox_color="green", text_color="green",
                      mask_color=None, thickness=2, font_scale=0.5, font_size=13, win_name="", fig_size=(15, 10), show=True,
                      wait_time=0, out_file=None):
    """radet.core.visualization.imshow_det_bboxes (image.py:26): bboxes ndarray [n,5] (with scores), labels [n] drawn on img
    (a file name or a BGR ndarray) by the GPU; returns the BGR ndarray and writes out_file (Pillow).  Differences, all
    stated: the filter is score > score_thr for every score_thr (the reference skips it at 0), at most 256 boxes are drawn,
    segms / mask_color are refused (the detector has no masks), bboxes [n,4] are refused (the label shows the score),
    font_scale is ignored as in the reference, and the pixels follow include/radet_hip.h, not matplotlib.  show=True shows
    the finished image with matplotlib (imported only then)."""
    if segms is not None or mask_color is not None:
        raise NotImplementedError("imshow_det_bboxes: segms / mask_color -- the detector has no masks")
    bboxes, labels = np.asarray(bboxes), np.asarray(labels)
    if bboxes.ndim != 2 or labels.ndim != 1 or bboxes.shape[0] != labels.shape[0] or bboxes.shape[1] != 5:
        raise ValueError(f"imshow_det_bboxes: bboxes {bboxes.shape} (expected [n, 5]) with labels {labels.shape} (expected [n])")
    from ..ops.draw import draw_detections
    frame = np.ascontiguousarray(imread_bgr(img))
    out = draw_detections([frame], [(bboxes.astype(np.float32), labels.astype(np.int64))], class_names=class_names,
                          score_thr=score_thr, bbox_color=bbox_color, text_color=text_color, thickness=thickness,
                          font_size=font_size)[0].cpu().numpy()
    if out_file is not None:
        imwrite_bgr(out, out_file)
    if show:
        import matplotlib.pyplot as plt
        plt.figure(win_name, figsize=fig_size)
        plt.title(win_name)
        plt.axis("off")
        plt.imshow(out[..., ::-1])
        if wait_time == 0:
            plt.show()
        else:
            plt.show(block=False)
            plt.pause(wait_time)
    return out


def result_to_dets(result):
    """the per-class result list -> (bboxes [n,5], labels [n]) as BaseDetector.show_result stacks them (base.py:318-329)"""
    if isinstance(result, tuple):
        if len(result) > 1 and result[1] is not None:
            raise NotImplementedError("show_result: segmentation results -- the detector has no masks")
        result = result[0]
    bboxes = np.vstack([np.asarray(b, np.float32).reshape(-1, 5) for b in result]) if len(result) else np.zeros((0, 5), np.float32)
    labels = np.concatenate([np.full(np.asarray(b).reshape(-1, 5).shape[0], i, np.int32) for i, b in enumerate(result)]) \
        if len(result) else np.zeros(0, np.int32)
    return bboxes, labels
