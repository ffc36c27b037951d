"""Test loops with the reference's names and return values (radet/apis/test.py: single_gpu_test, multi_gpu_test,
collect_results_cpu / collect_results_gpu).

The loops feed a test-mode `build_dataloader` to `DetectorRuntime.detect_stream`, so the host is one batch behind the device
(the reference's loop synchronises per batch).  Visualisation (`show`, `out_dir`) is out of scope.  No stream is
created here: detect_stream runs its post-processing on the engine's tower-chain stream (engine.py, "stream budget")."""
import os
import pickle
import shutil
import tempfile

import torch.distributed as dist

from ..core.bbox import bbox2result


def _test_batches(data_loader):
    """(img, img_metas) of the single test view of every batch"""
    for data in data_loader:
        imgs, metas = data["img"], data["img_metas"]
        if isinstance(imgs, (list, tuple)):
            if len(imgs) != 1:
                raise NotImplementedError("test-time augmentation is out of scope (flip=False in the BOP configs)")
            imgs, metas = imgs[0], metas[0]
        yield imgs, metas


def single_gpu_test(model, data_loader, show=False, out_dir=None, show_score_thr=0.3, *, on_device=False):
    """One entry per image of the loader's share, in dataset order: the per-class list of ndarray[k, 5] that `simple_test`
    returns (boxes in the original image's coordinates).  on_device=True returns `(results, raw)`, raw[i] = the image's
    (dets f32[k, 5], labels i64[k]) device tensors -- what DeviceCOCOeval and `dataset.evaluate(raw, device=...)` take."""
    if show or out_dir:
        raise NotImplementedError("visualisation of test results (show / out_dir) is out of scope")
    if model.training:
        model.eval()
    rt = model.runtime()
    num_classes = model.bbox_head.num_classes
    results, raw = [], []
    for dets in rt.detect_stream(_test_batches(data_loader), model.test_cfg, rescale=True):
        for boxes, labels in dets:
            results.append(bbox2result(boxes, labels, num_classes))
            if on_device:
                raw.append((boxes, labels))
    return (results, raw) if on_device else results


def _rank_world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def collect_results_gpu(part, size):
    """every rank's part through the process group (all_gather_object); rank 0 returns the parts joined in rank order and
    cut to `size`, the others None.  Shares are contiguous (loader.group_batches, shuffle=False), so joining is concatenation."""
    rank, world = _rank_world()
    if world == 1:
        return part[:size]
    parts = [None] * world
    dist.all_gather_object(parts, part)
    if rank != 0:
        return None
    return [r for p in parts for r in p][:size]


def collect_results_cpu(part, size, tmpdir=None):
    """the same through files part_<rank>.pkl in a directory all ranks can reach (`tmpdir`; None: a fresh temporary directory
    whose name rank 0 broadcasts).  The directory is removed by rank 0."""
    rank, world = _rank_world()
    if world == 1:
        return part[:size]
    if tmpdir is None:
        name = [tempfile.mkdtemp(prefix="radet_collect_") if rank == 0 else None]
        dist.broadcast_object_list(name, src=0)
        tmpdir = name[0]
    else:
        os.makedirs(tmpdir, exist_ok=True)
    with open(os.path.join(tmpdir, f"part_{rank}.pkl"), "wb") as f:
        pickle.dump(part, f)
    dist.barrier()
    if rank != 0:
        return None
    out = []
    for r in range(world):
        with open(os.path.join(tmpdir, f"part_{r}.pkl"), "rb") as f:
            out += pickle.load(f)
    shutil.rmtree(tmpdir)
    return out[:size]


def multi_gpu_test(model, data_loader, tmpdir=None, gpu_collect=False):
    """Every rank tests the share its loader gives it (build_dataloader(..., rank=, world=)); rank 0 returns the results of
    the whole dataset in dataset order, the other ranks None.  Works on any initialised process group (gloo included)."""
    part = single_gpu_test(model, data_loader)
    size = len(data_loader.dataset)
    if gpu_collect:
        return collect_results_gpu(part, size)
    return collect_results_cpu(part, size, tmpdir)
