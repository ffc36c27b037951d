"""CPU side of the test / evaluation loops: the public names, result collection of multi_gpu_test over gloo ranks with uneven
shares, and the command line of tools/test.py.  No kernel is launched here."""
import inspect
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IMAGES, N_CLASSES = 7, 3


def test_public_names():
    from radet_amd.apis import multi_gpu_test, single_gpu_test
    from radet_amd.datasets import BOPDataset
    assert callable(single_gpu_test) and callable(multi_gpu_test)
    sig = inspect.signature(BOPDataset.evaluate)
    assert sig.parameters["device"].default is None
    assert inspect.signature(single_gpu_test).parameters["on_device"].kind is inspect.Parameter.KEYWORD_ONLY
    tr = inspect.signature(__import__("radet_amd.apis", fromlist=["train_detector"]).train_detector)
    assert tr.parameters["val_loader"].default is None and tr.parameters["eval_log"].default is None


def test_wrapped_datasets_still_refuse_evaluation():
    from radet_amd.datasets import ConcatDataset, RepeatDataset
    for cls in (ConcatDataset, RepeatDataset):
        assert "device" not in inspect.signature(cls.evaluate).parameters


def test_kernel_cap_matches_the_header():
    from radet_amd import kernels as K
    hdr = open(os.path.join(REPO, "include", "radet_hip.h")).read()
    assert f"#define RADET_COCO_MAX_GT {K.COCO_MAX_GT}\n" in hdr
    assert f"#define RADET_ERR_COCO_OVERSIZE {K.COCO_ERR_OVERSIZE}\n" in hdr


# ---------------------------------------------------------------------------------------------- collection over gloo ranks
def _dets_of(idx):
    """what the stub detector finds in image idx: idx % 4 boxes whose numbers name the image"""
    k = idx % 4
    boxes = torch.tensor([[idx, j, idx + 10.0 + j, j + 20.0, 0.9 - 0.1 * j] for j in range(k)], dtype=torch.float32).reshape(-1, 5)
    return boxes, torch.tensor([(idx + j) % N_CLASSES for j in range(k)], dtype=torch.int64)


class _StubRuntime:
    def detect_stream(self, batches, test_cfg, rescale=False):
        assert rescale
        for img, metas in batches:
            yield [_dets_of(m["idx"]) for m in metas]


class _StubModel:
    training = False
    test_cfg = dict()

    class bbox_head:
        num_classes = N_CLASSES

    def runtime(self):
        return _StubRuntime()


class _StubLoader:
    """the test-mode loader's surface: `dataset`, batches of dict(img=[tensor], img_metas=[[...]]), contiguous shares"""

    def __init__(self, rank, world, samples_per_gpu=2):
        from radet_amd.datasets.loader import group_batches
        self.dataset = list(range(N_IMAGES))
        self.batches = group_batches(np.zeros(N_IMAGES, np.uint8), samples_per_gpu, 0, 0, rank, world, shuffle=False)

    def __iter__(self):
        for b in self.batches:
            yield dict(img=[torch.zeros(len(b), 3, 8, 8)], img_metas=[[dict(idx=i) for i in b]])


def _expected():
    from radet_amd.core.bbox import bbox2result
    return [bbox2result(*_dets_of(i), N_CLASSES) for i in range(N_IMAGES)]


def _collect_worker(rank, world, port, q, tmpdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from radet_amd.apis import multi_gpu_test
    out = []
    for kw in (dict(gpu_collect=True), dict(), dict(tmpdir=os.path.join(tmpdir, "parts"))):
        res = multi_gpu_test(_StubModel(), _StubLoader(rank, world), **kw)
        if rank == 0:
            want = _expected()
            ok = len(res) == N_IMAGES and all(len(a) == N_CLASSES and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))
                                              for a, b in zip(res, want))
        else:
            ok = res is None
        out.append(bool(ok))
    q.put((rank, out, len(_StubLoader(rank, world).batches)))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3], ids=["2ranks", "3ranks"])
def test_multi_gpu_test_collects_uneven_shares(tmp_path, world):
    """7 images over 2 ranks (4 + 3) and 3 ranks (3 + 3 + 1): rank 0 gets the 7 entries in dataset order, the others None --
    through all_gather_object, through a broadcast temporary directory and through a given tmpdir."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_collect_worker, args=(r, world, port, q, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert [r[0] for r in res] == list(range(world)) and all(all(r[1]) for r in res), res
    assert len({r[2] for r in res}) > 1 or world == 2                  # the shares differ in batch count at 3 ranks


def test_single_process_collection_and_refusals():
    from radet_amd.apis import multi_gpu_test, single_gpu_test
    res = multi_gpu_test(_StubModel(), _StubLoader(0, 1))
    assert all(np.array_equal(x, y) for a, b in zip(res, _expected()) for x, y in zip(a, b)) and len(res) == N_IMAGES
    lists, raw = single_gpu_test(_StubModel(), _StubLoader(0, 1), on_device=True)
    assert len(raw) == N_IMAGES and torch.equal(raw[3][0], _dets_of(3)[0]) and torch.equal(raw[3][1], _dets_of(3)[1])
    for kw in (dict(show=True), dict(out_dir="x")):
        with pytest.raises(NotImplementedError):
            single_gpu_test(_StubModel(), _StubLoader(0, 1), **kw)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---------------------------------------------------------------------------------------------- tools/test.py
def _tool(*argv):
    return subprocess.run([sys.executable, os.path.join(REPO, "tools", "test.py"), *argv], capture_output=True, text=True,
                          timeout=240, cwd=REPO)


@pytest.mark.timeout(300)
def test_tools_test_command_line():
    r = _tool("--help")
    assert r.returncode == 0
    for opt in ("--out", "--eval", "--format-only", "--eval-options", "--cfg-options", "--launcher", "--host-eval"):
        assert opt in r.stdout, opt
    assert "--show" not in r.stdout and "--fuse-conv-bn" not in r.stdout
    r = _tool("cfg.py", "ckpt.pth", "--eval", "mAP")
    assert r.returncode == 2 and "metric mAP is not supported" in r.stderr
    r = _tool("cfg.py", "ckpt.pth", "--eval", "segm")
    assert r.returncode == 2 and "segm" in r.stderr
    r = _tool("cfg.py", "ckpt.pth")
    assert r.returncode == 2 and "at least one" in r.stderr
    r = _tool("cfg.py", "ckpt.pth", "--eval", "bbox", "--format-only")
    assert r.returncode == 2
