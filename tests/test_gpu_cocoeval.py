"""The device evaluator (csrc/cocoeval.hip, radet_amd/datasets/cocoeval_device.py) and the test / evaluation loops against
the unchanged host evaluator (radet_amd/datasets/cocoeval.py:COCOeval) on the same inputs: matching decisions equal,
precision / recall / scores equal bit for bit, the 12 statistics equal.

Figures: none recorded here; every comparison is exact equality (the kernels use IEEE fp64 + - * / and comparisons in the
host evaluator's operation order, compiled with -ffp-contract=off)."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CATS = (1, 2, 3, 4)                       # category 4 never has a ground truth
CONFIGS = {
    "default": dict(),
    "agnostic": dict(useCats=0),
    "custom": dict(maxDets=[3, 7, 50], iouThrs=np.array([0.3, 0.55, 0.8])),
}


def _xyxy32(b):
    """xywh doubles -> the detector's fp32 [x1, y1, x2, y2]"""
    return np.array([b[0], b[1], b[0] + b[2], b[1] + b[3]], np.float32)


def random_case(seed):
    """9 images x 4 categories: crowds, fp32 score ties within and across images, boxes of all four area ranges, image 4 without
    ground truth, image 7 without detections, category 4 without ground truth, 120 detections in (image 2, category 1),
    70 ground truths in (image 3, category 2).  Returns (annotation dict, per-class fp32 result lists, image ids)."""
    rng = np.random.RandomState(seed)
    images, anns = list(range(1, 10)), []
    results = []
    for img in images:
        per_class = []
        for c in CATS:
            n_gt = 0 if (img == 4 or c == 4) else (70 if (img, c) == (3, 2) else rng.randint(0, 5))
            mine = []
            for _ in range(n_gt):
                w, h = rng.choice([12, 40, 150]) * rng.uniform(0.8, 1.2), rng.choice([12, 40, 150]) * rng.uniform(0.8, 1.2)
                x, y = rng.uniform(0, 400), rng.uniform(0, 300)
                mine.append(dict(id=len(anns) + len(mine) + 1, image_id=img, category_id=c,
                                 bbox=[float(x), float(y), float(w), float(h)], area=float(w * h), iscrowd=int(rng.rand() < 0.15)))
            anns += mine
            n_dt = 0 if img == 7 else (120 if (img, c) == (2, 1) else (90 if (img, c) == (3, 2) else rng.randint(0, 14)))
            rows = []
            for _ in range(n_dt):
                if mine and rng.rand() < 0.6:                       # a jittered copy of a ground truth
                    g = mine[rng.randint(len(mine))]["bbox"]
                    b = [g[0] + rng.uniform(-8, 8), g[1] + rng.uniform(-8, 8), g[2] * rng.uniform(0.8, 1.2), g[3] * rng.uniform(0.8, 1.2)]
                else:
                    b = [rng.uniform(0, 400), rng.uniform(0, 300), rng.uniform(8, 160), rng.uniform(8, 160)]
                score = np.float32(rng.choice([0.3, 0.5, 0.9]) if rng.rand() < 0.3 else rng.rand())
                rows.append(np.concatenate([_xyxy32(b), [score]]).astype(np.float32))
            per_class.append(np.stack(rows).astype(np.float32) if rows else np.zeros((0, 5), np.float32))
        results.append(per_class)
    gt = dict(images=[dict(id=i, width=640, height=480, file_name=f"000000/rgb/{i:06d}.jpg") for i in images],
              categories=[dict(id=c, name=f"c{c}") for c in CATS], annotations=anns)
    return gt, results, images


def records(results, img_ids, cat_ids):
    """what BOPDataset._det2json writes for these results"""
    out = []
    for idx, per_class in enumerate(results):
        for label, dets in enumerate(per_class):
            for det in dets:
                x1, y1, x2, y2 = (float(v) for v in det[:4])
                out.append(dict(image_id=img_ids[idx], category_id=cat_ids[label], bbox=[x1, y1, x2 - x1, y2 - y1],
                                score=float(det[4])))
    return out


def run_both(gt_dict, results, img_ids, cat_ids, cfg, device_results=None):
    from radet_amd.datasets.cocoeval import COCO, COCOeval
    from radet_amd.datasets.cocoeval_device import DeviceCOCOeval
    gt = COCO(gt_dict)
    host = COCOeval(gt, gt.loadRes(records(results, img_ids, cat_ids)), "bbox")
    dev = DeviceCOCOeval(gt, results if device_results is None else device_results, cat_ids, img_ids, torch.device("cuda"),
                         logger="silent")
    for ev in (host, dev):
        ev.params.catIds, ev.params.imgIds = list(cat_ids), list(img_ids)
        for k, v in cfg.items():
            setattr(ev.params, k, v)
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
    return host, dev


def assert_same(host, dev):
    he, de = host.evalImgs, dev.evalImgs
    assert len(he) == len(de)
    matched = 0
    for h, d in zip(he, de):
        assert (h is None) == (d is None)
        if h is None:
            continue
        assert h["image_id"] == d["image_id"] and h["category_id"] == d["category_id"] and h["aRng"] == d["aRng"]
        assert list(h["dtIds"]) == list(d["dtIds"]) and list(h["gtIds"]) == list(d["gtIds"])
        assert h["dtScores"] == d["dtScores"]
        for key in ("dtMatches", "gtMatches", "dtIgnore", "gtIgnore"):      # ids are a bijection of the matched-gt index
            np.testing.assert_array_equal(np.asarray(h[key]), np.asarray(d[key]), err_msg=f"{key} {h['image_id']} {h['category_id']}")
        matched += int(np.count_nonzero(h["dtMatches"]))
    for key in ("precision", "recall", "scores"):
        a, b = host.eval[key], dev.eval[key]
        assert a.shape == b.shape and a.dtype == b.dtype == np.float64
        bad = np.flatnonzero(a.view(np.uint64).ravel() != b.view(np.uint64).ravel())
        assert bad.size == 0, (key, bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])
    assert host.eval["counts"] == dev.eval["counts"]
    np.testing.assert_array_equal(np.asarray(host.stats), np.asarray(dev.stats))
    assert len(dev.stats) == 12
    return matched


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("seed", range(8))
def test_device_cocoeval_random_vs_host(seed, cfg):
    gt, results, images = random_case(seed)
    areas = np.array([a["area"] for a in gt["annotations"]])
    assert (areas < 32 ** 2).any() and ((areas > 32 ** 2) & (areas < 96 ** 2)).any() and (areas > 96 ** 2).any()
    assert any(a["iscrowd"] for a in gt["annotations"])
    host, dev = run_both(gt, results, images, list(CATS), CONFIGS[cfg])
    assert dev.host is None                                        # the kernels ran, not the fallback
    assert assert_same(host, dev) > 50
    assert (host.eval["precision"] > -1).any() and (cfg == "agnostic" or (host.eval["precision"] == -1).any())


@pytest.mark.timeout(600)
def test_device_results_form_equals_list_form():
    """the (dets, labels) device tensors of single_gpu_test(on_device=True), labels interleaved as NMS leaves them"""
    gt, results, images = random_case(3)
    rng = np.random.RandomState(0)
    raw = []
    for per_class in results:
        rows = np.concatenate(per_class)
        labels = np.concatenate([np.full(len(c), k, np.int64) for k, c in enumerate(per_class)])
        # any interleaving of the classes that keeps every class's own row order
        pos = {k: iter(np.flatnonzero(labels == k)) for k in range(len(per_class))}
        mixed = [next(pos[k]) for k in labels[rng.permutation(len(rows))]] if len(rows) else []
        mixed = np.asarray(mixed, np.int64)
        raw.append((torch.from_numpy(rows[mixed].reshape(-1, 5)).cuda(), torch.from_numpy(labels[mixed]).cuda()))
    for cfg in ("default", "agnostic"):
        host, dev = run_both(gt, results, images, list(CATS), CONFIGS[cfg], device_results=raw)
        assert dev.host is None
        assert_same(host, dev)


@pytest.mark.timeout(300)
def test_exact_ties_on_an_integer_grid():
    """IoU exactly 0.5 and exactly 0.75 against thresholds 0.5 and 0.75 (equality matches), two ground truths with the same
    IoU (the host's `if ious < iou: continue` lets the later one take it), a zero-width detection next to a ground truth of positive area (IoU 0, not NaN)."""
    box = [0.0, 0.0, 10.0, 10.0]
    anns = [dict(id=1, image_id=1, category_id=1, bbox=box, area=100.0, iscrowd=0),
            dict(id=2, image_id=2, category_id=1, bbox=box, area=100.0, iscrowd=0),
            dict(id=3, image_id=3, category_id=1, bbox=box, area=100.0, iscrowd=0),
            dict(id=4, image_id=3, category_id=1, bbox=box, area=100.0, iscrowd=0),
            dict(id=5, image_id=4, category_id=1, bbox=box, area=100.0, iscrowd=0)]
    dets = {1: [[0, 0, 10, 5, 0.9]],                         # inter 50 / union 100
            2: [[0, 0, 10, 7.5, 0.9]],                       # inter 75 / union 100
            3: [[0, 0, 10, 10, 0.9], [0, 0, 10, 10, 0.9]],   # both gts at IoU 1
            4: [[5, 5, 5, 15, 0.9], [0, 0, 10, 10, 0.5]]}    # w = 0
    images = [1, 2, 3, 4]
    gt = dict(images=[dict(id=i, width=64, height=64, file_name=f"000000/rgb/{i:06d}.jpg") for i in images],
              categories=[dict(id=1, name="c1")], annotations=anns)
    results = [[np.asarray(dets[i], np.float32).reshape(-1, 5)] for i in images]
    host, dev = run_both(gt, results, images, [1], dict(iouThrs=np.array([0.5, 0.75])))
    assert dev.host is None
    assert_same(host, dev)
    by_img = {e["image_id"]: e for e in dev.evalImgs[:4]}     # area range "all"
    assert by_img[1]["dtMatches"].ravel().tolist() == [1.0, 0.0]          # 0.5 matches at 0.5, not at 0.75
    assert by_img[2]["dtMatches"].ravel().tolist() == [2.0, 2.0]          # 0.75 matches at both
    assert by_img[3]["dtMatches"].tolist() == [[4.0, 3.0], [4.0, 3.0]]   # `ious < iou: continue`: the later gt takes an equal IoU
    assert by_img[4]["dtMatches"].tolist() == [[0.0, 5.0], [0.0, 5.0]]


def _write_dataset(tmp_path, n_gt_in_first, n_images=3):
    from tools.synth_bop import YCBV_NAMES
    rng = np.random.RandomState(5)
    images = [dict(id=i + 1, file_name=f"000000/rgb/{i:06d}.jpg", width=640, height=480) for i in range(n_images)]
    anns = []
    for i in range(n_images):
        for _ in range(n_gt_in_first if i == 0 else 3):
            x, y, w, h = rng.uniform(0, 400), rng.uniform(0, 300), rng.uniform(10, 150), rng.uniform(10, 150)
            anns.append(dict(id=len(anns) + 1, image_id=i + 1, category_id=1 if i == 0 else int(rng.randint(1, 4)),
                             bbox=[float(x), float(y), float(w), float(h)], area=float(w * h), iscrowd=0, ignore=False, visib_fract=1.0))
    path = os.path.join(str(tmp_path), "ann.json")
    with open(path, "w") as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=i + 1, name=n) for i, n in enumerate(YCBV_NAMES)]), f)
    results = []
    for i in range(n_images):
        per_class = [np.zeros((0, 5), np.float32) for _ in YCBV_NAMES]
        mine = [a for a in anns if a["image_id"] == i + 1][:4]
        for a in mine:
            b = a["bbox"]
            row = np.concatenate([_xyxy32([b[0] + 2, b[1] - 1, b[2], b[3] * 0.9]), [np.float32(rng.rand())]]).astype(np.float32)
            k = a["category_id"] - 1
            per_class[k] = np.concatenate([per_class[k], row[None]])
        results.append(per_class)
    return path, results


@pytest.mark.timeout(600)
def test_oversize_segment_is_refused_and_falls_back(tmp_path):
    """A segment with more ground truths than the LDS row holds: radet_coco_match returns its error code before anything is
    launched (its outputs keep their fill), and the evaluation runs on the host evaluator with the same dict.  An argument
    check, not a fault."""
    from radet_amd import kernels as K
    from radet_amd.datasets import BOPDataset
    dev = torch.device("cuda")
    n = K.COCO_MAX_GT + 1
    hdr = open(os.path.join(REPO, "include", "radet_hip.h")).read()
    assert f"#define RADET_COCO_MAX_GT {K.COCO_MAX_GT}" in hdr and f"#define RADET_ERR_COCO_OVERSIZE {K.COCO_ERR_OVERSIZE}" in hdr
    T, A, D = 10, 4, 6
    out = dict(dt_match=torch.full((D, A * T), 77, dtype=torch.int32, device=dev),
               dt_flag=torch.full((D, A * T), 77, dtype=torch.uint8, device=dev),
               gt_match=torch.full((n, A * T), 77, dtype=torch.int32, device=dev),
               gt_ignore=torch.full((n, A), 77, dtype=torch.uint8, device=dev))
    with pytest.raises(K.CocoShapeError):
        K.coco_match(torch.zeros((D, 4), device=dev), torch.tensor([0, D], dtype=torch.int32, device=dev),
                     torch.ones((n, 4), dtype=torch.float64, device=dev), torch.ones(n, dtype=torch.float64, device=dev),
                     torch.zeros(n, dtype=torch.uint8, device=dev), torch.tensor([0, n], dtype=torch.int32, device=dev), 1, n,
                     torch.linspace(0.5, 0.95, T, dtype=torch.float64, device=dev),
                     torch.tensor([[0, 1e10]] * A, dtype=torch.float64, device=dev), **out)
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in out.values())
    path, results = _write_dataset(tmp_path, n)
    ds = BOPDataset(path, pipeline=[], test_mode=True)
    said = []
    import logging
    logger = logging.getLogger("radet_test_oversize")
    logger.setLevel(logging.INFO)
    handler = logging.Handler()
    handler.emit = lambda rec: said.append(rec.getMessage())
    logger.addHandler(handler)
    a = ds.evaluate(results, metric="bbox", logger=logger, device=dev)
    assert sum("host evaluator" in s for s in said) == 1
    b = ds.evaluate(results, metric="bbox", logger="silent")
    assert a == b and a["bbox_mAP"] >= 0
    # at the cap itself the kernel runs
    path, results = _write_dataset(tmp_path, K.COCO_MAX_GT)
    ds = BOPDataset(path, pipeline=[], test_mode=True)
    said.clear()
    a = ds.evaluate(results, metric=["bbox", "proposal"], logger=logger, device=dev)
    assert not any("host evaluator" in s for s in said)
    assert a == ds.evaluate(results, metric=["bbox", "proposal"], logger="silent")


# ------------------------------------------------------------------------------------------ end to end on a synthetic BOP tree
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL", reason="PIL decodes the generated JPEG files")
    from tools.synth_bop import write_tree
    return write_tree(str(tmp_path_factory.mktemp("bop")), n_frames=7, objects=(3, 6), n_backgrounds=1, seed=17)


def _datasets(tree):
    from radet_amd.datasets import build_dataset
    from tools.synth_bop import pipelines
    train, test = pipelines(tree["background_dir"])
    common = dict(type="BOPDataset", ann_file=tree["ann_file"], img_prefix=tree["img_prefix"], seg_prefix=tree["seg_prefix"])
    return build_dataset(dict(common, pipeline=train)), build_dataset(dict(common, pipeline=test, test_mode=True))


def _detector(seed=0):
    from radet_amd.models import build_detector
    from radet_amd.utils import Config
    from radet_amd.utils.synth_init import synth_fill
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", "r50_ycbv_pbr.py"))
    cfg.model["pretrained"] = None
    torch.manual_seed(seed)
    det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda()
    synth_fill(det, seed=0)
    return cfg, det


def _same_results(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert len(ra) == len(rb)
        for ca, cb in zip(ra, rb):
            np.testing.assert_array_equal(ca, cb)


@pytest.mark.timeout(900)
def test_single_gpu_test_and_device_evaluate(tree, tmp_path):
    from radet_amd.apis import single_gpu_test
    from radet_amd.core.bbox import bbox2result
    from radet_amd.datasets import BOPDataset, build_dataloader
    _, det = _detector()
    det.eval()
    _, ds = _datasets(tree)
    loader = build_dataloader(ds, samples_per_gpu=2, workers=2, seed=0, shuffle=False)
    ref = []
    with torch.no_grad():
        for batch in loader:
            ref += det(img=batch["img"], img_metas=batch["img_metas"], return_loss=False, rescale=True)
    results = single_gpu_test(det, loader)
    assert len(results) == len(ds) == 7
    _same_results(results, ref)
    results2, raw = single_gpu_test(det, loader, on_device=True)
    _same_results(results2, ref)
    assert all(b.is_cuda and b.dtype == torch.float32 and l.dtype == torch.int64 for b, l in raw)
    _same_results([bbox2result(b, l, 21) for b, l in raw], ref)
    n_det = sum(len(c) for r in results for c in r)
    print("detections:", n_det)
    assert n_det > 0
    with pytest.raises(NotImplementedError):
        single_gpu_test(det, loader, show=True)
    dev = torch.device("cuda")
    for classwise in (False, True):
        host = ds.evaluate(results, metric=["bbox", "proposal"], classwise=classwise, logger="silent")
        assert host and ds.evaluate(results, metric=["bbox", "proposal"], classwise=classwise, logger="silent", device=dev) == host
        assert ds.evaluate(raw, metric=["bbox", "proposal"], classwise=classwise, logger="silent", device=dev) == host
    # a JSON file only when a prefix is given; the same records as the host path writes
    prefix = os.path.join(str(tmp_path), "dev")
    ds.evaluate(raw, metric="bbox", logger="silent", device=dev, jsonfile_prefix=prefix)
    assert json.load(open(prefix + ".bbox.json")) == ds._det2json(results)
    # --format-only with bop_submission=True: the records _bop_det2json writes
    sub = BOPDataset(tree["ann_file"], pipeline=[], test_mode=True, bop_submission=True, img_prefix=tree["img_prefix"])
    files, scratch = sub.format_results(results, jsonfile_prefix=os.path.join(str(tmp_path), "submission"))
    assert scratch is None and json.load(open(files["bbox"])) == sub._bop_det2json(results)
    # inference_detector on file names: the same pipeline, one image per pass
    from radet_amd.apis import inference_detector
    from radet_amd.utils import Config
    det.cfg = Config(dict(data=dict(test=dict(pipeline=ds.pipeline.cfg))))
    names = [os.path.join(ds.img_prefix, ds.data_infos[i]["filename"]) for i in (0, 3)]
    one = inference_detector(det, names[0])
    both = inference_detector(det, names)
    _same_results([one], [both[0]])
    assert len(both) == 2 and sum(len(c) for c in both[1]) == sum(len(c) for c in results[3])


@pytest.mark.timeout(900)
def test_evaluation_does_not_move_the_training_trajectory(tree):
    """6 iterations from the loader with evaluation.interval = 3 and a val_loader against the same run without one: logged
    losses, all parameters and the AdamW moments bit-identical; two evaluations logged."""
    from radet_amd.apis import train_detector
    from radet_amd.datasets import build_dataloader
    train_ds, test_ds = _datasets(tree)

    def run(with_eval):
        cfg, det = _detector()
        cfg.merge_from_dict({"lr_config.total_steps": 40, "log_config.interval": 1, "evaluation.interval": 3})
        loader = build_dataloader(train_ds, samples_per_gpu=4, workers=4, seed=0)
        val = build_dataloader(test_ds, samples_per_gpu=2, workers=2, seed=0, shuffle=False) if with_eval else None

        def batches():
            epoch = 0
            while True:
                loader.set_epoch(epoch)
                yield from loader
                epoch += 1
        eval_log, lines = [], []
        hist = train_detector(det, batches(), cfg, max_iters=6, log=lines.append, val_loader=val, eval_log=eval_log)
        rt = det.runtime()
        torch.cuda.synchronize()
        state = {k: v.detach().cpu().clone() for k, v in det.state_dict().items()}
        return hist, state, rt.opt_state["m"].cpu().clone(), rt.opt_state["v"].cpu().clone(), eval_log, lines, det.training

    h0, s0, m0, v0, log0, _, _ = run(False)
    h1, s1, m1, v1, log1, lines, training = run(True)
    assert log0 == [] and [it for it, _ in log1] == [3, 6] and training
    assert all("bbox_mAP" in d and "bbox_mAP_50" in d for _, d in log1)
    assert sum("Iter(val)" in ln and "bbox_mAP:" in ln for ln in lines) == 2
    assert len(h0) == len(h1) == 6 and h0 == h1
    assert s0.keys() == s1.keys() and all(torch.equal(s0[k], s1[k]) for k in s0)
    assert torch.equal(m0, m1) and torch.equal(v0, v1)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, tree, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), GPU_MAX_HW_QUEUES="8")
    sys.path.insert(0, REPO)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from radet_amd.apis import multi_gpu_test
    from radet_amd.datasets import build_dataloader
    _, det = _detector()
    det.eval()
    _, ds = _datasets(tree)
    loader = build_dataloader(ds, samples_per_gpu=2, workers=2, seed=0, rank=rank, world=world, shuffle=False)
    for mode, kw in (("gpu", dict(gpu_collect=True)), ("cpu", dict(tmpdir=os.path.join(out_dir, "collect")))):
        res = multi_gpu_test(det, loader, **kw)
        assert (res is None) == (rank != 0)
        if rank == 0:
            torch.save(res, os.path.join(out_dir, f"results_{mode}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_multi_gpu_test_two_ranks_on_one_gpu(tree, tmp_path):
    import torch.multiprocessing as mp
    from radet_amd.apis import single_gpu_test
    from radet_amd.datasets import build_dataloader
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, tree, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(800)
        assert p.exitcode == 0
    _, det = _detector()
    _, ds = _datasets(tree)
    ref = single_gpu_test(det.eval(), build_dataloader(ds, samples_per_gpu=2, workers=2, seed=0, shuffle=False))
    for mode in ("gpu", "cpu"):
        _same_results(torch.load(os.path.join(str(tmp_path), f"results_{mode}.pt"), weights_only=False), ref)
