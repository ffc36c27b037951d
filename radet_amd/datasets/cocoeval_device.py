"""COCO-protocol bounding-box evaluation on the device (csrc/cocoeval.hip), pinned bit for bit to the host evaluator of
radet_amd/datasets/cocoeval.py (whose own "parity with pycocotools unpinned" note therefore carries over).

DeviceCOCOeval has COCOeval's surface: `params`, evaluate(), accumulate(), summarize(), `eval` (precision / recall / scores
as NumPy fp64) and `stats`.  The detections are the detector's fp32 [x1, y1, x2, y2, score] rows, either the per-class NumPy
lists of `simple_test` or the per-image device tensors of `single_gpu_test(..., on_device=True)`; the second form never
leaves the device before the three tables come back.

What is torch plumbing here and what is kernel: grouping detections into (category, image) segments, the stable descending
score sorts (per segment for the matching, per category over all images for the tables) and the gathers that follow them
are torch ops on the device; IoU, the greedy matching, the tp / fp scans, the precision envelope and the recall-threshold
searches are the two kernels.  Ground truths are tabulated and uploaded once per (annotation index, id lists, useCats).

A segment with more ground truths than the kernel's LDS row holds (kernels.COCO_MAX_GT), or more (area range, threshold)
pairs than a wave has lanes, makes the whole evaluation run on the host evaluator instead; the logger says so once."""
import logging

import numpy as np
import torch

from .. import kernels as K
from .cocoeval import COCOeval, Params


def _is_device_results(results):
    return len(results) > 0 and isinstance(results[0], tuple) and torch.is_tensor(results[0][0])


def results_to_lists(results, num_classes):
    """per-image (dets, labels) device tensors -> the per-class NumPy lists of simple_test"""
    from ..core.bbox import bbox2result
    return [bbox2result(b, l, num_classes) for b, l in results]


class DeviceCOCOeval:
    def __init__(self, cocoGt, results, cat_ids, img_ids, device, logger=None):
        """cat_ids[label] / img_ids[index into results]: what BOPDataset._det2json writes into the records"""
        self.cocoGt, self.device, self.logger = cocoGt, torch.device(device), logger
        self.cat_ids, self.img_ids = list(cat_ids), list(img_ids)
        self.results = results[:len(self.img_ids)]
        if sum(self._count(r) for r in self.results) == 0:
            raise IndexError("empty results")                                     # (what COCO.loadRes raises)
        self.params = Params()
        self.params.imgIds = sorted(cocoGt.get_img_ids())
        self.params.catIds = sorted(cocoGt.get_cat_ids())
        self.eval, self.stats, self.host = {}, [], None

    @staticmethod
    def _count(r):
        return int(r[0].shape[0]) if isinstance(r, tuple) else sum(int(np.asarray(c).reshape(-1, 5).shape[0]) for c in r)

    # ------------------------------------------------------------------ host fallback
    def _records(self):
        lists = results_to_lists(self.results, len(self.cat_ids)) if _is_device_results(self.results) else self.results
        out = []
        for idx, per_class in enumerate(lists):
            for label, dets in enumerate(per_class):
                for det in np.asarray(dets).reshape(-1, 5):
                    x1, y1, x2, y2 = (float(v) for v in det[:4])
                    out.append(dict(image_id=self.img_ids[idx], category_id=self.cat_ids[label], bbox=[x1, y1, x2 - x1, y2 - y1],
                                    score=float(det[4])))
        return out

    def _fall_back(self, why):
        msg = f"DeviceCOCOeval: {why}; this evaluation runs on the host evaluator"
        if isinstance(self.logger, logging.Logger):
            self.logger.warning(msg)
        elif self.logger != "silent":
            print(msg)
        self.host = COCOeval(self.cocoGt, self.cocoGt.loadRes(self._records()), "bbox")
        self.host.params = self.params
        self.host.evaluate()

    # ------------------------------------------------------------------ tables
    def _gt_tables(self, p):
        """ground truths of the evaluated (category, image) grid in COCOeval._prepare's order; cached on the annotation index"""
        key = (int(p.useCats), tuple(p.catIds), tuple(p.imgIds), str(self.device))
        cache = self.cocoGt.__dict__.setdefault("_device_gt_tables", {})
        if key in cache:
            return cache[key]
        ipos = {v: i for i, v in enumerate(p.imgIds)}
        kpos = {v: i for i, v in enumerate(p.catIds)}
        n_img = len(p.imgIds)
        seg, box, area, flags, ids = [], [], [], [], []
        for g in self.cocoGt.dataset.get("annotations", []):
            if g["image_id"] not in ipos or (p.useCats and g["category_id"] not in kpos):
                continue
            seg.append((kpos[g["category_id"]] if p.useCats else 0) * n_img + ipos[g["image_id"]])
            box.append([float(v) for v in g["bbox"]])
            area.append(float(g["area"]))
            flags.append((1 if g.get("iscrowd", 0) else 0) | (2 if g["id"] == 0 else 0))
            ids.append(g["id"])
        seg = np.asarray(seg, np.int64)
        order = np.argsort(seg, kind="mergesort")
        nseg = len(p.catIds) * n_img
        counts = np.bincount(seg, minlength=nseg) if seg.size else np.zeros(nseg, np.int64)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        t = dict(nseg=nseg, n=int(seg.size), max_seg=int(counts.max()) if nseg else 0, off_host=off,
                 ids=np.asarray(ids, object)[order] if seg.size else np.zeros(0, object),
                 off=torch.from_numpy(off).to(self.device),
                 box=torch.from_numpy(np.asarray(box, np.float64).reshape(-1, 4)[order]).to(self.device),
                 area=torch.from_numpy(np.asarray(area, np.float64)[order]).to(self.device),
                 flags=torch.from_numpy(np.asarray(flags, np.uint8)[order]).to(self.device),
                 cat_off=torch.from_numpy(np.ascontiguousarray(off[::n_img] if n_img else off[:1])).to(self.device))
        if n_img == 0:
            t["cat_off"] = torch.zeros(len(p.catIds) + 1, dtype=torch.int32, device=self.device)
        cache.clear()                                                  # one entry: the tables of the last configuration
        cache[key] = t
        return t

    def _detections(self):
        """(rows f32[D,5], results index i64[D], label i64[D]) on the device, in the record order of BOPDataset._det2json
        (image, then label, then row)"""
        dev = self.device
        if _is_device_results(self.results):
            rows = torch.cat([b.to(dev, torch.float32).reshape(-1, 5) for b, _ in self.results])
            label = torch.cat([l.to(dev, torch.int64).reshape(-1) for _, l in self.results])
            n = torch.tensor([int(b.shape[0]) for b, _ in self.results], dtype=torch.int64)
            ridx = torch.repeat_interleave(torch.arange(len(self.results)), n).to(dev)
            order = torch.sort(ridx * len(self.cat_ids) + label, stable=True)[1]
            return rows[order].contiguous(), ridx[order], label[order]
        rows, ridx, label = [], [], []
        for idx, per_class in enumerate(self.results):
            for lb, dets in enumerate(per_class):
                d = np.asarray(dets, np.float32).reshape(-1, 5)
                rows.append(d)
                ridx.append(np.full(d.shape[0], idx, np.int64))
                label.append(np.full(d.shape[0], lb, np.int64))
        return (torch.from_numpy(np.concatenate(rows)).to(dev), torch.from_numpy(np.concatenate(ridx)).to(dev),
                torch.from_numpy(np.concatenate(label)).to(dev))

    # ------------------------------------------------------------------ COCOeval's three steps
    def evaluate(self):
        p, dev = self.params, self.device
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds)) if p.useCats else [-1]
        p.maxDets = sorted(p.maxDets)
        self.host = None
        gt = self._gt_tables(p)
        rows, ridx, label = self._detections()
        n_img = len(p.imgIds)
        ipos = {v: i for i, v in enumerate(p.imgIds)}
        imap = torch.tensor([ipos.get(v, -1) for v in self.img_ids[:len(self.results)]], dtype=torch.int64, device=dev)
        if p.useCats:
            kpos = {v: i for i, v in enumerate(p.catIds)}
            kmap = torch.tensor([kpos.get(v, -1) for v in self.cat_ids], dtype=torch.int64, device=dev)
            kidx = kmap[label]
        else:
            kidx = torch.zeros_like(label)
        iidx = imap[ridx]
        fid = torch.arange(1, rows.shape[0] + 1, device=dev)                    # COCO.loadRes: id = position in the file + 1
        keep = (iidx >= 0) & (kidx >= 0)
        rows, fid, seg = rows[keep], fid[keep], (kidx * n_img + iidx)[keep]
        # per segment: descending score, stable (equal scores keep the record order), cut to maxDets[-1]
        o = torch.sort(rows[:, 4], descending=True, stable=True)[1]
        o = o[torch.sort(seg[o], stable=True)[1]]
        rows, fid, seg = rows[o], fid[o], seg[o]
        counts = torch.bincount(seg, minlength=gt["nseg"])
        start = torch.cumsum(counts, 0) - counts
        rank = torch.arange(seg.numel(), device=dev) - start[seg]
        cut = rank < int(p.maxDets[-1])
        rows, fid, seg, rank = rows[cut], fid[cut], seg[cut], rank[cut]
        counts = torch.clamp(counts, max=int(p.maxDets[-1]))
        dt_off = torch.zeros(gt["nseg"] + 1, dtype=torch.int32, device=dev)
        dt_off[1:] = torch.cumsum(counts, 0)
        self._dt = dict(xyxy=rows[:, :4].contiguous(), score=rows[:, 4].contiguous(), fid=fid, seg=seg,
                        rank=rank.to(torch.int32), off=dt_off)
        try:
            self._match(gt, self._dt["xyxy"], dt_off)
        except K.CocoShapeError as e:
            return self._fall_back(str(e))

    def _match(self, gt, xyxy, dt_off):
        p, dev = self.params, self.device
        T, A = len(p.iouThrs), len(p.areaRng)
        thr = torch.tensor(np.asarray(p.iouThrs, np.float64), dtype=torch.float64, device=dev)
        rng = torch.tensor(np.asarray(p.areaRng, np.float64).reshape(-1, 2), dtype=torch.float64, device=dev)
        D, G = xyxy.shape[0], gt["n"]
        m = dict(dt_match=torch.empty((D, A * T), dtype=torch.int32, device=dev),
                 dt_flag=torch.empty((D, A * T), dtype=torch.uint8, device=dev),
                 gt_match=torch.full((G, A * T), -1, dtype=torch.int32, device=dev),
                 gt_ignore=torch.zeros((G, A), dtype=torch.uint8, device=dev))
        K.coco_match(xyxy, dt_off, gt["box"], gt["area"], gt["flags"], gt["off"], gt["nseg"], gt["max_seg"], thr, rng,
                     m["dt_match"], m["dt_flag"], m["gt_match"], m["gt_ignore"])
        self._gt, self._m = gt, m

    def accumulate(self):
        if self.host is not None:
            self.host.accumulate()
            self.eval = self.host.eval
            return
        p, dev, dt, m = self.params, self.device, self._dt, self._m
        T, R, Kc, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
        n_img = len(p.imgIds)
        cat = torch.div(dt["seg"], max(n_img, 1), rounding_mode="floor")
        # per category over all images (imgIds order, then rank): descending score, stable
        o = torch.sort(dt["score"], descending=True, stable=True)[1]
        o = o[torch.sort(cat[o], stable=True)[1]]
        cat_off = torch.zeros(Kc + 1, dtype=torch.int32, device=dev)
        cat_off[1:] = torch.cumsum(torch.bincount(cat, minlength=Kc), 0)
        precision = torch.full((T, R, Kc, A, M), -1.0, dtype=torch.float64, device=dev)
        scores = torch.full((T, R, Kc, A, M), -1.0, dtype=torch.float64, device=dev)
        recall = torch.full((T, Kc, A, M), -1.0, dtype=torch.float64, device=dev)
        K.coco_accumulate(m["dt_flag"][o].contiguous(), dt["rank"][o].contiguous(), dt["score"][o].contiguous(), cat_off,
                          m["gt_ignore"], self._gt["cat_off"], torch.tensor(p.maxDets, dtype=torch.int32, device=dev),
                          torch.tensor(np.asarray(p.recThrs, np.float64), dtype=torch.float64, device=dev), T, Kc, A,
                          precision, recall, scores)
        self.eval = dict(params=p, counts=[T, R, Kc, A, M], precision=precision.cpu().numpy(), recall=recall.cpu().numpy(),
                         scores=scores.cpu().numpy())

    _summarize = COCOeval._summarize
    summarize = COCOeval.summarize

    # ------------------------------------------------------------------ inspection
    @property
    def evalImgs(self):
        """the matching in COCOeval.evalImgs' form (same order, same dictionaries, annotation / record ids), downloaded
        and rebuilt on the host: for inspection and for the tests that hold the kernel to the host evaluator"""
        if self.host is not None:
            return self.host.evalImgs
        p, gt = self.params, self._gt
        T, A, n_img = len(p.iouThrs), len(p.areaRng), len(p.imgIds)
        dt_off, gt_off = self._dt["off"].cpu().numpy(), gt["off_host"]
        fid, score = self._dt["fid"].cpu().numpy(), self._dt["score"].cpu().numpy()
        dt_match, dt_flag = self._m["dt_match"].cpu().numpy(), self._m["dt_flag"].cpu().numpy()
        gt_match, gt_ignore = self._m["gt_match"].cpu().numpy(), self._m["gt_ignore"].cpu().numpy()
        out = []
        for k, cat in enumerate(p.catIds):
            for a, a_rng in enumerate(p.areaRng):
                for i, img in enumerate(p.imgIds):
                    s = k * n_img + i
                    g0, g1, d0, d1 = gt_off[s], gt_off[s + 1], dt_off[s], dt_off[s + 1]
                    if g0 == g1 and d0 == d1:
                        out.append(None)
                        continue
                    g_ig = gt_ignore[g0:g1, a].astype(int)
                    gtind = np.argsort(g_ig, kind="mergesort")
                    gids = np.asarray([float(v) for v in gt["ids"][g0:g1]], np.float64)
                    cols = slice(a * T, (a + 1) * T)
                    dm, gm = dt_match[d0:d1, cols].T, gt_match[g0:g1, cols].T[:, gtind]
                    dtm = np.where(dm >= 0, gids[np.maximum(dm, 0)] if g1 > g0 else 0.0, 0.0)
                    gtm = np.where(gm >= 0, fid[d0 + np.maximum(gm, 0)].astype(np.float64) if d1 > d0 else 0.0, 0.0)
                    out.append(dict(image_id=img, category_id=cat, aRng=a_rng, maxDet=p.maxDets[-1], dtIds=[int(v) for v in fid[d0:d1]],
                                    gtIds=[gt["ids"][g0 + j] for j in gtind], dtMatches=dtm.reshape(T, d1 - d0),
                                    gtMatches=gtm.reshape(T, g1 - g0), dtScores=[float(v) for v in score[d0:d1]],
                                    gtIgnore=g_ig[gtind], dtIgnore=((dt_flag[d0:d1, cols].T >> 1) & 1).astype(bool)))
        return out
