"""radet.ops-compatible entry points (radet/ops/__init__.py:1-11 of the reference), executed by the
HIP NMS kernels (radet_amd/csrc/decode_nms.hip, soft_nms.hip).  Inputs may be CPU / GPU tensors or ndarrays; results come
back on the input's device, same shapes / dtypes / ordering as the reference's C++ ops."""
import functools

import numpy as np
import torch

from .. import kernels as K

__all__ = ["vote_nms", "global_vote_nms", "cluster_nms", "batched_nms", "soft_nms", "MBD_box2distance", "GDT_box2distance", "MBD", "GDT",
           "mbd_batch", "gdt_batch", "border_seeds", "resize_batch", "gaussian_blur9_batch", "sobel_edge_batch", "crop_detections",
           "Crops", "merge_view_candidates", "plan_tiles", "merge_tile_candidates", "draw_detections", "build_atlas",
           "adjust_brightness", "adjust_contrast", "adjust_color", "imequalize", "Tracker", "track_detections"]

_MAX = 65536      # 16-bit positions in the kernel's sort keys (above 8192 the sorts run in global memory)


def _dev():
    if not torch.cuda.is_available():
        from .._lib import RadetHipError
        raise RadetHipError("radet_amd.ops need an MI355X (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _t(x, dtype):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    return x.to(_dev(), dtype).contiguous()


def _run(mode, boxes, cscore, vscore, labels, thr, iou_enable=False, sigma=0.025, max_out=0):
    n = int(boxes.shape[0])
    if n > _MAX:
        raise ValueError(f"NMS input of {n} boxes exceeds the kernel's capacity ({_MAX})")
    dev = _dev()
    cap = max(n, 1)
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    k = max_out if max_out > 0 else cap
    ob = torch.zeros(1, k, 4, device=dev)
    osc = torch.zeros(1, k, device=dev)
    ol = torch.zeros(1, k, dtype=torch.long, device=dev)
    oc = torch.zeros(1, dtype=torch.int32, device=dev)
    a0 = torch.zeros(1, cap, dtype=torch.long, device=dev)
    a1 = torch.zeros(1, cap, dtype=torch.long, device=dev)
    ws = torch.empty(K.nms_ws_bytes(1, cap), dtype=torch.uint8, device=dev)
    if n == 0:
        return ob[0, :0], osc[0, :0], ol[0, :0], a0[0, :0], a1[0, :0]
    K.nms(boxes, cscore, vscore, labels, cnt, 1, cap, mode, float(thr), bool(iou_enable), float(sigma), int(max_out), ob,
          osc, ol, oc, a0, a1, ws)
    kk = int(oc.item())
    return ob[0, :kk], osc[0, :kk], ol[0, :kk], a0[0], a1[0]


def _vote(mode, bboxes, cls_scores, labels, nms_cfg, score_factor, max_num):
    """Wrapper semantics of radet/ops/vote/vote_wrapper.py:7-83: list-valued score types select
    cls*score_factor; the op pops 'sigma' (the BOP configs spell it 'sima', so the default 0.025 applies)."""
    src = bboxes.device if isinstance(bboxes, torch.Tensor) else torch.device("cpu")
    cfg = dict(nms_cfg)
    thr = cfg.pop("iou_threshold", 0.6)
    ctype = cfg.pop("cluster_score", "cls")
    vtype = cfg.pop("vote_score", "iou")
    iou_enable = cfg.pop("iou_enable", False)
    sigma = cfg.pop("sigma", 0.025)
    b = _t(bboxes, torch.float32).reshape(-1, 4)
    c = _t(cls_scores, torch.float32).reshape(-1)
    f = None if score_factor is None else _t(score_factor, torch.float32).reshape(-1)
    lab = _t(labels, torch.long).reshape(-1)

    def pick(t):
        if isinstance(t, (list, tuple)):
            return (c * f).contiguous()
        if t == "cls":
            return c
        if t == "iou":
            return f
        raise RuntimeError(f"Unexpected score type:{t}")

    ob, osc, ol, _, _ = _run(mode, b, pick(ctype), pick(vtype), lab, thr, iou_enable, sigma, max_out=max_num)
    dets = torch.cat([ob, osc[:, None]], dim=-1)
    return dets.to(src), ol.to(src)


def vote_nms(bboxes, cls_scores, labels, nms_cfg, score_factor=None, max_num=0):
    return _vote(0, bboxes, cls_scores, labels, nms_cfg, score_factor, max_num)


def global_vote_nms(bboxes, cls_scores, labels, nms_cfg, score_factor=None, max_num=0):
    return _vote(1, bboxes, cls_scores, labels, nms_cfg, score_factor, max_num)


def cluster_nms(bboxes, scores, categories, iou_threshold=0.65):
    """radet/ops/cluster/cluster_wrapper.py:7-22 -> (instance_ids i64[N], clusters_num i64[N])."""
    src = bboxes.device if isinstance(bboxes, torch.Tensor) else torch.device("cpu")
    b = _t(bboxes, torch.float32).reshape(-1, 4)
    s = _t(scores, torch.float32).reshape(-1)
    lab = _t(categories, torch.long).reshape(-1)
    _, _, _, ids, num = _run(2, b, s, s, lab, iou_threshold)
    n = b.shape[0]
    return ids[:n].to(src), num[:n].to(src)


def _soft_args(iou_threshold, sigma, min_score, method, offset):
    """the refusals of the Soft-NMS entry points (nothing is approximated): -> the kernel's method code"""
    if offset != 0:
        raise NotImplementedError(f"soft_nms(offset={offset}): only offset=0 (mmcv's default for float boxes) is implemented")
    if method not in K.SOFT_NMS_METHODS:
        raise ValueError(f"soft_nms method {method!r}: expected one of {sorted(K.SOFT_NMS_METHODS)}")
    if method == "gaussian" and not float(sigma) > 0:
        raise ValueError(f"soft_nms(method='gaussian') needs sigma > 0, got {sigma}")
    return K.SOFT_NMS_METHODS[method]


def _run_soft(b, s, lab, method, thr, sigma, min_score, class_agnostic):
    """-> (boxes [k,4], decayed scores [k], keep [k]) of the device tensors b [n,4], s [n], lab i64 [n]"""
    n = int(b.shape[0])
    if n > _MAX:
        raise ValueError(f"Soft-NMS input of {n} boxes exceeds the kernel's capacity ({_MAX})")
    dev = _dev()
    cap = max(n, 1)
    ob = torch.zeros(1, cap, 4, device=dev)
    osc = torch.zeros(1, cap, device=dev)
    ol = torch.zeros(1, cap, dtype=torch.long, device=dev)
    okp = torch.zeros(1, cap, dtype=torch.long, device=dev)
    if n == 0:
        return ob[0, :0], osc[0, :0], okp[0, :0]
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    oc = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(K.soft_nms_ws_bytes(1, cap), dtype=torch.uint8, device=dev)
    K.soft_nms(b, s, lab, cnt, 1, cap, method, float(thr), float(sigma), float(min_score), bool(class_agnostic), cap, ob,
               osc, ol, okp, oc, ws)
    kk = int(oc.item())
    return ob[0, :kk], osc[0, :kk], okp[0, :kk]


def soft_nms(boxes, scores, iou_threshold=0.3, sigma=0.5, min_score=1e-3, method="linear", offset=0):
    """mmcv.ops.soft_nms (one class, no class offset) -> (dets [k,5] = boxes and decayed scores in pick order, inds [k]).
    Restates mmcv 1.3.18's softnms_cpu (parity unpinned: include/radet_hip.h, "Soft-NMS"); refuses offset != 0, an
    unknown method and sigma <= 0 with 'gaussian'."""
    m = _soft_args(iou_threshold, sigma, min_score, method, offset)
    src = boxes.device if isinstance(boxes, torch.Tensor) else torch.device("cpu")
    b = _t(boxes, torch.float32).reshape(-1, 4)
    s = _t(scores, torch.float32).reshape(-1)
    ob, osc, keep = _run_soft(b, s, torch.zeros(b.shape[0], dtype=torch.long, device=b.device), m, iou_threshold, sigma,
                              min_score, True)
    return torch.cat([ob, osc[:, None]], -1).to(src), keep.to(src)


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """mmcv.ops.batched_nms semantics as used by radet_head.py:160: returns (cat[boxes, score], keep).  nms_cfg['type'] ==
    'soft_nms' runs Soft-NMS (scores = the decayed ones); a missing type, 'nms' and every other type run hard NMS."""
    src = boxes.device if isinstance(boxes, torch.Tensor) else torch.device("cpu")
    cfg = dict(nms_cfg)
    class_agnostic = cfg.pop("class_agnostic", class_agnostic)
    if cfg.get("type") == "soft_nms":
        m = _soft_args(cfg.get("iou_threshold", 0.3), cfg.get("sigma", 0.5), cfg.get("min_score", 1e-3),
                       cfg.get("method", "linear"), cfg.get("offset", 0))
        split_thr = cfg.get("split_thr", 10000)
        n = int(np.prod(tuple(scores.shape)))
        if 0 <= split_thr <= n:
            raise NotImplementedError(
                f"batched_nms(type='soft_nms') with {n} >= split_thr={split_thr} boxes: mmcv's per-class split path returns "
                "the undecayed scores there; pass split_thr=-1 in nms_cfg for Soft-NMS over all boxes")
        b = _t(boxes, torch.float32).reshape(-1, 4)
        s = _t(scores, torch.float32).reshape(-1)
        lab = _t(idxs, torch.long).reshape(-1)
        ob, osc, keep = _run_soft(b, s, lab, m, cfg.get("iou_threshold", 0.3), cfg.get("sigma", 0.5),
                                  cfg.get("min_score", 1e-3), class_agnostic)
        return torch.cat([ob, osc[:, None]], -1).to(src), keep.to(src)
    thr = cfg.get("iou_threshold", cfg.get("iou_thr", 0.5))
    b = _t(boxes, torch.float32).reshape(-1, 4)
    s = _t(scores, torch.float32).reshape(-1)
    lab = _t(idxs, torch.long).reshape(-1)
    if class_agnostic:
        lab = torch.zeros_like(lab)
    n = b.shape[0]
    ob, osc, _, keep, _ = _run(3, b, s, s, lab, thr, max_out=max(n, 1))
    k = ob.shape[0]
    return torch.cat([ob, osc[:, None]], -1).to(src), keep[:k].to(src)


def border_seeds(h, w, interval=3):
    """Seeds on the crop border every `interval` pixels -- top, bottom, left, right -- as the reference wrapper lays
    them out (bbox2distance_wrapper.py:22-36).  Returns (seeds_x, seeds_y) int64 tensors."""
    hx = list(range(0, w, interval))
    if hx[-1] != w - 1:
        hx.append(w - 1)
    hx = torch.tensor(hx, dtype=torch.int64)
    vy = torch.arange(1, h - 1, interval, dtype=torch.int64)
    sx = torch.cat((hx, hx, torch.zeros_like(vy), torch.full_like(vy, w - 1)))
    sy = torch.cat((torch.zeros_like(hx), torch.full_like(hx, h - 1), vy, vy))
    return sx, sy


def _upload(array, dev):
    """host ndarray -> device tensor through pinned memory, without blocking the host (the device chain of the mask-free
    sampler reads nothing back and waits for nothing)"""
    t = torch.from_numpy(np.ascontiguousarray(array))
    if not t.numel():
        return torch.empty(t.shape, dtype=t.dtype, device=dev)
    return t.pin_memory().to(dev, non_blocking=True)


@functools.lru_cache(maxsize=4096)
def _border_seeds_np(h, w, interval):
    sx, sy = border_seeds(h, w, interval)
    return sx.numpy().astype(np.int32), sy.numpy().astype(np.int32)


def _seed_desc(p, seeds):
    """distance-kernel descriptor rows (pixel offset, h, w, first seed, seeds) of a _Packed and its per-crop seeds"""
    sxs, sys_, desc, so = [], [], [], 0
    for o, (h, w), (sx, sy) in zip(p.offs, p.hw, seeds):
        assert h >= 2 and w >= 2
        sx = (sx.cpu().numpy() if isinstance(sx, torch.Tensor) else np.asarray(sx)).reshape(-1).astype(np.int32)
        sy = (sy.cpu().numpy() if isinstance(sy, torch.Tensor) else np.asarray(sy)).reshape(-1).astype(np.int32)
        desc.append((o, h, w, so, sx.size))
        sxs.append(sx); sys_.append(sy)
        so += sx.size
    dev = p.data.device
    return (_upload(np.array(desc, np.int32), dev), _upload(np.concatenate(sxs), dev), _upload(np.concatenate(sys_), dev))


def _mbd_packed(p, seeds, alpha=0.1, niter=4, base_size=300):
    """u8 HWC crops (_Packed) -> f64 maps packed at the same offsets"""
    out = p.empty_like(dtype=torch.float64, channels=1)
    if len(p.hw):
        desc, sx, sy = _seed_desc(p, seeds)
        ws = torch.empty(K.mbd_ws_bytes(p.px), dtype=torch.uint8, device=p.data.device)
        K.mbd(p.data, desc, len(p.hw), sx, sy, float(alpha), int(niter), int(base_size), out.data, p.px, ws)
    return out


def _gdt_packed(p, seeds):
    """f32 cost maps (_Packed) -> f32 distances packed at the same offsets"""
    out = p.empty_like()
    if len(p.hw):
        desc, sx, sy = _seed_desc(p, seeds)
        ws = torch.empty(p.px, dtype=torch.int32, device=p.data.device)
        K.gdt(p.data, desc, len(p.hw), sx, sy, out.data, ws)
    return out


def mbd_batch(images, seeds, alpha=0.1, niter=4, base_size=300):
    """Minimum-barrier distance maps of a list of u8 HWC crops (one workgroup per crop); seeds: list of (sx, sy).
    Returns a list of f64 [h, w] device tensors == bbox2distance_ext.MBD per crop (bit-identical)."""
    if not len(images):
        return []
    return _mbd_packed(_Packed.pack(images, torch.uint8, 3), seeds, alpha, niter, base_size).unpack()


def gdt_batch(costs, seeds):
    """Geodesic distance transforms of a list of f32 [h, w] cost maps; == bbox2distance_ext.GDT per map."""
    if not len(costs):
        return []
    return _gdt_packed(_Packed.pack(costs, torch.float32, 1), seeds).unpack()


def MBD(image, seeds_x, seeds_y, alpha, niter, base_size):
    """Signature of the reference's pybind op `bbox2distance_ext.MBD` (bbox2distance_ext.cpp:127-133)."""
    return mbd_batch([image], [(seeds_x, seeds_y)], alpha, niter, base_size)[0]


def GDT(costmap, seeds_x, seeds_y):
    """Signature of `bbox2distance_ext.GDT` (bbox2distance_ext.cpp:225-236)."""
    return gdt_batch([costmap], [(seeds_x, seeds_y)])[0]


# ---------------------------------------------------------------------------------------------- image processing (packed crops)
class _Packed:
    """box crops of one call packed on the device: data [px (* c)], desc i32 [n, 3] = (pixel offset, h, w).  Crops lie back
    to back unless `offs` says where they start (a selection out of a larger pack shares its data)."""

    def __init__(self, data, hw, channels, offs=None, desc=None):
        self.data, self.hw, self.c = data, [(int(h), int(w)) for h, w in hw], channels
        if offs is None:
            offs, o = [], 0
            for h, w in self.hw:
                offs.append(o)
                o += h * w
        self.offs = [int(o) for o in offs]
        self.px = max([o + h * w for o, (h, w) in zip(self.offs, self.hw)], default=0)      # pixels the crops span
        self.desc = desc if desc is not None else _upload(
            np.array([[o_, h, w] for o_, (h, w) in zip(self.offs, self.hw)], np.int32).reshape(-1, 3), data.device)
        self.max_px = max([h * w for h, w in self.hw], default=0)

    @staticmethod
    def pack(items, dtype, channels):
        dev = _dev()
        ts = [torch.as_tensor(it).to(dev, dtype) for it in items]
        for t in ts:
            assert (t.dim() == 3 and t.shape[2] == channels) if channels > 1 else t.dim() == 2, tuple(t.shape)
        flat = torch.cat([t.reshape(-1) for t in ts]) if ts else torch.empty(0, dtype=dtype, device=dev)
        return _Packed(flat.contiguous(), [t.shape[:2] for t in ts], channels)

    def select(self, idx):
        """the crops idx of this pack, in place"""
        return _Packed(self.data, [self.hw[i] for i in idx], self.c, offs=[self.offs[i] for i in idx])

    def empty_like(self, hw=None, dtype=None, channels=None):
        """uninitialised pack of other sizes (back to back), or of the same crops at the same offsets"""
        c = self.c if channels is None else channels
        if hw is None:
            return _Packed(torch.empty(self.px * c, dtype=dtype or self.data.dtype, device=self.data.device), self.hw, c,
                           offs=self.offs, desc=self.desc)
        n = sum(int(h) * int(w) for h, w in hw) * c
        return _Packed(torch.empty(n, dtype=dtype or self.data.dtype, device=self.data.device), hw, c)

    def unpack(self):
        out = []
        for o, (h, w) in zip(self.offs, self.hw):
            t = self.data[o * self.c:(o + h * w) * self.c]
            out.append(t.view(h, w, self.c) if self.c > 1 else t.view(h, w))
        return out


def _resize(p, dsizes):
    """cv2.resize(crop, (w, h)) per crop (INTER_LINEAR): uint8 HWC, float32 or float64 HW"""
    out = p.empty_like(hw=[(int(h), int(w)) for (w, h) in dsizes])
    if len(p.hw):
        if p.data.dtype == torch.uint8:
            K.resize_linear_u8(p.data, p.desc, out.data, out.desc, len(p.hw), out.max_px, p.c)
        else:
            K.resize_linear_f(p.data, p.desc, out.data, out.desc, len(p.hw), out.max_px)
    return out


def _blur9(p):
    out = p.empty_like()
    if len(p.hw):
        tmp = torch.empty(p.px * 3, dtype=torch.float32, device=p.data.device)
        K.gaussian_blur9_u8(p.data, p.desc, out.data, tmp, len(p.hw), p.max_px)
    return out


def _sobel(p):
    out = p.empty_like(dtype=torch.float32, channels=1)
    if len(p.hw):
        gray = torch.empty(p.px, dtype=torch.uint8, device=p.data.device)
        mx = torch.empty(len(p.hw), dtype=torch.int32, device=p.data.device)
        K.sobel_edge(p.data, p.desc, out.data, gray, mx, len(p.hw), p.max_px)
    return out


def resize_batch(images, dsizes):
    """list of crops (uint8 [h, w, 3] or float [h, w]) resized to dsizes = [(w, h), ...] like cv2.resize(img, (w, h))"""
    t0 = torch.as_tensor(images[0])
    if t0.dtype == torch.uint8:
        p = _Packed.pack(images, torch.uint8, 3 if t0.dim() == 3 else 1)
    else:
        p = _Packed.pack(images, torch.float64 if t0.dtype == torch.float64 else torch.float32, 1)
    return _resize(p, dsizes).unpack()


def gaussian_blur9_batch(images):
    """cv2.GaussianBlur(img, (9, 9), sigmaX=0, borderType=BORDER_DEFAULT) per uint8 [h, w, 3] crop"""
    return _blur9(_Packed.pack(images, torch.uint8, 3)).unpack()


def sobel_edge_batch(images):
    """GDT_box2distance.sobel_extract_edge per uint8 [h, w, 3] crop -> float32 [h, w]"""
    return _sobel(_Packed.pack(images, torch.uint8, 3)).unpack()


def _center_prepare(p, size):
    """mode='center': short edge -> `size` pixels (cv2.resize), then the 9x9 Gaussian (wrapper.py:80-88 / 170-177);
    p: _Packed u8 HWC crops.  Returns (blurred _Packed, the crops' own (w, h))"""
    orig, dsz = [], []
    for h, w in p.hw:
        ratio = size / min(w, h)
        dsz.append((int(w * ratio), int(h * ratio)))
        orig.append((w, h))
    return _blur9(_resize(p, dsz)), orig


def _cropped(box_images, mask_enable, bbox_images_xy, maps, idx, ones_dtype):
    """the wrappers' return value: per box its region of its map, ones for a disabled box"""
    maps = dict(zip(idx, maps.unpack()))
    out = []
    for i, (img, xy) in enumerate(zip(box_images, bbox_images_xy)):
        d = maps[i] if i in maps else torch.ones(tuple(img.shape[:2]), dtype=ones_dtype, device=_dev())
        out.append(d[xy[1]:xy[-1], xy[0]:xy[2]])
    return out


class MBD_box2distance:
    """`radet.ops.MBD_box2distance` (bbox2distance_wrapper.py:9-95) on the GPU, all enabled crops of a call batched:
    mode='center' (the reference default) = resize to a 150-pixel short edge -> 9x9 Gaussian -> MBD -> resize back;
    mode='mean' = MBD on the crop itself.  `multi_scale` is stored and, like in the reference's __call__, not used."""

    def __init__(self, mode="center", multi_scale=False, alpha=0.1, niter=4, base_size=300, interval=3):
        assert mode in ["center", "mean"]
        self.mode, self.multi_scale, self.alpha, self.niter = mode, multi_scale, alpha, niter
        self.base_size, self.interval, self.size = base_size, interval, 150

    def cal_dmap_single_scale(self, image):
        h, w = image.shape[:2]
        return MBD(image, *border_seeds(h, w, self.interval), self.alpha, self.niter, self.base_size)

    def packed_maps(self, canvases, mask_enable):
        """canvases: _Packed of u8 HWC crops on the device -> (_Packed of the enabled crops' f64 maps, each of its crop's
        size, and their indices).  Every size and seed follows from the crops' shapes: nothing is read back."""
        idx = [i for i, e in enumerate(mask_enable) if e]
        p = canvases.select(idx)
        if self.mode == "center" and idx:
            p, orig = _center_prepare(p, self.size)
        maps = _mbd_packed(p, [_border_seeds_np(h, w, self.interval) for h, w in p.hw], self.alpha, self.niter, self.base_size)
        if self.mode == "center" and idx:
            maps = _resize(maps, orig)
        return maps, idx

    def __call__(self, box_images, mask_enable, bbox_images_xy):
        idx = [i for i, e in enumerate(mask_enable) if e]          # (disabled crops never leave the host)
        maps, _ = self.packed_maps(_Packed.pack([box_images[i] for i in idx], torch.uint8, 3), [True] * len(idx))
        return _cropped(box_images, mask_enable, bbox_images_xy, maps, idx, torch.uint8)


class GDT_box2distance:
    """`radet.ops.GDT_box2distance` (bbox2distance_wrapper.py:98-185) on the GPU.  edge_mode='sobel' runs the Sobel edge
    extractor as HIP passes; the reference's default edge_mode='sed' needs OpenCV's structured-edge model file
    (cv2.ximgproc, 'model.yml'), which is data this repository does not have: pass `extract_edge_func(image) -> f32[h, w]`
    for it."""

    def __init__(self, edge_mode="sed", interval=3, mode="center", extract_edge_func=None):
        self.interval, self.mode, self.size, self.edge_mode = interval, mode, 150, edge_mode
        self.extract_edge_func = extract_edge_func
        if extract_edge_func is None and edge_mode == "sed":
            raise NotImplementedError("GDT_box2distance(edge_mode='sed') needs cv2.ximgproc's structured-edge model "
                                      "(model.yml); use edge_mode='sobel' or pass extract_edge_func")

    def sobel_extract_edge(self, image):
        return sobel_edge_batch([image])[0]

    def _edges(self, p):
        """_Packed u8 crops -> _Packed f32 cost maps at the same offsets (a host callback reads the crops back)"""
        if self.extract_edge_func is None:
            return _sobel(p)
        out = p.empty_like(dtype=torch.float32, channels=1)
        for o, (h, w), c in zip(p.offs, p.hw, p.unpack()):
            out.data[o:o + h * w] = torch.as_tensor(self.extract_edge_func(c.cpu().numpy())).to(out.data.device, torch.float32).reshape(-1)
        return out

    def cal_dmap_single_scale(self, box_image):
        h, w = box_image.shape[:2]
        cost = self._edges(_Packed.pack([box_image], torch.uint8, 3)).unpack()[0]
        return GDT(cost, *border_seeds(h, w, self.interval))

    def packed_maps(self, canvases, mask_enable):
        """canvases: _Packed of u8 HWC crops on the device -> (_Packed of the enabled crops' f32 maps, their indices); with
        the Sobel extractor nothing is read back"""
        idx = [i for i, e in enumerate(mask_enable) if e]
        p = canvases.select(idx)
        if self.mode == "center" and idx:
            p, orig = _center_prepare(p, self.size)
        maps = _gdt_packed(self._edges(p), [_border_seeds_np(h, w, self.interval) for h, w in p.hw])
        if self.mode == "center" and idx:
            maps = _resize(maps, orig)
        return maps, idx

    def __call__(self, box_images, mask_enable, bbox_images_xy):
        idx = [i for i, e in enumerate(mask_enable) if e]          # (disabled crops never leave the host)
        maps, _ = self.packed_maps(_Packed.pack([box_images[i] for i in idx], torch.uint8, 3), [True] * len(idx))
        return _cropped(box_images, mask_enable, bbox_images_xy, maps, idx, torch.float32)


from .crops import Crops, crop_detections  # noqa: E402  (RoI crops of detections: its own module, it needs _dev from here)
from .tta import merge_view_candidates  # noqa: E402  (test-time augmentation: the views' candidates merged per image)
from .tiles import merge_tile_candidates, plan_tiles  # noqa: E402  (tiled inference: the tile plan, the rows' candidates merged per image)
from .draw import build_atlas, draw_detections  # noqa: E402  (detections drawn on frames: one overlay launch)
from .track import Tracker, track_detections  # noqa: E402  (detections tracked across frames: one update launch per batch)
from .color import adjust_brightness, adjust_color, adjust_contrast, imequalize  # noqa: E402  (mmcv's photometric functions)
