"""Thin Python launchers over the C ABI (include/radet_hip.h): torch tensors are used only as device
buffers (data_ptr) and for the current HIP stream.  No arithmetic happens in PyTorch here."""
import collections
import ctypes as C
import os

import torch

from . import _lib

# ---------------------------------------------------------------------- launch flag words
# The two packed integers that steer a conv launch, defined in include/radet_hip.h: RADET_TILE_<N> is <N> here, RADET_WGRAD_<N>
# is WG_<N>; TAG_<N> are the bits of conv_igemmg_kernel's template argument (csrc/conv_igemm_kernel.h).  tests/test_host.py
# holds the two sides together.  The same number means different things in the two words: use the names.
# tile_override of radet_conv2d_igemm*:
ID_MASK = 0xFF                            # block tile, TILE_SHAPE below (0: launcher heuristic)
SYMBOL = 0x100                            # tagged kernel symbol (profiling)
BK32 = 0x200                              # K step 32 instead of 16 channels (no meaning with P3)
MATH_BF16 = 0x400                         # bf16 math: fp32 tensors, operands rounded to bf16 in front of the matrix core
STORE_BF16, OUT_F32 = 0x800, 0x10000      # bf16 tensors in HBM / fp32 output from bf16 inputs (predictor heads)
SPLITK, SPLITK_MASK = 0x1000, 0xF000      # * n (1..15): forced split-K factor, splitk(n)
STAGES3 = 0x20000                         # 3 LDS stages in the fp32 implicit-GEMM kernel (forward launches)
STAGES4 = 0x40000                         # 4 LDS stages (fp16 hi / lo arithmetic, K-divided tile 8)
ROWPAIRS = 0x80000                        # plane-pair operands, 8-wave tiles: both planes of a tile row in one 128-byte piece per load
STREAMK, STREAMK_MASK = 0x100000, 0x700000    # * w (1..7): stream-K schedule with w persistent workgroups per CU (fp32 tags), streamk(w)
X3 = 0x1000000                            # fp32 tensors, products from three bf16 planes per operand on the bf16 matrix cores
P3 = 0x2000000                            # x / w arrive as plane tensors (bf16 triples, or fp16 pairs with H2); fp32 outputs
H2 = 0x8000000                            # fp16 hi / lo arithmetic (with X3 or P3): 3 f16 MFMAs per K = 16 step, needs amax slots
MASKQ = 0x10000000                        # the launch's ReLU mask tensor is an fp16 plane-pair tensor (round 6: pairs-only activations)
# flags of radet_conv2d_wgrad*:
WG_MATH_BF16, WG_STORE_BF16 = 0x1, 0x2    # bf16 math / dy and x are bf16 tensors
WG_TILE, WG_TILE_MASK = 0x10, 0x30        # * t: tile of the one-tap kernel, WG_TILE_SHAPE below (0: the launcher's choice)
WG_ONE_TAP = 0x40                         # never the all-taps kernel
WG_PX32 = 0x80                            # 32 instead of 16 pixels per LDS stage
WG_X3 = 0x100                             # fp32 products from three bf16 planes per operand
WG_P3 = 0x200                             # dy / x arrive as plane tensors
WG_KDIV4, WG_KDIV2 = 0x400, 0x800         # 64 x 64 tile: the waves divide a 64-pixel stage four ways / a 32-pixel stage two ways
WG_H2 = 0x1000                            # fp16 hi / lo arithmetic
WG_DEEP, WG_WINDOWS = 0x2000, 0x4000      # all-taps pair kernel: conv_wgrad9d_kernel / conv_wgrad9r_kernel (experiments)
# template argument TAG of conv_igemmg_kernel:
TAG_SYMBOL, TAG_BF16_MATH, TAG_H16, TAG_X3, TAG_P3, TAG_KDIV, TAG_H2, TAG_PAIRS = 1, 2, 4, 8, 16, 32, 64, 128
# ---------------------------------------------------------------------- end of the launch flag words
# flag word of the layer entry points (stem, max-pool, GroupNorm, upsample-add, ReLU backward): RADET_LAYER_<N> is LAYER_<N>
LAYER_BF16 = 0x1                          # the activation tensors are bf16 (no plane output, no amax slot)
LAYER_PAIRS = 0x2                         # the optional plane output holds fp16 plane pairs, not bf16 plane triples

TILE_SHAPE = {1: (128, 128), 2: (128, 64), 3: (64, 64), 4: (128, 32), 5: (128, 128), 6: (256, 128), 7: (64, 64), 8: (64, 64)}   # rows x Cout
WG_TILE_SHAPE = {1: (128, 128), 2: (64, 64), 3: (128, 64)}                                                                   # Cout x Cin


def splitk(n):
    return n * SPLITK


def streamk(w):
    return w * STREAMK


def tile_id(t):
    return t & ID_MASK


def with_tile(t, tid):
    """t with block tile tid and no forced split-K factor (which belonged to the tile it replaces)"""
    return (t & ~(ID_MASK | SPLITK_MASK)) | tid


def wg_tile(flags):
    return (flags & WG_TILE_MASK) // WG_TILE



def _ptr(t):
    """device address of a contiguous device tensor (None -> NULL) as a plain int: ctypes converts it per the argtypes.
    This runs ~1500 times per train step: the bf16-storage step and single-image inference are bound by the host's enqueue
    time, so the checks are two attribute reads and one call."""
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous()):
        raise AssertionError("HIP kernels need contiguous device tensors")
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """the current HIP stream's handle (plain int).  torch._C._cuda_getCurrentRawStream avoids building a torch.cuda.Stream
    object per launch (2 us each, 250 launches per step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def ev_record(ev, stream=None):
    """ev.record() on `stream` (a torch stream; None: the current one).  The engine's cross-stream dependencies go through
    these two helpers so that a launch tape being recorded (radet_amd/tape.py) sees them."""
    if stream is None:
        ev.record()
    else:
        ev.record(stream)
    t = _lib.TAPE
    if t is not None:
        t.record_event(ev, _stream() if stream is None else stream.cuda_stream)


def ev_wait(ev, stream=None):
    """`stream` (None: the current one) waits for event ev"""
    (torch.cuda.current_stream() if stream is None else stream).wait_event(ev)
    t = _lib.TAPE
    if t is not None:
        t.wait_event(ev, _stream() if stream is None else stream.cuda_stream)


def fill_zero(t):
    """stream-ordered zero fill of a contiguous device tensor (hipMemsetAsync; tape-able, unlike Tensor.zero_())"""
    _lib.call("radet_fill_zero", _ptr(t), C.c_size_t(t.numel() * t.element_size()), _stream())


def copy_d2d(dst, src):
    """stream-ordered device-to-device copy between contiguous tensors of equal byte size"""
    n = dst.numel() * dst.element_size()
    assert n == src.numel() * src.element_size()
    _lib.call("radet_copy_d2d", _ptr(dst), _ptr(src), C.c_size_t(n), _stream())


COPY_DESC_INTS, COPY_TILE_BYTES = 6, 16384       # include/radet_hip.h


def copy_segments_table(rows):
    """The descriptor table of radet_copy_segments for rows of (source byte address, destination byte address, bytes):
    (int32 [n, COPY_DESC_INTS] host array, tile total).  Host arithmetic only."""
    import numpy as np
    r = np.asarray(rows, np.int64).reshape(-1, 3)
    if (r[:, 2] < 0).any() or (r[:, 2] >= 2 ** 31).any():
        raise ValueError("a segment holds 0 .. 2^31 - 1 bytes")
    tiles = np.where(r[:, 2] > 0, ((r[:, 1] & 15) + r[:, 2] + COPY_TILE_BYTES - 1) // COPY_TILE_BYTES, 0)
    total = int(tiles.sum())
    if total >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 tiles in one table")
    t = np.empty((len(r), COPY_DESC_INTS), np.int32)
    t[:, 0:4] = np.ascontiguousarray(r[:, :2]).view(np.uint32).reshape(-1, 4).view(np.int32)   # (little endian: lo, hi)
    t[:, 4] = r[:, 2]
    t[:, 5] = np.cumsum(tiles) - tiles
    return t, total


def copy_segments(desc, n, n_tiles):
    """one launch that copies every row of a device descriptor table (copy_segments_table, uploaded by the caller)"""
    _lib.call("radet_copy_segments", _ptr(desc), int(n), int(n_tiles), _stream())


class Levels:
    """Row-concatenated multi-level NHWC geometry: level l = B images of h_l x w_l pixels."""

    def __init__(self, hw, B):
        self.hw = [(int(h), int(w)) for h, w in hw]
        self.B = int(B)
        self.offsets = []
        r = 0
        for h, w in self.hw:
            self.offsets.append(r)
            r += self.B * h * w
        self.rows = r

    def __len__(self):
        return len(self.hw)

    def conv_out(self, k, stride, pad):
        return Levels([((h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1) for h, w in self.hw], self.B)

    def level_rows(self, l):
        h, w = self.hw[l]
        return self.offsets[l], self.offsets[l] + self.B * h * w

    def sub(self, l):
        return Levels([self.hw[l]], self.B)


def _desc(pairs):
    """pairs: list of (Hi, Wi, Ho, Wo, in_off, out_off) -> ctypes int array"""
    flat = [int(v) for p in pairs for v in p]
    return (C.c_int * len(flat))(*flat), len(pairs)


class _LRU(dict):
    """dict with a size bound: the oldest insertions are dropped first (a dropped gather table / tune entry is simply
    rebuilt on its next use)."""

    def __init__(self, cap):
        super().__init__()
        self.cap = cap

    def __setitem__(self, k, v):
        super().__setitem__(k, v)
        while len(self) > self.cap:
            del self[next(iter(self))]


_TABLE_CACHE = _LRU(1024)      # gather tables / parity classes per conv geometry (~80 per (B, H, W) plan)

# Measurement hook (bench.py): when EVENTS is a list, every conv GEMM launch issued through this module is bracketed by a
# pair of HIP events on the stream it is launched on and appended as dict(key, flops, start, end, replay).  `key` names
# the kernel instantiation the launcher dispatches to, `flops` = 2 * rows * Cout * Cin * taps of the launch (x 2 for a
# grouped pair), `replay()` issues the same launch again (same buffers) for the "alone on the device" timing.
EVENTS = None
STAGE = ""          # part of the detector the engine is enqueueing (stem, layer1..4, neck, head): recorded with every event
_TILES = {1: "128, 128, 2, 2", 2: "128, 64, 2, 2", 3: "64, 64, 2, 2", 4: "128, 32, 4, 1", 5: "128, 128, 2, 4", 6: "256, 128, 4, 2",
          7: "64, 64, 2, 2", 8: "64, 64, 2, 2"}


def _igemm_key(t, x):
    """kernel symbol an implicit-GEMM launch with tile_override word t dispatches to (conv_igemm.hip: igemm_impl)"""
    tid = tile_id(t)
    if tid == 0:
        return "conv_igemmg_kernel<launcher heuristic>"
    sym = TAG_SYMBOL if t & SYMBOL else 0
    if t & H2 and (t & P3 or t & X3):
        if t & P3 and tid == 7:                 # K-divided 64 x 64 tile on plane pairs (round 6)
            return f"conv_igemmg_kernel<64, 64, 2, 2, {TAG_X3 | TAG_KDIV | TAG_H2 | TAG_PAIRS}, 64, 2, false>"
        if t & P3 and t & ROWPAIRS and tid in (5, 6):
            return f"conv_igemmg_kernel<{_TILES[tid]}, {TAG_P3 | TAG_H2 | TAG_PAIRS | sym}, 32, 2, false>"
        if t & P3:
            tag, bk = TAG_P3 | TAG_H2 | sym, 16
        else:
            tag, bk = TAG_X3 | TAG_H2 | sym, 32
            if tid >= 7:
                nst = 2 if tid == 7 else (4 if t & STAGES4 else (3 if t & STAGES3 else 2))
                return f"conv_igemmg_kernel<{_TILES[tid]}, {TAG_X3 | TAG_H2 | TAG_KDIV}, {64 if tid == 7 else 32}, {nst}, false>"
        return f"conv_igemmg_kernel<{_TILES.get(tid, '?')}, {tag}, {bk}, {3 if t & STAGES3 else 2}, false>"
    if t & P3:
        tag, bk = TAG_P3 | sym, 16
    elif t & STORE_BF16:
        tag, bk = TAG_H16 | sym, 32 if t & BK32 else 16
    elif t & X3:
        tag, bk = TAG_X3 | sym, 32
        if tid >= 7:                        # K-divided 64 x 64 tiles: 7 = four k-groups of a 64-channel stage,
            tag, bk = tag | TAG_KDIV, 64 if tid == 7 else 32    # 8 = two k-groups x two column halves of 32 channels
            return f"conv_igemmg_kernel<{_TILES[tid]}, {tag}, {bk}, 2, false>"
    else:
        tag, bk = sym | (TAG_BF16_MATH if t & MATH_BF16 else 0), 32 if t & BK32 else 16
    skw = (t & STREAMK_MASK) // STREAMK
    stages = 3 if (t & STAGES3) and (tag <= TAG_SYMBOL or tag & (TAG_X3 | TAG_P3)) and not skw else 2
    return f"conv_igemmg_kernel<{_TILES.get(tid, '?')}, {tag}, {bk}, {stages}, {'true' if skw and tag == 0 else 'false'}>"


def _timed(key, flops, fn, nbytes=0.0, kind="fwd", geom=None):
    """key: the kernel's name, or a callable producing it (only evaluated when a measurement is running); kind: fwd / dgrad /
    wgrad; the engine's STAGE at the time of the call goes into the record (bench.py's per-stage table)"""
    ev = EVENTS
    if ev is None:
        return fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    ev.append(dict(key=key() if callable(key) else key, flops=float(flops), bytes=float(nbytes), start=s, end=e, replay=fn,
                   stage=STAGE, kind=kind, geom=geom))


def _conv_bytes(g, groups=1):
    """algorithmic HBM bytes of one conv launch at fp32: input once + weights + output once"""
    return 4.0 * groups * (g.lin.rows * g.cin + g.cout * g.k * g.k * g.cin + g.lout.rows * g.cout)

STRIDED_DGRAD_CLASSES = True   # parity-class dgrad for strided convs (False = one dense launch)
IDENTITY_NO_TABLE = os.environ.get("RADET_IDENTITY_TABLE", "0") != "1"   # 1 x 1 / stride 1 convs run without a gather table


def _gather_table(key, B, k, so, sr, off, div, desc, nseg, rows):
    """Device gather table for one conv geometry, shared by every conv with the same geometry."""
    dev = torch.cuda.current_device()
    key = (dev,) + key
    t = _TABLE_CACHE.get(key)
    if t is None:
        mp = _lib.load().radet_gather_table_rows(rows)
        t = torch.empty(k * k * mp, dtype=torch.int32, device=torch.device("cuda", dev))
        _lib.call("radet_build_gather_table", _ptr(t), B, k, k, so, sr, off, div, desc, nseg, _stream())
        # Tables are shared by every conv of this geometry, whatever stream it launches on (the cls tower's dgrad builds
        # the table on the main stream, the reg tower's dgrad picks it out of the cache and launches on the side
        # stream a few microseconds later): finish the build before anyone can see the table.  Once per geometry.
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream().synchronize()
        _TABLE_CACHE[key] = t
    return t


class ConvGeom:
    """Geometry of one convolution over a multi-level input (same weights on every level)."""

    def __init__(self, lin, cin, cout, k, stride, pad):
        self.lin, self.cin, self.cout, self.k, self.stride, self.pad = lin, cin, cout, k, stride, pad
        self.lout = lin.conv_out(k, stride, pad)
        self.B = lin.B
        # the kernels' tile loads address a tensor with 32-bit byte offsets (buffer_load ... lds, round 6): 4 GiB - 256 B per tensor
        # (5.7x the largest tensor of the reference config at samples_per_gpu = 16: 314 MB)
        big = max(lin.rows * cin, self.lout.rows * cout) * 4
        if big >= (1 << 32) - 256:
            raise _lib.RadetHipError(f"conv geometry {cin}->{cout} k{k} over {lin.rows} rows: a {big / 2 ** 30:.1f} GiB activation tensor "
                                     "exceeds the 4 GiB the MI355X kernels address per tensor; use a smaller batch per GPU")
        f, b = [], []
        for (hi, wi), (ho, wo), io, oo in zip(lin.hw, self.lout.hw, lin.offsets, self.lout.offsets):
            f.append((hi, wi, ho, wo, io, oo))
            b.append((ho, wo, hi, wi, oo, io))   # dgrad: rows over the conv INPUT grid, gather from dy
        self.fwd_desc, self.nseg = _desc(f)
        self.bwd_desc, _ = _desc(b)
        self._key = (tuple(lin.hw), tuple(lin.offsets), lin.B, k, stride, pad)
        self.fwd_tile = self.bwd_tile = 0     # 0 = launcher heuristic; set by autotune()
        self.math = 0                         # 1: bf16 math mode (operands rounded to bf16, fp32 accumulate)
        self.wgrad_flags = 0                  # tile override of the wgrad launcher (set by autotune_wgrad)
        self.h16 = False                      # bf16 tensors in HBM (tuning runs use the matching kernels)
        self._x3 = False                      # fp32 tensors, conv products from 16-bit planes of the operands (tile flag X3) ...
        self.h2 = False                       # ... two fp16 planes and 3 plane products (tile flag H2) instead of three bf16 / 6
        self.nsplit = _lib.load().radet_conv2d_wgrad_splits(self.lout.rows, cin, cout, k, k)
        self.pairs = False                    # forward launches read x as plane pairs written by its producer (fwd_tile_q)
        self.fwd_tile_q = 0
        self.bwd_tile_q = 0                   # dgrad launches whose dy arrives as plane pairs (pairs-only gradients, round 6)
        self.wgrad_pair_flags = 0             # weight gradient on fp16 plane pairs: WG_ONE_TAP = one-tap kernel, WG_TILE its tile (1: 128 x 128)
        self.nsplit_pairs = 0                 # its pixel splits (0: nsplit)
        self._ft = self._bt = self._classes = None
        self._cgroup = 0                                   # 0 = not looked at yet, None = no class launch for this geometry

    @property
    def x3(self):
        return self._x3

    @x3.setter
    def x3(self, v):                          # True: the bf16-plane arithmetic; "h2": the fp16 hi / lo arithmetic
        self._x3 = bool(v)
        if v == "h2":
            self.h2 = True

    # The geometry keeps its tables alive: _TABLE_CACHE only dedupes them across geometries and may drop its own
    # reference at any time -- a table freed while a launch on a side stream still reads it would be recycled by the
    # caching allocator and overwritten under that launch.
    @property
    def identity(self):
        """1 x 1 / stride 1 / no padding: GEMM row m reads row m (input and output levels coincide) -- no gather table, the
        launchers take NULL and save the dependent table load in every workgroup's prologue"""
        return self.k == 1 and self.stride == 1 and self.pad == 0 and IDENTITY_NO_TABLE

    @property
    def fwd_table(self):
        if self.identity:
            return None
        if self._ft is None:
            self._ft = _gather_table(("f",) + self._key, self.B, self.k, self.stride, 1, -self.pad, 1, self.fwd_desc,
                                     self.nseg, self.lout.rows)
        return self._ft

    @property
    def bwd_table(self):
        if self.identity:
            return None
        if self._bt is None:
            self._bt = _gather_table(("b",) + self._key, self.B, self.k, 1, -1, self.pad, self.stride, self.bwd_desc,
                                     self.nseg, self.lin.rows)
        return self._bt


_SPLITK_WS = {}


def splitk_ws_for(stream):
    """Create the split-K workspace of `stream` now (e.g. before a hipGraph capture on it)."""
    with torch.cuda.stream(stream):
        return splitk_ws()


def splitk_ws():
    """One split-K workspace per (device, stream): launches on one stream are ordered, so all convs issued
    there can share it; concurrent streams get their own."""
    dev = torch.cuda.current_device()
    key = (dev, torch.cuda.current_stream().cuda_stream)
    t = _SPLITK_WS.get(key)
    if t is None:
        # 64 MiB; zero-initialised: the first words are the arrival tickets of the in-launch split-K reduction
        t = torch.zeros(16 * 1024 * 1024, device=torch.device("cuda", dev))
        _SPLITK_WS[key] = t
    return t


def _strided_dgrad_classes(g):
    """Parity classes of the dgrad of a strided conv (built once per geometry).

    dx[h, w] only receives taps r with (h + pad - r) % stride == 0, so the rows of the dgrad GEMM split
    into stride^2 classes by (h % stride, w % stride), each with a fixed subset of contributing taps.
    One tap-subset launch per class does only the non-zero work (a dense launch wastes 75 % of the MFMAs
    of a 3x3/2 conv).  Returns a list of dicts(table, out_rows, tap_ids, ntaps, rows, zero)."""
    import numpy as np
    if g._classes is not None:
        return g._classes
    key = ("cls",) + g._key
    dev = torch.cuda.current_device()
    ck = (dev,) + key
    if ck in _TABLE_CACHE:
        g._classes = _TABLE_CACHE[ck]
        return g._classes
    KT = g.k * g.k
    M = g.lin.rows
    mp = _lib.load().radet_gather_table_rows(M)
    full = g.bwd_table.cpu().numpy().reshape(KT, mp)[:, :M]
    cls_id = np.empty(M, np.int64)
    for (h, w), off in zip(g.lin.hw, g.lin.offsets):
        hh, ww = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        c = ((hh % g.stride) * g.stride + (ww % g.stride)).reshape(-1)
        cls_id[off:off + g.B * h * w] = np.tile(c, g.B)
    out, zero_rows = [], []
    for c in range(g.stride * g.stride):
        rows = np.nonzero(cls_id == c)[0]
        if rows.size == 0:
            continue
        taps = [t for t in range(KT) if (full[t, rows] >= 0).any()]
        if not taps:
            zero_rows.append(rows)
            continue
        mpc = _lib.load().radet_gather_table_rows(rows.size)
        tab = np.full((len(taps), mpc), -1, np.int32)
        tab[:, :rows.size] = full[taps][:, rows]
        out.append(dict(table=torch.from_numpy(tab).cuda(), out_rows=torch.from_numpy(rows.astype(np.int32)).cuda(),
                        tap_ids=(C.c_int * len(taps))(*taps), ntaps=len(taps), rows=int(rows.size), zero=False))
    if zero_rows:
        rows = np.concatenate(zero_rows)
        mpc = _lib.load().radet_gather_table_rows(rows.size)
        tab = np.full((1, mpc), -1, np.int32)
        out.append(dict(table=torch.from_numpy(tab).cuda(), out_rows=torch.from_numpy(rows.astype(np.int32)).cuda(),
                        tap_ids=(C.c_int * 1)(0), ntaps=1, rows=int(rows.size), zero=True))
    if not torch.cuda.is_current_stream_capturing():
        torch.cuda.current_stream().synchronize()      # the uploads above have landed before another stream can use them
    _TABLE_CACHE[ck] = g._classes = out
    return out


STRIDED_DGRAD_GROUP = os.environ.get("RADET_DGRAD_CLASS_GROUP", "1") != "0"


def _strided_dgrad_group(g):
    """All tap-carrying parity classes of a strided dgrad as ONE launch (radet_conv2d_igemm_classes): rows sorted by
    class (most taps first), each class padded to 128 rows.  None when the geometry has a single class (1x1 / 2) or a
    class with more than 4 taps.  Returns dict(table [kmax][M], out_rows [M], tap_ids[16], ntaps[4], start[4], ncls, M)."""
    import numpy as np
    if g._cgroup is None or g._cgroup != 0:
        return g._cgroup
    cls = sorted((c for c in _strided_dgrad_classes(g) if not c["zero"]), key=lambda c: -c["ntaps"])
    grp = None
    if STRIDED_DGRAD_GROUP and 2 <= len(cls) <= 4 and all(c["ntaps"] <= 4 for c in cls):
        ck = (torch.cuda.current_device(), "clsgrp") + g._key
        grp = _TABLE_CACHE.get(ck)
        if grp is None:
            kmax = max(c["ntaps"] for c in cls)
            starts, m = [], 0
            for c in cls:
                starts.append(m)
                m += -(-c["rows"] // 128) * 128
            tab = np.full((kmax, _lib.load().radet_gather_table_rows(m)), -1, np.int32)   # row stride = the launcher's Mp
            orow = np.full(m, -1, np.int32)
            tids = [0] * 16
            for i, (c, s0) in enumerate(zip(cls, starts)):
                t = c["table"].cpu().numpy()
                tab[:c["ntaps"], s0:s0 + c["rows"]] = t[:, :c["rows"]]
                orow[s0:s0 + c["rows"]] = c["out_rows"].cpu().numpy()
                tids[4 * i:4 * i + c["ntaps"]] = list(c["tap_ids"])
            pad4 = lambda v: list(v) + [0] * (4 - len(v))  # noqa: E731
            grp = dict(table=torch.from_numpy(tab).cuda(), out_rows=torch.from_numpy(orow).cuda(),
                       tap_ids=(C.c_int * 16)(*tids), ntaps=(C.c_int * 4)(*pad4([c["ntaps"] for c in cls])),
                       start=(C.c_int * 4)(*pad4(starts)), ncls=len(cls), M=m)
            if not torch.cuda.is_current_stream_capturing():
                torch.cuda.current_stream().synchronize()
            _TABLE_CACHE[ck] = grp
    g._cgroup = grp
    return grp


_TUNE_CACHE = _LRU(8192)
_TUNE_DIRTY = False
TUNE_RUNS = 0                  # number of shapes actually timed in this process (tests: no re-tune after the first pass)


# Tile / split choices are persisted per conv geometry:
#   1. radet_amd/tune_gfx950.json -- shipped with the package: the choices for the standard geometries (r50 640x480 at
#      B = 1, 2, 4, 8 in the three arithmetic modes, r101 800x800 B = 2), produced by tools/make_tune.py on an MI355X, so
#      that identical runs pick identical tiles (reproducible losses, no start-up tuning);
#   2. the user file ($RADET_TUNE_FILE, default ~/.cache/radet_amd/tune_gfx950.json) -- shapes tuned on this machine.
# Unknown shapes are timed once and appended to the user file.  RADET_AUTOTUNE=0 disables tuning AND the files
# (launcher heuristics only).
_PACKAGED_TUNE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tune_gfx950.json")
_TUNE_LOADED = False


def _tune_file():
    return os.environ.get("RADET_TUNE_FILE") or os.path.join(os.path.expanduser("~"), ".cache", "radet_amd", "tune_gfx950.json")


def _read_tune(path):
    import ast
    import json
    with open(path) as fh:
        d = json.load(fh)
    return ({ast.literal_eval(k): tuple(v) for k, v in d.get("igemm", {}).items()},
            {ast.literal_eval(k): tuple(v) for k, v in d.get("wgrad", {}).items()})


def load_tune_cache():
    global _TUNE_LOADED
    if _TUNE_LOADED:
        return
    _TUNE_LOADED = True
    for path in (_PACKAGED_TUNE, _tune_file()):
        if os.path.exists(path):
            try:
                a, b = _read_tune(path)
            except (ValueError, SyntaxError, OSError):
                continue                      # unreadable cache: tune again
            for k, v in a.items():
                _TUNE_CACHE[k] = v
            for k, v in b.items():
                _WTUNE_CACHE[k] = v


def save_tune_cache(path=None):
    """Write every known choice (packaged + tuned here) to the user file; silent if the location is not writable."""
    import json
    global _TUNE_DIRTY
    if not _TUNE_DIRTY and path is None:
        return
    f = path or _tune_file()
    try:
        os.makedirs(os.path.dirname(f) or ".", exist_ok=True)
        tmp = f + f".{os.getpid()}.tmp"
        with open(tmp, "w") as fh:
            json.dump(dict(igemm={repr(k): list(v) for k, v in _TUNE_CACHE.items()},
                           wgrad={repr(k): list(v) for k, v in _WTUNE_CACHE.items()}), fh, indent=0, sort_keys=True)
        os.replace(tmp, f)
        _TUNE_DIRTY = False
    except OSError:
        pass


TUNE_REPS = int(os.environ.get("RADET_TUNE_REPS", "3"))      # timed samples per candidate (the fastest counts)
# launches per sample, back to back between one pair of events: a single 30-60 us launch per sample carries 5-10 us of
# event / launch-gap jitter, more than the differences between the candidates
TUNE_BURST = max(1, int(os.environ.get("RADET_TUNE_BURST", "4")))


def _ntiles(t, m, n):
    bm, bn = TILE_SHAPE[tile_id(t)]
    return -(-m // bm) * -(-n // bn)


def _splitk_cands(t, m, n, nk):
    """short grids: t with explicit split-K factors (that leave >= 4 of its nk K stages per split) instead of the launcher's heuristic"""
    return [t | splitk(sk) for sk in (1, 2, 3, 4, 5, 6, 8) if nk // sk >= 4] if _ntiles(t, m, n) < 1024 else []


def autotune(g, need_dgrad=True, reps=None):
    """Pick the fastest (block tile, K step) of the implicit-GEMM kernel for this geometry by timing the
    candidates once (results cached per shape, so identical layers and identical models agree)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    reps = reps or TUNE_REPS

    def best_of(fn, cands):
        """fastest candidate: `reps` interleaved rounds over all candidates (clock / cache drift hits every candidate
        alike), each candidate scored by its fastest round"""
        for t in cands:
            fn(t)
        torch.cuda.synchronize()
        best = [float("inf")] * len(cands)
        for _ in range(reps):
            for i, t in enumerate(cands):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _b in range(TUNE_BURST):
                    fn(t)
                e.record()
                e.synchronize()
                best[i] = min(best[i], s.elapsed_time(e) / TUNE_BURST)
        return cands[min(range(len(cands)), key=lambda i: (best[i], i))]

    def cands(kdim, n, m, taps):
        tiles = [4] if n <= 32 else [1, 2, 3]
        c = [t for t in tiles]
        if kdim % 32 == 0:
            c += [t | BK32 for t in tiles]
        if getattr(g, "x3", False) and not g.math and not g.h16 and n > 32:
            # K-divided 64 x 64 tiles (the waves share the operand splits): K steps of 64 / 32 channels
            c += ([7] if kdim % 64 == 0 else []) + ([8] if kdim % 32 == 0 else [])
            if _h2key(g) and kdim % 32 == 0 and KW_DEEP:
                # fp16 hi / lo arithmetic: tile 8 with loads two / three stages ahead (16 KiB of LDS per stage)
                c += [8 | STAGES3, 8 | STAGES4]
        out = list(c)
        for t in c:
            ntiles = _ntiles(t, m, n)
            nk = taps * kdim // (64 if tile_id(t) == 7 else (32 if (t & BK32 or tile_id(t) == 8) else 16))
            out += _splitk_cands(t, m, n, nk)
            # stream-K (fp32 tensors, fp32 / bf16-rounded math is decided by the launcher's tag: fp32 only)
            if ntiles < 1024 and not g.math and not g.h16 and tile_id(t) in (2, 3, 4) and ntiles % 256:      # (not the K-divided tiles)
                out += [t | streamk(w) for w in (1, 2, 3, 4) if ntiles * nk >= 256 * w]
        return out

    global _TUNE_DIRTY, TUNE_RUNS
    key = (g._key, g.cin, g.cout, g.math, g.h16) + (("x3",) if getattr(g, "x3", False) else ()) + _h2key(g)
    if key not in _TUNE_CACHE:
        _TUNE_DIRTY = True
        TUNE_RUNS += 1
        dt = torch.bfloat16 if g.h16 else torch.float32
        x = torch.randn(g.lin.rows, g.cin, device=dev).to(dt)
        w = (torch.randn(g.cout * g.k * g.k * g.cin, device=dev) * 0.05).to(dt)
        y = torch.empty(g.lout.rows, g.cout, device=dev, dtype=dt)
        tmp_keys = _tune_slots(g, x, w, outputs=(y,))
        fc = cands(g.cin, g.cout, g.lout.rows, g.k * g.k)
        if not g.math and not g.h16:      # forward launches run alone on the device: 3 LDS stages may pay
            fc = fc + [t | STAGES3 for t in fc if tile_id(t) < 7 and not t & (STAGES3 | STAGES4)]
        ft = best_of(lambda t: conv_fwd(g, x, w, None, y, relu=True, tile=t), fc)
        bt = 0
        if need_dgrad and g.cout % 16 == 0:
            dx = torch.empty(g.lin.rows, g.cin, device=dev, dtype=dt)
            tmp_keys += _tune_slots(g, outputs=(dx,))
            # (no 3-stage candidates for dgrad: timed alone they win, next to the wgrad streams they lose -- a tune file
            # that allowed them made the step 1 % slower)
            bt = best_of(lambda t: conv_dgrad(g, y, w, dx, mask=x, tile=t), cands(g.cout, g.cin, g.lin.rows, g.k * g.k))
        _TUNE_CACHE[key] = (ft, bt)
        unregister_amax(tmp_keys)
        if os.environ.get("RADET_TUNE_LOG"):
            print(f"[tune igemm] M={g.lout.rows} {g.cin}->{g.cout} k{g.k}s{g.stride}: fwd tile={ft:#x} dgrad tile={bt:#x}")
    g.fwd_tile, g.bwd_tile = _TUNE_CACHE[key]
    if getattr(g, "pairs", False) and _h2key(g) and g.cin % 32 == 0:
        # forward launches whose x arrives as fp16 plane pairs (the producer's epilogue wrote them): the 4-wave plane tiles
        keyq = key + ("q",)
        if keyq not in _TUNE_CACHE:
            _TUNE_DIRTY = True
            TUNE_RUNS += 1
            x = torch.randn(g.lin.rows, g.cin, device=dev)
            w = torch.randn(g.cout * g.k * g.k, g.cin, device=dev) * 0.05
            xq, wq = Planes.from_float(x, kind="h2"), Planes.from_float(w, kind="h2")
            y = torch.empty(g.lout.rows, g.cout, device=dev)
            cq = [1, 2, 3, 1 | STAGES3, 2 | STAGES3, 3 | STAGES3] + ([7] if g.cin % 64 == 0 else [])
            for t in list(cq):
                cq += _splitk_cands(t, g.lout.rows, g.cout, g.k * g.k * g.cin // (64 if tile_id(t) == 7 else 32))
            ftq = best_of(lambda t: conv_fwd(g, xq, wq, None, y, relu=True, tile=t), cq)
            btq = 0
            if need_dgrad and g.stride == 1 and g.cout % 32 == 0:
                # ... and dgrad launches whose dy arrives as pairs (with the ReLU mask read from a pair tensor)
                dyq = Planes.from_float(torch.randn(g.lout.rows, g.cout, device=dev), kind="h2")
                wtq = Planes.from_float(torch.randn(g.cin * g.k * g.k, g.cout, device=dev) * 0.05, kind="h2")
                dx = torch.empty(g.lin.rows, g.cin, device=dev)
                tmp_q = _tune_slots(g, outputs=(dx,))
                cb = [1, 2, 3] + ([7] if g.cout % 64 == 0 else [])
                for t in list(cb):
                    cb += _splitk_cands(t, g.lin.rows, g.cin, g.k * g.k * g.cout // (64 if tile_id(t) == 7 else 32))
                btq = best_of(lambda t: conv_dgrad(g, dyq, wtq, dx, mask=xq, tile=t), cb)
                unregister_amax(tmp_q)
            _TUNE_CACHE[keyq] = (ftq, btq)
            if os.environ.get("RADET_TUNE_LOG"):
                print(f"[tune igemm pairs] M={g.lout.rows} {g.cin}->{g.cout} k{g.k}s{g.stride}: fwd tile={ftq:#x} dgrad tile={btq:#x}")
        g.fwd_tile_q, g.bwd_tile_q = _TUNE_CACHE[keyq]


KW_DEEP = os.environ.get("RADET_KW_DEEP", "1") != "0"


def _h2key(g):
    return ("h2",) if (getattr(g, "h2", False) and getattr(g, "x3", False) and not g.math and not g.h16) else ()


def _tune_slots(g, *tensors, outputs=()):
    """amax slots for the tuner's scratch tensors (fp16 hi / lo arithmetic): the operands' slots are MEASURED once (a constant
    would overflow fp16 for a K or an init whose sums leave its range), the outputs' start at zero and are raised by the timed
    launches' epilogues; registered by address, so that the timed launches do not each run a stand-alone absmax pass.
    Returns the registry keys."""
    keys = []
    if _h2key(g):
        for t in tensors:
            s = new_amax(t.device)
            if t.is_floating_point() and t.dtype == torch.float32 and t.is_contiguous() and t.numel() % 4 == 0:
                absmax(t, s)
            elif t.is_floating_point() and t.dtype == torch.float32:
                s.fill_(int(t.abs().max().view(torch.int32)) if t.numel() else 0)
            keys.append(register_amax(t, s))
        for t in outputs:
            t.zero_()                               # (an uninitialised output may hold NaN bit patterns: they must not be read back)
            keys.append(register_amax(t, new_amax(t.device)))
    return keys


# ---------------------------------------------------------------------- amax slots (fp16 hi / lo arithmetic, radet_hip.h)
# A slot is AMAX_WORDS (64) int32 words of device memory; its value -- the LARGEST word, read as the bit pattern of a float -- is
# >= every |element| of "its" tensor (64 words: thousands of waves raise a slot at once, include/radet_hip.h).  The
# engine registers the slots of its buffers here (activations by storage, so that row slices of a buffer resolve to the
# buffer's slot; weights by exact address, they are views of one arena); the conv launchers look the operands' slots up.
# A tensor without a slot (ad-hoc calls: tests, the autotuner) gets one computed on the spot by a stand-alone pass.
AMAX_WORDS = 64
_AMAX_EXACT = {}
_AMAX_STORAGE = {}


def new_amax(device, n=None):
    """a zeroed slot (int32 [radet_amax_slot_words()]), or n of them ([n, words])"""
    global AMAX_WORDS
    AMAX_WORDS = _lib.load().radet_amax_slot_words()
    return torch.zeros((AMAX_WORDS,) if n is None else (n, AMAX_WORDS), dtype=torch.int32, device=device)


def amax_value(slot):
    """the float a slot stands for (host synchronisation: tests / debugging)"""
    return float(slot.max().view(torch.float32))


def register_amax(t, slot, by_storage=False):
    """slot: a new_amax() tensor.  Returns the registry key (for unregister_amax).  The entry is only honoured while `t` is
    alive: the registry is keyed by device address, and the caching allocator hands a dead tensor's address to the next one."""
    import weakref
    if by_storage:
        k = ("s", t.untyped_storage().data_ptr())
        _AMAX_STORAGE[k[1]] = (slot, weakref.ref(t))
    else:
        k = ("e", t.data_ptr())
        _AMAX_EXACT[k[1]] = (slot, weakref.ref(t))
    return k


def _live(table, ptr):
    ent = table.get(ptr)
    if ent is None:
        return None
    if ent[1]() is None:                    # the registered tensor is gone: whoever lives at this address now is someone else
        del table[ptr]
        return None
    return ent


def unregister_amax(keys):
    for kind, ptr in keys:
        (_AMAX_STORAGE if kind == "s" else _AMAX_EXACT).pop(ptr, None)
    _AMAX_MEMO.clear()
    _SCALES.clear()


_AMAX_MEMO = {}


def amax_slot(t, compute=False):
    """the registered slot of tensor / Planes t (or of the buffer it is a slice of); None, or -- with compute=True -- a
    fresh slot filled by radet_absmax"""
    if t is None:
        return None
    if _isp(t):
        return t.amax
    p = t.data_ptr()
    ent = _live(_AMAX_EXACT, p)
    if ent is None:
        ent = _live(_AMAX_MEMO, p)
        if ent is None and _AMAX_STORAGE:
            ent = _live(_AMAX_STORAGE, t.untyped_storage().data_ptr())
            if ent is not None:
                _AMAX_MEMO[p] = ent         # (a row slice of a registered buffer: remembered by its own address)
    s = ent[0] if ent is not None else None
    if s is None and compute:
        s = new_amax(t.device)
        absmax(t, s)
    return s


def absmax(t, slot):
    """raise `slot` to the largest magnitude of the fp32 tensor t (contiguous, any element count)"""
    assert t.dtype == torch.float32 and t.is_contiguous()
    _lib.call("radet_absmax", _ptr(t), C.c_size_t(t.numel()), _ptr(slot), _stream())


_SCALES = _LRU(4096)


def _scales(x, w, y, x1=None, w1=None, y1=None, need=True, yq=None, wmeta=None, addend=None):
    """RadetScales for a launch (cached per slot combination).  need: the x / w slots are required (h2 arithmetic): missing
    ones are computed on the spot; otherwise only the output slot matters and None is returned when there is none.
    yq (Planes "h2"): the pair copy of the output, with wmeta = (w_l1 slot, bias amax slot or None) of the conv and the
    launch's addend (its slot bounds the residual term)."""
    sx, sw, sy = amax_slot(x, need), amax_slot(w, need), amax_slot(y)
    if y is None and yq is not None:       # pairs-only output: the slot of its TRUE largest magnitude is still raised
        sy = getattr(yq, "true_amax", None)
    sx1, sw1, sy1 = amax_slot(x1, need), amax_slot(w1, need), amax_slot(y1)
    if not need and sy is None and sy1 is None and yq is None:
        return None
    ext = (None,) * 6
    if yq is not None:
        xt = getattr(x, "true_amax", None) if _isp(x) else amax_slot(x, True)
        assert xt is not None and wmeta is not None, "pair copy of a conv output: the true amax slot of x and the conv's L1 slot"
        ext = (yq.t, yq.amax, xt, wmeta[0], wmeta[1], amax_slot(addend, True) if addend is not None else None)
    slots = (sx, sw, sy, sx1, sw1, sy1) + ext
    key = tuple(0 if t is None else t.data_ptr() for t in slots)
    ent = _SCALES.get(key)
    if ent is None:
        sc = _lib.RadetScales(*[None if v == 0 else v for v in key])
        ent = _SCALES[key] = (C.byref(sc), sc, slots)              # (the struct and the slots stay alive with it)
    return ent[0]


class Planes:
    """A [rows, C] fp32 tensor in the operand format of the conv GEMMs (include/radet_hip.h).  kind "b3": bf16 plane triples,
    `t` is a bf16 tensor [rows, 3 * C] whose row r holds hi | mid | lo with hi + mid + lo == the fp32 value exactly.
    kind "h2": fp16 plane pairs, `t` is an fp16 tensor [rows, 2 * C] (32-channel groups [hi | lo]) of the values scaled by
    the power of two of `amax` (the tensor's amax slot, see new_amax).  Only the conv GEMMs read it."""

    def __init__(self, rows, C, device=None, t=None, kind="b3", amax=None):
        self.rows, self.C, self.kind = int(rows), int(C), kind
        if t is None:
            t = (torch.empty(self.rows, 2 * self.C, device=device, dtype=torch.float16) if kind == "h2"
                 else torch.empty(self.rows, 3 * self.C, device=device, dtype=torch.bfloat16))
        self.t = t
        self.amax = amax
        if kind == "h2" and amax is None:
            self.amax = new_amax(t.device)

    def __getitem__(self, sl):
        assert isinstance(sl, slice) and sl.step in (None, 1)
        v = self.t[sl]
        return Planes(v.shape[0], self.C, t=v, kind=self.kind, amax=self.amax)

    def data_ptr(self):
        return self.t.data_ptr()

    def to_float(self):
        out = torch.empty(self.rows, self.C, device=self.t.device)
        merge_planes(self, out)
        return out

    @staticmethod
    def from_float(x, kind="b3"):
        p = Planes(x.shape[0], x.shape[1], device=x.device, kind=kind)
        split_planes(x, p)
        return p


def _isp(t):
    return isinstance(t, Planes)


def _ptr_any(t):
    return _ptr(t.t) if _isp(t) else _ptr(t)


def split_planes(src, dst, src_amax=None):
    """dst (Planes) = plane split of the 2-D fp32 tensor src (row stride may exceed the width): exact bf16 triples, or fp16
    pairs scaled by the power of two of src's amax slot (src_amax, else the registered one, else computed here)"""
    assert src.dim() == 2 and src.dtype == torch.float32 and src.stride(1) == 1 and dst.C == src.shape[1]
    if dst.kind == "h2":
        sa = src_amax if src_amax is not None else amax_slot(src)
        if sa is None:
            sa = new_amax(src.device)
            absmax(src.contiguous(), sa)
        _lib.call("radet_split_pairs", src.data_ptr(), _ptr(dst.t), C.c_size_t(src.shape[0]), src.shape[1], src.stride(0),
                  _ptr(sa), _ptr(dst.amax), _stream())
        return
    _lib.call("radet_split_planes", C.c_void_p(src.data_ptr()), _ptr(dst.t), C.c_size_t(src.shape[0]), src.shape[1],
              src.stride(0), _stream())


def merge_planes(src, dst):
    assert dst.dim() == 2 and dst.dtype == torch.float32 and dst.stride(1) == 1 and src.C == dst.shape[1]
    if src.kind == "h2":
        _lib.call("radet_merge_pairs", _ptr(src.t), dst.data_ptr(), C.c_size_t(dst.shape[0]), dst.shape[1], dst.stride(0),
                  _ptr(src.amax), _stream())
        return
    _lib.call("radet_merge_planes", _ptr(src.t), C.c_void_p(dst.data_ptr()), C.c_size_t(dst.shape[0]), dst.shape[1],
              dst.stride(0), _stream())


def _is16(t):
    return t is not None and not _isp(t) and t.dtype == torch.bfloat16


def _tile(g, tile, default, x=None, y=None):
    """tile_override word: explicit or tuned tile + arithmetic mode flags, derived from the tensors' dtypes"""
    t = (tile or default) | (MATH_BF16 if g.math else 0)
    if _isp(x):                                          # plane operands: BK32 (the fp32 paths' K-step bit) has no meaning here
        if tile_id(t) == 8:                              # (tile 8 splits in registers: fp32 operands only; tile 7 has a pair reader)
            t = with_tile(t, 3)
        return (t & ~(MATH_BF16 | BK32)) | P3 | (H2 if x.kind == "h2" else 0)
    if getattr(g, "x3", False) and not g.math and not _is16(x):
        t |= X3 | (H2 if getattr(g, "h2", False) else 0)
    if _is16(x):
        t = (t & ~MATH_BF16) | STORE_BF16 | (OUT_F32 if (y is not None and y.dtype == torch.float32) else 0)
    return t


def conv_fwd(g, x, wf, bias, y, addend=None, mask=None, relu=False, tile=0, splitk=True, yq=None, wmeta=None):
    """yq (Planes "h2", optional): y once more as fp16 plane pairs, scaled by the bound the launch can form before it starts
    (include/radet_hip.h RadetScales.yq); wmeta = (w_l1 slot, bias amax slot) of the conv, from the fold.  y = None with a
    yq: the output exists ONLY as pairs (round 6: tensors that nothing but conv GEMMs and ReLU masks read)"""
    assert y is not None or yq is not None
    tile = _tile(g, tile, g.fwd_tile, x, y)
    ws = splitk_ws() if splitk else None
    table = g.fwd_table
    sc = _scales(x, wf, y, need=bool(tile & H2), yq=yq, wmeta=wmeta, addend=addend)

    def launch():
        _lib.call("radet_conv2d_igemm_s", _ptr_any(x), _ptr_any(wf), _ptr(bias), _ptr(addend), _ptr(mask), _ptr(y), _ptr(table),
                  g.lout.rows, g.cin, g.cout, g.k, g.k, int(relu), tile, _ptr(ws), C.c_size_t(ws.numel() if splitk else 0),
                  _stream(), sc)
    _timed(lambda: _igemm_key(tile, x), 2.0 * g.lout.rows * g.cout * g.cin * g.k * g.k, launch, _conv_bytes(g), geom=g)


def _pred_tiles(lv):
    """8 x 16 output blocks of every (level, image) of the pyramid `lv` for radet_pred3x3_patch (built once per Levels)."""
    import numpy as np
    t = getattr(lv, "_pred_tiles", None)
    if t is None:
        rows = []
        for (h, w), off in zip(lv.hw, lv.offsets):
            for n in range(lv.B):
                for ty in range(-(-h // 8)):
                    for tx in range(-(-w // 16)):
                        rows.append((off + n * h * w, h, w, (ty << 16) | tx))
        t = torch.from_numpy(np.asarray(rows, np.int32)).cuda()
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream().synchronize()
        lv._pred_tiles = t
    return t


def pred_conv_patch(lv, x, a, b=None):
    """Predictor 3x3 convs from an LDS patch: a, b = (wf [c][9][Cin], bias, y [rows][c], c); b shares a's input."""
    t = _pred_tiles(lv)
    cin = x.shape[1]
    w1, b1, y1, c1 = b if b is not None else (None, None, None, 0)
    _timed("pred3x3_patch_kernel", 2.0 * lv.rows * (a[3] + c1) * cin * 9,
           lambda: _lib.call("radet_pred3x3_patch", _ptr(x), cin, _ptr(t), t.shape[0], _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), a[3],
                             _ptr(w1), _ptr(b1), _ptr(y1), c1, _stream()))


_WTUNE_CACHE = _LRU(8192)


def autotune_wgrad(g, reps=None):
    """Pick (tile, pixel splits S) of the one-tap wgrad kernel for this geometry: time the candidates and charge each
    split its downstream cost (a weight-sized slab is written here and read again by unfold: ~2 * 4 B / weight at
    ~3 TB/s).  Must run before the slab buffers are sized (it changes g.nsplit)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    reps = reps or TUNE_REPS
    global _TUNE_DIRTY, TUNE_RUNS
    key = (g._key, g.cin, g.cout, g.math, g.h16, "w") + (("x3",) if getattr(g, "x3", False) else ()) + _h2key(g)
    if key not in _WTUNE_CACHE:
        _TUNE_DIRTY = True
        TUNE_RUNS += 1
        M, kk = g.lout.rows, g.k * g.k
        s0 = g.nsplit
        cands = [(0, s0)]
        if g.cout > 64 and g.cin > 64:
            for tid in (1, 2, 3) if getattr(g, "x3", False) else (1, 2):   # (3, 128 x 64, plane arithmetic only: fewer operand splits per MFMA block)
                tflag, (t, tn) = tid * WG_TILE, WG_TILE_SHAPE[tid]
                tiles = -(-g.cout // t) * -(-g.cin // tn) * kk
                for blocks in (256, 512, 768, 1024):
                    S = max(1, min(64, round(blocks / tiles), (M + 127) // 128))
                    cands.append((tflag | WG_ONE_TAP, S))
                    if not g.math and not g.h16:
                        cands.append((tflag | WG_ONE_TAP | WG_PX32, S))
                    if getattr(g, "x3", False) and t == 64:
                        # the waves divide the pixels of a stage (64 four ways / 32 two ways) and share the operand splits
                        cands += [(tflag | WG_ONE_TAP | WG_KDIV4, S), (tflag | WG_ONE_TAP | WG_KDIV2, S)]
        cands = sorted(set(cands))
        dt = torch.bfloat16 if g.h16 else torch.float32
        dy = torch.randn(M, g.cout, device=dev).to(dt)
        x = torch.randn(g.lin.rows, g.cin, device=dev).to(dt)
        tmp_keys = _tune_slots(g, dy, x)
        slabs = torch.empty(max(c[1] for c in cands) * g.cout * kk * g.cin, device=dev)
        for fl, S in cands:
            g.wgrad_flags, g.nsplit = fl, S
            conv_wgrad(g, dy, x, slabs)
        torch.cuda.synchronize()
        tbest = [float("inf")] * len(cands)
        for _ in range(reps):
            for i, (fl, S) in enumerate(cands):
                g.wgrad_flags, g.nsplit = fl, S
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _b in range(TUNE_BURST):
                    conv_wgrad(g, dy, x, slabs)
                e.record()
                e.synchronize()
                tbest[i] = min(tbest[i], s.elapsed_time(e) / TUNE_BURST)
        best = None
        for (fl, S), t in zip(cands, tbest):
            cost = t + S * g.cout * kk * g.cin * 8 / 3e12 * 1e3
            if best is None or cost < best[0]:
                best = (cost, fl, S)
        _WTUNE_CACHE[key] = best[1:]
        unregister_amax(tmp_keys)
        if os.environ.get("RADET_TUNE_LOG"):
            print(f"[tune wgrad] M={M} {g.cin}->{g.cout} k{g.k}s{g.stride}: heuristic S={s0} -> flags={best[1]:#x} S={best[2]} "
                  f"({best[0] * 1e3:.1f} us incl. slab cost)")
    g.wgrad_flags, g.nsplit = _WTUNE_CACHE[key]


def conv_fwd_pair(g, a, b, relu=False, tile=0):
    """a, b: dicts(x, w, bias, addend, mask, y) -- two convs of geometry g in one launch."""
    ws = splitk_ws()
    q = lambda d: [_ptr_any(d.get(k)) for k in ("x", "w", "bias", "addend", "mask", "y")]  # noqa: E731
    t, table = _tile(g, tile, g.fwd_tile, a["x"], a["y"]), g.fwd_table
    sc = _scales(a["x"], a["w"], a["y"], b["x"], b["w"], b["y"], need=bool(t & H2))
    _timed(lambda: _igemm_key(t, a["x"]), 4.0 * g.lout.rows * g.cout * g.cin * g.k * g.k,
           lambda: _lib.call("radet_conv2d_igemm_pair_s", *q(a), *q(b), _ptr(table), g.lout.rows, g.cin, g.cout, g.k, g.k,
                             int(relu), t, _ptr(ws), C.c_size_t(ws.numel()), _stream(), sc), _conv_bytes(g, 2))


def conv_dgrad_pair(g, a, b, tile=0):
    """a, b: dicts(x=dy, w=wft, addend, mask, y=dx) -- two stride-1 dgrads of geometry g in one launch."""
    assert g.stride == 1
    ws = splitk_ws()
    q = lambda d: [_ptr_any(d.get(k)) for k in ("x", "w", "bias", "addend", "mask", "y")]  # noqa: E731
    t, table = _tile(g, tile, g.bwd_tile, a["x"], a["y"]), g.bwd_table
    sc = _scales(a["x"], a["w"], a["y"], b["x"], b["w"], b["y"], need=bool(t & H2))
    _timed(lambda: _igemm_key(t, a["x"]), 4.0 * g.lin.rows * g.cout * g.cin * g.k * g.k,
           lambda: _lib.call("radet_conv2d_igemm_pair_s", *q(a), *q(b), _ptr(table), g.lin.rows, g.cout, g.cin, g.k, g.k, 0,
                             t, _ptr(ws), C.c_size_t(ws.numel()), _stream(), sc), _conv_bytes(g, 2), kind="dgrad")


def conv_dgrad(g, dy, wft, dx, addend=None, mask=None, k_channels=None, tile=0, splitk=True, skip_zero_rows=False,
               yq=None, wmeta=None):
    """dx[rows_in, cin] = dgrad(dy[rows_out, k_channels]); k_channels = (padded) channel count of dy/wft.
    skip_zero_rows: the caller accumulates in place (addend is dx) with a mask already applied to dx, so the
    input positions a strided conv never touches (3/4 of them for a 1x1 / 2) are left alone instead of being
    rewritten by an epilogue-only launch.
    mask may be a Planes "h2" (the ReLU mask of an activation that exists only as pairs).  yq (Planes "h2") with wmeta =
    (w_l1t slot, None): dx as fp16 plane pairs scaled by amax(dy) * the weights' largest input-channel L1 norm; dx = None:
    only as pairs (stride-1 convs)."""
    kc = g.cout if k_channels is None else k_channels
    tile = _tile(g, tile, (g.bwd_tile_q if _isp(dy) and getattr(g, "bwd_tile_q", 0) else g.bwd_tile), dy, dx)
    if _isp(mask):
        tile |= MASKQ
    assert dx is not None or (yq is not None and g.stride == 1)
    ws = splitk_ws() if splitk else None
    if EVENTS is not None:
        # algorithmic work of the dgrad = that of the forward conv (a strided conv's dgrad touches each weight tap once
        # per output pixel; the padded K of the small predictor heads is not counted)
        real_k = min(kc, g.cout)
        _timed(_igemm_key(tile, dy) + (" [strided dgrad, class launch]" if g.stride > 1 else ""),
               2.0 * g.lout.rows * real_k * g.cin * g.k * g.k,
               lambda: _conv_dgrad(g, dy, wft, dx, addend, mask, kc, tile, ws, splitk, skip_zero_rows, yq, wmeta),
               _conv_bytes(g), kind="dgrad", geom=g)
        return
    _conv_dgrad(g, dy, wft, dx, addend, mask, kc, tile, ws, splitk, skip_zero_rows, yq, wmeta)


def _conv_dgrad(g, dy, wft, dx, addend, mask, kc, tile, ws, splitk, skip_zero_rows, yq=None, wmeta=None):
    # (a K that cannot be split into planes -- the 16-channel padded gradient of the reg / iou predictors -- runs on the
    # native fp32 MFMA inside the launcher and needs no operand slots)
    sc = _scales(dy, wft, dx, need=bool(tile & H2) and (_isp(dy) or kc % 32 == 0), yq=yq, wmeta=wmeta, addend=addend)
    if g.stride > 1 and STRIDED_DGRAD_CLASSES:
        assert yq is None and not _isp(mask) and not _isp(dy), "strided dgrad: fp32 tensors only"
        grp = _strided_dgrad_group(g)
        if grp is not None:
            _lib.call("radet_conv2d_igemm_classes_s", _ptr(dy), _ptr(wft), _ptr(addend), _ptr(mask), _ptr(dx),
                      _ptr(grp["table"]), _ptr(grp["out_rows"]), grp["tap_ids"], grp["ntaps"], grp["start"], grp["ncls"],
                      g.k * g.k, grp["M"], kc, g.cin, tile, _ptr(ws), C.c_size_t(ws.numel() if splitk else 0), _stream(), sc)
        for c in _strided_dgrad_classes(g):
            if grp is not None and not c["zero"]:
                continue
            if c["zero"] and skip_zero_rows:
                assert addend is not None and addend.data_ptr() == dx.data_ptr()
                continue
            # rows that receive no tap at all only need the epilogue: one 16-deep stage over an all-(-1) table (a K-divided
            # tile needs 32 / 64 channels per stage: the plain 64 x 64 tile instead, no split-K)
            ct = with_tile(tile, 3) if (c["zero"] and tile_id(tile) >= 7) else tile
            _lib.call("radet_conv2d_igemm_taps_s", _ptr(dy), _ptr(wft), _ptr(addend), _ptr(mask), _ptr(dx), _ptr(c["table"]),
                      _ptr(c["out_rows"]), c["tap_ids"], c["ntaps"], g.k * g.k, c["rows"],
                      (32 if _is16(dy) else 16) if c["zero"] else kc, g.cin,
                      ct, _ptr(ws), C.c_size_t(ws.numel() if splitk else 0), _stream(), sc)
        return
    _lib.call("radet_conv2d_igemm_s", _ptr_any(dy), _ptr_any(wft), None, _ptr(addend), _ptr_any(mask), _ptr(dx), _ptr(g.bwd_table),
              g.lin.rows, kc, g.cin, g.k, g.k, 0, tile, _ptr(ws), C.c_size_t(ws.numel() if splitk else 0), _stream(), sc)


# all-taps weight gradient on fp16 plane pairs, unit-stride 3 x 3 convs: RADET_WGRAD9_WINDOWS=1 selects conv_wgrad9r_kernel (x as
# shifted windows of three row segments, every tile load a whole cache line: 15 instead of 26 KiB and 118 lines instead of 416
# half lines of LDS fill per 16 pixels; bit-identical results) -- built, tested, and SLOWER (167 against 107-117 us on the tower
# shape: neither the bytes nor the number of requests bound conv_wgrad9q_kernel), so off by default
WGRAD9_WINDOWS = os.environ.get("RADET_WGRAD9_WINDOWS", "0") == "1"
# ... RADET_WGRAD9_DEEP=1 selects conv_wgrad9d_kernel: conv_wgrad9q_kernel with five stage buffers, the loads four 16-pixel stages
# ahead, the gather table of the pixel split in LDS; bit-identical results.  4-9 % faster alone (91 against 95 us on the tower
# shape, 105 against 115 with bias sums), 0.3-0.5 % SLOWER in the step: its 159 KiB of LDS leave no room for a dgrad workgroup
# on the same CU (the two-buffer kernel: 104 KiB).  Off by default
WGRAD9_DEEP = os.environ.get("RADET_WGRAD9_DEEP", "0") == "1"


def _wgrad_key(g, dy, co):
    def onetap(fl):
        tile = ("launcher tile" if not wg_tile(fl) else "%d, %d" % WG_TILE_SHAPE[wg_tile(fl)]) if co > 32 else "32, 128"
        kd = ", 64 px / 4 waves" if fl & WG_KDIV4 else (", 32 px / 2 waves" if fl & WG_KDIV2 else "")
        return tile, (", 32 px" if fl & WG_PX32 else "") + kd

    if _isp(dy):
        if dy.kind == "h2" and (g.k != 3 or g.wgrad_pair_flags & WG_ONE_TAP):
            return f"conv_wgradq_kernel<{'128, 128' if wg_tile(g.wgrad_pair_flags) == 1 else '64, 64'}> (fp16 plane pairs)"
        if dy.kind == "h2":
            if g.stride == 1 and g.pad == 1 and WGRAD9_DEEP and -(-g.lout.rows // (16 * (g.nsplit_pairs or g.nsplit))) * 16 <= 1664:
                return "conv_wgrad9d_kernel"
            return "conv_wgrad9r_kernel" if (g.stride == 1 and g.pad == 1 and WGRAD9_WINDOWS) else "conv_wgrad9q_kernel"
        return "conv_wgrad9p_kernel"
    tile, px = onetap(g.wgrad_flags)
    if getattr(g, "h2", False) and getattr(g, "x3", False) and not g.math and not _is16(dy):
        return f"conv_wgradg_kernel<{tile}> (fp16 hi/lo in registers{px})"
    nine = g.k == 3 and g.cin % 32 == 0 and co >= 256 and g.lout.rows >= 16384 and not (g.wgrad_flags & WG_ONE_TAP)
    mode = "bf16 storage" if _is16(dy) else ("bf16 math" if g.math else ("planes in registers" if getattr(g, "x3", False) else "fp32 MFMA"))
    if nine:
        return f"conv_wgrad9{'h' if _is16(dy) else 'g'}_kernel ({mode})"
    return f"conv_wgrad{'h' if _is16(dy) else 'g'}_kernel<{tile}> ({mode}{px})"


def conv_wgrad(g, dy, x, slabs, dbias_partials=None, cout=None, ld_dy=None):
    if EVENTS is not None:
        co_ = g.cout if cout is None else cout
        _timed(_wgrad_key(g, dy, co_), 2.0 * g.lout.rows * co_ * g.cin * g.k * g.k,
               lambda: _conv_wgrad(g, dy, x, slabs, dbias_partials, cout, ld_dy),
               4.0 * (g.lout.rows * co_ + g.lin.rows * g.cin + g.nsplit * co_ * g.k * g.k * g.cin), kind="wgrad", geom=g)
        return
    _conv_wgrad(g, dy, x, slabs, dbias_partials, cout, ld_dy)


def _conv_wgrad(g, dy, x, slabs, dbias_partials=None, cout=None, ld_dy=None):
    co = g.cout if cout is None else cout
    if _isp(dy):
        assert _isp(x) and x.kind == dy.kind
        if dy.kind == "h2":
            # all nine taps per workgroup for 3 x 3 convs unless the geometry's flags ask for the one-tap pair kernel (WG_ONE_TAP;
            # WG_TILE = its tile), which also serves every other kernel size
            nine = g.k == 3 and not (g.wgrad_pair_flags & WG_ONE_TAP)
            fl = WG_H2 | WG_P3 | (g.wgrad_pair_flags if nine else (WG_ONE_TAP | (g.wgrad_pair_flags & WG_TILE_MASK)))
            if nine and g.stride == 1 and g.pad == 1:       # unit stride, padding 1 (what the two kernels below rely on)
                fl |= (WG_DEEP if WGRAD9_DEEP else 0) | (WG_WINDOWS if WGRAD9_WINDOWS else 0)
            _lib.call("radet_conv2d_wgrad_s", _ptr(dy.t), _ptr(x.t), _ptr(slabs), _ptr(dbias_partials), _ptr(g.fwd_table),
                      g.lout.rows, g.cin, co, co if ld_dy is None else ld_dy, g.k, g.k,
                      g.nsplit_pairs or g.nsplit, fl, _stream(), _scales(dy, x, None))
            return
        _lib.call("radet_conv2d_wgrad", _ptr(dy.t), _ptr(x.t), _ptr(slabs), _ptr(dbias_partials), _ptr(g.fwd_table), g.lout.rows,
                  g.cin, co, co if ld_dy is None else ld_dy, g.k, g.k, g.nsplit, WG_P3 | (g.wgrad_flags & WG_ONE_TAP), _stream())
        return
    if getattr(g, "h2", False) and getattr(g, "x3", False) and not g.math and not _is16(dy):
        # fp16 hi / lo arithmetic on fp32 tensors: one-tap tiles only (an accumulator pair per tap does not fit the all-taps
        # tile); WG_ONE_TAP keeps the launcher away from it for the geometries the tuner has not seen
        _lib.call("radet_conv2d_wgrad_s", _ptr(dy), _ptr(x), _ptr(slabs), _ptr(dbias_partials), _ptr(g.fwd_table), g.lout.rows,
                  g.cin, co, co if ld_dy is None else ld_dy, g.k, g.k, g.nsplit, WG_H2 | WG_ONE_TAP | g.wgrad_flags, _stream(),
                  _scales(dy, x, None))
        return
    _lib.call("radet_conv2d_wgrad", _ptr(dy), _ptr(x), _ptr(slabs), _ptr(dbias_partials), _ptr(g.fwd_table), g.lout.rows,
              g.cin, co, co if ld_dy is None else ld_dy, g.k, g.k, g.nsplit,
              (WG_STORE_BF16 if _is16(dy) else (WG_MATH_BF16 if g.math else (WG_X3 if getattr(g, "x3", False) else 0))) | g.wgrad_flags, _stream())


def conv_wgrad_group(jobs, tile=128, math=0):
    """jobs: list of dict(g=ConvGeom, dy, x, slabs, dbias) -- one grouped launch per <= 32 jobs (longest first)."""
    jobs = sorted(jobs, key=lambda j: -(j["g"].lout.rows // j["g"].nsplit))
    for i in range(0, len(jobs), 32):
        part = jobs[i:i + 32]
        arr = (_lib.RadetWgradJob * len(part))()
        for a, j in zip(arr, part):
            g = j["g"]
            a.dy, a.x, a.slabs = _ptr(j["dy"]), _ptr(j["x"]), _ptr(j["slabs"])
            a.dbias_partials, a.gather_table = _ptr(j.get("dbias")), _ptr(g.fwd_table)
            a.M, a.Cin, a.Cout, a.ld_dy, a.KH, a.KW, a.S = g.lout.rows, g.cin, g.cout, g.cout, g.k, g.k, g.nsplit
        _lib.call("radet_conv2d_wgrad_group", arr, len(part), (WG_MATH_BF16 if math else 0) | (1 if tile == 128 else 2) * WG_TILE, _stream())


def group_splits(geoms, tile=128, slots=512):
    """Pixel splits S per conv of one wgrad group: S = round(M / px) with the pixel target px chosen so that the group's
    workgroup count fills `slots` resident workgroups (2 per CU) in whole rounds; ties -> fewer splits (fewer slabs)."""
    best = None
    for px in (6400, 4800, 3200, 2400, 1600, 1200, 800, 600, 400):
        S = [max(1, min(64, round(g.lout.rows / px), (g.lout.rows + 127) // 128)) for g in geoms]
        blocks = sum((g.cout // tile) * (g.cin // tile) * g.k * g.k * s for g, s in zip(geoms, S))
        eff = blocks / (slots * -(-blocks // slots))
        cost = -eff + 0.02 * sum(S) / len(S)            # every split is a slab written here and read by the reduction
        if best is None or cost < best[0] - 1e-9:
            best = (cost, S)
    return best[1]


def fold_weights(table_dev, n):
    _lib.call("radet_fold_weights", _ptr(table_dev), n, _stream())


def unfold_grads(table_dev, n, max_cout):
    _lib.call("radet_unfold_grads", _ptr(table_dev), n, max_cout, _stream())


def _layer(t):
    """(flag word, amax slot address) for the tensor t a layer kernel writes: its registered slot is raised; bf16 storage has none"""
    return (LAYER_BF16, None) if _is16(t) else (0, _ptr(amax_slot(t)))


def stem(img, wf, bias, y, B, H, W):
    ho, wo = (H + 1) // 2, (W + 1) // 2
    flags, sl = _layer(y)
    fn = lambda: _lib.call("radet_stem_conv_bn_relu", _ptr(img), _ptr(wf), _ptr(bias), _ptr(y), B, H, W, flags, sl, _stream())  # noqa: E731
    _timed("stem_kernel", 2.0 * B * ho * wo * 64 * 147, fn, 4.0 * (B * 3 * H * W + 64 * 147 + B * ho * wo * 64))


def convert_rows(src, dst, ncols=None, src_off=0, dst_off=0):
    """dst[:, dst_off:dst_off+ncols] = src[:, src_off:src_off+ncols] across fp32 <-> bf16 (2-D row-major tensors)"""
    assert src.dim() == 2 and dst.dim() == 2 and src.shape[0] == dst.shape[0] and src.dtype != dst.dtype
    n = src.shape[1] if ncols is None else ncols
    _lib.call("radet_convert_rows", _ptr(src), _ptr(dst), C.c_size_t(src.shape[0]), n, src.stride(0), src_off,
              dst.stride(0), dst_off, 1 if dst.dtype == torch.bfloat16 else 0, _stream())


def maxpool(x, y, B, H, W, Cch, yq=None):
    """yq (Planes "h2", optional, fp32 x only): the output once more as plane pairs, scaled by x's amax slot"""
    flags, sl = _layer(y)
    q = (None, None, None) if yq is None else (_ptr(yq.t), _ptr(yq.amax), _ptr(amax_slot(x, True)))
    _lib.call("radet_maxpool3x3s2", _ptr(x), _ptr(y), B, H, W, Cch, flags | (LAYER_PAIRS if yq is not None else 0), sl, *q,
              _stream())


def maxpool_bwd_relu(s, dpool, ds, B, H, W, Cch):
    """ds = [s > 0] * max-pool backward of dpool (s = the stem's ReLU output [B*H*W, C], fp32)"""
    _lib.call("radet_maxpool3x3s2_bwd_relu", _ptr(s), _ptr(dpool), _ptr(ds), B, H, W, Cch, _stream())


def stem_wgrad_splits(B, H, W):
    return _lib.load().radet_stem_wgrad_splits(B, H, W)


def stem_wgrad(img, ds, slabs, dbias_partials, B, H, W, S):
    """slabs[S][64][49][3], dbias_partials[S][64] from the NCHW image and the stem's pre-activation gradient"""
    _lib.call("radet_stem_wgrad", _ptr(img), _ptr(ds), _ptr(slabs), _ptr(dbias_partials), B, H, W, S, _stream())


def gn_ws_floats(levels):
    d, n = _desc([(h, w, h, w, o, o) for (h, w), o in zip(levels.hw, levels.offsets)])
    return _lib.load().radet_gn_workspace_floats(levels.B, d, n)


def _gn_desc(levels):
    return _desc([(h, w, h, w, o, o) for (h, w), o in zip(levels.hw, levels.offsets)])


class GnFwd(collections.namedtuple("GnFwd", "z gamma beta stats ws y planes zhat_amax", defaults=(None, None, None))):
    """One tensor of a GroupNorm + ReLU forward launch.  z: fp32 or bf16 rows; stats / ws: its statistics and workspace.  Outputs: y
    (tensor of z's type or None) and / or planes (Planes or None, fp32 z only; kind "h2": scaled by a bound on |y| that is
    written to planes.amax).  zhat_amax: slot raised to the largest |zhat| (the backward's bound on dz uses it)."""
    __slots__ = ()

    def pointers(self):
        pl = self.planes
        return (_ptr(self.z), _ptr(self.gamma), _ptr(self.beta), _ptr(self.y), _ptr_any(pl), _ptr(self.stats), _ptr(self.ws),
                None if _is16(self.z) else _ptr(amax_slot(self.y)), None if pl is None else _ptr(pl.amax), _ptr(self.zhat_amax))


def _gn_flags(z, *planes):
    """RADET_LAYER_* word of a GroupNorm launch: bf16 storage from the tensor's dtype, pairs from the kind of its plane outputs"""
    kinds = {pl.kind for pl in planes if pl is not None}
    assert len(kinds) <= 1, "one launch writes bf16 plane triples or fp16 plane pairs, not both"
    return (LAYER_BF16 if _is16(z) else 0) | (LAYER_PAIRS if "h2" in kinds else 0)


def gn_relu_fwd(levels, a, b=None, eps=1e-5, relu=True):
    """GroupNorm + ReLU of the GnFwd a -- and of b, a second tensor of the same geometry, in the same pair of launches.  The amax
    slot registered for an fp32 y is raised whatever else the launch writes (the engine registers activation slots only under the
    fp16 hi / lo arithmetic, whose conv GEMMs read them)."""
    d, n = _gn_desc(levels)
    _lib.call("radet_gn_relu_fwd", *a.pointers(), *(b.pointers() if b is not None else (None,) * 10), levels.B, 256, 32, eps,
              int(relu), _gn_flags(a.z, a.planes, b.planes if b is not None else None), d, n, _stream())


def gn_relu_bwd(levels, dy, z, stats, gamma, beta, dgamma, dbeta, ws, *, dz=None, planes=None, zhat_amax=None, dy_amax=None,
                relu=True):
    """dz as a tensor of dy's type (or None) and / or as Planes (or None, fp32 only).  Planes of kind "h2" are scaled by a bound
    built from dy's amax slot -- dy_amax, else the registered one, else computed here -- and zhat_amax (the forward's); the bound
    goes to planes.amax.  The outputs are keyword-only: ten positional arguments in the earlier order (dz, dgamma, dbeta, ws)
    are a TypeError, not a launch that takes the workspace for dz."""
    d, n = _gn_desc(levels)
    flags = _gn_flags(dy, planes)
    if dy_amax is None and flags & LAYER_PAIRS:
        dy_amax = amax_slot(dy, compute=True)
    _lib.call("radet_gn_relu_bwd", _ptr(dy), _ptr(z), _ptr(stats), _ptr(gamma), _ptr(beta), _ptr(dz), _ptr_any(planes),
              _ptr(dgamma), _ptr(dbeta), _ptr(ws), levels.B, 256, 32, int(relu), flags, d, n, _stream(), _ptr(dy_amax),
              _ptr(zhat_amax), None if planes is None else _ptr(planes.amax))


def upsample_add(dst, src, B, ho, wo, hi, wi, ch):
    flags, sl = _layer(dst)
    _lib.call("radet_upsample_add", _ptr(dst), _ptr(src), B, ho, wo, hi, wi, ch, flags, sl, _stream())


def upsample_add_bwd(dsrc, ddst, B, ho, wo, hi, wi, ch):
    flags, sl = _layer(dsrc)
    _lib.call("radet_upsample_add_bwd", _ptr(dsrc), _ptr(ddst), B, ho, wo, hi, wi, ch, flags, sl, _stream())


def relu_bwd(dy, addend, act, dx):
    flags, sl = _layer(dx)
    _lib.call("radet_relu_bwd", _ptr(dy), _ptr(addend), _ptr(act), _ptr(dx), C.c_size_t(dx.numel()), flags, sl, _stream())


def nchw_to_nhwc(x, y, B, ch, H, W):
    """module-API boundary (fp32 NCHW in); a bf16 row buffer is filled through an fp32 staging tensor"""
    if _is16(y):
        tmp = torch.empty(y.shape, device=y.device, dtype=torch.float32)
        _lib.call("radet_nchw_to_nhwc", _ptr(x), _ptr(tmp), B, ch, H, W, _stream())
        convert_rows(tmp.view(-1, ch), y.view(-1, ch))
        return
    _lib.call("radet_nchw_to_nhwc", _ptr(x), _ptr(y), B, ch, H, W, _stream())
    sl = amax_slot(y)
    if sl is not None:                                 # data entering an engine buffer from outside: its amax slot follows
        absmax(y, sl)


def nhwc_to_nchw(x, y, B, ch, H, W):
    """module-API boundary (fp32 NCHW out)"""
    if _is16(x):
        tmp = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        convert_rows(x.reshape(-1, ch), tmp.view(-1, ch))
        x = tmp
    _lib.call("radet_nhwc_to_nchw", _ptr(x), _ptr(y), B, ch, H, W, _stream())


def level_desc(levels, strides):
    flat = []
    for (h, w), s in zip(levels.hw, strides):
        flat += [h, w, int(s)]
    return (C.c_int * len(flat))(*flat), len(levels.hw)


def head_loss_ws_ints(R):
    return _lib.load().radet_head_loss_ws_ints(R)


def head_loss(cls, reg_u, iou, scales, gt_boxes, gt_labels, gt_off, p2g, pw, ldesc, nlvl, B, num_classes, alpha, gamma,
              lbw, giou_eps, grad_scale, losses, dcls, dcls_ld, dreg, dreg_ld, diou, diou_ld, dscales, ws,
              labels_out=None, tgt_out=None, flags=0):
    _lib.call("radet_head_loss", _ptr(cls), _ptr(reg_u), _ptr(iou), _ptr(scales), _ptr(gt_boxes), _ptr(gt_labels),
              _ptr(gt_off), _ptr(p2g), _ptr(pw), ldesc, nlvl, B, num_classes, alpha, gamma, lbw, giou_eps,
              _ptr(grad_scale), _ptr(losses), _ptr(dcls), dcls_ld, _ptr(dreg), dreg_ld, _ptr(diou), diou_ld,
              _ptr(dscales), _ptr(labels_out), _ptr(tgt_out), flags, _ptr(ws), _stream())


def scale_relu(reg_u, scales, out, ldesc, nlvl, B):
    _lib.call("radet_scale_relu", _ptr(reg_u), _ptr(scales), _ptr(out), ldesc, nlvl, B, _stream())


def grid_anchors(out, ldesc, nlvl, base_scale=8):
    _lib.call("radet_grid_anchors", _ptr(out), ldesc, nlvl, base_scale, _stream())


# ---------------------------------------------------------------------- stand-alone box / loss operators
OVERLAP_MODES = dict(iou=0, iof=1, giou=2)


def bbox_overlaps(b1, b2, out, batch, M, N, mode, aligned, eps):
    _lib.call("radet_bbox_overlaps", _ptr(b1), _ptr(b2), _ptr(out), batch, M, N, OVERLAP_MODES[mode], int(aligned), eps,
              _stream())


def _norm4(normalizer):
    v = [float(normalizer)] * 4 if isinstance(normalizer, (int, float)) else [float(x) for x in normalizer]
    assert len(v) == 4, "Normalizer must have length = 4"
    return (C.c_float * 4)(*v)


def tblr_encode(priors, gts, out, normalizer, normalize_by_wh=True):
    _lib.call("radet_tblr_encode", _ptr(priors), _ptr(gts), _ptr(out), priors.shape[0], _norm4(normalizer),
              int(normalize_by_wh), _stream())


def tblr_decode(priors, tblr, out, normalizer, normalize_by_wh=True, max_shape=None, clip_border=True):
    clip = bool(clip_border and max_shape is not None)
    mh, mw = (float(max_shape[0]), float(max_shape[1])) if clip else (0.0, 0.0)
    _lib.call("radet_tblr_decode", _ptr(priors), _ptr(tblr), _ptr(out), priors.shape[0], _norm4(normalizer),
              int(normalize_by_wh), mh, mw, int(clip), _stream())


def loss_partials(n_elem):
    return _lib.load().radet_loss_partials(n_elem)


def loss_finalize(partials, avg_factor, scale, out):
    _lib.call("radet_loss_finalize", _ptr(partials), partials.numel(), _ptr(avg_factor), scale, _ptr(out), _stream())


def sigmoid_focal_loss(x, target, weight, wcols, N, Cc, gamma, alpha, elem, partials, elem_scale=1.0):
    _lib.call("radet_sigmoid_focal_loss", _ptr(x), _ptr(target), _ptr(weight), wcols, C.c_size_t(N), Cc, gamma, alpha,
              _ptr(elem), elem_scale, _ptr(partials), _stream())


def sigmoid_focal_loss_bwd(x, target, weight, wcols, N, Cc, gamma, alpha, grad_elem, grad_scalar, avg_factor, scale, dx):
    _lib.call("radet_sigmoid_focal_loss_bwd", _ptr(x), _ptr(target), _ptr(weight), wcols, C.c_size_t(N), Cc, gamma, alpha,
              _ptr(grad_elem), _ptr(grad_scalar), _ptr(avg_factor), scale, _ptr(dx), _stream())


def bce_logits_loss(x, target, weight, wcols, N, Cc, elem, partials, elem_scale=1.0):
    _lib.call("radet_bce_logits_loss", _ptr(x), _ptr(target), _ptr(weight), wcols, C.c_size_t(N), Cc, _ptr(elem),
              elem_scale, _ptr(partials), _stream())


def bce_logits_loss_bwd(x, target, weight, wcols, N, Cc, grad_elem, grad_scalar, avg_factor, scale, dx):
    _lib.call("radet_bce_logits_loss_bwd", _ptr(x), _ptr(target), _ptr(weight), wcols, C.c_size_t(N), Cc, _ptr(grad_elem),
              _ptr(grad_scalar), _ptr(avg_factor), scale, _ptr(dx), _stream())


def giou_loss(pred, target, weight, N, eps, elem, partials, elem_scale=1.0):
    _lib.call("radet_giou_loss", _ptr(pred), _ptr(target), _ptr(weight), C.c_size_t(N), eps, _ptr(elem), elem_scale, _ptr(partials),
              _stream())


def giou_loss_bwd(pred, target, weight, N, eps, grad_elem, grad_scalar, avg_factor, scale, dpred):
    _lib.call("radet_giou_loss_bwd", _ptr(pred), _ptr(target), _ptr(weight), C.c_size_t(N), eps, _ptr(grad_elem),
              _ptr(grad_scalar), _ptr(avg_factor), scale, _ptr(dpred), _stream())


# the `loss_bbox` kinds (RADET_BOX_LOSS_* of include/radet_hip.h); radet_head_loss takes one in flags bits 1-3
BOX_LOSS_KINDS = dict(giou=0, iou=1, iou_linear=2, diou=3, ciou=4)
HEAD_LOSS_POSTACT = 1
HEAD_LOSS_KIND_SHIFT = 1


def head_loss_flags(kind="giou", postact=False):
    return (HEAD_LOSS_POSTACT if postact else 0) | (BOX_LOSS_KINDS[kind] << HEAD_LOSS_KIND_SHIFT)


def box_loss(kind, pred, target, weight, N, eps, elem, partials, elem_scale=1.0, hp1=0.0):
    _lib.call("radet_box_loss", BOX_LOSS_KINDS[kind], _ptr(pred), _ptr(target), _ptr(weight), C.c_size_t(N), eps, hp1,
              _ptr(elem), elem_scale, _ptr(partials), _stream())


def box_loss_bwd(kind, pred, target, weight, N, eps, grad_elem, grad_scalar, avg_factor, scale, dpred, hp1=0.0):
    _lib.call("radet_box_loss_bwd", BOX_LOSS_KINDS[kind], _ptr(pred), _ptr(target), _ptr(weight), C.c_size_t(N), eps, hp1,
              _ptr(grad_elem), _ptr(grad_scalar), _ptr(avg_factor), scale, _ptr(dpred), _stream())


def threshold_compact(scores, thr, idx, count):
    _lib.call("radet_threshold_compact", _ptr(scores), C.c_size_t(scores.numel()), thr, _ptr(idx), _ptr(count), _stream())


def sqnorm_partials(g, n, partials):
    _lib.call("radet_sqnorm_partials", _ptr(g), C.c_size_t(n), _ptr(partials), partials.numel(), _stream())


def adamw_step(p, g, m, v, n, lr, betas, eps, wd, step, max_norm, grad_div, partials, grad_norm_out):
    _lib.call("radet_adamw_step", _ptr(p), _ptr(g), _ptr(m), _ptr(v), C.c_size_t(n), lr, betas[0], betas[1], eps, wd,
              step, max_norm, grad_div, _ptr(partials), partials.numel(), _ptr(grad_norm_out), _stream())


OPT_MAX_RUNS = 1024                # RADET_OPT_MAX_RUNS of include/radet_hip.h: runs of a parameter-group table (16 KiB of LDS)

def adamw_step_runs(p, g, m, v, n, lr, betas, eps, wd, step, max_norm, grad_div, partials, grad_norm_out, runs, nruns):
    """radet_adamw_step with a device run table (`runs`: uint8 tensor holding nruns RadetOptRun records)"""
    _lib.call("radet_adamw_step_runs", _ptr(p), _ptr(g), _ptr(m), _ptr(v), C.c_size_t(n), lr, betas[0], betas[1], eps, wd,
              step, max_norm, grad_div, _ptr(partials), partials.numel(), _ptr(grad_norm_out), _ptr(runs), nruns, _stream())


def sgd_step(p, g, buf, n, lr, momentum, dampening, wd, nesterov, step, max_norm, grad_div, partials, grad_norm_out,
             runs=None, nruns=0):
    _lib.call("radet_sgd_step", _ptr(p), _ptr(g), _ptr(buf), C.c_size_t(n), lr, momentum, dampening, wd, int(bool(nesterov)),
              step, max_norm, grad_div, _ptr(partials), partials.numel(), _ptr(grad_norm_out), _ptr(runs), nruns, _stream())


GRAD_ACC_SET, GRAD_ACC_ADD, GRAD_ACC_RESTORE = 0, 1, 2       # acc = g / acc += g / g = acc + g


def grad_accumulate(acc, g, n, mode):
    _lib.call("radet_grad_accumulate", _ptr(acc), _ptr(g), C.c_size_t(n), mode, _stream())


def ema_update(ema, p, n, momentum):
    """ema = ema * (1 - momentum) + momentum * p with torch's CPU rounding (radet_ema_update): `momentum` is a Python float
    (a double); it and 1 - momentum are each rounded once to fp32 on the way into the call"""
    _lib.call("radet_ema_update", _ptr(ema), _ptr(p), C.c_size_t(n), float(momentum), 1.0 - float(momentum), _stream())


def ema_swap(a, b, n):
    _lib.call("radet_ema_swap", _ptr(a), _ptr(b), C.c_size_t(n), _stream())


def decode_ws_bytes(B, nlvl, nms_pre):
    return int(_lib.load().radet_decode_ws_bytes(B, nlvl, nms_pre))


def decode_candidates(cls, reg_u, iou, scales, ldesc, nlvl, B, num_classes, score_thr, nms_pre, img_hw, scale_factor,
                      cand_boxes, cand_scores, cand_ctr, cand_labels, cand_count, ws):
    _lib.call("radet_decode_candidates", _ptr(cls), _ptr(reg_u), _ptr(iou), _ptr(scales), ldesc, nlvl, B, num_classes,
              score_thr, nms_pre, _ptr(img_hw), _ptr(scale_factor), _ptr(cand_boxes), _ptr(cand_scores), _ptr(cand_ctr),
              _ptr(cand_labels), _ptr(cand_count), _ptr(ws), _stream())


def nms_ws_bytes(B, cap):
    return int(_lib.load().radet_nms_ws_bytes(B, cap))


NMS_MODES = dict(vote=0, global_vote=1, cluster=2, nms=3)


def nms(boxes, cluster_scores, vote_scores, labels, counts, B, cap, mode, iou_thr, iou_enable, sigma, max_out, out_boxes,
        out_scores, out_labels, out_count, aux0, aux1, ws):
    _lib.call("radet_nms", _ptr(boxes), _ptr(cluster_scores), _ptr(vote_scores), _ptr(labels), _ptr(counts), B, cap, mode,
              iou_thr, int(iou_enable), sigma, max_out, _ptr(out_boxes), _ptr(out_scores), _ptr(out_labels),
              _ptr(out_count), _ptr(aux0), _ptr(aux1), _ptr(ws), _stream())


def soft_nms_ws_bytes(B, cap):
    return int(_lib.load().radet_soft_nms_ws_bytes(B, cap))


SOFT_NMS_METHODS = dict(naive=0, linear=1, gaussian=2)


def soft_nms(boxes, scores, labels, counts, B, cap, method, iou_thr, sigma, min_score, class_agnostic, max_out, out_boxes,
             out_scores, out_labels, out_keep, out_count, ws):
    _lib.call("radet_soft_nms", _ptr(boxes), _ptr(scores), _ptr(labels), _ptr(counts), B, cap, method, iou_thr, sigma,
              min_score, int(class_agnostic), max_out, _ptr(out_boxes), _ptr(out_scores), _ptr(out_labels), _ptr(out_keep),
              _ptr(out_count), _ptr(ws), _stream())


def mbd_ws_bytes(px):
    return int(_lib.load().radet_mbd_ws_bytes(px))


def mbd(images, desc, n, sx, sy, alpha, niter, base_size, dmap, px, ws):
    _lib.call("radet_mbd", _ptr(images), _ptr(desc), n, _ptr(sx), _ptr(sy), alpha, niter, base_size, _ptr(dmap),
              C.c_size_t(px), _ptr(ws), _stream())


def gdt(cost, desc, n, sx, sy, dist, ws):
    _lib.call("radet_gdt", _ptr(cost), _ptr(desc), n, _ptr(sx), _ptr(sy), _ptr(dist), _ptr(ws), _stream())


def assign_ws_bytes(B, N):
    return int(_lib.load().radet_assign_ws_bytes(B, N))


FLIP = {None: 0, "none": 0, "horizontal": 1, "vertical": 2, "diagonal": 3}


VIEW_INTS = 12                            # include/radet_hip.h RADET_VIEW_INTS


def _views(views, n):
    """view rows {Hr, Wr, wy0, wx0, wh, ww, oy, ox, h, w, flip, fill}: i32 [n, VIEW_INTS] on the device, or None"""
    assert views is None or (tuple(views.shape) == (n, VIEW_INTS) and views.dtype == torch.int32 and views.is_contiguous())
    return _ptr(views)


def mask_max(src):
    """src: u8[G,Hs,Ws] device tensor (G > 0) -> i32[G]: each mask's maximum, what normalize=True divides by"""
    G, Hs, Ws = src.shape
    mx = torch.empty(G, dtype=torch.int32, device=src.device)
    _lib.call("radet_mask_max", _ptr(src), _ptr(mx), G, C.c_size_t(Hs * Ws), _stream())
    return mx


def mask_transform(src, out_hw=None, resized_hw=None, flip=None, pad_val=0, normalize=False, views=None, norm_max=None):
    """src: u8[G,Hs,Ws] device tensor -> u8[G,Hd,Wd]: nearest resize to resized_hw, flip, pad to out_hw (one pass).
    views: one view row per mask instead of resized_hw and flip (out_hw is then required) -- the window of the source mask
    (zeros outside it) that the row names, resized, the row's output window of that, flipped inside the window.
    norm_max: the masks' maxima from mask_max (several passes over one stack share them) instead of normalize=True"""
    G, Hs, Ws = src.shape
    Hr, Wr = resized_hw or (Hs, Ws)
    Hd, Wd = out_hw or (Hr, Wr)
    dst = torch.empty(G, Hd, Wd, dtype=torch.uint8, device=src.device)
    if G == 0:
        return dst
    mx = norm_max
    if mx is not None:
        assert tuple(mx.shape) == (G,) and mx.dtype == torch.int32 and mx.is_contiguous()
    elif normalize:
        mx = mask_max(src)
    _lib.call("radet_mask_transform", _ptr(src), _ptr(dst), _ptr(mx), _views(views, G), G, Hs, Ws, Hr, Wr, Hd, Wd, FLIP[flip],
              int(pad_val), _stream())
    return dst


RLE_MASK_INTS, RLE_PART_INTS = 5, 2       # include/radet_hip.h
RLE_MAX_W = 8192


def rle_masks(run_ends, part_desc, mask_desc, out_hw, resized_hw=None, pad_val=0, with_plain=False, views=None):
    """Run-length masks -> u8[G,Hd,Wd] in one launch (radet_amd.core.rle.pack_runs makes the three arrays): what
    mask_transform(normalize=True) gives for the decoded bitmaps, each mask with the flip of its descriptor row.
    run_ends: int32 / uint32 bit patterns [R]; part_desc i32 [P, 2]; mask_desc i32 [G, 5], all on the device.
    with_plain: also returns the unflipped masks -- defined only for masks whose flip bit is set (the others are
    unflipped in the first result).  views: one view row per mask instead of resized_hw, as mask_transform's (the flip
    stays mask_desc's, applied inside the output window; a sample outside the source image decodes as 0)."""
    G = mask_desc.shape[0]
    Hd, Wd = out_hw
    Hr, Wr = resized_hw or (Hd, Wd)
    dst = torch.empty(G, Hd, Wd, dtype=torch.uint8, device=mask_desc.device)
    plain = torch.empty_like(dst) if with_plain else None
    if G:
        _lib.call("radet_rle_masks", _ptr(run_ends), run_ends.numel(), _ptr(part_desc), part_desc.shape[0], _ptr(mask_desc),
                  _views(views, G), G, _ptr(dst), _ptr(plain), Hr, Wr, Hd, Wd, int(pad_val), _stream())
    return (dst, plain) if with_plain else dst


JPEG_ROW_INTS, JPEG_DESC_INTS, JPEG_HUFF_BYTES = 8, 20, 1424       # include/radet_hip.h


def jpeg_decode(blob, sections, sizes, nimg, dst, stages=7, work=None):
    """Baseline JPEG files -> packed u8 BGR pixels in `dst`, three launches (radet_jpeg_decode).  blob: the device copy of
    radet_amd.core.jpeg.pack_batch's buffer, sections / sizes as it returned them.  stages: bits 1 | 2 | 4 select the
    entropy / IDCT / convert launch (a benchmark times them one by one, with work = the (coef, planes) of a full call).
    Returns (err i32 [nimg] device view of the blob: error bits per image, zero for a good one; coef; planes)."""
    def sec(name):
        o, n = sections[name]
        return blob[o:o + n]
    coef, planes = work if work is not None else (
        torch.empty(sizes["coef_blocks"] * 64, dtype=torch.int16, device=blob.device),
        torch.empty(sizes["plane_bytes"], dtype=torch.uint8, device=blob.device))
    err = sec("err").view(torch.int32)
    _lib.call("radet_jpeg_decode", _ptr(sec("files")), _ptr(sec("desc")), nimg, _ptr(sec("wgs")), sizes["n_wg"], _ptr(sec("huff")),
              _ptr(sec("quant")), _ptr(sec("rows")), sizes["n_rows"], _ptr(coef), _ptr(planes), _ptr(dst), _ptr(err),
              sizes["max_blocks"], sizes["max_px"], int(stages), _stream())
    return err, coef, planes


def assign_points(gt_boxes, gt_off, masks, H, W, rng_words, U, ldesc, ranges, nlvl, B, positive_num, neg_thr, p2g, pw, used,
                  ws, flags=1):
    """masks: u8 [sumG, H, W] visible masks, or f32 per-box distance maps (mask-free sampler); rng_words: int32 / uint32 bit
    patterns [B, U] of the RandomStates' next raw outputs; flags: bit 0 balance_sample, bit 1 multiply_samplepro_for_weight,
    bit 2 adapt_positive_num, bit 3 uniform integer draws (random_sample_by_distance=False)"""
    _lib.call("radet_assign_points_f" if masks.dtype == torch.float32 else "radet_assign_points", _ptr(gt_boxes), _ptr(gt_off),
              _ptr(masks), H, W, _ptr(rng_words), U, ldesc, ranges, nlvl, B, positive_num, int(flags), neg_thr, _ptr(p2g), _ptr(pw),
              _ptr(used), _ptr(ws), _stream())


# ---------------------------------------------------------------------- image processing around MBD / GDT (packed crops)
def gauss9_kernel():
    """cv::getGaussianKernel(9, sigma <= 0 -> 0.3 * ((9 - 1) * 0.5 - 1) + 0.8 = 1.7, CV_32F): float taps, normalised with a
    double sum; returned as (centre, +-1, +-2, +-3, +-4)"""
    import numpy as np
    sigma = 0.3 * ((9 - 1) * 0.5 - 1) + 0.8
    x = np.arange(9, dtype=np.float64) - 4.0
    cf = np.exp(-0.5 / (sigma * sigma) * x * x).astype(np.float32)
    s = 0.0
    for v in cf:
        s += float(v)
    cf = (cf.astype(np.float64) * (1.0 / s)).astype(np.float32)
    return (C.c_float * 5)(*[float(v) for v in cf[4:]])


def resize_linear_u8(src, sdesc, dst, ddesc, n, max_dst_px, channels=3, views=None):
    """packed u8 images -> packed u8 images of the sizes of ddesc.  views: one view row per image -- the window of the
    source (the row's fill colour outside it) that is resized, and the window of the virtual resized image that is written;
    its h, w are ddesc's"""
    _lib.call("radet_resize_linear_u8", _ptr(src), _ptr(sdesc), _ptr(dst), _ptr(ddesc), _views(views, n), n, max_dst_px, channels,
              _stream())


# ---------------------------------------------------------------------- affine augmentation (csrc/warp.hip)
WARP_DESC_INTS, WARP_DESC_MATRIX, WARP_SKIP = 20, 8, 1      # include/radet_hip.h
WARP_MAX_COORD = float(1 << 21)


def invert_affine(M):
    """the inverse of a 2 x 3 forward matrix as cv2.warpAffine computes it (float64, its operation order; a singular
    matrix inverts to zeros, as there) -> float64 [6]"""
    import numpy as np
    m = np.array(M, np.float64).reshape(6)
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def warp_fits(inv, h, w):
    """whether the kernel's coordinates of an h x w image under the inverse matrix `inv` stay inside 32-bit fixed point"""
    import numpy as np
    m = np.abs(np.asarray(inv, np.float64).reshape(6))
    lim = WARP_MAX_COORD - 1                                      # (room for the rounding offsets)
    return bool(np.isfinite(m).all() and m[0] * w + m[1] * h + m[2] < lim and m[3] * w + m[4] * h + m[5] < lim)


def warp_desc_row(row, src_off, dst_off, h, w, channels, forward=None, fill=(0, 0, 0)):
    """fills one int32 [WARP_DESC_INTS] row; forward: the 2 x 3 forward matrix (what cv2.warpAffine is handed), None for a
    row that is copied unchanged (WARP_SKIP)"""
    import numpy as np
    f = tuple(int(v) for v in fill) + (0, 0, 0)
    row[:8] = [src_off, dst_off, h, w, channels, f[0] | f[1] << 8 | f[2] << 16, WARP_SKIP if forward is None else 0, 0]
    inv = np.zeros(6, np.float64) if forward is None else invert_affine(forward)
    if forward is not None and not warp_fits(inv, h, w):
        raise ValueError(f"affine matrix {np.asarray(forward).tolist()} on an image of {h} x {w}: the warp kernel's coordinates "
                         f"leave 32-bit fixed point")
    row[WARP_DESC_MATRIX:] = inv.view(np.int32)


def warp_affine_u8(src, dst, desc, n, max_px, channels=3):
    """src / dst: packed u8 device buffers (distinct); desc i32 [n, WARP_DESC_INTS] on the device (warp_desc_row): per row
    cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT) of an h x w x channels image in its classic fixed-point arithmetic, or a
    copy (WARP_SKIP); bytes of dst outside the rows' images are not written"""
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8 and src.is_contiguous() and dst.is_contiguous()
    assert desc.dtype == torch.int32 and desc.is_contiguous() and desc.numel() >= n * WARP_DESC_INTS
    _lib.call("radet_warp_affine_u8", _ptr(src), C.c_size_t(src.numel() // channels), _ptr(dst), C.c_size_t(dst.numel() // channels),
              _ptr(desc), int(n), int(max_px), int(channels), _stream())


def warp_affine_masks(src, forward):
    """src: u8 [G, H, W] device masks; forward: per mask a 2 x 3 forward matrix or None (copied) -> u8 [G, H, W]: the
    one-channel form of warp_affine_u8 with fill 0, one launch"""
    import numpy as np
    G, H, W = src.shape
    dst = torch.empty_like(src)
    if G == 0 or H * W == 0:
        return dst
    rows = np.zeros((G, WARP_DESC_INTS), np.int32)
    for g, M in enumerate(forward):
        warp_desc_row(rows[g], g * H * W, g * H * W, H, W, 1, M)
    warp_affine_u8(src, dst, torch.from_numpy(rows).to(src.device), G, H * W, 1)
    return dst


# ---------------------------------------------------------------------- CutOut (csrc/cutout.hip)
CUTOUT_DESC_INTS = 8                                        # include/radet_hip.h
CUTOUT_SKIP, CUTOUT_FLIP, CUTOUT_TO_RGB = 1, 2, 4


def cutout_desc_row(row, off, h, w, fill=(0, 0, 0), first=0, count=0, skip=False, flip=False, to_rgb=False):
    """fills one int32 [CUTOUT_DESC_INTS] row.  off: the image's pixel offset in the packed u8 buffer (cutout_u8) or its
    index in the f32 batch (cutout_f32); fill: three bytes in the u8 image's channel order (BGR); first / count: the
    image's rows of the hole table; flip / to_rgb: cutout_f32 only"""
    f = tuple(int(v) for v in fill)
    flags = (CUTOUT_SKIP if skip else 0) | (CUTOUT_FLIP if flip else 0) | (CUTOUT_TO_RGB if to_rgb else 0)
    row[:] = [off, h, w, f[0] | f[1] << 8 | f[2] << 16, first, count, flags, 0]


def cutout_launch_dims(holes_per_image, hw):
    """(most holes of any image, the largest clipped hole area) of a launch; holes_per_image: per image an int array [n, 4]
    of {x1, y1, x2, y2} (None: no holes), hw: per image (h, w).  Host arithmetic only."""
    import numpy as np
    most = area = 0
    for r, (h, w) in zip(holes_per_image, hw):
        if r is None or not len(r):
            continue
        r = np.asarray(r, np.int64).reshape(-1, 4)
        most = max(most, len(r))
        rw = np.clip(r[:, 2], 0, w) - np.clip(r[:, 0], 0, w)
        rh = np.clip(r[:, 3], 0, h) - np.clip(r[:, 1], 0, h)
        area = max(area, int((np.maximum(rw, 0) * np.maximum(rh, 0)).max()))
    return most, area


def cutout_u8(img, desc, holes, n, max_holes, max_area, channels=3):
    """img: the packed u8 BGR device buffer, changed in place; desc i32 [n, CUTOUT_DESC_INTS] and holes i32 [total, 4] on
    the device: every hole of every row's image is filled with the row's fill bytes, in one launch (one thread per hole
    pixel); no byte outside the holes is written"""
    assert img.dtype == torch.uint8 and img.is_contiguous()
    assert desc.dtype == torch.int32 and desc.is_contiguous() and desc.numel() >= n * CUTOUT_DESC_INTS
    assert holes.dtype == torch.int32 and holes.is_contiguous() and holes.numel() % 4 == 0
    _lib.call("radet_cutout_u8", _ptr(img), C.c_size_t(img.numel() // 3), _ptr(desc), int(n), _ptr(holes), holes.numel() // 4,
              int(max_holes), int(max_area), int(channels), _stream())


def cutout_f32(out, desc, holes, n, max_holes, max_area, mean, stdinv):
    """out: f32 [B, 3, Hp, Wp] as augment_finish wrote it, changed in place: every hole pixel becomes what augment_finish
    writes for a u8 pixel equal to the row's fill with no blend active (mean / stdinv: its operands), mirrored for a
    flipped sample; one launch"""
    assert out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4 and out.shape[1] == 3
    assert desc.dtype == torch.int32 and desc.is_contiguous() and desc.numel() >= n * CUTOUT_DESC_INTS
    assert holes.dtype == torch.int32 and holes.is_contiguous() and holes.numel() % 4 == 0
    _lib.call("radet_cutout_f32", _ptr(out), int(out.shape[0]), int(out.shape[2]), int(out.shape[3]), _ptr(desc), int(n),
              _ptr(holes), holes.numel() // 4, int(max_holes), int(max_area), *[float(v) for v in mean],
              *[float(v) for v in stdinv], _stream())


# ---------------------------------------------------------------------- AutoAugment's colour stages (csrc/color.hip)
COLOR_DESC_INTS, COLOR_CHUNK_PX = 8, 4096                   # include/radet_hip.h
COLOR_SKIP = 1
COLOR_KINDS = dict(brightness=1, contrast=2, color=3, equalize=4)
COLOR_STATS_KINDS = ("contrast", "equalize")                # the kinds whose map is built from the image's histogram


def color_factors(factor):
    """(fp32 bits of alpha = fl32(factor), fp32 bits of beta = fl32(1 - factor)), 1 - factor formed in double"""
    import numpy as np
    return tuple(int(np.array([v], np.float64).astype(np.float32).view(np.int32)[0]) for v in (factor, 1.0 - float(factor)))


def color_desc_row(row, off, h, w, kind=None, factor=1.0, skip=False):
    """fills one int32 [COLOR_DESC_INTS] row.  off: the image's pixel offset in the packed u8 buffer; kind: a key of
    COLOR_KINDS (None: the row is not run); factor: the stage's factor as a Python float (unused by 'equalize')"""
    alpha, beta = color_factors(factor)
    row[:] = [off, h, w, COLOR_KINDS[kind] if kind is not None else 0, alpha, beta, COLOR_SKIP if skip else 0, 0]


def color_stats_u8(img, desc, hist, n, max_px, channels=3):
    """img: the packed u8 BGR device buffer; desc i32 [n, COLOR_DESC_INTS]; hist u32-as-i32 [n, 4, 256], zeroed by the
    caller: the histograms of B, G, R and gray of every 'equalize' / 'contrast' row's image are added to it, one launch"""
    assert img.dtype == torch.uint8 and img.is_contiguous()
    assert desc.dtype == torch.int32 and desc.is_contiguous() and desc.numel() >= n * COLOR_DESC_INTS
    assert hist.dtype == torch.int32 and hist.is_contiguous() and hist.numel() >= n * 4 * 256
    _lib.call("radet_color_stats_u8", _ptr(img), C.c_size_t(img.numel() // 3), _ptr(desc), int(n), int(max_px), _ptr(hist),
              int(channels), _stream())


def color_apply_u8(img, desc, hist, n, max_px, channels=3):
    """img: the packed u8 BGR device buffer, changed in place: every row's image under the row's colour stage, one launch;
    hist: what color_stats_u8 filled for the same rows (None when no row is 'equalize' / 'contrast')"""
    assert img.dtype == torch.uint8 and img.is_contiguous()
    assert desc.dtype == torch.int32 and desc.is_contiguous() and desc.numel() >= n * COLOR_DESC_INTS
    assert hist is None or (hist.dtype == torch.int32 and hist.is_contiguous() and hist.numel() >= n * 4 * 256)
    _lib.call("radet_color_apply_u8", _ptr(img), C.c_size_t(img.numel() // 3), _ptr(desc), int(n), int(max_px), _ptr(hist),
              int(channels), _stream())


def resize_linear_f(src, sdesc, dst, ddesc, n, max_dst_px):
    _lib.call("radet_resize_linear_f", _ptr(src), _ptr(sdesc), _ptr(dst), _ptr(ddesc), n, max_dst_px,
              1 if src.dtype == torch.float64 else 0, _stream())


def gaussian_blur9_u8(src, desc, dst, tmp, n, max_px):
    _lib.call("radet_gaussian_blur9_u8", _ptr(src), _ptr(desc), _ptr(dst), _ptr(tmp), gauss9_kernel(), n, max_px, _stream())


def sobel_edge(src, desc, edge, gray_ws, max_ws, n, max_px):
    _lib.call("radet_sobel_edge", _ptr(src), _ptr(desc), _ptr(edge), _ptr(gray_ws), _ptr(max_ws), n, max_px, _stream())


# ---------------------------------------------------------------------- BOP training-image augmentation (csrc/augment.hip)
AUG_PARAM_INTS = 16
AUG_MAX_W = 8192


def augment_merge_hblur(src, bg, params, dst, n, max_h, max_w):
    _lib.call("radet_augment_merge_hblur", _ptr(src), _ptr(bg), _ptr(params), _ptr(dst), n, max_h, max_w, _stream())


def augment_vblur(src, params, dst, n, max_h, max_w):
    _lib.call("radet_augment_vblur", _ptr(src), _ptr(params), _ptr(dst), n, max_h, max_w, _stream())


def augment_sharp(src, params, dst, lsum, n, max_px):
    _lib.call("radet_augment_sharp", _ptr(src), _ptr(params), _ptr(dst), _ptr(lsum), n, max_px, _stream())


def augment_finish(src, lsum, params, out, n, Hp, Wp, mean, stdinv):
    _lib.call("radet_augment_finish", _ptr(src), _ptr(lsum), _ptr(params), _ptr(out), n, Hp, Wp, *[float(v) for v in mean],
              *[float(v) for v in stdinv], _stream())


AUG2_PARAM_INTS = 16


def augment_hsv_noise(src, params2, dst, n, max_px):
    _lib.call("radet_augment_hsv_noise", _ptr(src), _ptr(params2), _ptr(dst), n, max_px, _stream())


def augment_box(src, params2, dst, n, max_h, max_w):
    _lib.call("radet_augment_box", _ptr(src), _ptr(params2), _ptr(dst), src.numel() * src.element_size(), n, max_h, max_w,
              _stream())


# ---------------------------------------------------------------------- mask-free sampler inside the image pipeline
CROP_DESC_INTS = 12
PASTE_DESC_INTS = 10


def crop_canvases(src, lsum, params, nimg, desc, n, max_px, dst):
    """the padded box crops of a batch cut from the augmented image (src / lsum / params: what augment_finish reads);
    desc i32 [n, CROP_DESC_INTS]; dst u8 [sum h * w * 3], the canvases back to back"""
    _lib.call("radet_crop_canvases", _ptr(src), C.c_size_t(src.numel()), _ptr(lsum), _ptr(params), nimg, _ptr(desc), n, max_px,
              _ptr(dst), C.c_size_t(dst.numel() // 3), _stream())


def paste_maps(maps, desc, n, H, W, out):
    """packed f32 / f64 distance maps -> out f32 [n, H, W] (zero fill and paste in one pass); desc i32 [n, PASTE_DESC_INTS]"""
    assert maps.dtype in (torch.float32, torch.float64) and out.dtype == torch.float32 and out.numel() == n * H * W
    _lib.call("radet_paste_maps", _ptr(maps), C.c_size_t(maps.numel()), 1 if maps.dtype == torch.float64 else 0, _ptr(desc), n,
              H, W, _ptr(out), _stream())


# ---------------------------------------------------------------------- in-memory frames, one launch (csrc/preprocess.hip)
PREP_DESC_INTS = 8                 # include/radet_hip.h
PREP_TO_RGB, PREP_FLIP_H, PREP_FLIP_V = 1, 2, 4
PREP_FLIP = dict(horizontal=PREP_FLIP_H, vertical=PREP_FLIP_V, diagonal=PREP_FLIP_H | PREP_FLIP_V)


def preprocess_frames(desc, n, Hp, Wp, mean, stdinv, out):
    """u8 HWC BGR frames at the addresses of desc i32 [n, PREP_DESC_INTS] -> out f32 [n, 3, Hp, Wp]: resize, optional
    BGR->RGB, (q - mean) * stdinv, zero pad -- what resize_linear_u8 -> augment_finish give, in one launch"""
    assert out.dtype == torch.float32 and out.numel() >= n * 3 * Hp * Wp and desc.dtype == torch.int32
    assert desc.numel() >= n * PREP_DESC_INTS
    _lib.call("radet_preprocess_frames", _ptr(desc), int(n), int(Hp), int(Wp), *[float(v) for v in mean],
              *[float(v) for v in stdinv], _ptr(out), _stream())


# ---------------------------------------------------------------------- test-time augmentation (csrc/tta.hip)
TTA_MAX_VIEWS = 16                 # include/radet_hip.h
MERGE_DESC_INTS = 9                # {h, w, sx, sy, sx, sy (f32 bits), flip code, start, cap}
FLIP_CODES = {None: 0, "horizontal": 1, "vertical": 2, "diagonal": 3}


def merge_desc_rows(hw, sf, flips, starts, caps):
    """the descriptor rows of radet_merge_views for V * B (view, image) rows, row r = v * B + b: hw [R, 2] the views'
    img_shape, sf [R, 4] their scale factors, flips [R] codes 0..3, starts / caps [R] in candidates.  Host arithmetic only."""
    import numpy as np
    R = len(flips)
    rows = np.zeros((R, MERGE_DESC_INTS), np.int32)
    rows[:, 0:2] = np.asarray(hw, np.float32).reshape(R, 2).view(np.int32)
    rows[:, 2:6] = np.asarray(sf, np.float32).reshape(R, 4).view(np.int32)
    rows[:, 6], rows[:, 7], rows[:, 8] = flips, starts, caps
    return rows


def merge_views(desc_host, desc, V, B, pool_boxes, pool_scores, pool_ctr, pool_labels, counts, cap_out, out_boxes, out_scores,
                out_ctr, out_labels, out_count):
    """the candidates of V * B (view, image) rows back in the frame and packed per image (include/radet_hip.h,
    radet_merge_views).  desc_host: i32 ndarray [V * B, MERGE_DESC_INTS], read during the call (the argument checks); desc:
    the same words on the device.  The pool is flat: boxes f32 [pool, 4], the others [pool]."""
    import numpy as np
    assert isinstance(desc_host, np.ndarray) and desc_host.dtype == np.int32 and desc_host.flags.c_contiguous
    assert desc_host.size == V * B * MERGE_DESC_INTS and desc.dtype == torch.int32 and desc.numel() >= desc_host.size
    pool = int(pool_scores.numel())
    assert pool_boxes.dtype == torch.float32 and pool_boxes.numel() == 4 * pool and pool_ctr.numel() == pool
    assert pool_labels.dtype == torch.int64 and pool_labels.numel() == pool and counts.dtype == torch.int32 and counts.numel() >= V * B
    assert out_boxes.numel() >= B * cap_out * 4 and min(out_scores.numel(), out_ctr.numel(), out_labels.numel()) >= B * cap_out
    assert out_labels.dtype == torch.int64 and out_count.dtype == torch.int32 and out_count.numel() >= B
    _lib.call("radet_merge_views", desc_host.ctypes.data, _ptr(desc), int(V), int(B), C.c_size_t(pool), _ptr(pool_boxes),
              _ptr(pool_scores), _ptr(pool_ctr), _ptr(pool_labels), _ptr(counts), int(cap_out), _ptr(out_boxes), _ptr(out_scores),
              _ptr(out_ctr), _ptr(out_labels), _ptr(out_count), _stream())


# ---------------------------------------------------------------------- tiled inference (csrc/tiles.hip)
TILE_MAX_ROWS = 64                 # include/radet_hip.h
TILE_DESC_INTS = 11                # {h, w, sx, sy, sx, sy, x0, y0 (f32 bits), edge mask, start, cap}
TILE_EDGE_L, TILE_EDGE_T, TILE_EDGE_R, TILE_EDGE_B = 1, 2, 4, 8


def tile_desc_rows(hw, sf, offsets, edges, starts, caps):
    """the descriptor rows of radet_merge_tiles for R rows, image-major: hw [R, 2] the rows' img_shape, sf [R, 4] their scale
    factors, offsets [R, 2] (x0, y0) of the row's source rectangle in its frame, edges [R] TILE_EDGE_* masks, starts / caps [R]
    in candidates.  Host arithmetic only."""
    import numpy as np
    R = len(edges)
    rows = np.zeros((R, TILE_DESC_INTS), np.int32)
    rows[:, 0:2] = np.asarray(hw, np.float32).reshape(R, 2).view(np.int32)
    rows[:, 2:6] = np.asarray(sf, np.float32).reshape(R, 4).view(np.int32)
    rows[:, 6:8] = np.asarray(offsets, np.float32).reshape(R, 2).view(np.int32)
    rows[:, 8], rows[:, 9], rows[:, 10] = edges, starts, caps
    return rows


def merge_tiles(desc_host, desc, row_start_host, row_start, B, pool_boxes, pool_scores, pool_ctr, pool_labels, counts,
                edge_margin, cap_out, out_boxes, out_scores, out_ctr, out_labels, out_count, out_dropped):
    """the candidates of a tiled batch's rows filtered at the tile borders, back in the frame and packed per image
    (include/radet_hip.h, radet_merge_tiles).  desc_host: i32 ndarray [R, TILE_DESC_INTS] and row_start_host: i32 ndarray
    [B + 1], read during the call (the argument checks); desc, row_start: the same words on the device.  The pool is flat:
    boxes f32 [pool, 4], the others [pool]."""
    import numpy as np
    for a in (desc_host, row_start_host):
        assert isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous
    assert row_start_host.size == B + 1 and row_start.dtype == torch.int32 and row_start.numel() >= B + 1
    R = int(row_start_host[B]) if B else 0
    assert 0 <= R and desc_host.size == R * TILE_DESC_INTS and desc.dtype == torch.int32 and desc.numel() >= desc_host.size
    pool = int(pool_scores.numel())
    assert pool_boxes.dtype == torch.float32 and pool_boxes.numel() == 4 * pool and pool_ctr.numel() == pool
    assert pool_labels.dtype == torch.int64 and pool_labels.numel() == pool and counts.dtype == torch.int32 and counts.numel() >= R
    assert out_boxes.numel() >= B * cap_out * 4 and min(out_scores.numel(), out_ctr.numel(), out_labels.numel()) >= B * cap_out
    assert out_labels.dtype == torch.int64 and out_count.dtype == torch.int32 and out_dropped.dtype == torch.int32
    assert min(out_count.numel(), out_dropped.numel()) >= B
    _lib.call("radet_merge_tiles", desc_host.ctypes.data, _ptr(desc), row_start_host.ctypes.data, _ptr(row_start), int(B),
              C.c_size_t(pool), _ptr(pool_boxes), _ptr(pool_scores), _ptr(pool_ctr), _ptr(pool_labels), _ptr(counts),
              float(edge_margin), int(cap_out), _ptr(out_boxes), _ptr(out_scores), _ptr(out_ctr), _ptr(out_labels), _ptr(out_count),
              _ptr(out_dropped), _stream())


# ---------------------------------------------------------------------- detections -> RoI crops (csrc/crops.hip)
CROP_ROW_INTS = 6                  # include/radet_hip.h: {b, j, wx0, wy0, ww, wh}
CROP_MAX_SIDE = 16384
CROP_MAX_OUT = 4096                # largest output side
CROP_MAX_SLOTS = 65535             # largest cap (the pixel kernel's second grid dimension)
CROP_TO_RGB, CROP_F32 = 1, 2


def crop_plan(boxes, scores, counts, size, scale, score_thr, cap, rows, counters):
    """the NMS outputs boxes f32 [B,K,4], scores f32 [B,K], counts i32 [B] -> rows i32 [cap, CROP_ROW_INTS] (the windows of
    the valid detections, in order, the first cap of them) and counters i32 [2 + B] = {n_out, n_total, ends [B]}: frame b's
    rows are [ends[b - 1] (0 for b == 0), ends[b]); size = (Ho, Wo)"""
    B, Kd = int(boxes.shape[0]), int(boxes.shape[1])
    assert boxes.dtype == torch.float32 and tuple(boxes.shape) == (B, Kd, 4) and scores.dtype == torch.float32
    assert tuple(scores.shape) == (B, Kd) and counts.dtype == torch.int32 and counts.numel() == B
    assert rows.dtype == torch.int32 and rows.numel() >= cap * CROP_ROW_INTS and counters.dtype == torch.int32 and counters.numel() >= 2 + B
    _lib.call("radet_crop_plan", _ptr(boxes), _ptr(scores), _ptr(counts), B, Kd, int(size[0]), int(size[1]), float(scale),
              float(score_thr), int(cap), _ptr(rows), _ptr(counters), _stream())


def crop_frames(rows, counters, desc, B, cap, size, out, fill=0, mean=None, stdinv=None, to_rgb=False):
    """the slots n < counters[0] of out: the window of rows[n] cut from the frame of desc i32 [B, PREP_DESC_INTS] and resized
    to size = (Ho, Wo).  out f32 [cap,3,Ho,Wo] (mean, stdinv given: Normalize, to_rgb as there) or u8 [cap,Ho,Wo,3] (raw
    BGR); fill = c0 | c1 << 8 | c2 << 16 in the frames' channel order"""
    Ho, Wo = int(size[0]), int(size[1])
    f32 = out.dtype == torch.float32
    assert f32 or out.dtype == torch.uint8
    assert out.numel() >= cap * 3 * Ho * Wo and desc.dtype == torch.int32 and desc.numel() >= B * PREP_DESC_INTS
    assert rows.dtype == torch.int32 and rows.numel() >= cap * CROP_ROW_INTS and f32 == (mean is not None) == (stdinv is not None)
    flags = (CROP_F32 if f32 else 0) | (CROP_TO_RGB if f32 and to_rgb else 0)
    _lib.call("radet_crop_frames", _ptr(rows), _ptr(counters), _ptr(desc), int(B), int(cap), Ho, Wo, flags, int(fill),
              *[float(v) for v in (mean if f32 else (0, 0, 0))], *[float(v) for v in (stdinv if f32 else (1, 1, 1))], _ptr(out),
              _stream())


# ---------------------------------------------------------------------- detections drawn on frames (csrc/draw.hip)
DRAW_MAX_DETS = 256                # include/radet_hip.h
DRAW_MAX_THICKNESS = 255
DRAW_MAX_TEXT_W = 4096
DRAW_MAX_GLYPH_H = 256
DRAW_MAX_PAD = 64
DRAW_INPLACE = 1
DRAW_STRIP_DOT, DRAW_STRIP_BAR, DRAW_STRIP_CLASS, DRAW_STRIP_NAME0 = 10, 11, 12, 13


def draw_detections(src_desc, dst_desc, B, max_h, max_w, boxes, scores, labels, counts, thickness, box_colour, palette,
                    text_colour, a_bg, score_thr, max_dets, n_names, pad, inplace, atlas, widths):
    """one launch: the detections boxes f32 [B,K,4], scores f32 [B,K], labels i64 [B,K], counts i32 [B] drawn on the frames of
    src_desc i32 [B, PREP_DESC_INTS] into those of dst_desc (the same table with inplace).  box_colour: b | g << 8 | r << 16,
    or None with palette u8 [n,3]; atlas u8 [S,Hc,Wa] with widths i32 [S], or None for no labels (include/radet_hip.h)"""
    Kd = int(boxes.shape[1])
    assert boxes.dtype == torch.float32 and tuple(boxes.shape) == (B, Kd, 4) and scores.dtype == torch.float32
    assert tuple(scores.shape) == (B, Kd) and labels.dtype == torch.int64 and tuple(labels.shape) == (B, Kd)
    assert counts.dtype == torch.int32 and counts.numel() == B
    assert all(d.dtype == torch.int32 and d.numel() >= B * PREP_DESC_INTS for d in (src_desc, dst_desc))
    assert (box_colour is None) != (palette is None)
    assert palette is None or (palette.dtype == torch.uint8 and palette.dim() == 2 and palette.shape[1] == 3 and palette.is_contiguous())
    S = Hc = Wa = 0
    if atlas is not None:
        S, Hc, Wa = (int(v) for v in atlas.shape)
        assert atlas.dtype == torch.uint8 and atlas.is_contiguous() and widths.dtype == torch.int32 and widths.numel() == S
    _lib.call("radet_draw_detections", _ptr(src_desc), _ptr(dst_desc), int(B), int(max_h), int(max_w), _ptr(boxes), _ptr(scores),
              _ptr(labels), _ptr(counts), Kd, int(thickness), -1 if box_colour is None else int(box_colour),
              None if palette is None else _ptr(palette), 0 if palette is None else int(palette.shape[0]), int(text_colour),
              int(a_bg), float(score_thr), int(max_dets), int(n_names), int(pad), DRAW_INPLACE if inplace else 0,
              None if atlas is None else _ptr(atlas), None if atlas is None else _ptr(widths), S, Hc, Wa, _stream())


# ---------------------------------------------------------------------- detections tracked across frames (csrc/track.hip)
TRACK_MAX_TRACKS = 256             # include/radet_hip.h
TRACK_MAX_DETS = 4096
TRACK_STATE_BYTES = 13328
TRACK_MOTIONS = dict(none=0, constant=1)


def track_state_bytes(nseq):
    return int(_lib.load().radet_track_state_bytes(nseq))


def track_update(boxes, scores, labels, counts, nseq, B, cap, state, iou_thr, track_thr, new_thr, max_age, max_tracks, motion,
                 class_aware, ids, hits):
    """one launch: the B consecutive frames of each of nseq sequences -- boxes f32 [nseq,B,cap,4], scores f32 [nseq,B,cap],
    labels i64, counts i32 [nseq,B] -- through the trackers of state (u8 [nseq, TRACK_STATE_BYTES]); ids / hits i32
    [nseq,B,cap] are written (include/radet_hip.h)"""
    assert boxes.dtype == torch.float32 and tuple(boxes.shape) == (nseq, B, cap, 4) and scores.dtype == torch.float32
    assert tuple(scores.shape) == (nseq, B, cap) and labels.dtype == torch.int64 and tuple(labels.shape) == (nseq, B, cap)
    assert counts.dtype == torch.int32 and counts.numel() == nseq * B
    assert state.numel() * state.element_size() == nseq * TRACK_STATE_BYTES
    assert all(t.dtype == torch.int32 and tuple(t.shape) == (nseq, B, cap) for t in (ids, hits))
    _lib.call("radet_track_update", _ptr(boxes), _ptr(scores), _ptr(labels), _ptr(counts), int(nseq), int(B), int(cap),
              _ptr(state), float(iou_thr), float(track_thr), float(new_thr), int(max_age), int(max_tracks), int(motion),
              int(class_aware), _ptr(ids), _ptr(hits), _stream())


# ---------------------------------------------------------------------- COCO-protocol evaluation (csrc/cocoeval.hip)
COCO_MAX_GT = 512                  # RADET_COCO_MAX_GT of include/radet_hip.h: ground truths per (category, image) segment
COCO_ERR_OVERSIZE = -3             # RADET_ERR_COCO_OVERSIZE


class CocoShapeError(_lib.RadetHipError):
    """radet_coco_match refused its arguments before launching anything: a segment with more than COCO_MAX_GT ground truths
    (code -3), or more (area range, threshold) pairs than lanes (code -1).  DeviceCOCOeval falls back to the host evaluator."""


def coco_match(dt_xyxy, dt_off, gt_xywh, gt_area, gt_flags, gt_off, nseg, max_seg_gt, iou_thrs, area_rng, dt_match, dt_flag,
               gt_match, gt_ignore):
    """see include/radet_hip.h.  The return code is read here, not by _lib.call: the two argument refusals are a result."""
    T, A = iou_thrs.numel(), area_rng.shape[0]
    assert dt_match.shape == (dt_xyxy.shape[0], A * T) and dt_flag.shape == dt_match.shape
    assert gt_match.shape == (gt_xywh.shape[0], A * T) and gt_ignore.shape == (gt_xywh.shape[0], A)
    assert dt_off.numel() == nseg + 1 and gt_off.numel() == nseg + 1
    _lib.load()
    if "radet_coco_match" not in _lib._FN:
        _lib._FN["radet_coco_match"] = _lib.load().radet_coco_match
    rc = _lib._FN["radet_coco_match"](_ptr(dt_xyxy), _ptr(dt_off), _ptr(gt_xywh), _ptr(gt_area), _ptr(gt_flags), _ptr(gt_off),
                                      nseg, int(max_seg_gt), _ptr(iou_thrs), T, _ptr(area_rng), A, _ptr(dt_match),
                                      _ptr(dt_flag), _ptr(gt_match), _ptr(gt_ignore), _stream())
    if rc == COCO_ERR_OVERSIZE:
        raise CocoShapeError(f"a segment holds {max_seg_gt} ground truths, radet_coco_match at most {COCO_MAX_GT}")
    if rc == -1:
        raise CocoShapeError(f"radet_coco_match refuses {A} area ranges x {T} IoU thresholds (at most 8 ranges, 64 pairs)")
    _lib.check(rc, "radet_coco_match")


def coco_accumulate(dt_flag_sorted, dt_rank_sorted, dt_score_sorted, dt_cat_off, gt_ignore, gt_cat_off, max_dets, rec_thrs,
                    T, K, A, precision, recall, scores):
    R, M = rec_thrs.numel(), max_dets.numel()
    assert precision.shape == (T, R, K, A, M) and scores.shape == precision.shape and recall.shape == (T, K, A, M)
    assert dt_cat_off.numel() == K + 1 and gt_cat_off.numel() == K + 1 and dt_flag_sorted.shape[1] == A * T
    _lib.call("radet_coco_accumulate", _ptr(dt_flag_sorted), _ptr(dt_rank_sorted), _ptr(dt_score_sorted), _ptr(dt_cat_off),
              _ptr(gt_ignore), _ptr(gt_cat_off), _ptr(max_dets), _ptr(rec_thrs), T, R, K, A, M, _ptr(precision), _ptr(recall),
              _ptr(scores), _stream())
