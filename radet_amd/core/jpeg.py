"""The host side of device JPEG decoding: what is serial and tiny.

`parse_jpeg(bytes)` reads the headers of a file and says whether the device decoder takes it (baseline / extended
sequential Huffman, 8 bits, grey or YCbCr with luma sampling 1x1 / 2x1 / 2x2, one interleaved scan); everything else
returns None and is decoded by Pillow as before.  `scan_index` walks the entropy-coded data once (radet_jpeg_index, plain
C) and returns the entry points at which the device's lanes enter the Huffman stream; it is also the validator: a stream
it rejects (ValueError naming the file) never reaches the device.  `IndexCache` keeps the indexes in memory and, given a
directory, on disk.  `pack_batch` lays a batch's files, tables and index rows out as ONE host buffer for
radet_jpeg_decode (radet_amd/kernels.py:jpeg_decode)."""
import hashlib
import os
import threading

import numpy as np

ROW_INTS, DESC_INTS, HUFF_BYTES = 8, 20, 1424            # include/radet_hip.h
LOOK_BITS = 9
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                   61, 54, 47, 55, 62, 63])
ERRORS = {1: "an undefined Huffman code", 2: "a coefficient index past 63", 4: "the stream ends early",
          8: "a restart marker out of sequence", 16: "an MCU count that does not match the frame",
          32: "a segment does not end where its index entry says", 64: "more index rows than expected"}
DEFAULT_SEG_MCUS = 16


class JpegHeader:
    """what parse_jpeg found in a supported file"""
    __slots__ = ("width", "height", "ncomp", "hs", "vs", "quant", "huff", "restart_interval", "scan_lo", "scan_hi",
                 "mcux", "mcuy")

    @property
    def n_mcus(self):
        return self.mcux * self.mcuy

    @property
    def comp_blocks(self):
        return [self.hs * self.vs] + [1] * (self.ncomp - 1)

    def resolve_seg_mcus(self, seg_mcus):
        return self.mcux if seg_mcus == "row" else int(seg_mcus)


def _u16(b, i):
    return (b[i] << 8) | b[i + 1]


def parse_jpeg(data):
    """JpegHeader of a file the device decoder takes, None for any other (also for a file that is no JPEG at all):
    size, components, sampling factors, quantisation tables [ncomp, 64] (natural order), Huffman tables as (bits[16],
    vals) per component (DC, AC), restart interval and the scan's byte range.  Never raises for a foreign file."""
    b = bytes(data)
    n = len(b)
    if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
        return None
    qt, ht = {}, {}
    frame = None
    jfif, adobe, ri = False, None, 0
    i = 2
    try:
        while True:
            while i < n and b[i] != 0xFF:          # (garbage between segments is skipped, as libjpeg does with a warning)
                i += 1
            while i < n and b[i] == 0xFF:
                i += 1
            if i >= n:
                return None
            m = b[i]
            i += 1
            if m in (0x01,) or 0xD0 <= m <= 0xD7:
                continue
            if m == 0xD9:
                return None
            L = _u16(b, i)
            seg = b[i + 2:i + L]
            if L < 2 or len(seg) != L - 2:
                return None
            if m == 0xC0 or m == 0xC1:
                if frame is not None:
                    return None
                frame = seg
            elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
                return None                         # progressive, lossless, arithmetic, hierarchical
            elif m == 0xCC or m == 0xDC:
                return None                         # arithmetic conditioning, DNL
            elif m == 0xC4:
                j = 0
                while j < len(seg):
                    tc, th = seg[j] >> 4, seg[j] & 15
                    bits = list(seg[j + 1:j + 17])
                    cnt = sum(bits)
                    if tc > 1 or th > 3 or len(bits) != 16 or cnt > 256 or j + 17 + cnt > len(seg):
                        return None
                    ht[(tc, th)] = (bytes(bits), bytes(seg[j + 17:j + 17 + cnt]))
                    j += 17 + cnt
            elif m == 0xDB:
                j = 0
                while j < len(seg):
                    pq, tq = seg[j] >> 4, seg[j] & 15
                    if pq != 0 or tq > 3:
                        return None                 # (16-bit tables belong to 12-bit files; the device dequantises 8-bit ones)
                    t = np.frombuffer(seg, np.uint8, 64, j + 1).astype(np.int64)
                    j += 65
                    nat = np.zeros(64, np.uint16)
                    nat[ZIGZAG] = t
                    qt[tq] = nat
            elif m == 0xDD:
                ri = _u16(seg, 0)
            elif m == 0xE0 and seg[:5] == b"JFIF\0":
                jfif = True
            elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
                adobe = seg[11]
            elif m == 0xDA:
                break
            i += L
        if frame is None or frame[0] != 8:
            return None
        H, W, nc = _u16(frame, 1), _u16(frame, 3), frame[5]
        if H == 0 or W == 0 or nc not in (1, 3) or len(frame) != 6 + 3 * nc:
            return None
        comps = [(frame[6 + 3 * c], frame[7 + 3 * c] >> 4, frame[7 + 3 * c] & 15, frame[8 + 3 * c]) for c in range(nc)]
        if nc == 3:
            # libjpeg's colour space guess: JFIF -> YCbCr; Adobe transform 0 -> RGB; neither: ids R G B -> RGB
            if not jfif and adobe is not None and adobe != 1:
                return None
            if not jfif and adobe is None and [c[0] for c in comps] == [ord("R"), ord("G"), ord("B")]:
                return None
            if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                return None
        hs, vs = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)    # (a single component's factors do not matter)
        if nc == 1 and (comps[0][1] not in (1, 2, 3, 4) or comps[0][2] not in (1, 2, 3, 4)):
            return None
        # the scan header: all components in frame order, Ss = 0, Se = 63, Ah = Al = 0
        if seg[0] != nc or len(seg) != 4 + 2 * nc:
            return None
        sel = []
        for c in range(nc):
            if seg[1 + 2 * c] != comps[c][0]:
                return None
            sel.append((seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15))
        if tuple(seg[1 + 2 * nc:4 + 2 * nc]) != (0, 63, 0):
            return None
        h = JpegHeader()
        h.width, h.height, h.ncomp, h.hs, h.vs, h.restart_interval = W, H, nc, hs, vs, ri
        h.mcux, h.mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
        if any(c[3] not in qt for c in comps) or any((0, d) not in ht or (1, a) not in ht for d, a in sel):
            return None
        h.quant = np.stack([qt[c[3]] for c in comps])
        h.huff = [t for d, a in sel for t in (ht[(0, d)], ht[(1, a)])]
        h.scan_lo = i + L
        # the scan ends at the first marker that is no restart marker; a second scan or a DNL makes the file foreign
        j = h.scan_lo
        while True:
            j = b.find(b"\xff", j)
            if j < 0 or j + 1 >= n:
                j = n
                break
            if b[j + 1] == 0 or 0xD0 <= b[j + 1] <= 0xD7 or b[j + 1] == 0xFF:
                j += 1 if b[j + 1] == 0xFF else 2
                continue
            if b[j + 1] != 0xD9:
                return None
            break
        h.scan_hi = j
        return h
    except (IndexError, ValueError):
        return None


# ------------------------------------------------------------------------------------------------------ Huffman records
_HUFF_CACHE = {}


def huff_record(bits, vals):
    """one table as the HUFF_BYTES record of csrc/jpeg_common.h (u8 array): 9-bit lookup, maxcode / valoff per length, vals"""
    key = (bytes(bits), bytes(vals))
    rec = _HUFF_CACHE.get(key)
    if rec is not None:
        return rec
    look = np.zeros(1 << LOOK_BITS, np.uint16)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    v = np.zeros(256, np.uint8)
    v[:len(key[1])] = np.frombuffer(key[1], np.uint8)
    code = k = 0
    for l in range(1, 17):
        cnt = key[0][l - 1]
        valoff[l] = k - code
        for _ in range(cnt):
            if l <= LOOK_BITS and code < (1 << l):
                look[code << (LOOK_BITS - l):(code + 1) << (LOOK_BITS - l)] = (l << 8) | key[1][k]
            code += 1
            k += 1
        if cnt and code - 1 < (1 << l):
            maxcode[l] = code - 1
        code <<= 1
    rec = np.concatenate([look.view(np.uint8), maxcode.view(np.uint8), valoff.view(np.uint8), v])
    assert rec.size == HUFF_BYTES
    rec.setflags(write=False)
    if len(_HUFF_CACHE) < 4096:
        _HUFF_CACHE[key] = rec
    return rec


def huff_records(header):
    """u8 [2 * ncomp * HUFF_BYTES]: DC, AC per component"""
    return np.concatenate([huff_record(*t) for t in header.huff])


# ------------------------------------------------------------------------------------------------------ the scan index
def scan_index(data, header, seg_mcus=DEFAULT_SEG_MCUS, name="<bytes>"):
    """int32 [S, ROW_INTS] entry points of the file's scan (radet_jpeg_index); ValueError naming the file for a corrupt one"""
    from .. import _lib
    seg = header.resolve_seg_mcus(seg_mcus)
    if seg < 1:
        raise ValueError(f"seg_mcus = {seg_mcus}")
    ri = header.restart_interval
    per = ri if ri else header.n_mcus
    max_rows = -(-header.n_mcus // per) * -(-per // seg)
    rows = np.empty((max_rows, ROW_INTS), np.int32)
    buf = np.frombuffer(data, np.uint8)
    huff = huff_records(header)
    blocks = np.array(header.comp_blocks, np.int32)
    fn = getattr(_lib.load(), "radet_jpeg_index")
    n = fn(buf.ctypes.data, header.scan_lo, header.scan_hi, header.ncomp, blocks.ctypes.data, huff.ctypes.data,
           header.n_mcus, ri, seg, rows.ctypes.data, max_rows)
    if n < 0:
        raise ValueError(f"{name}: corrupt JPEG scan: {ERRORS.get(-n, f'error {-n}')}")
    return rows[:n]


def rows_fit(rows, header):
    """whether index rows cover the header's frame and scan: consecutive segments over all MCUs, offsets inside the scan"""
    return bool(len(rows) and rows[0, 2] == 0 and (rows[:, 3] > 0).all() and int(rows[:, 3].sum()) == header.n_mcus
                and (np.diff(rows[:, 2]) == rows[:-1, 3]).all() and (rows[:, 0] >= header.scan_lo).all()
                and (rows[:, 0] <= header.scan_hi).all() and (rows[:, 7] >= rows[:, 0] * 8 + rows[:, 1]).all()
                and (rows[:, 7] <= header.scan_hi * 8).all())


class IndexCache:
    """scan indexes by (path, size, mtime, seg_mcus): in memory, and as .npy files in `directory` if one is given"""

    def __init__(self, directory=None):
        self.directory = directory
        self.mem = {}
        self.lock = threading.Lock()
        self.hits = self.misses = 0
        if directory:
            os.makedirs(directory, exist_ok=True)

    @staticmethod
    def key(path, seg_mcus):
        st = os.stat(path)
        return (os.path.abspath(path), st.st_size, st.st_mtime_ns, str(seg_mcus))

    def _file(self, key):
        return os.path.join(self.directory, hashlib.sha1(repr(key).encode()).hexdigest() + ".npy")

    def get(self, path, data, header, seg_mcus):
        key = self.key(path, seg_mcus)
        rows = self.mem.get(key)
        if rows is None and self.directory and os.path.exists(self._file(key)):
            rows = np.load(self._file(key), allow_pickle=False)
            if rows.ndim != 2 or rows.shape[1] != ROW_INTS or rows.dtype != np.int32 or not rows_fit(rows, header):
                rows = None                         # (a stale or foreign file: walk again and replace it)
        if rows is not None:
            with self.lock:
                self.hits += 1
                self.mem[key] = rows
            return rows
        rows = scan_index(data, header, seg_mcus, path)
        rows.setflags(write=False)
        if self.directory:
            tmp = self._file(key) + f".{os.getpid()}.{threading.get_ident()}.tmp"
            with open(tmp, "wb") as fh:
                np.save(fh, rows)
            os.replace(tmp, self._file(key))
        with self.lock:
            self.misses += 1
            self.mem[key] = rows
        return rows


class DeviceJpeg:
    """a file planned for the device decoder: its bytes, header and index rows; `.shape` is the decoded image's"""
    __slots__ = ("path", "data", "header", "rows", "shape")

    def __init__(self, path, data, header, rows):
        self.path, self.data, self.header, self.rows = path, data, header, rows
        self.shape = (header.height, header.width, 3)


def plan_file(path, cache, seg_mcus=DEFAULT_SEG_MCUS):
    """DeviceJpeg of a supported file, None of any other (the caller decodes that one on the host)"""
    with open(path, "rb") as fh:
        data = fh.read()
    header = parse_jpeg(data)
    if header is None:
        return None
    return DeviceJpeg(path, data, header, cache.get(path, data, header, seg_mcus))


# ------------------------------------------------------------------------------------------------------ a batch's buffer
def _align(n, a=16):
    return -(-n // a) * a


def pack_batch(items, dst_offs):
    """One u8 host buffer with everything radet_jpeg_decode reads for `items` (DeviceJpeg) whose pixels go to the pixel
    offsets `dst_offs` of the packed destination, and the section table.  Returns (blob u8, sections: name -> (byte offset,
    byte length), sizes: dict(n_wg, n_rows, coef_blocks, plane_bytes, max_blocks, max_px))."""
    n = len(items)
    desc = np.zeros((n, DESC_INTS), np.int32)
    quant = np.zeros((n, 3, 64), np.uint16)
    huff = np.zeros((n, 6 * HUFF_BYTES), np.uint8)
    wgs, rows = [], []
    foff = boff = poff = roff = 0
    max_blocks = max_px = 0
    for k, (it, dst) in enumerate(zip(items, dst_offs)):
        h = it.header
        d = desc[k]
        d[0:9] = [foff, h.scan_hi, h.width, h.height, h.ncomp, h.hs, h.vs, h.mcux, h.mcuy]
        for c in range(h.ncomp):
            nb = h.n_mcus * (h.hs * h.vs if c == 0 else 1)
            d[9 + c], d[12 + c] = boff, poff
            boff += nb
            poff += nb * 64
            max_blocks = max(max_blocks, nb)
        d[15], d[16], d[17] = dst, roff, len(it.rows)
        quant[k, :h.ncomp] = h.quant
        huff[k, :2 * h.ncomp * HUFF_BYTES] = huff_records(h)
        wgs += [(k, r) for r in range(roff, roff + len(it.rows), 64)]
        rows.append(it.rows)
        roff += len(it.rows)
        foff += len(it.data)
        max_px = max(max_px, h.width * h.height)
    parts = [("huff", huff.reshape(-1)), ("quant", quant.reshape(-1).view(np.uint8)), ("desc", desc.reshape(-1).view(np.uint8)),
             ("wgs", np.array(wgs, np.int32).reshape(-1).view(np.uint8)),
             ("rows", np.concatenate(rows).reshape(-1).view(np.uint8)), ("err", np.zeros(4 * n, np.uint8)),
             ("files", np.frombuffer(b"".join(it.data for it in items), np.uint8))]
    sections, o = {}, 0
    for name, a in parts:
        sections[name] = (o, a.size)
        o = _align(o + a.size)
    blob = np.zeros(o, np.uint8)
    for name, a in parts:
        blob[sections[name][0]:sections[name][0] + a.size] = a
    sizes = dict(n_wg=len(wgs), n_rows=roff, coef_blocks=boff, plane_bytes=poff, max_blocks=max_blocks, max_px=max_px)
    return blob, sections, sizes

