"""The sample cache of an ImagePipeline (sample_cache="device"): decoded frames and backgrounds resident in HBM, and the
mask PNGs of LoadAnnotations(with_bop_mask=True) as run lists in host memory.

Pixels.  The first time a file is seen it is decoded by whatever path the pipeline is configured for; ImagePipeline.run
then copies its u8 BGR pixels (source size, before Resize) from the batch's packed source buffer into an arena of
fixed-size u8 device chunks, allocated lazily up to `cache_bytes`.  Entries start at multiples of 256 bytes and never
span chunks.  Nothing is evicted: an entry the budget cannot hold, or one larger than a chunk, is not cached
(`rejected_full`) and that file keeps being decoded.  From then on `lookup` (on a loader thread: one stat, no open)
returns a CachedImage placeholder -- `.shape` and the entry's device address, like jpeg.DeviceJpeg for its plans -- and
run() gathers all hits of a batch into the packed buffer with one radet_copy_segments launch.

Keys are (realpath, st_size, st_mtime_ns).  A file whose key changed is a miss: its old entry leaves the table
(`invalidated`), its bytes stay where they are and are not reused.

Threads: loader threads read the table, run() inserts on the calling thread; both under one lock, and an entry is entered
only after its copy has been enqueued.  Streams: insertions and gathers run on the stream current in run(); the cache
keeps an event behind its last insertion, and a call on another stream makes that stream wait for it (no host wait).

Masks.  `normalised_runs` turns a decoded mask PNG into the COCO run list of the bitmap that radet_mask_max +
radet_mask_transform(normalize=True) produce from it: 1 where the value equals the mask's own maximum, nothing for an
all-zero mask.  The run lists are kept by the same keys; their bytes are counted (`mask_bytes`) but not against
cache_bytes."""
import os
import threading

import numpy as np

from ..core import rle

ALIGN = 256
DEFAULT_CHUNK_BYTES = 256 << 20
COUNTERS = ("hits", "misses", "inserted", "bytes", "rejected_full", "invalidated", "mask_hits", "mask_bytes")


def cache_args(sample_cache, cache_bytes):
    """the checked (sample_cache, cache_bytes) options of a dataset config / ImagePipeline"""
    if sample_cache not in (None, "device"):
        raise ValueError(f"sample_cache is None or 'device', got {sample_cache!r}")
    if sample_cache is None:
        if cache_bytes is not None:
            raise ValueError("cache_bytes is the budget of sample_cache='device'")
        return None, None
    if isinstance(cache_bytes, bool) or not isinstance(cache_bytes, (int, np.integer)) or cache_bytes <= 0:
        raise ValueError(f"sample_cache='device' needs cache_bytes, the HBM budget in bytes (a positive int), got {cache_bytes!r}")
    return sample_cache, int(cache_bytes)


def file_key(path):
    real = os.path.realpath(path)
    st = os.stat(real)
    return real, st.st_size, st.st_mtime_ns


def normalised_runs(mask):
    """u8 [H, W] mask as decoded -> counts of (mask / mask.max()).astype(u8): set where the value equals the maximum; an
    all-zero mask is 0 / 0 = NaN -> 0 everywhere (csrc/masks.hip: mask_transform_kernel)"""
    m = np.asarray(mask)
    mx = m.max() if m.size else 0
    return rle.rle_from_mask((m == mx) if mx else np.zeros(m.shape, bool))


class CachedImage:
    """a cache hit planned for ImagePipeline.run: `.shape` is the decoded image's, `.addr` the device address of its pixels"""
    __slots__ = ("path", "shape", "addr", "nbytes")

    def __init__(self, path, shape, addr, nbytes):
        self.path, self.shape, self.addr, self.nbytes = path, shape, addr, nbytes


def _device_alloc(nbytes):
    import torch
    return torch.empty(nbytes, dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))


class SampleCache:
    def __init__(self, cache_bytes, chunk_bytes=DEFAULT_CHUNK_BYTES, alloc=None):
        """cache_bytes: budget of the pixel arena; chunk_bytes: size of one arena chunk (the largest entry the cache takes);
        alloc(nbytes) -> u8 tensor: the chunk allocator (default: the current device)"""
        _, self.cache_bytes = cache_args("device", cache_bytes)
        if chunk_bytes <= 0:
            raise ValueError(f"chunk_bytes = {chunk_bytes}")
        self.chunk_bytes = int(chunk_bytes)
        self.alloc = alloc or _device_alloc
        self.chunks, self.allocated, self.fill = [], 0, 0
        self.table, self.mask_table = {}, {}
        self.stats = dict.fromkeys(COUNTERS, 0)
        self.lock = threading.Lock()
        self._event = self._stream = None

    # ------------------------------------------------------------------------------------------------ table (any thread)
    def lookup(self, path):
        """(CachedImage of a cached file or None, the file's key); stat only"""
        key = file_key(path)
        with self.lock:
            e = self.table.get(key[0])
            if e is not None and e[0] == key[1:]:
                self.stats["hits"] += 1
                return CachedImage(key[0], *e[1]), key
            if e is not None:
                del self.table[key[0]]
                self.stats["invalidated"] += 1
            self.stats["misses"] += 1
        return None, key

    def drop(self, path):
        """forget a file (its device decode failed after it was entered)"""
        with self.lock:
            self.table.pop(os.path.realpath(path), None)

    def mask_lookup(self, path, hw):
        """(run list of a cached mask file of h x w or None, the file's key)"""
        key = file_key(path)
        with self.lock:
            e = self.mask_table.get(key[0])
            if e is not None and e[0] == key[1:] and e[2] == tuple(hw):
                return e[1], key
            if e is not None:
                del self.mask_table[key[0]]
                self.stats["mask_bytes"] -= e[1].nbytes
                self.stats["invalidated"] += 1
        return None, key

    def mask_insert(self, key, counts, hw):
        counts = np.ascontiguousarray(counts, np.int64)
        counts.setflags(write=False)
        with self.lock:
            if key[0] not in self.mask_table:
                self.mask_table[key[0]] = (key[1:], counts, tuple(hw))
                self.stats["mask_bytes"] += counts.nbytes

    def count_mask_hits(self, n):
        with self.lock:
            self.stats["mask_hits"] += n

    # ------------------------------------------------------------------------------------------------ arena (run()'s thread)
    def _reserve(self, nbytes):
        """device address of `nbytes` fresh arena bytes, or None when the budget or the chunk size does not allow them"""
        if nbytes > self.chunk_bytes:
            return None
        off = -(-self.fill // ALIGN) * ALIGN
        if not self.chunks or off + nbytes > self.chunks[-1].numel():
            size = min(self.chunk_bytes, self.cache_bytes - self.allocated)
            if size < nbytes:
                return None
            self.chunks.append(self.alloc(size))
            base = self.chunks[-1].data_ptr()
            if base % ALIGN:
                raise RuntimeError("the allocator returned a chunk that is not 256-byte aligned")
            self.allocated += size
            off = 0
        self.fill = off + nbytes
        return self.chunks[-1].data_ptr() + off

    def reserve(self, items):
        """items: (key, shape) of newly decoded files.  Returns [(key, shape, arena address, bytes)] for those that are not
        in the table yet and fit; the caller copies the pixels there and then calls commit()"""
        out, seen = [], set()
        for key, shape in items:
            nbytes = int(np.prod(shape))
            with self.lock:
                e = self.table.get(key[0])
                if key[0] in seen or (e is not None and e[0] == key[1:]) or nbytes == 0:
                    continue                      # (twice in one batch, or entered while this sample was being planned)
            addr = self._reserve(nbytes)
            if addr is None:
                with self.lock:
                    self.stats["rejected_full"] += 1
                continue
            seen.add(key[0])
            out.append((key, tuple(shape), addr, nbytes))
        return out

    def commit(self, reserved):
        with self.lock:
            for key, shape, addr, nbytes in reserved:
                self.table[key[0]] = (key[1:], (shape, addr, nbytes))
                self.stats["inserted"] += 1
                self.stats["bytes"] += nbytes

    # ------------------------------------------------------------------------------------------------ device (run()'s thread)
    def wait_inserts(self):
        """the current stream waits for the last insertion if that ran on another stream"""
        import torch
        if self._event is not None and self._stream != torch.cuda.current_stream():
            torch.cuda.current_stream().wait_event(self._event)

    def record_insert(self):
        import torch
        self._event = torch.cuda.Event()
        self._event.record()
        self._stream = torch.cuda.current_stream()

    @staticmethod
    def copy(rows, dev):
        """rows of (source address, destination address, bytes): one pinned upload of the table, one launch"""
        import torch
        from .. import kernels as K
        table, tiles = K.copy_segments_table(rows)
        desc = torch.from_numpy(table).pin_memory().to(dev, non_blocking=True)
        K.copy_segments(desc, len(table), tiles)
