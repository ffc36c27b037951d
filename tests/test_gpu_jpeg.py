"""radet_jpeg_decode on the GPU against Pillow on the host: the case matrix of tests/_jpeg_ref.py decoded in ONE batch
(mixed sizes, samplings, table sets and segment lengths), with and without the mix pipelines' 4-pixel alignment, a batch
with a file the device does not take, and the stage under synchronising-calls-are-errors.  Every comparison is
array_equal.  Corrupt streams are the CPU walker's business (tests/test_jpeg_cpu.py): none is sent to the device."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytest.importorskip("PIL", reason="Pillow writes the JPEG fixtures")
import _jpeg_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """(paths, host pixels per file, segment length per file): the matrix, written once; the segment lengths cycle through
    1, 2, 8, one MCU row and one segment for the whole image"""
    from radet_amd.datasets.loading import decode_bgr
    root = tmp_path_factory.mktemp("jpeg")
    paths, want, segs = [], [], []
    for k, (name, d) in enumerate(R.matrix().items()):
        p = str(root / (name + ".jpg"))
        open(p, "wb").write(d)
        paths.append(p)
        want.append(decode_bgr(p))
        want[-1].setflags(write=False)
        segs.append((1, 2, 8, "row", 1 << 20)[k % 5])
    # beyond the matrix: images with more segments than a workgroup has lanes (64), so that an image spans workgroups
    for name, d, seg in (("wide-444", R.encode("checker", 136, 72, "444", 90, seed=1), 1),
                         ("wide-420", R.encode("noise", 250, 130, "420", 85, optimize=True, restart=2, seed=2), 1)):
        p = str(root / (name + ".jpg"))
        open(p, "wb").write(d)
        paths.append(p)
        want.append(decode_bgr(p))
        segs.append(seg)
    return paths, want, segs


def _pipeline():
    from radet_amd.datasets.loading import ImagePipeline
    return ImagePipeline([dict(type="LoadImageFromFile", decode="device"), dict(type="Normalize", **NORM),
                          dict(type="Collect", keys=["img"])])


def _decode(pipe, paths, segs, align, no_sync=False):
    from radet_amd.core import jpeg
    from radet_amd.datasets.loading import decode_bgr
    cache = jpeg.IndexCache()
    sources = [jpeg.plan_file(p, cache, s) for p, s in zip(paths, segs)]
    sources = [decode_bgr(p) if s is None else s for p, s in zip(paths, sources)]
    dev = torch.device("cuda", torch.cuda.current_device())
    if no_sync:
        torch.cuda.set_sync_debug_mode("error")
    try:
        src, offs = pipe._decode_packed(sources, dev, align=align)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    pipe.check_decode_errors(wait=True)
    host = src.cpu().numpy()
    return [host[o * 3:o * 3 + a.shape[0] * a.shape[1] * 3].reshape(a.shape) for o, a in zip(offs, sources)], offs, sources


@pytest.mark.parametrize("align", [1, 4])
def test_matrix_in_one_batch(batch, align):
    from radet_amd import _lib
    from radet_amd.core import jpeg
    paths, want, segs = batch
    pipe = _pipeline()
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        got, offs, sources = _decode(pipe, paths, segs, align, no_sync=True)
    finally:
        _lib.call = call
    assert seen == ["radet_jpeg_decode"]                                     # one call = three launches, whatever the batch
    assert all(o % align == 0 for o in offs) and (align == 1) == any(o % 4 for o in offs)
    assert pipe.decode_stats == dict(device=len(paths), fallback=0)
    # the batch holds a one-MCU image, single-segment indexes, seg_mcus = 1 indexes with many rows
    assert any(s.header.n_mcus == 1 for s in sources)
    assert any(len(s.rows) == 1 and s.header.n_mcus > 1 for s in sources)
    assert any(len(s.rows) == s.header.n_mcus > 64 for s in sources)          # more segments than a workgroup has lanes
    assert len({(s.header.hs, s.header.vs, s.header.ncomp) for s in sources}) == 4
    assert len({bytes(jpeg.huff_records(s.header)) for s in sources}) > 4     # optimised tables: many table sets
    for p, g, w in zip(paths, got, want):
        assert g.shape == w.shape and np.array_equal(g, w), os.path.basename(p)


def test_fallback_in_the_batch(batch, tmp_path):
    paths, want, segs = batch
    from radet_amd.datasets.loading import decode_bgr
    prog = str(tmp_path / "progressive.jpg")
    open(prog, "wb").write(R.encode("checker", 37, 51, "420", 75, progressive=True))
    some = list(range(0, len(paths), 29))
    ps = [paths[i] for i in some[:3]] + [prog] + [paths[i] for i in some[3:]]
    ws = [want[i] for i in some[:3]] + [decode_bgr(prog)] + [want[i] for i in some[3:]]
    pipe = _pipeline()
    got, _, _ = _decode(pipe, ps, [8] * len(ps), 4)
    assert pipe.decode_stats == dict(device=len(ps) - 1, fallback=1)
    for p, g, w in zip(ps, got, ws):
        assert np.array_equal(g, w), os.path.basename(p)


def test_stages_split(batch):
    """the three launches one at a time (the benchmark times them so) give the same bytes"""
    from radet_amd import kernels as K
    from radet_amd.core import jpeg
    paths, want, _ = batch
    cache = jpeg.IndexCache()
    items = [jpeg.plan_file(p, cache, "row") for p in paths[-12:]]
    offs = np.cumsum([0] + [it.shape[0] * it.shape[1] for it in items])
    blob, sections, sizes = jpeg.pack_batch(items, offs[:-1])
    dev = torch.device("cuda", torch.cuda.current_device())
    blob = torch.from_numpy(blob).to(dev)
    dst = torch.empty(int(offs[-1]) * 3, dtype=torch.uint8, device=dev)
    err, coef, planes = K.jpeg_decode(blob, sections, sizes, len(items), dst)
    ref = dst.clone()
    dst.zero_()
    K.jpeg_decode(blob, sections, sizes, len(items), dst, stages=2, work=(coef, planes))
    K.jpeg_decode(blob, sections, sizes, len(items), dst, stages=4, work=(coef, planes))
    assert torch.equal(dst, ref) and int(err.abs().sum()) == 0
    host = ref.cpu().numpy()
    for it, o, w in zip(items, offs, want[-12:]):
        assert np.array_equal(host[o * 3:o * 3 + w.size].reshape(w.shape), w)


def test_error_word_reaches_the_host_and_names_the_file(batch):
    """A valid stream under an index row whose end position is wrong (the consistency check of a segment, not a fault:
    every read and write stays where it was): error 32 for that image only, raised by the next call or the drain, with the
    file's name; the pixels of the batch are decoded all the same."""
    from radet_amd.core import jpeg
    paths, want, _ = batch
    cache = jpeg.IndexCache()
    some = [paths[i] for i in (5, 77, 200)]
    items = [jpeg.plan_file(p, cache, 8) for p in some]
    rows = items[1].rows.copy()
    rows[-1, 7] += 1
    items[1] = jpeg.DeviceJpeg(items[1].path, items[1].data, items[1].header, rows)
    pipe = _pipeline()
    dev = torch.device("cuda", torch.cuda.current_device())
    src, offs = pipe._decode_packed(items, dev)
    with pytest.raises(ValueError) as e:
        pipe.check_decode_errors(wait=True)
    assert some[1] in str(e.value) and some[0] not in str(e.value) and some[2] not in str(e.value)
    assert "does not end where its index entry says" in str(e.value)
    pipe.check_decode_errors(wait=True)                                   # (reported once)
    host = src.cpu().numpy()
    for k, i in enumerate((5, 77, 200)):
        assert np.array_equal(host[offs[k] * 3:offs[k] * 3 + want[i].size].reshape(want[i].shape), want[i])


def test_all_fallback_batch_is_counted(tmp_path):
    """a decode='device' pipeline whose files all go to the host decoder: counted, no decode launch, the host's pixels"""
    import random
    from radet_amd import _lib
    from radet_amd.datasets.loading import decode_bgr
    p = str(tmp_path / "progressive.jpg")
    open(p, "wb").write(R.encode("checker", 48, 64, "420", 75, progressive=True))
    pipe = _pipeline()
    planned = [pipe.plan(dict(img_info=dict(filename=p), img_prefix=None, bbox_fields=[], mask_fields=[], seg_fields=[]),
                         random.Random(0), np.random.RandomState(0)) for _ in range(2)]
    seen, call = [], _lib.call
    _lib.call = lambda name, *a: seen.append(name) or call(name, *a)
    try:
        out = pipe.run(planned)
    finally:
        _lib.call = call
    assert "radet_jpeg_decode" not in seen and pipe.decode_stats == dict(device=0, fallback=2)
    ref = _host_pipeline().run([_host_pipeline().plan(dict(img_info=dict(filename=p), img_prefix=None, bbox_fields=[],
                                                           mask_fields=[], seg_fields=[]), random.Random(0), np.random.RandomState(0))])
    assert torch.equal(out[0]["img"], ref[0]["img"]) and np.array_equal(planned[0]["img"], decode_bgr(p))


def _host_pipeline():
    from radet_amd.datasets.loading import ImagePipeline
    return ImagePipeline([dict(type="LoadImageFromFile"), dict(type="Normalize", **NORM), dict(type="Collect", keys=["img"])])


def test_symbols_are_exported():
    from radet_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "radet_jpeg_decode") and hasattr(lib, "radet_jpeg_index")
