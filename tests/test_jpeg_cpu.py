"""The host side of device JPEG decoding, without a GPU: the NumPy restatement of the decoder (tests/_jpeg_ref.py) against
Pillow on the whole case matrix, the C scan walker against the Python walker, the index cache, the walker as validator and
parse_jpeg's routing of foreign files to the host decoder."""
import io
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytest.importorskip("PIL", reason="Pillow writes the JPEG fixtures")
import _jpeg_ref as R  # noqa: E402
from radet_amd.core import jpeg  # noqa: E402


@pytest.fixture(scope="module")
def files():
    return R.matrix()


@pytest.fixture(scope="module")
def walked(files):
    """name -> (header, rows at seg_mcus = 1, stats, coefficient blocks): one walk per file, shared"""
    out = {}
    for name, d in files.items():
        h = jpeg.parse_jpeg(d)
        assert h is not None, name
        out[name] = (h,) + R.walk(d, h, 1, decode=True)
    return out


def test_matrix_covers_the_issue(files):
    names = list(files)
    for w, h in R.SIZES:
        for s in R.SAMPLINGS:
            sub = [n for n in names if n.startswith(f"{w}x{h}-{s}-")]
            assert {n.split("-")[2] for n in sub} == {"q10", "q75", "q95", "q100"}
            assert {n.split("-")[3] for n in sub} == set(R.CONTENTS)
            assert {n.split("-")[4] for n in sub} == {"o0", "o1"} and {n.split("-")[5] == "r0" for n in sub} == {True, False}


def test_restatement_equals_pillow(files):
    for name, d in files.items():
        got, want = R.decode_bgr(d), R.pillow_bgr(d)
        assert got.shape == want.shape and np.array_equal(got, want), name


def test_fixtures_are_not_easy(files, walked):
    scans = {n: files[n][walked[n][0].scan_lo:walked[n][0].scan_hi] for n in files}
    assert any(b"\xff\x00" in s for s in scans.values())                                   # byte stuffing
    assert any(walked[n][2]["ac"][0xF0] > 0 for n in files)                                # a ZRL symbol
    assert any(walked[n][2]["max_len"] > 8 for n in files)                                 # a code the 8-bit lookups miss
    assert any(walked[n][2]["max_len"] > jpeg.LOOK_BITS for n in files)                    # ... and this decoder's 9-bit lookup
    # a non-zero DC predictor at an entry that is no restart point: a file without restart markers, an entry past MCU 0
    assert any(((walked[n][1][:, 2] > 0) & (walked[n][1][:, 4:7] != 0).any(1)).any()
               for n in files if not walked[n][0].restart_interval)
    assert any(walked[n][0].restart_interval for n in files) and any(not walked[n][0].restart_interval for n in files)


def test_c_walker_equals_python_walker(files, walked):
    for name, d in files.items():
        h = walked[name][0]
        for seg in (1, 2, 8, "row"):
            want = walked[name][1] if seg == 1 else R.walk(d, h, seg)[0]
            got = jpeg.scan_index(d, h, seg, name)
            assert got.dtype == np.int32 and np.array_equal(got, want), (name, seg)
            assert int(got[:, 3].sum()) == h.n_mcus and (np.diff(got[:, 2]) == got[:-1, 3]).all()


def test_huffman_records(files, walked):
    """the 9-bit lookup and the maxcode / valoff arrays of a record decode every code of the table"""
    for name in list(files)[::17]:
        for bits, vals in walked[name][0].huff:
            rec = jpeg.huff_record(bits, vals)
            look = rec[:1024].view(np.uint16)
            maxcode, valoff = rec[1024:1096].view(np.int32), rec[1096:1168].view(np.int32)
            v = rec[1168:]
            for (l, code), sym in R.code_table(bits, vals).items():
                if l <= jpeg.LOOK_BITS:
                    assert look[code << (jpeg.LOOK_BITS - l)] == (l << 8 | sym)
                assert code <= maxcode[l] and v[code + valoff[l]] == sym


def test_index_cache_round_trip(files, tmp_path):
    name = next(n for n in files if n.startswith("48x64-420-q95"))
    path = str(tmp_path / "a.jpg")
    open(path, "wb").write(files[name])
    cache = jpeg.IndexCache(str(tmp_path / "idx"))
    a = jpeg.plan_file(path, cache, 8)
    assert (cache.hits, cache.misses) == (0, 1) and len(os.listdir(tmp_path / "idx")) == 1
    fresh = jpeg.IndexCache(str(tmp_path / "idx"))                 # another process: from the directory, no walk
    seen, walk = [], jpeg.scan_index
    jpeg.scan_index = lambda *a, **k: seen.append(1) or walk(*a, **k)
    try:
        b = jpeg.plan_file(path, fresh, 8)
        c = jpeg.plan_file(path, fresh, 8)                         # from memory
        d = jpeg.plan_file(path, fresh, 2)                         # another segment length: another index
    finally:
        jpeg.scan_index = walk
    assert (fresh.hits, fresh.misses) == (2, 1) and seen == [1]
    assert np.array_equal(a.rows, b.rows) and c.rows is b.rows and len(d.rows) > len(a.rows)
    assert a.shape == (64, 48, 3)


def _noise(sampling="420", restart=0, **kw):
    return R.encode("noise", 48, 64, sampling, 95, restart=restart, seed=3, **kw)


def test_walker_rejects_corrupt_scans():
    d = _noise()
    h = jpeg.parse_jpeg(d)
    # truncated: the scan loses its second half (the header keeps the frame size)
    cut = d[:h.scan_lo + (h.scan_hi - h.scan_lo) // 2] + b"\xff\xd9"
    with pytest.raises(ValueError, match="cut.jpg.*ends early"):
        jpeg.scan_index(cut, jpeg.parse_jpeg(cut), 8, "cut.jpg")
    with pytest.raises(R.Corrupt):
        R.walk(cut, jpeg.parse_jpeg(cut), 8)
    # a flipped byte that yields an undefined code: all ones is no code of a JPEG table; sixteen of them reach no symbol
    k = (h.scan_lo + h.scan_hi) // 2
    flipped = d[:k] + b"\xff\x00\xff\x00\xff\x00" + d[k + 6:]
    assert jpeg.parse_jpeg(flipped) is not None
    with pytest.raises(ValueError, match="flip.jpg.*undefined Huffman code"):
        jpeg.scan_index(flipped, jpeg.parse_jpeg(flipped), 8, "flip.jpg")
    # a missing restart marker: the second one renumbered
    r = _noise(restart=1)
    hr = jpeg.parse_jpeg(r)
    assert hr.restart_interval > 0
    k = r.index(b"\xff\xd1", hr.scan_lo)
    broken = r[:k] + b"\xff\xd3" + r[k + 2:]
    with pytest.raises(ValueError, match="rst.jpg.*restart marker out of sequence"):
        jpeg.scan_index(broken, jpeg.parse_jpeg(broken), 8, "rst.jpg")
    # ... and removed altogether
    gone = r[:k] + r[k + 2:]
    with pytest.raises(ValueError, match="gone.jpg"):
        jpeg.scan_index(gone, jpeg.parse_jpeg(gone), 8, "gone.jpg")


def test_foreign_files_go_to_the_host_decoder(tmp_path):
    from PIL import Image
    a = R.content("ramp", 24, 32, 0)

    def saved(fmt, im, **kw):
        buf = io.BytesIO()
        im.save(buf, fmt, **kw)
        return buf.getvalue()
    foreign = dict(progressive=R.encode("ramp", 32, 24, "420", 90, progressive=True),
                   png=saved("PNG", Image.fromarray(a)),
                   rgb=saved("JPEG", Image.fromarray(a), keep_rgb=True, quality=90),
                   cmyk=saved("JPEG", Image.fromarray(a).convert("CMYK"), quality=90),
                   empty=b"", short=b"\xff\xd8\xff", headless=b"\xff\xd8\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00")
    for name, d in foreign.items():
        assert jpeg.parse_jpeg(d) is None, name
    assert jpeg.parse_jpeg(R.encode("ramp", 32, 24, "420", 90)) is not None
    # plan_file hands such a file back to the caller, who decodes it on the host
    path = str(tmp_path / "p.jpg")
    open(path, "wb").write(foreign["progressive"])
    assert jpeg.plan_file(path, jpeg.IndexCache(), 8) is None


def test_default_stage_plans_as_before(tmp_path):
    """LoadImageFromFile() without arguments: host pixels in s['img']; decode='device': a plan with the same shape, and the
    host pixels for a progressive file"""
    import random
    from radet_amd.datasets.loading import LoadImageFromFile, decode_bgr
    d = R.encode("checker", 37, 51, "420", 75)
    open(tmp_path / "a.jpg", "wb").write(d)
    open(tmp_path / "p.jpg", "wb").write(R.encode("checker", 37, 51, "420", 75, progressive=True))

    def plan(stage, name):
        s = dict(img_info=dict(filename=name), img_prefix=str(tmp_path))
        stage.plan(s, random.Random(0), np.random.RandomState(0))
        return s
    s = plan(LoadImageFromFile(), "a.jpg")
    assert isinstance(s["img"], np.ndarray) and np.array_equal(s["img"], decode_bgr(str(tmp_path / "a.jpg")))
    assert s["img_shape"] == s["ori_shape"] == s["pad_shape"] == (51, 37, 3)
    t = plan(LoadImageFromFile(decode="device"), "a.jpg")
    assert isinstance(t["img"], jpeg.DeviceJpeg) and t["img_shape"] == t["ori_shape"] == t["pad_shape"] == (51, 37, 3)
    assert {k: v for k, v in t.items() if k != "img"} == {k: v for k, v in s.items() if k != "img"}
    u = plan(LoadImageFromFile(decode="device"), "p.jpg")
    assert isinstance(u["img"], np.ndarray) and np.array_equal(u["img"], decode_bgr(str(tmp_path / "p.jpg")))
    with pytest.raises(ValueError):
        LoadImageFromFile(decode="gpu")


def test_stale_index_file_is_replaced(files, tmp_path):
    """an index file that does not cover the frame (another file's rows under this key) is walked again, not used"""
    name = next(n for n in files if n.startswith("48x64-420-q95"))
    path = str(tmp_path / "a.jpg")
    open(path, "wb").write(files[name])
    d = str(tmp_path / "idx")
    good = jpeg.plan_file(path, jpeg.IndexCache(d), 8).rows
    (f,) = os.listdir(d)
    for bad in (good[:-1], good[:, ::-1].copy(), np.concatenate([good, good])):
        np.save(os.path.join(d, f), bad)
        cache = jpeg.IndexCache(d)
        assert np.array_equal(jpeg.plan_file(path, cache, 8).rows, good) and (cache.hits, cache.misses) == (0, 1)
        assert np.array_equal(np.load(os.path.join(d, f)), good)
    h = jpeg.parse_jpeg(files[name])
    assert jpeg.rows_fit(good, h) and not jpeg.rows_fit(good[1:], h) and not jpeg.rows_fit(good[:0], h)


def test_sixteen_bit_quantisation_tables_go_to_the_host_decoder(files):
    """Pq = 1 belongs to 12-bit files; the device dequantises 8-bit tables only"""
    d = files[next(n for n in files if n.startswith("16x16-444-q75"))]
    k = d.index(b"\xff\xdb")
    n = (d[k + 2] << 8) | d[k + 3]
    seg = d[k + 4:k + 2 + n]
    wide, j = b"", 0
    while j < len(seg):
        wide += bytes([0x10 | seg[j]]) + b"".join(bytes([0, v]) for v in seg[j + 1:j + 65])
        j += 65
    d16 = d[:k + 2] + bytes([(len(wide) + 2) >> 8, (len(wide) + 2) & 255]) + wide + d[k + 2 + n:]
    assert jpeg.parse_jpeg(d) is not None and jpeg.parse_jpeg(d16) is None


def test_index_tool_writes_what_the_pipeline_reads(tmp_path):
    """tools/jpeg_index.py <config>: a dataset built on the same index_cache afterwards plans every frame and background
    without a walk"""
    import random
    import subprocess
    from radet_amd.datasets import build_dataset
    from tools.synth_bop import write_tree
    t = write_tree(str(tmp_path / "bop"), n_frames=3, objects=(1, 2), n_backgrounds=2, seed=3, size=(64, 48))
    norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
    data = dict(type="BOPDataset", ann_file=t["ann_file"], img_prefix=t["img_prefix"], filter_empty_gt=False,
                pipeline=[dict(type="LoadImageFromFile"), dict(type="RandomBackground", background_dir=t["background_dir"], prob=1.0),
                          dict(type="Normalize", **norm), dict(type="Collect", keys=["img"])])
    cfg = str(tmp_path / "cfg.py")
    open(cfg, "w").write(f"data = dict(train={data!r})\n")
    idx = str(tmp_path / "idx")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "jpeg_index.py"), cfg, "--index-cache", idx, "--seg-mcus", "8"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "5 indexes" in r.stdout, r.stdout + r.stderr
    assert len(os.listdir(idx)) == 5
    ds = build_dataset(dict(data, image_decode="device", index_cache=idx, seg_mcus=8))
    walk, seen = jpeg.scan_index, []
    jpeg.scan_index = lambda *a, **k: seen.append(1) or walk(*a, **k)
    try:
        planned = [ds.plan_sample(i, random.Random(i), np.random.RandomState(i)) for i in range(3)]
    finally:
        jpeg.scan_index = walk
    assert not seen and all(isinstance(s["img"], jpeg.DeviceJpeg) and isinstance(s["background"], jpeg.DeviceJpeg) for s in planned)
    assert len(os.listdir(idx)) == 5 and ds.pipeline.transforms[0].seg_mcus == 8


def test_loader_drains_the_error_words():
    """the decoder's pending error words are read when an epoch ends and when the loader closes (the last batch's too)"""
    from radet_amd.datasets.loader import DataLoader

    class Pipe:
        def __init__(self):
            self.calls = []

        def plan(self, results, rnd, nprnd):
            return results

        def run(self, planned, collate=False):
            self.calls.append("run")
            return planned

        def check_decode_errors(self, wait=False):
            self.calls.append(("check", wait))

    class DS:
        test_mode = True
        pipeline = Pipe()

        def __len__(self):
            return 4

        def plan_sample(self, i, rnd, nprnd):
            return i
    ds = DS()
    loader = DataLoader(ds, 2, 1, 0)
    assert len(list(loader)) == 2
    assert ds.pipeline.calls == ["run", "run", ("check", True)]
    loader.close()
    assert ds.pipeline.calls[-1] == ("check", True)
