"""The detection tables of the draw tests (tests/test_draw_cpu.py, tests/test_gpu_draw.py) on the scene of
tests/test_gpu_crops.py: frame 0 is 37 x 53 (h x w), frame 1 is 64 x 48, frame 2 is 40 x 50.  A row is (x1, y1, x2, y2, score,
label).  Frame 0 has count 0 unless a case says otherwise: its slots hold valid-looking boxes that must be ignored."""
import functools

import numpy as np

import _draw_ref as R

NAN, INF = float("nan"), float("inf")
THR = 0.3
NAMES = ("can", "box", "bottle", "a", "mug")
SHAPES = ((37, 53), (64, 48), (40, 50))
THICKNESSES = (1, 2, 3, 5)
IGNORED = [(2, 3, 20, 30, 0.9, 1)] * 3

# case -> dict(dets=[rows of frame 0, 1, 2], counts=..., and the style: names (False: the 'class N' text), colour ('class' or
# BGR), max_dets, font (False: font_size=0), atlas ('wide': names wider than the frames))
CASES = {
    # an interior box, one over each of the four edges, one wholly outside; a box thinner than the line (the hole is empty),
    # valid-looking slots beyond the count
    "edges": dict(dets=[IGNORED,
                        [(16, 24, 28, 36, 0.9, 0), (-6, 20, 9, 33, 0.8, 1), (15, -9, 30, 8, 0.7, 2), (40, 30, 55, 44, 0.6, 3),
                         (12, 55, 29, 70, 0.5, 4), (70, 80, 90, 95, 0.9, 0)],
                        [(20.25, 10.5, 21.5, 30.75, 0.8, 2), (5, 30, 40, 30.5, 0.7, 1), (1, 1, 9, 9, 0.9, 0), (1, 1, 9, 9, 0.9, 0)]],
                  counts=(0, 6, 2)),
    # NaN and inf coordinates, +-1e9 (valid after the clamp: its outline is out of sight, its label is not), x2 < x1, a score
    # below the threshold and one equal to it, a NaN score, a label of -1 and one past the names; a valid one behind them
    "invalid": dict(dets=[IGNORED,
                          [(NAN, 10, 30, 30, 0.9, 0), (10, 10, INF, 30, 0.9, 0), (-1e9, -1e9, 1e9, 1e9, 0.9, 1),
                           (30, 10, 10, 30, 0.9, 0), (10, 10, 30, 30, 0.2, 0), (8, 9, 31, 22, THR, 0), (5, 5, 20, 20, NAN, 0),
                           (5, 5, 20, 20, 0.9, -1), (5, 5, 20, 20, 0.9, 5), (5.5, 27.5, 33, 49, 0.6, 3)],
                          [(10, 30, 10, 12, 0.9, 0), (10, 10, 10, 10, 0.9, 2)]],
                    counts=(0, 10, 2)),
    # labels that overhang the right and the bottom edge and are moved into the frame; on frame 0 too
    "shifted": dict(dets=[[(40, 30, 50, 35, 0.95, 2), (-5, -5, 10, 10, 0.5, 0)],
                          [(38, 10, 46, 30, 0.9, 2), (5, 58, 30, 62, 0.8, 0), (40, 60, 47, 63, 0.7, 1)],
                          [(45, 36, 49, 39, 0.9, 4)]],
                    counts=(2, 3, 1)),
    # a label wider than the frame
    "wide": dict(dets=[IGNORED, [(10, 10, 30, 30, 0.9, 1), (20, 40, 40, 60, 0.8, 3)], [(5, 5, 45, 35, 0.9, 0)]],
                 counts=(0, 2, 1), atlas="wide"),
    # two outlines of different class colours that cross, two labels that overlap
    "crossing": dict(dets=[IGNORED,
                           [(8, 20, 30, 45, 0.9, 0), (20, 30, 42, 58, 0.8, 1), (10, 22, 28, 40, 0.7, 2)],
                           [(5, 5, 30, 30, 0.9, 3), (8, 7, 40, 35, 0.85, 4)]],
                     counts=(0, 3, 2), colour="class"),
    # 130 valid detections that all cover the pixel tile at the frame's origin: the hit list spans more than two wavefronts
    "many": dict(dets=[IGNORED,
                       [(i % 11, i % 7, 20 + i % 23, 14 + (i * 5) % 37, 0.99 - 0.005 * i, i % 5) for i in range(130)],
                       [(i % 13, i % 5, 15 + i % 31, 10 + (i * 3) % 25, 0.99 - 0.005 * i, (i * 3) % 5) for i in range(130)]],
                 counts=(0, 130, 130), colour="class"),
    # max_dets cuts a list (invalid ones in front do not count)
    "max_dets": dict(dets=[IGNORED,
                           [(NAN, 1, 2, 3, 0.9, 0), (4, 4, 20, 20, 0.9, 0), (10, 10, 10, 30, 0.1, 0), (22, 25, 40, 50, 0.8, 1),
                            (6, 30, 30, 60, 0.7, 2), (1, 1, 46, 62, 0.6, 3)],
                           [(1, 1, 9, 9, 0.9, 0), (12, 12, 30, 30, 0.9, 1), (20, 5, 45, 20, 0.9, 2), (3, 20, 25, 38, 0.9, 3)]],
                     counts=(0, 6, 4), max_dets=2),
    # the 'class N' text, one to five digits, a label of 100000 is refused; class colours without names
    "class_text": dict(dets=[[(3, 3, 30, 20, 0.31, 7)],
                             [(2, 2, 30, 14, 0.995, 0), (4, 18, 40, 30, 0.125, 42), (1, 33, 44, 45, 1.0, 123),
                              (3, 48, 45, 60, 0.304, 99999), (6, 6, 20, 20, 0.9, 100000)],
                             [(5, 5, 40, 30, 0.5, 1234)]],
                       counts=(1, 5, 1), names=False),
    "class_colour": dict(dets=[IGNORED, [(8, 20, 30, 45, 0.9, 0), (20, 30, 42, 58, 0.8, 12)], [(5, 5, 30, 30, 0.9, 3)]],
                         counts=(0, 2, 1), names=False, colour="class"),
    # no labels at all
    "nofont": dict(dets=[IGNORED, [(16, 24, 28, 36, 0.9, 0), (20, 30, 42, 58, 0.8, 1)], [(5, 5, 30, 30, 0.9, 3)]],
                   counts=(0, 2, 1), font=False),
}
BOX_COLOUR, TEXT_COLOUR = (72, 101, 241), (0, 255, 0)
FONT_SIZE = 13


def frames_host():
    """the three frames as host arrays: the bytes of tests/test_gpu_crops.py's scene (frame 2 is what the device view shows)"""
    import torch
    rng = np.random.RandomState(5)
    f0, f1 = (rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SHAPES[:2])
    big = torch.randint(0, 256, (60, 401), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    f2 = big.as_strided((40, 50, 3), (401, 3, 1), 5 * 401 + 8).numpy().copy()
    return [f0, f1, f2], big


def padded(case):
    """-> boxes f32 [3,K,4], scores f32 [3,K], labels i64 [3,K], counts i32 [3]"""
    c = CASES[case]
    Kd = max(len(d) for d in c["dets"])
    t = np.zeros((3, Kd, 6), np.float64)
    for b, d in enumerate(c["dets"]):
        t[b, :len(d)] = np.array(d, np.float64).reshape(-1, 6)
    return (np.ascontiguousarray(t[..., :4], np.float32), np.ascontiguousarray(t[..., 4], np.float32),
            np.ascontiguousarray(t[..., 5]).astype(np.int64), np.array(c["counts"], np.int32))


@functools.lru_cache(maxsize=None)
def atlas_for(case):
    c = CASES[case]
    if not c.get("font", True):
        return None
    n = len(NAMES) if c.get("names", True) else 0
    cov, widths = R.synthetic_atlas(n, Wa=70 if c.get("atlas") == "wide" else 19)
    if c.get("atlas") == "wide":
        widths[R.NAME0:] = [61, 70, 55, 66, 58]
    return cov, widths


def style_for(case, thickness):
    """the restatements' Style of a case; the keyword arguments of ops.draw.draw_detections for the same: api_kwargs"""
    c = CASES[case]
    n = len(NAMES) if c.get("names", True) else 0
    colour = None if c.get("colour") == "class" else BOX_COLOUR
    palette = None
    if colour is None:
        rs = np.random.RandomState(42)
        palette = np.concatenate([rs.randint(0, 256, (1, 3), dtype=np.uint8) for _ in range(n if n else 13)])
    font = FONT_SIZE if c.get("font", True) else 0
    return R.Style(thickness, colour, palette, TEXT_COLOUR, int(np.floor(0.8 * 255 + 0.5)), THR, c.get("max_dets", 256), n,
                   1 + font // 8)


def api_kwargs(case, thickness):
    c = CASES[case]
    kw = dict(class_names=list(NAMES) if c.get("names", True) else None, score_thr=THR,
              bbox_color="class" if c.get("colour") == "class" else BOX_COLOUR, text_color=TEXT_COLOUR, thickness=thickness,
              font_size=FONT_SIZE if c.get("font", True) else 0, label_alpha=0.8, max_dets=c.get("max_dets"))
    if atlas_for(case) is not None:
        kw["atlas"] = atlas_for(case)
    return kw


@functools.lru_cache(maxsize=None)
def expected(case, thickness):
    """the gather restatement's frames for a case, computed once and shared (read-only)"""
    frames, _ = frames_host()
    out = R.gather(frames, *padded(case), style_for(case, thickness), atlas_for(case))
    for o in out:
        o.setflags(write=False)
    return out
