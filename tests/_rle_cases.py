"""What the run-length mask tests share: the masks a run-length codec can get wrong."""
import numpy as np


def edge_masks(h, w, seed=0):
    """name -> u8 [h, w]: the cases a run-length codec can get wrong"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    first = np.zeros((h, w), np.uint8)
    first[0, 0] = 1
    first[h // 2:, w // 3] = 1
    span = np.zeros((h, w), np.uint8)
    span[h // 2:, 2] = 1
    span[:, 3:6] = 1                                              # one run over columns 2 (lower half) .. 6 (upper part)
    span[:h // 3, 6] = 1
    return dict(zeros=np.zeros((h, w), np.uint8), ones=np.ones((h, w), np.uint8), first=first,
                checker=((yy + xx) & 1).astype(np.uint8), span=span, random=(rs.rand(h, w) > 0.6).astype(np.uint8))
