"""What the affine-augmentation tests share: the rotate config pointed at a generated BOP tree."""
from _jitter_cfg import jitter_train_cfg


def rotate_train_cfg(tree):
    """data.train of configs/bop/r50_ycbv_pbr_rotate.py with the paths of a generated tree"""
    return jitter_train_cfg(tree, name="r50_ycbv_pbr_rotate.py")
