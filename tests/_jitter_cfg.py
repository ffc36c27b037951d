"""What the scale-jitter tests share: a jitter config pointed at a generated BOP tree."""
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def jitter_train_cfg(tree, name="r50_ycbv_pbr_jitter.py"):
    """data.train of a jitter config with the paths of a generated tree"""
    from radet_amd.utils import Config
    cfg = Config.fromfile(os.path.join(REPO, "configs", "bop", name))
    train = dict(cfg.data.train, ann_file=tree["ann_file"], img_prefix=tree["img_prefix"], seg_prefix=tree["seg_prefix"])
    train["pipeline"] = [dict(t, background_dir=tree["background_dir"]) if t["type"] == "RandomBackground" else t
                         for t in train["pipeline"]]
    return cfg, train
