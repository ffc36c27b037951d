"""The reference's dataset wrappers (radet/datasets/dataset_wrappers.py): ConcatDataset, RepeatDataset and MixDataset (the
mixpbr configs' pbr + real training set, `ConcatDataset([RepeatDataset(d, r) ...])`), with the same lengths, index
mapping, `flag` and `CLASSES`.  `plan_sample(idx, rnd, nprnd)` delegates to the sub-dataset that owns `idx`, so
`build_dataloader` seeds every sample from the wrapper-level index: the repeated copies of a frame get different draws.

`pipeline` is the one ImagePipeline the sub-datasets share (their pipeline configs must be equal, as in every mixpbr
config), so a loader batch that mixes sub-datasets still runs one device pass.  Evaluation of a wrapped dataset and
ClassBalancedDataset are not implemented."""
import bisect

import numpy as np

from .bop import DATASETS
from .loading import ImagePipeline


def _shared_pipeline(datasets):
    """the pipeline every sub-dataset runs: one ImagePipeline when their configs are equal (it then replaces theirs);
    None when none of them is an image pipeline (samples are then only reachable through __getitem__)"""
    pipes = [d.pipeline for d in datasets]
    if not any(isinstance(p, ImagePipeline) for p in pipes):
        return None
    first = pipes[0]
    if not all(isinstance(p, ImagePipeline) and p.cfg == first.cfg for p in pipes):
        raise NotImplementedError("wrapped datasets with different pipelines: one loader batch runs one device pass, so "
                                  "every sub-dataset must be built with the same pipeline config")
    for d in datasets:
        d.pipeline = first
    return first


def _test_mode(datasets):
    modes = {bool(getattr(d, "test_mode", False)) for d in datasets}
    if len(modes) != 1:
        raise ValueError("wrapped datasets mix test_mode=True and test_mode=False")
    return modes.pop()


@DATASETS.register_module()
class ConcatDataset:
    """datasets back to back; flag = the concatenated flags"""

    def __init__(self, datasets, separate_eval=True):
        self.datasets = list(datasets)
        if not self.datasets:
            raise ValueError("ConcatDataset of no datasets")
        if not separate_eval:
            raise NotImplementedError("Evaluating concatenated CocoDataset as a whole is not supported! "
                                      "Please set \"separate_eval=True\"")
        self.separate_eval = separate_eval
        self.CLASSES = self.datasets[0].CLASSES
        self.cumulative_sizes = np.cumsum([len(d) for d in self.datasets]).tolist()
        if hasattr(self.datasets[0], "flag"):
            self.flag = np.concatenate([d.flag for d in self.datasets])
        self.test_mode = _test_mode(self.datasets)
        self.pipeline = _shared_pipeline(self.datasets)

    def __len__(self):
        return self.cumulative_sizes[-1]

    def _locate(self, idx):
        """(sub-dataset, index in it) of wrapper index idx"""
        if idx < 0:
            if -idx > len(self):
                raise ValueError("absolute value of index should not exceed dataset length")
            idx += len(self)
        if idx >= len(self):
            raise IndexError(f"index {idx} of a dataset of {len(self)}")
        d = bisect.bisect_right(self.cumulative_sizes, idx)
        return d, idx - (self.cumulative_sizes[d - 1] if d else 0)

    def __getitem__(self, idx):
        d, j = self._locate(idx)
        return self.datasets[d][j]

    def plan_sample(self, idx, rnd, nprnd):
        d, j = self._locate(idx)
        return self.datasets[d].plan_sample(j, rnd, nprnd)

    def get_cat_ids(self, idx):
        d, j = self._locate(idx)
        return self.datasets[d].get_cat_ids(j)

    def evaluate(self, *args, **kwargs):
        raise NotImplementedError("evaluation of a wrapped dataset is not implemented: evaluate its sub-datasets")


@DATASETS.register_module()
class RepeatDataset:
    """`dataset` `times` times over; index i is sample i % len(dataset)"""

    def __init__(self, dataset, times):
        self.dataset, self.times = dataset, int(times)
        self.CLASSES = dataset.CLASSES
        if hasattr(dataset, "flag"):
            self.flag = np.tile(dataset.flag, self.times)
        self._ori_len = len(dataset)
        self.test_mode = bool(getattr(dataset, "test_mode", False))

    @property
    def pipeline(self):
        return self.dataset.pipeline

    @pipeline.setter
    def pipeline(self, p):
        self.dataset.pipeline = p

    def __len__(self):
        return self.times * self._ori_len

    def __getitem__(self, idx):
        return self.dataset[idx % self._ori_len]

    def plan_sample(self, idx, rnd, nprnd):
        return self.dataset.plan_sample(idx % self._ori_len, rnd, nprnd)

    def get_cat_ids(self, idx):
        return self.dataset.get_cat_ids(idx % self._ori_len)

    def evaluate(self, *args, **kwargs):
        raise NotImplementedError("evaluation of a wrapped dataset is not implemented: evaluate its sub-datasets")


@DATASETS.register_module()
class MixDataset(ConcatDataset):
    """pbr and real images mixed with per-dataset ratios: ConcatDataset([RepeatDataset(d, r) for d, r in ...])"""

    def __init__(self, datasets, ratios):
        if len(datasets) != len(ratios):
            raise ValueError(f"{len(datasets)} datasets and {len(ratios)} ratios")
        super().__init__([RepeatDataset(d, r) for d, r in zip(datasets, ratios)])
        self.ratios = list(ratios)


@DATASETS.register_module()
class ClassBalancedDataset:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("ClassBalancedDataset is not used by the RADet configs and is not implemented")
