"""build_dataloader: batches of an image-pipeline dataset, ready for `train_detector` (training) or `forward_test` (test).

Sampling follows mmdet's (Distributed)GroupSampler: every batch holds images of one aspect-ratio group (`dataset.flag`),
each group is padded to whole batches of all ranks by repeating its own indices, the batch order is shuffled, and rank r
takes the r-th contiguous share.  Every sample draws from its own random.Random / np.random.RandomState, seeded from
(seed, epoch, index), so a batch depends neither on the batch size nor on the number of decode threads.

Decoding and the random draws of batch i + 1 run on host threads while the caller runs its step on batch i; the device
part of a batch (allocations, uploads, kernel launches) runs on the calling thread, on its current stream, when the
batch is requested -- never concurrently with a step that is being recorded on the launch tape."""
import math
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np

MAX_WORKERS = 16


def sample_seed(seed, epoch, idx):
    """32-bit seed of sample `idx` in `epoch` (idx = -1: the sampler's own order)"""
    return int(np.random.SeedSequence([int(seed), int(epoch), int(idx) + 1]).generate_state(1)[0])


def sample_generators(seed, epoch, idx):
    s = sample_seed(seed, epoch, idx)
    return random.Random(s), np.random.RandomState(s)


def group_batches(flag, samples_per_gpu, seed, epoch, rank=0, world=1, shuffle=True):
    """the batches (lists of dataset indices) of `rank` for `epoch`"""
    n = len(flag)
    if not shuffle:                                      # test order: consecutive indices, contiguous shares
        per = int(math.ceil(n / world))
        idx = list(range(n))[rank * per:(rank + 1) * per]
        return [idx[i:i + samples_per_gpu] for i in range(0, len(idx), samples_per_gpu)]
    rng = np.random.RandomState(sample_seed(seed, epoch, -1))
    flag = np.asarray(flag)
    chunk = samples_per_gpu * world
    batches = []
    for g in np.unique(flag):
        members = np.flatnonzero(flag == g)
        members = members[rng.permutation(len(members))]
        size = int(math.ceil(len(members) / chunk)) * chunk
        members = np.concatenate([members, members[np.arange(size - len(members)) % len(members)]])
        batches += [members[i:i + samples_per_gpu].tolist() for i in range(0, size, samples_per_gpu)]
    order = rng.permutation(len(batches))
    batches = [batches[i] for i in order]
    per = len(batches) // world
    return batches[rank * per:(rank + 1) * per]


class DataLoader:
    def __init__(self, dataset, samples_per_gpu, workers, seed, rank=0, world=1, shuffle=True):
        if not hasattr(dataset.pipeline, "run"):
            raise TypeError("build_dataloader needs a dataset whose pipeline starts with LoadImageFromFile")
        self.dataset, self.samples_per_gpu, self.seed = dataset, int(samples_per_gpu), int(seed)
        self.rank, self.world, self.shuffle = int(rank), int(world), bool(shuffle) and not dataset.test_mode
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.epoch = 0
        self._pool = None

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def batches(self):
        flag = getattr(self.dataset, "flag", None)
        if flag is None:
            flag = np.zeros(len(self.dataset), np.uint8)
        return group_batches(flag, self.samples_per_gpu, self.seed, self.epoch, self.rank, self.world, self.shuffle)

    def __len__(self):
        return len(self.batches())

    def plan(self, idx):
        return self.dataset.plan_sample(idx, *sample_generators(self.seed, self.epoch, idx))

    def __iter__(self):
        if self._pool is None:
            self._pool = ThreadPoolExecutor(self.workers, thread_name_prefix="radet-decode")
        batches = self.batches()
        submit = lambda b: [self._pool.submit(self.plan, i) for i in b]  # noqa: E731
        pending = submit(batches[0]) if batches else None
        for k in range(len(batches)):
            futures, pending = pending, (submit(batches[k + 1]) if k + 1 < len(batches) else None)
            yield self.dataset.pipeline.run([f.result() for f in futures], collate=True)
        self._drain()

    def _drain(self):
        """the device JPEG decoder's error words of the batches whose check is still pending (the last ones of an epoch)"""
        check = getattr(self.dataset.pipeline, "check_decode_errors", None)
        if check is not None:
            check(wait=True)

    def close(self):
        self._drain()
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __del__(self):
        pool = getattr(self, "_pool", None)
        if pool is not None:
            pool.shutdown(wait=False)


def build_dataloader(dataset, samples_per_gpu, workers, seed, rank=0, world=1, shuffle=True):
    """batches of `dataset` for one rank: dict(img=f32[B,3,H,W] on the device, gt_bboxes / gt_labels / points_to_gt_index /
    points_weight lists, img_metas) in training, dict(img=[f32[B,3,H,W]], img_metas=[[...]]) in test mode.
    `workers`: decode threads (at most 16)."""
    return DataLoader(dataset, samples_per_gpu, workers, seed, rank, world, shuffle)
