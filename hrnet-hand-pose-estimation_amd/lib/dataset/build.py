"""Loaders on the input side of the hot path (reference lib/dataset/build.py:31-97).

make_dataloader builds the named datasets (DATASET.DATASET with TRAIN_SET for training, TEST_DATASET with TEST_SET
otherwise) when they are RHD readers (dataset/rhd.py: RHD_kpt, RHD) and <DATA_DIR>/RHD/<subset>/anno_<subset>.pickle
exists, or MHP readers (dataset/mhp.py: MHP_kpt, MHP, MHP_seq, MHP_mv) and <DATA_DIR>/MHP/annotated_frames exists.
Otherwise it logs one warning naming what is missing and returns the synthetic RHD-shaped loader: it yields
the sample dict of the reference's RHD key-point dataset (lib/dataset/RHDDatasetKeypoints.py:126-134) from the
portable generator in hipnet/synth.py, so the tests and bench.py run without a dataset.

Real loaders: training shuffles with DistributedSampler semantics (this rank's share when `distributed` and
world > 1; set_epoch reshuffles), validation / evaluation keep order and every sample. The batch is
IMAGES_PER_GPU (one process per GPU). `max_batches` caps a real epoch; `num_batches` is the synthetic length."""
import logging
import os

import torch

from dataset import mhp, rhd
from hipnet import synth

logger = logging.getLogger(__name__)


class SyntheticRHD(torch.utils.data.Dataset):
    exception = False

    def __init__(self, cfg, length, seed):
        self.cfg, self.length, self.seed = cfg, length, seed
        self.img_w, self.img_h = cfg.MODEL.IMAGE_SIZE
        self._cache = {}

    def __len__(self):
        return self.length

    def batch(self, index, batch_size):
        key = (index, batch_size)
        if key not in self._cache:
            b = synth.rhd_batch(batch_size, seed=self.seed + index, img_h=self.img_h, img_w=self.img_w,
                                num_joints=self.cfg.MODEL.NUM_JOINTS, sigma=self.cfg.MODEL.SIGMA)
            self._cache = {key: {k: torch.from_numpy(v) for k, v in b.items()}}
        return self._cache[key]


class SyntheticLoader(object):
    """iterable of batches with the attributes the loops use (`batch_size`, `dataset`, `len`)"""

    def __init__(self, dataset, batch_size, num_batches, rank=0, world=1):
        self.dataset, self.batch_size, self.num_batches = dataset, batch_size, num_batches
        self.rank, self.world = rank, world
        self.sampler = self

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return self.num_batches

    def __iter__(self):
        for i in range(self.num_batches):
            yield self.dataset.batch(i * self.world + self.rank, self.batch_size)


def make_dataloader(cfg, is_train=True, distributed=False, num_batches=8, rank=0, world=1, max_batches=None,
                    heatmaps=None):
    """{dataset name: loader}. heatmaps=None: RHD_kpt, MHP_kpt and MHP_seq batches carry heat maps, RHD and MHP
    batches do not; True / False forces it (tools/train.py validates with heat maps)."""
    names = list(cfg.DATASET.DATASET if is_train else cfg.DATASET.TEST_DATASET)
    subset = cfg.DATASET.TRAIN_SET if is_train else cfg.DATASET.TEST_SET
    if names and all(n in mhp.READERS for n in names):
        module, anno = mhp, mhp.frames_dir(cfg.DATA_DIR)
    else:
        module, anno = rhd, rhd.annotation_path(cfg.DATA_DIR, subset)
    unknown = [n for n in names if n not in module.READERS]
    if names and not unknown and os.path.exists(anno):
        return {n: module.make_loader(cfg, n, subset, is_train, rank, world, distributed, max_batches, heatmaps)
                for n in names}
    why = 'no reader for {}'.format(unknown) if unknown else 'no datasets named' if not names else \
        '{} not found'.format(anno)
    logger.warning('%s: using the synthetic RHD-shaped loader', why)
    per_gpu = cfg.TRAIN.IMAGES_PER_GPU if is_train else cfg.TEST.IMAGES_PER_GPU
    ds = SyntheticRHD(cfg, length=per_gpu * num_batches * world, seed=1234 if is_train else 4321)
    return {'synthetic_kpt': SyntheticLoader(ds, per_gpu, num_batches, rank, world)}
