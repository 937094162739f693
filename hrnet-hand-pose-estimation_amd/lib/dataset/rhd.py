"""RHD reader: the reference's RHD (lib/dataset/RHDDataset.py:58-124) and RHD_kpt (RHDDatasetKeypoints.py:96-134)
with its transforms (transforms/build.py:35-89, transforms/transforms.py:54-175), split so that the pixels never
touch the host CPU beyond decoding:

- DataLoader workers (numpy and PIL only, never torch.cuda / HIP, not even pinned memory - a worker that opened the
  GPU would count against the per-machine process limit): decode, hand choice, crop, `idx_RHD` reorder, drawing the
  augmentation, the float64 forward / inverse matrices and the joints at heat-map scale. The batch's crops are packed
  into one u8 buffer (dataset/preprocess.py pack_images) in the worker.
- The main process (RHDLoader): the buffer is copied into one of two alternating pinned staging buffers, uploaded
  with one non_blocking copy, warped + flipped + normalised by ONE hrnet_affine_warp_normalize_u8 launch on the
  current stream, and for RHD_kpt the targets come from HeatmapGenerator (hrnet_gaussian_targets).

Sample semantics (reproduced, including the reference's quirks):
- images are RHD/<subset>/color/* in sorted order; annotations are anno_<subset>.pickle indexed by position,
  uv_vis 42 x 3; the hand with more visible key points is used (left 0..20, right 21..41, a tie goes to left);
- crop_size = min(W, int(2 * max(w, h))) and the corner is truncated with int() and clamped to the image, x against
  the image height and y against its width (the reference's shape indices; equal on RHD's 320 x 320 images);
- `pose2d` is reordered by idx_RHD, `visibility` is NOT (the reference returns the chosen hand's flags as read);
  the RHD_kpt heat maps pair the reordered joints with those flags, as the reference's do;
- augmentation (training with WITH_DATA_AUG only; otherwise a pure crop -> IMAGE_SIZE scale): aug_scale in
  [MIN_SCALE, MAX_SCALE], rotation in +-MAX_ROTATION, translation randint(-MAX_TRANSLATE*scale, MAX_TRANSLATE*scale)
  with the bounds truncated to integers; the image is mapped with the IMAGE_SIZE matrix (pixels outside the CROP are
  0) and the joints with the HEATMAP_SIZE matrix;
- the flip is x -> IMAGE_SIZE-1-x on the image and x -> HEATMAP_SIZE-1-x on the joints, WITHOUT flip_index, taken
  when random() < DATASET.FLIP: the shipped yaml's `FLIP: true` flips every augmented sample.

Deviations, all deliberate:
- the augmentation is drawn from numpy.random.default_rng((seed, epoch, index)) instead of the global np.random /
  random state, so a run is reproducible whatever the worker count;
- a translation range that truncates to empty (MAX_TRANSLATE * scale < 1) gives dx = dy = 0, where the reference's
  randint raises;
- a crop smaller than 1 px raises ValueError naming the file (the reference would fail later in cv2);
- SCALE_AWARE_SIGMA is not supported (ValueError);
- `orig_imgs` is not in the batch: no loop reads it and it would be 19 MB per batch of 64;
- images are decoded by PIL, and the warp is an exact bilinear blend (csrc/preprocess.hip), where cv2.warpAffine
  quantises the sampling position to 1/32 px: a u8 code may differ from cv2's.
"""
import os
import pickle
from collections import namedtuple

import numpy as np
import torch

from dataset.preprocess import pack_images, read_image_rgb

# reference lib/dataset/standard_legends.py:17
IDX_RHD = (0, 4, 3, 2, 1, 8, 7, 6, 5, 12, 11, 10, 9, 16, 15, 14, 13, 20, 19, 18, 17)

# the reference's build_transforms arguments (transforms/build.py:36-55); flip is the probability DATASET.FLIP
Augment = namedtuple('Augment', ['max_rotation', 'min_scale', 'max_scale', 'max_translate', 'scale_type', 'flip'])


def annotation_path(data_dir, subset):
    return os.path.join(data_dir, 'RHD', subset, 'anno_{}.pickle'.format(subset))


def augment_from_cfg(cfg, is_train):
    d = cfg.DATASET
    if d.SCALE_AWARE_SIGMA:
        raise ValueError('DATASET.SCALE_AWARE_SIGMA is not supported by the RHD reader')
    if is_train and cfg.WITH_DATA_AUG:
        return Augment(d.MAX_ROTATION, d.MIN_SCALE, d.MAX_SCALE, d.MAX_TRANSLATE, d.SCALE_TYPE, d.FLIP)
    return Augment(0, 1, 1, 0, d.SCALE_TYPE, 0)


def choose_hand(uv_vis):
    """42 x 3 uv_vis -> (pose2d 21 x 2 as stored, visibility 21 x 1 bool) of the hand with more visible key points"""
    uv_vis = np.asarray(uv_vis)
    uv, vis = uv_vis[:, :2], uv_vis[:, 2:] == 1
    if np.sum(vis[0:21]) >= np.sum(vis[21:42]):
        return uv[0:21], vis[0:21]
    return uv[21:42], vis[21:42]


def crop_box(pose2d, img_h, img_w):
    """the reference's crop arithmetic (RHDDataset.py:84-94) -> ((x0, y0) corner, crop_size)"""
    x, y = pose2d[:, 0], pose2d[:, 1]
    leftmost, rightmost = np.min(x), np.max(x)
    bottommost, topmost = np.max(y), np.min(y)
    w, h = rightmost - leftmost, bottommost - topmost
    crop = min(img_w, int(2 * w if w > h else 2 * h))
    corner = (max(0, min(int(leftmost - (crop - w) / 2), img_h - crop)),
              max(0, min(img_w - crop, int(topmost - (crop - h) / 2))))
    return corner, crop


def affine_matrix(center, scale, res, rot=0):
    """3 x 3 float64 forward matrix, restated from the reference's _get_affine_matrix (transforms.py:98-122)"""
    h = 200 * scale
    t = np.zeros((3, 3))
    t[0, 0] = float(res[1]) / h
    t[1, 1] = float(res[0]) / h
    t[0, 2] = res[1] * (-float(center[0]) / h + .5)
    t[1, 2] = res[0] * (-float(center[1]) / h + .5)
    t[2, 2] = 1
    if not rot == 0:
        rot_rad = -rot * np.pi / 180
        sn, cs = np.sin(rot_rad), np.cos(rot_rad)
        rot_mat = np.zeros((3, 3))
        rot_mat[0, :2] = [cs, -sn]
        rot_mat[1, :2] = [sn, cs]
        rot_mat[2, 2] = 1
        t_mat = np.eye(3)
        t_mat[0, 2] = -res[1] / 2
        t_mat[1, 2] = -res[0] / 2
        t_inv = t_mat.copy()
        t_inv[:2, 2] *= -1
        t = np.dot(t_inv, np.dot(rot_mat, np.dot(t_mat, t)))
    return t


def _base_scale(crop_h, crop_w, scale_type):
    if scale_type == 'long':
        return max(crop_h, crop_w) / 200
    if scale_type == 'short':
        return min(crop_h, crop_w) / 200
    raise ValueError('Unknown DATASET.SCALE_TYPE: {}'.format(scale_type))


def draw_params(rng, crop_h, crop_w, aug):
    """the random draws of RandomAffineTransform + RandomHorizontalFlip: u_scale and u_rot are the two uniform
    draws in [0, 1), dx / dy the integer translation, flip a bool"""
    u_scale, u_rot = float(rng.random()), float(rng.random())
    scale = _base_scale(crop_h, crop_w, aug.scale_type) * (u_scale * (aug.max_scale - aug.min_scale) + aug.min_scale)
    dx = dy = 0
    if aug.max_translate > 0:
        lo, hi = int(-aug.max_translate * scale), int(aug.max_translate * scale)
        if lo < hi:                      # empty range: the reference's randint raises; no translation here
            dx, dy = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
    flip = bool(rng.random() < aug.flip)
    return {'u_scale': u_scale, 'u_rot': u_rot, 'dx': dx, 'dy': dy, 'flip': flip}


def geometry(crop_h, crop_w, params, aug, input_size, hm_size):
    """float64 matrices of one sample: 'mat_input' (2 x 3, crop -> IMAGE_SIZE), 'mat_output' (2 x 3, crop ->
    HEATMAP_SIZE) and 'inverse' (2 x 3, output pixel -> crop pixel, the horizontal flip folded in)"""
    center = np.array((crop_w / 2, crop_h / 2))
    aug_scale = params['u_scale'] * (aug.max_scale - aug.min_scale) + aug.min_scale
    scale = _base_scale(crop_h, crop_w, aug.scale_type) * aug_scale
    rot = (params['u_rot'] * 2 - 1) * aug.max_rotation
    if aug.max_translate > 0:
        center[0] += params['dx']
        center[1] += params['dy']
    mat_output = affine_matrix(center, scale, (hm_size, hm_size), rot)[:2]
    mat_input = affine_matrix(center, scale, (input_size, input_size), rot)
    inverse = np.linalg.inv(mat_input)
    if params['flip']:                   # output x -> input_size-1-x before the inverse map
        inverse = inverse @ np.array([[-1., 0., input_size - 1], [0., 1., 0.], [0., 0., 1.]])
    return {'mat_input': mat_input[:2], 'mat_output': mat_output, 'inverse': inverse[:2]}


def transform_joints(pose2d, mat_output, flip, hm_size):
    """joints in crop pixels -> heat-map pixels (_affine_joints, then the flip's x -> hm_size-1-x)"""
    j = np.asarray(pose2d, dtype=np.float64).reshape(-1, 2)
    out = np.dot(np.concatenate((j, np.ones((len(j), 1))), axis=1), mat_output.T)
    if flip:
        out[:, 0] = hm_size - out[:, 0] - 1
    return out


class RHD(torch.utils.data.Dataset):
    """worker side of the reader. A key is an index or (index, epoch); __getitem__ returns numpy data only
    (the crop is a view into the decoded image)."""
    name = 'RHD'
    heatmaps = False                     # RHD_kpt: the loader adds heat maps

    def __init__(self, cfg, subset, is_train=False, seed=0):
        self.data_dir = os.path.join(cfg.DATA_DIR, 'RHD', subset)
        self.images = sorted(os.listdir(os.path.join(self.data_dir, 'color')))
        with open(annotation_path(cfg.DATA_DIR, subset), 'rb') as f:
            anno = pickle.load(f)
        if cfg.MODEL.NUM_JOINTS != 21 or cfg.DATASET.NUM_JOINTS != 21:
            raise ValueError('RHD has 21 joints per hand, the config asks for {}'.format(cfg.MODEL.NUM_JOINTS))
        missing = [i for i in range(len(self.images)) if i not in anno]
        if missing:
            raise ValueError('{}: no annotation for image index {} ({} images)'.format(
                annotation_path(cfg.DATA_DIR, subset), missing[0], len(self.images)))
        self.uv_vis = [np.asarray(anno[i]['uv_vis']) for i in range(len(self.images))]
        self.aug = augment_from_cfg(cfg, is_train)
        self.input_size, self.hm_size = cfg.MODEL.IMAGE_SIZE[0], cfg.MODEL.HEATMAP_SIZE[0]
        self.seed = seed

    def __len__(self):
        return len(self.images)

    def __getitem__(self, key):
        idx, epoch = key if isinstance(key, tuple) else (key, 0)
        path = os.path.join(self.data_dir, 'color', self.images[idx])
        img = read_image_rgb(path)
        pose2d, vis = choose_hand(self.uv_vis[idx])
        (x0, y0), crop = crop_box(pose2d, img.shape[0], img.shape[1])
        crop_img = img[y0:y0 + crop, x0:x0 + crop]
        if crop < 1 or crop_img.shape[0] < 1 or crop_img.shape[1] < 1:
            raise ValueError('{}: the hand crop is {} x {} px (crop_size {})'.format(
                path, crop_img.shape[0], crop_img.shape[1], crop))
        pose2d = (pose2d - np.array((x0, y0)))[list(IDX_RHD)]
        ch, cw = crop_img.shape[:2]
        params = draw_params(np.random.default_rng((self.seed, epoch, idx)), ch, cw, self.aug)
        g = geometry(ch, cw, params, self.aug, self.input_size, self.hm_size)
        return {'crop': crop_img, 'inverse': g['inverse'], 'corner': np.array((x0, y0)), 'crop_size': crop,
                'pose2d': transform_joints(pose2d, g['mat_output'], params['flip'], self.hm_size),
                'visibility': vis}


class RHD_kpt(RHD):
    name = 'RHD_kpt'
    heatmaps = True


READERS = {'RHD': RHD, 'RHD_kpt': RHD_kpt}


def collate(samples):
    """worker side: the batch's crops packed into one u8 CPU buffer + its slot table and the f32 inverse matrices"""
    p = pack_images([s['crop'] for s in samples], pin=False)
    return {'buffer': p.buffer, 'table': p.table,
            'inverse': torch.from_numpy(np.stack([s['inverse'] for s in samples]).astype(np.float32).reshape(-1, 6)),
            'pose2d': torch.from_numpy(np.stack([s['pose2d'] for s in samples]).astype(np.float32)),
            'visibility': torch.from_numpy(np.stack([s['visibility'] for s in samples])),
            'corner': torch.from_numpy(np.stack([s['corner'] for s in samples]).astype(np.int64)),
            'crop_size': torch.tensor([s['crop_size'] for s in samples], dtype=torch.int64)}


class _InOrder(object):
    """every index in order, with the set_epoch / epoch of DistributedSampler"""

    def __init__(self, n):
        self.n, self.epoch = n, 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(range(self.n))


class _EpochBatches(object):
    """batch sampler: lists of (index, epoch) keys, at most `limit` batches"""

    def __init__(self, sampler, batch_size, limit=None):
        self.sampler, self.batch_size, self.limit = sampler, batch_size, limit

    def __len__(self):
        n = -(-len(self.sampler) // self.batch_size)
        return n if self.limit is None else min(n, self.limit)

    def __iter__(self):
        keys, count = [], 0
        for i in self.sampler:
            if self.limit is not None and count >= self.limit:
                return
            keys.append((int(i), self.sampler.epoch))
            if len(keys) == self.batch_size:
                yield keys
                keys, count = [], count + 1
        if keys:
            yield keys


class RHDLoader(object):
    """main-process side: iterable of device batches {'imgs', ['heatmaps'], 'pose2d', 'visibility', 'corner',
    'crop_size'} with the attributes the loops use (`batch_size`, `dataset`, `sampler.set_epoch`, `len`).
    `collate_fn` (a module-level function: spawned workers import it) packs a worker batch into {'buffer', 'table',
    'inverse', ...}; every other key it returns reaches the device batch as it is (dataset/mhp.py adds
    'hm_inverse')."""

    def __init__(self, cfg, dataset, batch_size, shuffle, rank=0, world=1, max_batches=None, heatmaps=None,
                 workers=None, seed=0, collate_fn=None):
        self.dataset, self.batch_size = dataset, batch_size
        self.heatmaps = dataset.heatmaps if heatmaps is None else bool(heatmaps)
        self.num_joints, self.sigma = cfg.MODEL.NUM_JOINTS, cfg.DATASET.SIGMA
        self.hm_res = cfg.DATASET.OUTPUT_SIZE[0]
        self.size = (dataset.input_size, dataset.input_size)
        if shuffle:
            self.sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=world, rank=rank,
                                                                           shuffle=True, seed=seed)
        else:
            self.sampler = _InOrder(len(dataset))
        workers = cfg.WORKERS if workers is None else workers
        kw = {}
        if workers > 0:
            # spawned workers start from a fresh interpreter: nothing of this process's HIP state reaches them
            kw = {'multiprocessing_context': 'spawn', 'persistent_workers': True}
        self.loader = torch.utils.data.DataLoader(dataset, batch_sampler=_EpochBatches(self.sampler, batch_size,
                                                                                       max_batches),
                                                  num_workers=workers, collate_fn=collate_fn or collate, **kw)
        self._staging, self._copied, self._next = [None, None], [None, None], 0

    def __len__(self):
        return len(self.loader.batch_sampler)

    def __iter__(self):
        for b in self.loader:
            yield self.to_device(b)

    def to_device(self, b):
        from dataset.preprocess import affine_warp_normalize
        from dataset.target_generators import HeatmapGenerator
        dev = torch.device('cuda', torch.cuda.current_device())
        k, self._next = self._next, 1 - self._next
        if self._copied[k] is not None:
            self._copied[k].synchronize()            # the copy out of this staging buffer two batches ago is done
        n = b['buffer'].numel()
        if self._staging[k] is None or self._staging[k].numel() < n:
            self._staging[k] = torch.empty(n + n // 4, dtype=torch.uint8, pin_memory=True)
        stage = self._staging[k][:n]
        stage.copy_(b['buffer'])
        buf = stage.to(dev, non_blocking=True)
        self._copied[k] = torch.cuda.Event()
        self._copied[k].record()
        if getattr(self.dataset, 'resize', False):
            # a reader of whole frames resized to (width, height) with its own normalisation (dataset/mhp.py MHP_CPM_kpt)
            from dataset.preprocess import resize_normalize
            out = {'imgs': resize_normalize(buf, b['table'], (self.dataset.width, self.dataset.height),
                                            mean=self.dataset.mean, std=self.dataset.std)}
        else:
            out = {'imgs': affine_warp_normalize(buf, b['table'], b['inverse'], self.size)}
        if self.heatmaps:
            joints = torch.cat((b['pose2d'], b['visibility'].float()), 2).pin_memory().to(dev, non_blocking=True)
            out['heatmaps'] = HeatmapGenerator(self.hm_res, self.num_joints, self.sigma)(joints)
        for key in b:
            if key not in ('buffer', 'table', 'inverse'):
                out[key] = b[key]
        return out


def make_loader(cfg, name, subset, is_train, rank=0, world=1, distributed=False, max_batches=None, heatmaps=None):
    dataset = READERS[name](cfg, subset, is_train=is_train)
    if is_train:
        return RHDLoader(cfg, dataset, cfg.TRAIN.IMAGES_PER_GPU, True, rank if distributed else 0,
                         world if distributed else 1, max_batches, heatmaps)
    return RHDLoader(cfg, dataset, cfg.TEST.IMAGES_PER_GPU, False, max_batches=max_batches, heatmaps=heatmaps)
