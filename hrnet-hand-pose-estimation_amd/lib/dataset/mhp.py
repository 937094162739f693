"""MHP readers: the reference's MHP (lib/dataset/MHPDataset.py:46-126), MHP_kpt (MHPDatasetKeypoints.py:47-80),
MHP_seq (MHPSeqDataset.py:48-240) and MHP_mv (MHPMultiViewDataset.py:31-216), with the RHD transforms
(dataset/rhd.py) applied to the whole 640 x 480 frame.

Layout: <DATA_DIR>/MHP/annotated_frames/data_N/<f>_webcam_<c>.jpg, annotations/data_N/<f>_joints.txt (a name, then
x y z per line) and calibrations/data_N/webcam_<c>/{rvec,tvec}.pkl (pickles read with encoding='latin1').

Split of the work, as in the RHD reader:
- DataLoader workers (numpy and PIL only, never the GPU): read the joints and the calibration, project, draw the
  augmentation, build the float64 matrices; the batch's collate decodes every distinct frame ONCE, packs them into
  one u8 buffer and gives each slot a table row pointing at its frame (several slots may share one frame).
- The main process (dataset/rhd.py RHDLoader): one pinned upload, ONE hrnet_affine_warp_normalize_u8 launch,
  HeatmapGenerator for the targets.

MHP / MHP_kpt: one sample per image. The list is every `*_webcam_<digit>*` file, natural-sorted; training takes the
first 80 % (int(len * 0.8)), evaluation the rest. The 3-D joints are reordered by idx_MHP and projected with the
camera's rvec / tvec, K and the distortion (k1, k2, p1, p2, k3); a joint outside the 640 x 480 frame is not visible.
Reference quirk kept: these readers cv2.imread without cvtColor, so the network sees BGR (the worker swaps the
channels while packing). MHP_kpt carries heat maps, MHP does not.

MHP_seq: training reads data_1..16, evaluation data_17..21. A directory of n = files // 4 frames gives the centres
0, STRIDE, 2 STRIDE, ... < n, i.e. (n - 1) // STRIDE + 1 samples; window frame j is clamp(centre + SEQ_IDX[j], 0, n-1)
for views 1..4. Images are RGB, the distortion is zero, the rotation is Rodrigues(rvec). The batch is what the model
and the loss consume: `imgs` (5 * 4 * B, 3, H, W) frame-major, slot (j * B + b) * 4 + (c - 1) (the reference's Aggr
reorder, function.py:35-51); `pose2d`, `visibility` and `heatmaps` (4 * B, 21, ...) are those of the centre frame's
four views. Augmentation, when on, is drawn per image (5 x 4 draws per sample), as the reference's transform is called
once per image.

MHP_mv: the reference's MHPMultiViewDataset (MHPMultiViewDataset.py:31-216), read by tools/evaluate_3D.py. Training
reads data_1..16, evaluation data_17..21 (a missing directory is skipped, as for MHP_seq); index i is the (directory,
frame) pair i in natural order, n = files // 4 frames per directory; the views are 1..4 or the subset passed as
`views`. Images are RGB (the reference calls cvtColor here), the distortion is zero (:90). A sample is frames = 1,
views = V, so batch slot b * V + v. Besides `buffer` / `table` / `inverse` the batch carries `pose2d` (B*V, 21, 2) in
heat-map pixels, `visibility` (B*V, 21, 1), `hm_inverse` (B*V, 2, 3), and stacked per sample `pose3d` (B, 21, 3) (the
idx_MHP-reordered world joints), `extrinsic_matrices` (B, V, 3, 4) = [R | t] and `intrinsic_matrix` (B, 3, 3), all
float64. The reference's occlusion (:168-180) is kept, in evaluation too: for image (i, c) the generator
random.Random(4 i + c) (the sequence of random.seed(4 i + c)) draws j = randint(0, 20); the centre is the frame-pixel
projection of joint j truncated to int; `collate` paints a black disc of radius 50 on the decoded frame, and a joint
within 50 px of the centre (np.linalg.norm(p - centre) <= 50) is invisible, like one outside the frame. cv2.circle's
rasterisation is not available: the painted pixels are those with (x - cx)^2 + (y - cy)^2 <= 50^2 (unpinned).

MHP_CPM_kpt: the evaluation path of the reference's MHP_CPMDataset (MHP_CPMDataset.py:137-239), the reader of
MODEL.NAME CPM; its class below says what a sample holds. The loader resizes the whole frame (no crop, no warp).

Every batch also carries `hm_inverse` (N, 2, 3) float64: heat-map pixel -> original-image pixel, the inverse of the
sample's heat-map matrix with the flip folded in. tools/evaluate_2D.py maps predictions and ground truth back through
it; the reference scales x by 640/64 and y by 480/64 there (evaluate_2D.py:240-245), which does not invert its own
'short'-scale transform (that crops the frame's central 480 x 480 square).

Deviations, all deliberate:
- the reference's MHPSeqDataset ignores its index and walks a per-process cursor, and its `last_ret` reuse
  (:216-231) shifts the cached window by one frame, not by STRIDE: at STRIDE 2 the centre slot holds frame c-1 with
  the labels of frame c-2. Here index i maps to one fixed (directory, centre) and the window is exact, which makes
  shuffling, DistributedSampler and several workers possible;
- the reference's build_dataset passes `transforms=`, which neither MHP class accepts; the transforms here are the RHD
  ones from the same cfg (augmentation only under WITH_DATA_AUG in training, seeded by (seed, epoch, index));
- MHP / MHP_kpt list <DATA_DIR>/MHP/annotated_frames (the reference walks all of DATA_DIR); MHP_seq skips a data_N of
  its range that does not exist (the reference raises) and raises when none does;
- SCALE_AWARE_SIGMA is refused and `orig_imgs` is not in the batch, as in the RHD reader;
- a frame that does not decode to 640 x 480 raises ValueError naming the file;
- MHP_mv: the reference walks a per-process cursor and ignores its index (with num_workers = 8 every worker repeats
  the same samples); here index i is fixed, as for MHP_seq. `orig_imgs` is left out, the transforms are the RHD ones
  as for the other MHP readers, and the matrices are float64 (the reference's intrinsics are float32);
- cv2 is not used: Rodrigues and projectPoints are restated below in float64 numpy from OpenCV's documented model
  (pinhole plus k1, k2, p1, p2, k3) and are not pinned against cv2 itself.
"""
import fnmatch
import os
import pickle
import random
import re

import numpy as np
import torch

from dataset.preprocess import pack_images, read_image_rgb
from dataset.rhd import RHDLoader, augment_from_cfg, draw_params, geometry, transform_joints

# reference lib/dataset/standard_legends.py:31
IDX_MHP = (20, 17, 16, 18, 19, 1, 0, 2, 3, 5, 4, 6, 7, 13, 12, 14, 15, 9, 8, 10, 11)
# reference MHPDataset.py:69-77
INTRINSIC = np.array([[614.878, 0, 313.219], [0, 615.479, 231.288], [0, 0, 1]])
DISTORTION = np.array([0.092701, -0.175877, -0.0035687, -0.00302299, 0])
FRAME_W, FRAME_H = 640, 480
VIEWS = (1, 2, 3, 4)
OCCLUSION_RADIUS = 50          # MHPMultiViewDataset.py:170
SEQ_RANGES = {'train': range(1, 17), 'training': range(1, 17)}
SEQ_RANGES.update({k: range(17, 22) for k in ('eval', 'valid', 'val', 'evaluation', 'validation')})


def frames_dir(data_dir):
    return os.path.join(data_dir, 'MHP', 'annotated_frames')


def natural_sort(names):
    """the reference's natural_sort (MHPDataset.py:21-24)"""
    def key(text):
        return [int(c) if c.isdigit() else c.lower() for c in re.split('([0-9]+)', text)]
    return sorted(names, key=key)


def list_images(root):
    """every `*_webcam_<digit>*` file under root, natural-sorted (recursive_glob + natural_sort of the reference)"""
    found = []
    for d, _dirs, files in os.walk(root):
        found.extend(os.path.join(d, f) for f in fnmatch.filter(files, '*_webcam_[0-9]*'))
    return natural_sort(found)


def split_range(n, subset):
    """(start, end) of a subset of n images: the first 80 % train, the rest evaluate (MHPDataset.py:60-68)"""
    if subset in ('train', 'training'):
        return 0, int(n * 0.8)
    if subset in ('eval', 'valid', 'val', 'evaluation', 'validation'):
        return int(n * 0.8), n
    raise ValueError('MHP: unknown subset {!r}'.format(subset))


def read_joints(path):
    """21 x 3 float64 world joints of a <f>_joints.txt, in file order (readAnnotation3D)"""
    with open(path) as f:
        rows = [l.split() for l in f if l.strip()]
    return np.array([(float(r[1]), float(r[2]), float(r[3])) for r in rows], dtype=np.float64)


def read_calibration(data_dir, subdir, view):
    """(rvec, tvec) float64 (3,) of one camera"""
    d = os.path.join(data_dir, 'MHP', 'calibrations', subdir, 'webcam_{}'.format(view))
    out = []
    for name in ('rvec.pkl', 'tvec.pkl'):
        with open(os.path.join(d, name), 'rb') as f:
            out.append(np.asarray(pickle.load(f, encoding='latin1'), dtype=np.float64).reshape(3))
    return tuple(out)


def rodrigues(rvec):
    """3 x 3 rotation of a rotation vector (OpenCV's Rodrigues: angle |r| about r / |r|; the identity at 0)"""
    r = np.asarray(rvec, dtype=np.float64).reshape(3)
    theta = np.linalg.norm(r)
    if theta < np.finfo(np.float64).eps:
        return np.eye(3)
    k = r / theta
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(theta) * np.eye(3) + (1 - np.cos(theta)) * np.outer(k, k) + np.sin(theta) * kx


def project_points(points, rvec, tvec, K, dist):
    """N x 3 world points -> N x 2 pixels (OpenCV's projectPoints model): X = R X + t, x' = X / Z,
    r2 = x'^2 + y'^2, x'' = x' (1 + k1 r2 + k2 r2^2 + k3 r2^3) + 2 p1 x' y' + p2 (r2 + 2 x'^2),
    y'' = y' (...) + p1 (r2 + 2 y'^2) + 2 p2 x' y', u = fx x'' + cx, v = fy y'' + cy"""
    X = np.asarray(points, dtype=np.float64).reshape(-1, 3) @ rodrigues(rvec).T + np.asarray(tvec, np.float64).reshape(3)
    x, y = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    k1, k2, p1, p2, k3 = (float(v) for v in np.asarray(dist, dtype=np.float64).reshape(-1)[:5])
    r2 = x * x + y * y
    radial = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    K = np.asarray(K, dtype=np.float64)
    return np.stack((K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]), axis=1)


def visibility(pose2d, width=FRAME_W, height=FRAME_H):
    """21 x 1 bool: the joint lies inside the frame (MHPDataset.py:108-112)"""
    p = np.asarray(pose2d)
    return ((p[:, 0] >= 0) & (p[:, 1] >= 0) & (p[:, 0] < width) & (p[:, 1] < height))[:, None]


def hm_inverse(mat_output, flip, hm_size):
    """2 x 3: heat-map pixel (after the flip) -> original-image pixel"""
    inv = np.linalg.inv(np.vstack([mat_output, [0., 0., 1.]]))
    if flip:
        inv = inv @ np.array([[-1., 0., hm_size - 1], [0., 1., 0.], [0., 0., 1.]])
    return inv[:2]


def seq_windows(n, stride, seq_idx):
    """(centres, frames): the centres 0, stride, ... < n and, per centre, the clamped window frames"""
    centres = np.arange(0, n, stride)
    frames = np.clip(centres[:, None] + np.asarray(seq_idx)[None], 0, n - 1)
    return centres, frames


class _Base(torch.utils.data.Dataset):
    """worker side shared by the readers; a key is an index or (index, epoch). __getitem__ returns numpy data and
    the paths of the frames (decoded by `collate`, once per batch and frame)."""
    heatmaps = False
    bgr = False

    def __init__(self, cfg, is_train, seed):
        if cfg.MODEL.NUM_JOINTS != 21 or cfg.DATASET.NUM_JOINTS != 21:
            raise ValueError('MHP has 21 joints per hand, the config asks for {}'.format(cfg.MODEL.NUM_JOINTS))
        self.data_dir = cfg.DATA_DIR
        self.aug = augment_from_cfg(cfg, is_train)
        self.input_size, self.hm_size = cfg.MODEL.IMAGE_SIZE[0], cfg.MODEL.HEATMAP_SIZE[0]
        self.seed = seed

    def _scan(self, cfg, subset):
        """the directories data_N of the subset's range (SEQ_RANGES) that exist: self.dirs [(name, frames)], the
        reordered world joints self.joints[(name, frame)] and the calibrations self.calib[(name, view)]"""
        if subset not in SEQ_RANGES:
            raise ValueError('{}: unknown subset {!r}'.format(self.name, subset))
        self.dirs, self.joints, self.calib = [], {}, {}
        for i in SEQ_RANGES[subset]:
            subdir = 'data_{}'.format(i)
            d = os.path.join(frames_dir(cfg.DATA_DIR), subdir)
            if not os.path.isdir(d):
                continue
            n = len(os.listdir(d)) // 4
            if n < 1:
                continue
            self.dirs.append((subdir, n))
            for view in VIEWS:
                self.calib[(subdir, view)] = read_calibration(cfg.DATA_DIR, subdir, view)
            for f in range(n):
                self.joints[(subdir, f)] = read_joints(os.path.join(cfg.DATA_DIR, 'MHP', 'annotations', subdir,
                                                                    '{}_joints.txt'.format(f)))[list(IDX_MHP)]
        if not self.dirs:
            raise ValueError('{}: no data_N of {} under {}'.format(self.name, list(SEQ_RANGES[subset]),
                                                                 frames_dir(cfg.DATA_DIR)))

    def _view(self, rng, world, rvec, tvec, dist):
        """labels and matrices of one image of the whole frame"""
        pose2d = project_points(world, rvec, tvec, INTRINSIC, dist)
        params = draw_params(rng, FRAME_H, FRAME_W, self.aug)
        g = geometry(FRAME_H, FRAME_W, params, self.aug, self.input_size, self.hm_size)
        return {'inverse': g['inverse'], 'hm_inverse': hm_inverse(g['mat_output'], params['flip'], self.hm_size),
                'pose2d': transform_joints(pose2d, g['mat_output'], params['flip'], self.hm_size),
                'visibility': visibility(pose2d), 'frame2d': pose2d}


class MHP(_Base):
    name = 'MHP'
    bgr = True

    def __init__(self, cfg, subset, is_train=False, seed=0):
        _Base.__init__(self, cfg, is_train, seed)
        images = list_images(frames_dir(cfg.DATA_DIR))
        start, end = split_range(len(images), subset)
        self.images = images[start:end]
        self._calib = {}

    def __len__(self):
        return len(self.images)

    def __getitem__(self, key):
        idx, epoch = key if isinstance(key, tuple) else (key, 0)
        path = self.images[idx]
        subdir = os.path.basename(os.path.dirname(path))
        frame, _, view = os.path.splitext(os.path.basename(path))[0].split('_')
        world = read_joints(os.path.join(self.data_dir, 'MHP', 'annotations', subdir, frame + '_joints.txt'))
        if (subdir, view) not in self._calib:
            self._calib[(subdir, view)] = read_calibration(self.data_dir, subdir, view)
        rvec, tvec = self._calib[(subdir, view)]
        v = self._view(np.random.default_rng((self.seed, epoch, idx)), world[list(IDX_MHP)], rvec, tvec, DISTORTION)
        return {'paths': [path], 'frames': 1, 'views': 1, 'inverse': v['inverse'][None],
                'hm_inverse': v['hm_inverse'][None], 'pose2d': v['pose2d'][None], 'visibility': v['visibility'][None]}


class MHP_kpt(MHP):
    name = 'MHP_kpt'
    heatmaps = True


class MHP_seq(_Base):
    name = 'MHP_seq'
    heatmaps = True                      # the reference hands MHP_seq a heat-map generator (build.py:56-62)

    def __init__(self, cfg, subset, is_train=False, seed=0):
        _Base.__init__(self, cfg, is_train, seed)
        self.stride, self.seq_idx = int(cfg.DATASET.STRIDE), [int(s) for s in cfg.DATASET.SEQ_IDX]
        self.centre = self.seq_idx.index(0) if 0 in self.seq_idx else len(self.seq_idx) // 2
        self._scan(cfg, subset)
        self.index = []
        for d, (_subdir, n) in enumerate(self.dirs):
            centres, frames = seq_windows(n, self.stride, self.seq_idx)
            self.index.extend((d, int(c), [int(x) for x in w]) for c, w in zip(centres, frames))

    def __len__(self):
        return len(self.index)

    def window(self, idx):
        """(directory, centre frame, the window's frames)"""
        d, c, w = self.index[idx]
        return self.dirs[d][0], c, w

    def __getitem__(self, key):
        idx, epoch = key if isinstance(key, tuple) else (key, 0)
        subdir, centre, frames = self.window(idx)
        rng = np.random.default_rng((self.seed, epoch, idx))
        paths, views = [], []
        for f in frames:
            for c in VIEWS:
                paths.append(os.path.join(frames_dir(self.data_dir), subdir, '{}_webcam_{}.jpg'.format(f, c)))
                rvec, tvec = self.calib[(subdir, c)]
                # the window frame's image is mapped with its own draw; the labels are the centre frame's
                views.append(self._view(rng, self.joints[(subdir, centre)], rvec, tvec, np.zeros(5)))
        V = len(VIEWS)
        mid = slice(self.centre * V, (self.centre + 1) * V)
        stack = lambda k, s=slice(None): np.stack([v[k] for v in views[s]])
        return {'paths': paths, 'frames': len(frames), 'views': V, 'inverse': stack('inverse'),
                'hm_inverse': stack('hm_inverse', mid), 'pose2d': stack('pose2d', mid),
                'visibility': stack('visibility', mid)}


class MHP_mv(_Base):
    """the reference's MHPMultiViewDataset (MHPMultiViewDataset.py:31-216): sample i is frame i of the subset's
    directories in natural order, seen by the cameras `views` (default 1..4); batch slot b * V + v"""
    name = 'MHP_mv'

    def __init__(self, cfg, subset, is_train=False, seed=0, views=VIEWS):
        _Base.__init__(self, cfg, is_train, seed)
        self.views = tuple(int(c) for c in views)
        if len(set(self.views)) != len(self.views) or not set(self.views) <= set(VIEWS) or len(self.views) < 2:
            raise ValueError('MHP_mv: views {} (two or more distinct views of {})'.format(list(views), list(VIEWS)))
        self._scan(cfg, subset)
        self.index = [(subdir, f) for subdir, n in self.dirs for f in range(n)]

    def __len__(self):
        return len(self.index)

    def __getitem__(self, key):
        idx, epoch = key if isinstance(key, tuple) else (key, 0)
        subdir, f = self.index[idx]
        world = self.joints[(subdir, f)]
        rng = np.random.default_rng((self.seed, epoch, idx))
        paths, views, discs, extrinsic = [], [], [], []
        for c in self.views:
            paths.append(os.path.join(frames_dir(self.data_dir), subdir, '{}_webcam_{}.jpg'.format(f, c)))
            rvec, tvec = self.calib[(subdir, c)]
            v = self._view(rng, world, rvec, tvec, np.zeros(5))
            centre = occlusion_centre(v['frame2d'], idx, c)
            v['visibility'] = v['visibility'] & ~occluded(v['frame2d'], centre)
            views.append(v)
            discs.append(centre)
            extrinsic.append(np.c_[rodrigues(rvec), tvec])
        stack = lambda k: np.stack([v[k] for v in views])
        return {'paths': paths, 'frames': 1, 'views': len(self.views), 'inverse': stack('inverse'),
                'hm_inverse': stack('hm_inverse'), 'pose2d': stack('pose2d'), 'visibility': stack('visibility'),
                'occlusion': discs, 'pose3d': world, 'extrinsic_matrices': np.stack(extrinsic),
                'intrinsic_matrix': INTRINSIC}


def occlusion_centre(frame2d, index, view):
    """(x, y) int centre of the occlusion disc of image (index, view): the frame-pixel joint drawn by
    random.seed(4 index + view); random.randint(0, 20), truncated to int (MHPMultiViewDataset.py:168-172)"""
    j = random.Random(4 * index + view).randint(0, 20)
    return tuple(int(v) for v in np.asarray(frame2d[j]).astype(int))


def occluded(frame2d, centre, radius=OCCLUSION_RADIUS):
    """21 x 1 bool: the joint lies within `radius` of the disc's centre (np.linalg.norm(p - centre) <= radius)"""
    return (np.linalg.norm(np.asarray(frame2d) - np.asarray(centre), axis=1) <= radius)[:, None]


def paint_disc(img, centre, radius=OCCLUSION_RADIUS):
    """a copy of the u8 frame with every pixel (x, y), (x - cx)^2 + (y - cy)^2 <= radius^2, set to black"""
    out = np.array(img)
    cx, cy = centre
    y0, y1 = max(cy - radius, 0), min(cy + radius + 1, out.shape[0])
    x0, x1 = max(cx - radius, 0), min(cx + radius + 1, out.shape[1])
    if y0 < y1 and x0 < x1:
        yy, xx = np.ogrid[y0:y1, x0:x1]
        out[y0:y1, x0:x1][(xx - cx) ** 2 + (yy - cy) ** 2 <= radius * radius] = 0
    return out


def gaussian_map(height, width, cx, cy, sigma):
    """exp(-d^2 / (2 sigma^2)) around (cx, cy) on a height x width grid, clipped to <= 1, values < 0.0099 set to 0
    (MHP_CPMDataset.py:81-84 with :199-200, :222-223), float64"""
    yy, xx = np.mgrid[0:int(height), 0:int(width)]
    g = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 2.0 / sigma / sigma)
    g[g > 1] = 1
    g[g < 0.0099] = 0
    return g


def cpm_center(pose2d, width, height):
    """((cx, cy), exception) of MHP_CPMDataset.py:171-183: per axis the mean of the largest coordinate below the size
    and the smallest above 0; the middle of the frame, with `exception`, where no joint qualifies on an axis"""
    center, exception = [], False
    for axis, size in ((0, width), (1, height)):
        v = np.asarray(pose2d)[:, axis]
        below, above = v[v < size], v[v > 0]
        if below.size and above.size:
            center.append((below.max() + above.min()) / 2)
        else:
            center.append(size / 2)
            exception = True
    return tuple(center), exception


class MHP_CPM_kpt(MHP):
    """the evaluation path of the reference's MHP_CPMDataset (MHP_CPMDataset.py:137-239), the reader of MODEL.NAME CPM:
    the whole frame resized to MODEL.IMAGE_SIZE (no crop, so x and y scale differently: TestResized(256) behind that is
    the identity), BGR, normalised as (v - 128) / 256; `pose2d` (21, 2) in pixels of the stride-8 maps, `visibility`
    (21, 1), `heatmaps` (22, H/8, W/8) - channel 0 the background 1 - max, channel i + 1 the sigma = DATASET.SIGMA
    Gaussian of joint i at int(coordinate) / 8 - and `centermaps` (1, H, W), the sigma = 3 Gaussian at the hand's centre.
    `hm_inverse` maps a stride-8 map pixel back to the 640 x 480 frame. The reference's training transforms
    (RandomResized, RandomRotate, RandomCrop, RandomHorizontalFlip) are not built: is_train=True is refused."""
    name = 'MHP_CPM_kpt'
    stride = 8
    mean = (128.0 / 255.0,) * 3           # (u / 255 - mean) / std = (u - 128) / 256
    std = (256.0 / 255.0,) * 3
    resize = True                         # the loader resizes the frame (hrnet_resize_normalize_u8), it does not warp it

    def __init__(self, cfg, subset, is_train=False, seed=0):
        if is_train:
            raise ValueError('MHP_CPM_kpt: the training transforms of the reference (RandomResized, RandomRotate, '
                             'RandomCrop, RandomHorizontalFlip) are not built: evaluation only')
        MHP.__init__(self, cfg, subset, is_train, seed)
        self.width, self.height = (int(v) for v in cfg.MODEL.IMAGE_SIZE)
        if self.width % self.stride or self.height % self.stride:
            raise ValueError('MHP_CPM_kpt: MODEL.IMAGE_SIZE {}: multiples of {}'.format(list(cfg.MODEL.IMAGE_SIZE),
                                                                                       self.stride))
        self.sigma = cfg.DATASET.SIGMA
        self.exception = False

    def __getitem__(self, key):
        idx = key[0] if isinstance(key, tuple) else key
        path = self.images[idx]
        subdir = os.path.basename(os.path.dirname(path))
        frame, _, view = os.path.splitext(os.path.basename(path))[0].split('_')
        world = read_joints(os.path.join(self.data_dir, 'MHP', 'annotations', subdir, frame + '_joints.txt'))
        if (subdir, view) not in self._calib:
            self._calib[(subdir, view)] = read_calibration(self.data_dir, subdir, view)
        rvec, tvec = self._calib[(subdir, view)]
        sx, sy = self.width / FRAME_W, self.height / FRAME_H
        pose2d = project_points(world[list(IDX_MHP)], rvec, tvec, INTRINSIC, DISTORTION) * np.array((sx, sy))
        vis = visibility(pose2d, self.width, self.height)
        center, self.exception = cpm_center(pose2d, self.width, self.height)
        hh, hw = self.height // self.stride, self.width // self.stride
        heat = np.zeros((len(pose2d) + 1, hh, hw), dtype=np.float32)
        for i, (x, y) in enumerate(pose2d):
            heat[i + 1] = gaussian_map(hh, hw, int(x) / self.stride, int(y) / self.stride, self.sigma)
        heat[0] = 1.0 - heat[1:].max(axis=0)
        centermap = gaussian_map(self.height, self.width, center[0], center[1], 3).astype(np.float32)[None]
        s = self.stride
        return {'paths': [path], 'frames': 1, 'views': 1, 'inverse': np.array([[[1 / sx, 0., 0.], [0., 1 / sy, 0.]]]),
                'hm_inverse': np.array([[[s / sx, 0., 0.], [0., s / sy, 0.]]]), 'pose2d': (pose2d / s)[None],
                'visibility': vis[None], 'heatmaps': heat[None], 'centermaps': centermap[None],
                'exception': np.array([self.exception])}


class MHP_CPM_mv(MHP_mv):
    """the reference's MHP_CPMMultiViewDataset (MHP_CPMMultiViewDataset.py:36-274), the reader of MODEL.NAME vol_CPM:
    indexed like MHP_mv (frame i of the subset's directories, cameras `views`, slot b * V + v); per view what MHP_CPM_kpt
    does, with these specifics: the whole frame resized to MODEL.IMAGE_SIZE, BGR, normalised as (v - 128) / 256; joints
    projected without distortion (:97); `centermaps` (V, 1, H, W) the sigma = 3 Gaussian at the hand's centre; `heatmaps`
    (V, 22, hm_h, hm_w) at MODEL.HEATMAP_SIZE, not stride 8 - channel 0 the background 1 - max, channel i + 1 the
    sigma = DATASET.SIGMA Gaussian of joint i at int(coordinate) / (IMAGE_SIZE / HEATMAP_SIZE) (:211-226); `pose2d` in
    heat-map pixels; no occlusion disc. It carries `pose3d`, `extrinsic_matrices` and `intrinsic_matrix` as MHP_mv does.
    `hm_inverse` is the plain scale diag(640 / hm_w, 480 / hm_h): core.function_vol.heatmap_projections inverts it, which
    is the reference's update_after_resize(K) [R|t] (lib/core/function3D.py:89-93) exactly. The reference applies no
    random transform to this reader (TestResized(256) is the identity behind the resize), so is_train=True is allowed."""
    name = 'MHP_CPM_mv'
    bgr = True
    stride = 8
    mean = MHP_CPM_kpt.mean
    std = MHP_CPM_kpt.std
    resize = True

    def __init__(self, cfg, subset, is_train=False, seed=0, views=VIEWS):
        MHP_mv.__init__(self, cfg, subset, is_train, seed, views)
        self.width, self.height = (int(v) for v in cfg.MODEL.IMAGE_SIZE)
        if self.width % self.stride or self.height % self.stride:
            raise ValueError('MHP_CPM_mv: MODEL.IMAGE_SIZE {}: multiples of {}'.format(list(cfg.MODEL.IMAGE_SIZE),
                                                                                      self.stride))
        self.hm_w, self.hm_h = (int(v) for v in cfg.MODEL.HEATMAP_SIZE)
        self.sigma = cfg.DATASET.SIGMA

    def __getitem__(self, key):
        idx = key[0] if isinstance(key, tuple) else key
        subdir, f = self.index[idx]
        world = self.joints[(subdir, f)]
        sx, sy = self.width / FRAME_W, self.height / FRAME_H
        fx, fy = self.width / self.hm_w, self.height / self.hm_h
        out = {k: [] for k in ('paths', 'pose2d', 'visibility', 'heatmaps', 'centermaps', 'exception',
                               'extrinsic_matrices')}
        for c in self.views:
            out['paths'].append(os.path.join(frames_dir(self.data_dir), subdir, '{}_webcam_{}.jpg'.format(f, c)))
            rvec, tvec = self.calib[(subdir, c)]
            pose2d = project_points(world, rvec, tvec, INTRINSIC, np.zeros(5)) * np.array((sx, sy))
            center, exception = cpm_center(pose2d, self.width, self.height)
            heat = np.zeros((len(pose2d) + 1, self.hm_h, self.hm_w), dtype=np.float32)
            for i, (x, y) in enumerate(pose2d):
                heat[i + 1] = gaussian_map(self.hm_h, self.hm_w, int(x) / fx, int(y) / fy, self.sigma)
            heat[0] = 1.0 - heat[1:].max(axis=0)
            out['pose2d'].append(pose2d / np.array((fx, fy)))
            out['visibility'].append(visibility(pose2d, self.width, self.height))
            out['heatmaps'].append(heat)
            out['centermaps'].append(gaussian_map(self.height, self.width, center[0], center[1], 3).astype(np.float32)[None])
            out['exception'].append(exception)
            out['extrinsic_matrices'].append(np.c_[rodrigues(rvec), tvec])
        V = len(self.views)
        out = {k: v if k == 'paths' else np.stack(v) for k, v in out.items()}
        out.update(frames=1, views=V, pose3d=world, intrinsic_matrix=INTRINSIC,
                   inverse=np.tile(np.array([[1 / sx, 0., 0.], [0., 1 / sy, 0.]]), (V, 1, 1)),
                   hm_inverse=np.tile(np.array([[FRAME_W / self.hm_w, 0., 0.], [0., FRAME_H / self.hm_h, 0.]]), (V, 1, 1)))
        return out


READERS = {'MHP': MHP, 'MHP_kpt': MHP_kpt, 'MHP_seq': MHP_seq, 'MHP_mv': MHP_mv, 'MHP_CPM_kpt': MHP_CPM_kpt,
           'MHP_CPM_mv': MHP_CPM_mv}
CPM_KEYS = ('heatmaps', 'centermaps', 'exception')


def decode(path, bgr):
    img = read_image_rgb(path)
    if img.shape[:2] != (FRAME_H, FRAME_W):
        raise ValueError('{}: {} x {} px, MHP frames are {} x {}'.format(path, img.shape[1], img.shape[0], FRAME_W,
                                                                          FRAME_H))
    return img[:, :, ::-1] if bgr else img


def slot_order(batch, frames, views):
    """slot of image (b, j, v) of a batch: (j * batch + b) * views + v, frame-major"""
    b, j, v = np.meshgrid(np.arange(batch), np.arange(frames), np.arange(views), indexing='ij')
    return ((j * batch + b) * views + v).reshape(batch, frames * views)


MULTI_VIEW_KEYS = ('pose3d', 'extrinsic_matrices', 'intrinsic_matrix')


def collate(samples, bgr=False):
    """worker side: every distinct frame of the batch decoded once (with the sample's occlusion disc painted on it,
    when it carries one) and packed into one u8 CPU buffer; a slot table row per image (rows of a shared frame point
    at the same bytes), in slot_order; the f32 inverse matrices; the labels stacked over (sample, view); the
    multi-view extras of MHP_mv stacked over samples"""
    F, V = samples[0]['frames'], samples[0]['views']
    order = slot_order(len(samples), F, V)
    unique, where = [], {}
    for s in samples:
        discs = s.get('occlusion') or [None] * len(s['paths'])
        for key in zip(s['paths'], discs):
            if key not in where:
                where[key] = len(unique)
                unique.append(key)
    frames = []
    for p, disc in unique:
        img = decode(p, bgr)
        frames.append(img if disc is None else paint_disc(img, disc))
    packed = pack_images(frames, pin=False)
    n = len(samples) * F * V
    table = torch.empty((n, 4), dtype=torch.int64)
    inverse = np.empty((n, 2, 3))
    for b, s in enumerate(samples):
        slots = torch.from_numpy(order[b])
        discs = s.get('occlusion') or [None] * len(s['paths'])
        table[slots] = packed.table[[where[key] for key in zip(s['paths'], discs)]]
        inverse[order[b]] = s['inverse']
    cat = lambda k: np.concatenate([s[k] for s in samples])
    out = {'buffer': packed.buffer, 'table': table,
           'inverse': torch.from_numpy(inverse.astype(np.float32).reshape(-1, 6)),
           'pose2d': torch.from_numpy(cat('pose2d').astype(np.float32)),
           'visibility': torch.from_numpy(cat('visibility')),
           'hm_inverse': torch.from_numpy(cat('hm_inverse'))}
    for k in MULTI_VIEW_KEYS:                          # MHP_mv: one entry per sample, stacked to (B, ...) float64
        if k in samples[0]:
            out[k] = torch.from_numpy(np.stack([np.asarray(s[k], dtype=np.float64) for s in samples]))
    for k in CPM_KEYS:                                 # MHP_CPM_kpt: per image, stacked like the labels
        if k in samples[0]:
            out[k] = torch.from_numpy(np.concatenate([s[k] for s in samples]))
    return out


def collate_bgr(samples):
    return collate(samples, bgr=True)


def collate_rgb(samples):
    return collate(samples, bgr=False)


def make_loader(cfg, name, subset, is_train, rank=0, world=1, distributed=False, max_batches=None, heatmaps=None,
                **reader_kw):
    """reader_kw reach the reader (MHP_mv: views)"""
    dataset = READERS[name](cfg, subset, is_train=is_train, **reader_kw)
    fn = collate_bgr if dataset.bgr else collate_rgb
    if is_train:
        return RHDLoader(cfg, dataset, cfg.TRAIN.IMAGES_PER_GPU, True, rank if distributed else 0,
                         world if distributed else 1, max_batches, heatmaps, collate_fn=fn)
    return RHDLoader(cfg, dataset, cfg.TEST.IMAGES_PER_GPU, False, max_batches=max_batches, heatmaps=heatmaps,
                     collate_fn=fn)
