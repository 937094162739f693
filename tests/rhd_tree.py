"""A small fake RHD tree for the reader's tests (tests/test_rhd_dataset_cpu.py, tests/test_rhd_dataset_gpu.py):
<root>/RHD/<subset>/color/NNNNN.png (random 320 x 320 RGB, PIL) and anno_<subset>.pickle {index: {'uv_vis': 42 x 3}},
the annotations of tests/golden/rhd_geometry.npz."""
import os
import pickle

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), 'hrnet-hand-pose-estimation_amd')
YAML = os.path.join(PKG, 'experiments', 'RHD', 'RHD_HRNet_w32_max_hmloss_v1.yaml')


def golden():
    return np.load(os.path.join(HERE, 'golden', 'rhd_geometry.npz'))


def write_tree(root, subsets=('training', 'evaluation'), uv_vis=None, seed=0):
    """write the fake dataset under `root`; returns the uv_vis used"""
    from PIL import Image
    uv_vis = golden()['uv_vis'] if uv_vis is None else uv_vis
    rng = np.random.default_rng(seed)
    for subset in subsets:
        d = os.path.join(str(root), 'RHD', subset)
        os.makedirs(os.path.join(d, 'color'), exist_ok=True)
        for i in range(len(uv_vis)):
            img = rng.integers(0, 256, (320, 320, 3), dtype=np.uint8)
            Image.fromarray(img).save(os.path.join(d, 'color', '{:05d}.png'.format(i)))
        with open(os.path.join(d, 'anno_{}.pickle'.format(subset)), 'wb') as f:
            pickle.dump({i: {'uv_vis': uv_vis[i]} for i in range(len(uv_vis))}, f)
    return uv_vis


def config(data_dir, opts=()):
    from config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(['DATA_DIR', str(data_dir)] + list(opts))
    return cfg
