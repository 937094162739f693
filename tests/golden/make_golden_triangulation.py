"""Writes tests/golden/triangulation.npz: the reference's own DLT triangulation on fixed inputs, for
tests/test_triangulate_cpu.py and tests/test_triangulate_gpu.py.

    python tests/golden/make_golden_triangulation.py <reference checkout>

Imports only numpy, torch and the reference's lib/models/triangulation_model_utils/multiview.py (by file path). Cases:
the MHP intrinsics; a wide four-camera rig (cameras 600 units from the origin, 70 degrees apart) and the near-parallel
rig of tests/mhp_tree.calibration (directory 17: cameras 10-40 units apart at 600, restated below); noiseless and
1 px noise 2-D points; V = 2, 3, 4 (the first V cameras); with confidences (some zero) at V = 4.
- no confidences: triangulate_point_from_multiple_views_linear (numpy SVD, float64);
- confidences: triangulate_point_from_multiple_views_linear_torch in float64 (the per-point function of
  triangulate_batch_of_points, whose float32 output buffer would round the result; the batch function is run too and
  checked against it to that rounding).
The 2-D points are stored as float32 (the kernel's input type) and triangulated from exactly those values.
Also stored: the occlusion joint of the MHP multi-view reader, random.seed(4 i + c); random.randint(0, 20), for
i < 64 and c = 1..4 (reference MHPMultiViewDataset.py:168-172)."""
import importlib.util
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
INTRINSIC = np.array([[614.878, 0, 313.219], [0, 615.479, 231.288], [0, 0, 1]])
B, K = 4, 21


def rodrigues(r):
    theta = np.linalg.norm(r)
    if theta == 0:
        return np.eye(3)
    k = r / theta
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(theta) * np.eye(3) + (1 - np.cos(theta)) * np.outer(k, k) + np.sin(theta) * kx


def near_rig(d=17):
    """tests/mhp_tree.calibration(d, c), c = 1..4: rvec (0.05c, -0.03c, 0.02d), tvec (10c, -5c, 600 + d)"""
    out = []
    for c in range(1, 5):
        R = rodrigues(np.array([0.05 * c, -0.03 * c, 0.02 * d]))
        t = np.array([10.0 * c, -5.0 * c, 600.0 + d])
        out.append(INTRINSIC @ np.c_[R, t])
    return np.stack(out)


def wide_rig():
    """four cameras on a circle of radius 600 about the y axis, 70 degrees apart, slightly above, looking at 0"""
    out = []
    for c in range(4):
        a = np.deg2rad(-105 + 70 * c)
        centre = np.array([600 * np.sin(a), -80.0 + 40 * c, -600 * np.cos(a)])
        f = -centre / np.linalg.norm(centre)
        right = np.cross([0.0, 1.0, 0.0], f)
        right /= np.linalg.norm(right)
        down = np.cross(f, right)
        R = np.stack((right, down, f))
        out.append(INTRINSIC @ np.c_[R, -R @ centre])
    return np.stack(out)


def world_points(rng, n):
    """hand-sized points with |X| >= 50, so that a relative error is a fair measure"""
    pts = []
    while len(pts) < n:
        p = np.r_[rng.uniform(-120, 120, 2), rng.uniform(-40, 40)] + np.array([20.0, -10.0, 15.0])
        if np.linalg.norm(p) >= 50:
            pts.append(p)
    return np.array(pts)


def project(proj, X):
    h = np.einsum('vij,nj->vni', proj, np.c_[X, np.ones(len(X))])
    return h[..., :2] / h[..., 2:]


def main(ref_root):
    spec = importlib.util.spec_from_file_location(
        'ref_multiview', os.path.join(ref_root, 'lib', 'models', 'triangulation_model_utils', 'multiview.py'))
    mv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mv)
    rng = np.random.default_rng(20261016)
    out = {'intrinsic': INTRINSIC}
    for rig_name, rig in (('wide', wide_rig()), ('near', near_rig())):
        out['rig_' + rig_name] = rig
        for noise in (0.0, 1.0):
            for V in (2, 3, 4):
                confs = (False, True) if V == 4 and noise else (False,)
                for with_conf in confs:
                    name = '{}_{}_v{}{}'.format(rig_name, 'noisy' if noise else 'clean', V, '_conf' if with_conf else '')
                    world = world_points(rng, B * K).reshape(B, K, 3)
                    proj = np.broadcast_to(rig[:V], (B, V, 3, 4)).copy()
                    pts = np.stack([project(proj[b], world[b]) for b in range(B)])            # B V K 2
                    pts = (pts + rng.normal(0, noise, pts.shape)).astype(np.float32)
                    conf = None
                    if with_conf:
                        conf = rng.uniform(0.2, 1.0, (B, V, K)).astype(np.float32)
                        conf[:, 1, ::3] = 0.0             # view 1 dropped for every third joint
                        conf[:, 3, 1::4] = 0.0            # view 3 for every fourth
                    X = np.empty((B, K, 3))
                    for b in range(B):
                        for k in range(K):
                            p2 = pts[b, :, k].astype(np.float64)
                            if conf is None:
                                X[b, k] = mv.triangulate_point_from_multiple_views_linear(proj[b], p2)
                            else:
                                X[b, k] = mv.triangulate_point_from_multiple_views_linear_torch(
                                    torch.from_numpy(proj[b]), torch.from_numpy(p2),
                                    torch.from_numpy(conf[b, :, k].astype(np.float64))).numpy()
                    if conf is not None:
                        Xb = mv.triangulate_batch_of_points(torch.from_numpy(proj), torch.from_numpy(pts.astype(np.float64)),
                                                            torch.from_numpy(conf.astype(np.float64))).numpy()
                        assert np.allclose(Xb, X, rtol=1e-6, atol=1e-4), 'batch function disagrees'
                    out[name + '_proj'] = proj
                    out[name + '_pts'] = pts
                    out[name + '_X'] = X
                    out[name + '_world'] = world
                    if conf is not None:
                        out[name + '_conf'] = conf
    occl = np.empty((64, 4), dtype=np.int64)
    for i in range(64):
        for c in range(1, 5):
            random.seed(4 * i + c)
            occl[i, c - 1] = random.randint(0, 20)
    out['occlusion_joint'] = occl
    path = os.path.join(HERE, 'triangulation.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '/path/to/reference')
