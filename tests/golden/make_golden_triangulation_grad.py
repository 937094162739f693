"""Writes tests/golden/triangulation_grad.npz: the gradients of the reference's own DLT triangulation under float64 CPU
autograd, for tests/test_triangulate_grad_cpu.py and tests/test_triangulate_grad_gpu.py.

    python tests/golden/make_golden_triangulation_grad.py <reference checkout>

Imports only numpy, torch and the reference's lib/models/triangulation_model_utils/multiview.py (by file path). For
every case of tests/golden/triangulation.npz (the same proj, the pts as stored in float32, the conf) and a fixed random
gX (B, K, 3), the point function triangulate_point_from_multiple_views_linear_torch (torch.svd) is run in float64 with
the points and the confidences requiring grad, and (X * gX).sum() is back-propagated. Stored per case:
- <case>_gX   (B, K, 3) float64
- <case>_dpts (B, V, K, 2) float64, every case (a case without confidences is run with none)
- <case>_dconf (B, V, K) float64, the `noisy` cases with confidences only: on noiseless points the true dconf is zero
  and what autograd returns is the float32 rounding of the inputs."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref_root):
    spec = importlib.util.spec_from_file_location(
        'ref_multiview', os.path.join(ref_root, 'lib', 'models', 'triangulation_model_utils', 'multiview.py'))
    mv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mv)
    z = np.load(os.path.join(HERE, 'triangulation.npz'))
    rng = np.random.default_rng(20261017)
    out = {}
    for name in sorted(k[:-2] for k in z.files if k.endswith('_X')):
        proj = torch.from_numpy(z[name + '_proj'])
        pts = torch.from_numpy(z[name + '_pts'].astype(np.float64)).requires_grad_(True)
        conf = None
        if name + '_conf' in z.files:
            conf = torch.from_numpy(z[name + '_conf'].astype(np.float64)).requires_grad_(True)
        B, V, K = pts.shape[:3]
        gX = rng.normal(0.0, 1.0, (B, K, 3))
        total = 0.0
        for b in range(B):
            for k in range(K):
                X = mv.triangulate_point_from_multiple_views_linear_torch(
                    proj[b], pts[b, :, k], None if conf is None else conf[b, :, k])
                assert np.allclose(X.detach().numpy(), z[name + '_X'][b, k], rtol=1e-9, atol=1e-7), name
                total = total + (X * torch.from_numpy(gX[b, k])).sum()
        total.backward()
        out[name + '_gX'] = gX
        out[name + '_dpts'] = pts.grad.numpy()
        if conf is not None and '_noisy_' in name:
            out[name + '_dconf'] = conf.grad.numpy()
    path = os.path.join(HERE, 'triangulation_grad.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '/path/to/reference')
