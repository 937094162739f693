"""Host side of the multi-view triangulation (csrc/triangulate.hip, utils/multiview.py): the float64 numpy restatement
of the kernel's method (tests/triangulate_ref.py: Givens QR of the DLT rows, one-sided Jacobi SVD) against the
reference's own results in tests/golden/triangulation.npz (tests/golden/make_golden_triangulation.py); the float32
A^T A shortcut against the same results, to show that the GPU tests' 1e-6 tolerance rejects it; the C ABI entry."""
import os

import numpy as np
import pytest

import triangulate_ref as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'triangulation.npz')
GPU_RTOL = 1e-6             # tests/test_triangulate_gpu.py


def _cases(z):
    return sorted(k[:-2] for k in z.files if k.endswith('_X'))


def _case(z, name):
    conf = z[name + '_conf'] if name + '_conf' in z.files else None
    return z[name + '_proj'], z[name + '_pts'].astype(np.float64), conf, z[name + '_X']


def _rel(X, ref):
    return np.linalg.norm(X - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


def test_fixture_covers_the_cases():
    z = np.load(GOLD)
    names = _cases(z)
    for rig in ('wide', 'near'):
        for noise in ('clean', 'noisy'):
            for v in (2, 3, 4):
                assert '{}_{}_v{}'.format(rig, noise, v) in names
        assert '{}_noisy_v4_conf'.format(rig) in names
        assert (z['{}_noisy_v4_conf_conf'.format(rig)] == 0).any()
    assert z['occlusion_joint'].shape == (64, 4)


def test_restatement_matches_the_reference():
    z = np.load(GOLD)
    for name in _cases(z):
        proj, pts, conf, ref = _case(z, name)
        X = T.triangulate_batch(proj, pts, conf)
        assert _rel(X, ref).max() <= 1e-9, name


def test_null_vector_is_the_svd_one_sign_free():
    z = np.load(GOLD)
    proj, pts, conf, _ = _case(z, 'near_noisy_v4_conf')
    for b in range(pts.shape[0]):
        for k in range(pts.shape[2]):
            _, v = T.triangulate(proj[b], pts[b, :, k], conf[b, :, k])
            ref = np.linalg.svd(T.dlt_rows(proj[b], pts[b, :, k], conf[b, :, k]))[2][3]
            assert min(np.abs(v - ref).max(), np.abs(v + ref).max()) <= 1e-9


def test_f32_normal_equations_miss_the_gpu_tolerance():
    """the shortcut the kernel avoids: on the near-parallel rig (cond(A) ~ 3e3) a float32 A^T A eigen-solve misses the
    reference by more than the GPU tolerance for many points, so that tolerance pins a float64 method"""
    z = np.load(GOLD)
    for name in ('near_noisy_v4', 'near_clean_v4', 'near_noisy_v4_conf'):
        proj, pts, conf, ref = _case(z, name)
        B, V, K = pts.shape[:3]
        X = np.array([[T.triangulate_ata_f32(proj[b], pts[b, :, k], None if conf is None else conf[b, :, k])
                       for k in range(K)] for b in range(B)])
        rel = _rel(X, ref)
        assert (rel > GPU_RTOL).sum() >= 10, (name, rel.max())


def test_fixture_near_rig_is_the_mhp_tree_rig():
    import mhp_tree
    from dataset.mhp import INTRINSIC, rodrigues
    z = np.load(GOLD)
    for c in range(1, 5):
        rvec, tvec = mhp_tree.calibration(17, c)
        P = INTRINSIC @ np.c_[rodrigues(rvec), tvec.reshape(3)]
        assert np.allclose(z['rig_near'][c - 1], P, rtol=1e-12, atol=1e-9)
    assert np.array_equal(z['intrinsic'], INTRINSIC)


def test_degenerate_restatement_is_nan():
    z = np.load(GOLD)
    proj, pts, _, _ = _case(z, 'wide_clean_v4')
    X, _ = T.triangulate(proj[0], pts[0, :, 0], np.array([0.0, 0.7, 0.0, 0.0]))
    assert np.isnan(X).all()


def test_c_abi_entry_point():
    from hipnet import _capi
    header = open(os.path.join(os.path.dirname(_capi.LIB_PATH), '..', '..', 'include', 'hrnet_hip.h')).read()
    assert 'int hrnet_triangulate(const float* pts, const double* to_frame, const double* proj, const float* conf, ' \
           'float* X,' in header
    assert 'hrnet_triangulate' in _capi.EXPORTED and _capi.ABI_VERSION == 2
    assert hasattr(_capi.lib(), 'hrnet_triangulate')      # loads without a GPU; nothing is launched


def test_python_surface_checks_its_arguments():
    import torch
    from utils.multiview import triangulate_batch_of_points
    proj, pts = torch.zeros(2, 4, 3, 4), torch.zeros(2, 4, 21, 2)
    with pytest.raises(RuntimeError, match='HIP-device'):
        triangulate_batch_of_points(proj, pts)
    with pytest.raises(ValueError, match='proj_matricies_batch'):
        triangulate_batch_of_points(proj[:, :3], pts)
    with pytest.raises(ValueError, match='confidences_batch'):
        triangulate_batch_of_points(proj, pts, torch.ones(2, 4, 20))
    with pytest.raises(ValueError, match='to_frame'):
        triangulate_batch_of_points(proj, pts, to_frame=torch.zeros(2, 2, 3))
