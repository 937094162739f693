"""hrnet_triangulate (csrc/triangulate.hip) through utils/multiview.py on the device: the reference's own results in
tests/golden/triangulation.npz (tests/golden/make_golden_triangulation.py) to 1e-6 relative on every case, the
near-parallel rig included; noiseless recovery; zero weights; the heat-map -> frame mapping; batch sizes that do not
fill a wave; degenerate points. Each test runs in a spawned child (tests/spawned.py)."""
import os

import numpy as np
import pytest
import torch

from spawned import spawned

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'triangulation.npz')
RTOL = 1e-6


def _cases(z):
    return sorted(k[:-2] for k in z.files if k.endswith('_X'))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to('cuda', dtype) if dtype is not None else t.cuda()


def _run(proj, pts, conf=None, to_frame=None, frame_points=False):
    from utils.multiview import triangulate_batch_of_points
    out = triangulate_batch_of_points(_dev(proj), _dev(pts), None if conf is None else _dev(conf),
                                      to_frame=None if to_frame is None else _dev(to_frame),
                                      return_frame_points=frame_points)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out) if frame_points else out.cpu().numpy()


def _rel(X, ref):
    return np.linalg.norm(X.astype(np.float64) - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


@spawned
def test_matches_the_reference_on_every_case():
    z = np.load(GOLD)
    for name in _cases(z):
        conf = z[name + '_conf'] if name + '_conf' in z.files else None
        X = _run(z[name + '_proj'], z[name + '_pts'], conf)
        assert X.shape == z[name + '_X'].shape == (4, 21, 3)           # B * K = 84: not a multiple of 64
        rel = _rel(X, z[name + '_X'])
        assert rel.max() <= RTOL, (name, rel.max())


@spawned
def test_larger_and_odd_batches_and_eight_views():
    z = np.load(GOLD)
    name = 'near_noisy_v4_conf'
    proj, pts, conf, ref = z[name + '_proj'], z[name + '_pts'], z[name + '_conf'], z[name + '_X']
    for B in (1, 3, 32, 37):                       # B * K = 21, 63, 672, 777
        idx = np.arange(B) % 4
        X = _run(proj[idx], pts[idx], conf[idx])
        assert _rel(X, ref[idx]).max() <= RTOL, B
    for K in (1, 5, 64):
        kk = np.arange(K) % 21
        X = _run(proj, pts[:, :, kk], conf[:, :, kk])
        assert _rel(X, ref[:, kk]).max() <= RTOL, K
    # V = 8: every view twice (each row pair repeated) has the same null vector
    v8 = np.r_[0:4, 0:4]
    X = _run(proj[:, v8], pts[:, v8], conf[:, v8])
    assert _rel(X, ref).max() <= RTOL


@spawned
def test_noiseless_projections_recover_the_points():
    z = np.load(GOLD)
    for name in _cases(z):
        if '_clean_' in name:
            X = _run(z[name + '_proj'], z[name + '_pts'])
            err = np.abs(X - z[name + '_world']).max()
            assert err <= 1e-3, (name, err)


@spawned
def test_zero_weight_view_equals_dropping_it():
    z = np.load(GOLD)
    for rig in ('wide', 'near'):
        name = rig + '_noisy_v4'
        proj, pts = z[name + '_proj'], z[name + '_pts']
        conf = np.ones(pts.shape[:3], np.float32)
        conf[:, 2] = 0.0
        X = _run(proj, pts, conf)
        keep = [0, 1, 3]
        ref = _run(proj[:, keep], pts[:, keep])
        assert _rel(X, ref.astype(np.float64)).max() <= RTOL, rig


@spawned
def test_to_frame_equals_mapping_on_the_host():
    z = np.load(GOLD)
    name = 'wide_noisy_v4'
    proj, pts = z[name + '_proj'], z[name + '_pts'].astype(np.float64)
    B, V, K = pts.shape[:3]
    rng = np.random.default_rng(11)
    # per-slot affine frame -> heat map (a scale near 64/480, a small shear, a shift), and its inverse for the kernel
    fwd = np.zeros((B * V, 3, 3))
    fwd[:, 0, 0], fwd[:, 1, 1] = rng.uniform(0.12, 0.15, B * V), rng.uniform(0.12, 0.15, B * V)
    fwd[:, 0, 1], fwd[:, 1, 0] = rng.uniform(-0.01, 0.01, B * V), rng.uniform(-0.01, 0.01, B * V)
    fwd[:, :2, 2] = rng.uniform(-20, 5, (B * V, 2))
    fwd[:, 2, 2] = 1.0
    inv = np.linalg.inv(fwd)[:, :2]
    flat = pts.reshape(B * V, K, 2)
    hm = (np.einsum('sij,skj->ski', fwd[:, :2, :2], flat) + fwd[:, None, :2, 2]).astype(np.float32)
    X, frame = _run(proj, hm.reshape(B, V, K, 2), to_frame=inv, frame_points=True)
    mapped = np.einsum('sij,skj->ski', inv[:, :, :2], hm.astype(np.float64)) + inv[:, None, :, 2]
    assert np.abs(frame.reshape(B * V, K, 2) - mapped).max() <= 1e-3        # f32 output of ~600 px values
    ref = _run(proj, mapped.reshape(B, V, K, 2).astype(np.float32))
    assert _rel(X, ref.astype(np.float64)).max() <= 1e-5
    # null to_frame: the frame points come back as given
    _, same = _run(proj, pts.astype(np.float32), frame_points=True)
    assert np.array_equal(same, pts.astype(np.float32))


@spawned
def test_fewer_than_two_weighted_views_is_nan():
    z = np.load(GOLD)
    name = 'wide_noisy_v4'
    proj, pts, ref = z[name + '_proj'], z[name + '_pts'], z[name + '_X']
    conf = np.ones(pts.shape[:3], np.float32)
    conf[0, :, 3] = 0.0                              # no view
    conf[1, 1:, 5] = 0.0                             # one view
    conf[2, 2:, 7] = 0.0                             # two views: defined
    X = _run(proj, pts, conf)
    assert np.isnan(X[0, 3]).all() and np.isnan(X[1, 5]).all() and np.isfinite(X[2, 7]).all()
    mask = np.ones((4, 21), bool)
    mask[0, 3] = mask[1, 5] = mask[2, 7] = False
    assert _rel(X[mask], ref[mask]).max() <= RTOL
    # a non-finite point gives a non-finite result for that point only, and the launch ends
    bad = pts.copy()
    bad[3, 0, 0] = np.nan
    X = _run(proj, bad)
    assert not np.isfinite(X[3, 0]).all() and np.isfinite(np.delete(X.reshape(-1, 3), 3 * 21, 0)).all()
