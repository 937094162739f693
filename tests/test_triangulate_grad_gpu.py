"""hrnet_triangulate_bwd and hrnet_joints3d_loss_* on the device, through utils/multiview.py and core/loss.py: the
reference's own float64 autograd gradients (tests/golden/triangulation_grad.npz) to 1e-6 of each case's largest
gradient - the forward's RTOL of tests/test_triangulate_gpu.py: the f32 output rounds at 6e-8, the f64 inside is at
worst the 4e-9 the A^T A route shows on the CPU - on every case, the near-parallel rig included; sizes that do not fill
a wave; eight views; the same X bits with and without a graph; the heat-map -> frame mapping; zero weights; degenerate
points; the 3-D loss against float64 torch. Each test runs in a spawned child (tests/spawned.py)."""
import os

import numpy as np
import pytest
import torch

import triangulate_grad_ref as G
from spawned import spawned

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'triangulation.npz')
GRAD = os.path.join(HERE, 'golden', 'triangulation_grad.npz')
RTOL = 1e-6


def _cases(z):
    return sorted(k[:-2] for k in z.files if k.endswith('_X'))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to('cuda', dtype) if dtype is not None else t.cuda()


def _grads(proj, pts, gX, conf=None, to_frame=None):
    """-> (X, dpts, dconf or None) as numpy, through the public function and autograd"""
    from utils.multiview import triangulate_batch_of_points
    p = _dev(pts, torch.float32).requires_grad_(True)
    c = None if conf is None else _dev(conf, torch.float32).requires_grad_(True)
    X = triangulate_batch_of_points(_dev(proj), p, c, to_frame=None if to_frame is None else _dev(to_frame))
    assert X.requires_grad and X.dtype == torch.float32
    X.backward(_dev(gX, torch.float32))
    torch.cuda.synchronize()
    return X.detach().cpu().numpy(), p.grad.cpu().numpy(), None if c is None else c.grad.cpu().numpy()


def _err(got, ref):
    return np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max()


def _case(z, g, name):
    conf = z[name + '_conf'] if name + '_conf' in z.files else None
    return z[name + '_proj'], z[name + '_pts'], g[name + '_gX'], conf


@spawned
def test_gradients_match_the_reference_on_every_case():
    z, g = np.load(GOLD), np.load(GRAD)
    for name in _cases(z):
        proj, pts, gX, conf = _case(z, g, name)
        _, dpts, dconf = _grads(proj, pts, gX, conf)
        assert dpts.shape == pts.shape and dpts.dtype == np.float32
        err = _err(dpts, g[name + '_dpts'])
        print(name, 'dpts', err)
        assert err <= RTOL, (name, err)
        if name + '_dconf' in g.files:
            err = _err(dconf, g[name + '_dconf'])
            print(name, 'dconf', err)
            assert err <= RTOL, (name, err)


@spawned
def test_odd_sizes_and_eight_views():
    z, g = np.load(GOLD), np.load(GRAD)
    name = 'near_noisy_v4_conf'
    proj, pts, gX, conf = _case(z, g, name)
    rp, rc = g[name + '_dpts'], g[name + '_dconf']
    for B in (1, 3, 32, 37):                       # B * K = 21, 63, 672, 777
        idx = np.arange(B) % 4
        _, dpts, dconf = _grads(proj[idx], pts[idx], gX[idx], conf[idx])
        assert _err(dpts, rp[idx]) <= RTOL and _err(dconf, rc[idx]) <= RTOL, B
    for K in (1, 5, 64):
        kk = np.arange(K) % 21
        _, dpts, dconf = _grads(proj, pts[:, :, kk], gX[:, kk], conf[:, :, kk])
        # the bound is relative to the largest gradient of the whole case, as above
        assert np.abs(dpts - rp[:, :, kk]).max() <= RTOL * np.abs(rp).max(), K
        assert np.abs(dconf - rc[:, :, kk]).max() <= RTOL * np.abs(rc).max(), K
    # V = 8: every view twice, against the numpy restatement of the formula (itself held to the fixture on the CPU)
    v8 = np.r_[0:4, 0:4]
    ref_p, ref_c = G.grad_batch(proj[:, v8], pts[:, v8], conf[:, v8], gX)
    _, dpts, dconf = _grads(proj[:, v8], pts[:, v8], gX, conf[:, v8])
    assert _err(dpts, ref_p) <= RTOL and _err(dconf, ref_c) <= RTOL
    # the two copies of a view have the same inputs, so the same bits
    assert np.array_equal(dpts[:, :4], dpts[:, 4:]) and np.array_equal(dconf[:, :4], dconf[:, 4:])


@spawned
def test_x_is_the_forward_bit_for_bit():
    from utils.multiview import triangulate_batch_of_points
    z, g = np.load(GOLD), np.load(GRAD)
    rng = np.random.default_rng(5)
    for name in ('near_noisy_v4_conf', 'wide_noisy_v3'):
        proj, pts, gX, conf = _case(z, g, name)
        B, V = pts.shape[:2]
        to_frame = np.zeros((B * V, 2, 3))
        to_frame[:, 0, 0], to_frame[:, 1, 1] = rng.uniform(0.9, 1.1, B * V), rng.uniform(0.9, 1.1, B * V)
        to_frame[:, :, 2] = rng.uniform(-3, 3, (B * V, 2))
        for mat in (None, to_frame):
            X, _, _ = _grads(proj, pts, gX, conf, mat)
            plain = triangulate_batch_of_points(_dev(proj), _dev(pts), None if conf is None else _dev(conf),
                                                to_frame=None if mat is None else _dev(mat))
            assert not plain.requires_grad
            assert np.array_equal(X.view(np.uint32), plain.cpu().numpy().view(np.uint32)), name
            # under no_grad inputs that require a gradient take the plain path too
            with torch.no_grad():
                same = triangulate_batch_of_points(_dev(proj), _dev(pts).requires_grad_(True),
                                                   None if conf is None else _dev(conf),
                                                   to_frame=None if mat is None else _dev(mat))
            assert not same.requires_grad and torch.equal(same, plain)
    # frame points on request stay out of the graph and are the forward's
    proj, pts, gX, conf = _case(z, g, 'wide_noisy_v3')
    p = _dev(pts).requires_grad_(True)
    X, frame = triangulate_batch_of_points(_dev(proj), p, return_frame_points=True)
    assert X.requires_grad and not frame.requires_grad and torch.equal(frame, p.detach())


@spawned
def test_to_frame_gradient_is_the_transposed_linear_part():
    z, g = np.load(GOLD), np.load(GRAD)
    name = 'wide_noisy_v4'
    proj, pts, gX = z[name + '_proj'], z[name + '_pts'].astype(np.float64), g[name + '_gX']
    B, V, K = pts.shape[:3]
    rng = np.random.default_rng(11)
    # the per-slot affine of test_to_frame_equals_mapping_on_the_host: frame -> heat map, and its inverse for the kernel
    fwd = np.zeros((B * V, 3, 3))
    fwd[:, 0, 0], fwd[:, 1, 1] = rng.uniform(0.12, 0.15, B * V), rng.uniform(0.12, 0.15, B * V)
    fwd[:, 0, 1], fwd[:, 1, 0] = rng.uniform(-0.01, 0.01, B * V), rng.uniform(-0.01, 0.01, B * V)
    fwd[:, :2, 2] = rng.uniform(-20, 5, (B * V, 2))
    fwd[:, 2, 2] = 1.0
    inv = np.linalg.inv(fwd)[:, :2]
    flat = pts.reshape(B * V, K, 2)
    hm = (np.einsum('sij,skj->ski', fwd[:, :2, :2], flat) + fwd[:, None, :2, 2]).astype(np.float32)
    _, dhm, _ = _grads(proj, hm.reshape(B, V, K, 2), gX, to_frame=inv)
    mapped = np.einsum('sij,skj->ski', inv[:, :, :2], hm.astype(np.float64)) + inv[:, None, :, 2]
    _, dframe, _ = _grads(proj, mapped.reshape(B, V, K, 2).astype(np.float32), gX)
    expect = np.einsum('sji,skj->ski', inv[:, :, :2], dframe.reshape(B * V, K, 2).astype(np.float64))
    err = _err(dhm.reshape(B * V, K, 2), expect)
    print('to_frame', err)
    assert err <= 1e-5                             # the bound of test_to_frame_equals_mapping_on_the_host


@spawned
def test_zero_weight_views_get_exact_zeros():
    z, g = np.load(GOLD), np.load(GRAD)
    for name in ('near_noisy_v4_conf', 'wide_noisy_v4_conf'):
        proj, pts, gX, conf = _case(z, g, name)
        _, dpts, dconf = _grads(proj, pts, gX, conf)
        off = conf == 0
        assert off.sum() == 4 * (7 + 5)
        assert (dpts[off] == 0).all() and (dconf[off] == 0).all()
        assert (dpts[~off] != 0).all() and (dconf[~off] != 0).all()
        # with a to_frame as well
        mat = np.tile(np.array([[1.5, 0.1, -2.0], [-0.2, 0.8, 3.0]]), (pts.shape[0] * pts.shape[1], 1, 1))
        _, dpts, dconf = _grads(proj, pts, gX, conf, mat)
        assert (dpts[off] == 0).all() and (dconf[off] == 0).all() and np.isfinite(dpts).all()


@spawned
def test_degenerate_points_are_nan_for_that_point_only():
    z, g = np.load(GOLD), np.load(GRAD)
    name = 'wide_noisy_v4'
    proj, pts, gX = z[name + '_proj'], z[name + '_pts'], g[name + '_gX']
    ref = g[name + '_dpts']
    conf = np.ones(pts.shape[:3], np.float32)
    conf[0, :, 3] = 0.0                              # no view
    conf[1, 1:, 5] = 0.0                             # one view
    conf[2, 2:, 7] = 0.0                             # two views: defined
    X, dpts, dconf = _grads(proj, pts, gX, conf)
    assert np.isnan(X[0, 3]).all() and np.isnan(X[1, 5]).all()
    assert np.isnan(dpts[0, :, 3]).all() and np.isnan(dconf[0, :, 3]).all()
    assert np.isnan(dpts[1, :, 5]).all() and np.isnan(dconf[1, :, 5]).all()
    assert np.isfinite(dpts[2, :, 7]).all() and (dpts[2, 2:, 7] == 0).all() and (dpts[2, :2, 7] != 0).all()
    mask = np.ones((4, 4, 21), bool)
    mask[0, :, 3] = mask[1, :, 5] = mask[2, :, 7] = False
    assert np.isfinite(dpts[mask]).all() and np.isfinite(dconf[mask]).all()
    assert np.abs(dpts[mask] - ref[mask]).max() <= RTOL * np.abs(ref).max()      # unit weights: the unweighted case
    # a non-finite point gives non-finite gradients for that point only, and the launch ends
    bad = pts.copy()
    bad[3, 0, 0] = np.nan
    X, dpts, _ = _grads(proj, bad, gX)
    assert not np.isfinite(X[3, 0]).any() and not np.isfinite(dpts[3, :, 0]).any()
    keep = np.ones((4, 4, 21), bool)
    keep[3, :, 0] = False
    assert np.isfinite(dpts[keep]).all()
    assert np.abs(dpts[keep] - ref[keep]).max() <= RTOL * np.abs(ref).max()


@spawned
def test_joints3d_loss_against_float64_torch():
    from core.loss import Joints3DMSELoss
    rng = np.random.default_rng(3)
    for B, K in ((1, 1), (4, 21), (32, 21), (37, 64)):      # B * K up to 2368: several rounds of the 256 threads
        pred = rng.normal(0, 80, (B, K, 3)).astype(np.float32)
        gt = rng.normal(0, 80, (B, K, 3)).astype(np.float32)
        gt[0, 0] = pred[0, 0]                                # a zero difference: zero gradient, as torch.norm
        p64 = torch.from_numpy(pred).double().requires_grad_(True)
        ref = torch.norm(torch.from_numpy(gt).double() - p64, dim=2).sum() / K
        (ref * 0.75).backward()
        out = []
        for _ in range(2):
            p = _dev(pred).requires_grad_(True)
            loss = Joints3DMSELoss()(p, _dev(gt))
            (loss * 0.75).backward()
            torch.cuda.synchronize()
            out.append((loss.detach().cpu().numpy(), p.grad.cpu().numpy()))
        assert out[0][0].dtype == np.float32 and out[0][0].shape == ()
        assert abs(float(out[0][0]) - ref.item()) <= 1e-6 * abs(ref.item()), (B, K)
        gref = p64.grad.numpy()
        assert np.abs(out[0][1] - gref).max() <= 1e-6 * np.abs(gref).max(), (B, K)
        assert (out[0][1][0, 0] == 0).all()
        assert out[0][0].tobytes() == out[1][0].tobytes() and np.array_equal(out[0][1], out[1][1])
    with pytest.raises(ValueError, match='B x K x 3'):
        Joints3DMSELoss()(torch.zeros(2, 21, 2, device='cuda'), torch.zeros(2, 21, 2, device='cuda'))
