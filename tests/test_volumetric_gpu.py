"""The volumetric lifting kernels (csrc/volumetric.hip) on the device, through utils/volumetric.py and core/loss.py:
the reference's own float64 results (tests/golden/volumetric.npz) and, where a fixture would be too large, the float64
restatement tests/volumetric_ref.py (itself held to the fixture on the CPU, tests/test_volumetric_cpu.py).

Errors are max-abs over the case's largest reference magnitude. The unprojection bound, both directions, is 1e-5: a
sample carries at most 8 f32 roundings (5e-7 relative) per view, a gradient contribution about 6 (3.6e-7); contributions
are summed exactly (64-bit fixed point) or in f64, scaled by at most 1 + 2 max|sample| (about 6 here) under `softmax`,
and with S <= 2 max|grad| (S: the 'sum' gradient of |gV|, which bounds what reaches a pixel) that is <= 4.4e-6. The
integration: 1e-6 of max|coord| for the key points, 1e-6 of each map's largest p, 1e-5 of the largest dvols (f32 output
rounds at 6e-8, the sums are f64). Each test runs in a spawned child (tests/spawned.py)."""
import os

import numpy as np
import pytest
import torch

import volumetric_ref as R
from spawned import spawned

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'volumetric.npz')
METHODS = ('sum', 'max', 'softmax', 'conf')
TOL = 1e-5


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda', dtype)


def _err(got, ref):
    return np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max()


def _unproject(feat, proj, coord, gV, method, conf=None):
    """-> (vol, dfeat, dconf or None) as numpy, through the public function and autograd"""
    from utils.volumetric import unproject_heatmaps
    f = _dev(feat).requires_grad_(True)
    c = None if conf is None or not method.startswith('conf') else _dev(conf).requires_grad_(True)
    vol = unproject_heatmaps(f, _dev(proj), _dev(coord), method, c)
    assert vol.requires_grad and vol.dtype == torch.float32
    vol.backward(_dev(gV))
    torch.cuda.synchronize()
    return vol.detach().cpu().numpy(), f.grad.cpu().numpy(), None if c is None else c.grad.cpu().numpy()


def _rig(B, V, H, W, shape, rng, radius=600.0, side=100.0):
    """a box of `side` about a jittered centre seen by V ring cameras whose images overhang the H x W map a little"""
    centres = rng.uniform(-0.1 * side, 0.1 * side, (B, 3))
    axes = [np.linspace(-side / 2, side / 2, n) if n > 1 else np.zeros(1) for n in shape]
    grid = np.stack(np.meshgrid(*axes, indexing='ij'), -1)
    coord = (centres[:, None, None, None, :] + grid[None]).astype(np.float32)
    # column = u (W - 1) / H: a principal point of H / 2 is the middle column
    proj = np.stack([R.ring_cameras(V, radius, 1.0 * H * radius / side, (H / 2.0, W / 2.0)) for _ in range(B)])
    return proj.astype(np.float32), coord


def _bwd_planes(B, V, C, H, W):
    """planes per workgroup of hrnet_unproject_volume_bwd (the rule of csrc/volumetric.hip, restated so that a test
    that means to run the multi-plane path notices when the rule moves)"""
    ch = min(128 * 1024 // (H * W * 8), 4, C)
    while ch > 1 and B * V * -(-C // ch) < 512:
        ch -= 1
    return ch


@spawned
def test_unprojection_matches_the_reference():
    """achieved on one MI355X (max-abs / largest reference magnitude; bound 1e-5), forward / dfeatures: sum 9.7e-8 /
    5.9e-8, max 1.1e-7 / 5.7e-8, softmax 1.8e-7 / 1.0e-7, conf 1.0e-7 / 6.9e-8, dconf 7.4e-8; the case whose third
    camera looks away 1.2e-7 (dfeatures). The shapes of test_shapes_that_fill_nothing stay under 3.4e-7 / 1.8e-7, the
    64^3 volume of test_one_real_volume gives 3.0e-7 / 5.5e-8, the chain 3.3e-7."""
    z = np.load(GOLD)
    feat, proj, coord, conf, gV = (z['un_' + k] for k in ('feat', 'proj', 'coord', 'conf', 'gV'))
    for m in METHODS:
        vol, dfeat, dconf = _unproject(feat, proj, coord, gV, m, conf)
        assert vol.shape == (2, 3, 8, 6, 5) and dfeat.shape == feat.shape
        ev, ed = _err(vol, z['un_vol_' + m]), _err(dfeat, z['un_dfeat_' + m])
        print('fixture', m, 'forward {:.2e} dfeatures {:.2e}'.format(ev, ed))
        assert ev <= TOL and ed <= TOL, (m, ev, ed)
        if m == 'conf':
            ec = _err(dconf, z['un_dconf_conf'])
            print('fixture conf dconf {:.2e}'.format(ec))
            assert ec <= TOL, ec
    # any name beginning with 'conf' is the confidence-weighted sum
    a = _unproject(feat, proj, coord, gV, 'conf_norm', conf)
    b = _unproject(feat, proj, coord, gV, 'conf', conf)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the third camera looks away: its samples and its gradient are exactly zero
    away = z['un_proj_away']
    vol3, dfeat, _ = _unproject(feat, away, coord, gV, 'softmax')
    assert (dfeat[:, 2] == 0).all() and (dfeat[:, :2] != 0).any()
    ed = _err(dfeat[0], z['un_away_dfeat_softmax'])
    print('looking away: dfeatures {:.2e}'.format(ed))
    assert ed <= TOL
    for m in ('sum', 'max'):
        vol3, d3, _ = _unproject(feat, away, coord, gV, m)
        if m == 'max':                                      # the zeros take part in the maximum
            vol2 = np.maximum(_unproject(feat[:, :2], away[:, :2], coord, gV, m)[0], 0.0)
        else:
            vol2 = _unproject(feat[:, :2], away[:, :2], coord, gV, m)[0]
        assert np.array_equal(vol3, vol2) and (d3[:, 2] == 0).all(), m


@spawned
def test_shapes_that_fill_nothing():
    z = np.load(GOLD)
    rng = np.random.default_rng(5)
    cases = []
    for B, V, C, H, W, X, Y, Z in ((1, 1, 1, 4, 4, 2, 2, 2), (3, 2, 33, 12, 10, 65, 1, 1), (1, 4, 5, 96, 72, 4, 4, 4)):
        proj, coord = _rig(B, V, H, W, (X, Y, Z), rng)
        cases.append((rng.normal(0, 1, (B, V, C, H, W)).astype(np.float32), proj, coord,
                      rng.uniform(0.2, 1.0, (B, V, C)).astype(np.float32),
                      rng.normal(0, 1, (B, C, X, Y, Z)).astype(np.float32)))
    # eight views: the fixture's three cameras repeated, so that copies of a view must get the same gradient bits
    v8 = np.arange(8) % 3
    cases.append((z['un_feat'][:1, v8, :2], z['un_proj'][:1, v8], z['un_coord'][:1], z['un_conf'][:1, v8, :2],
                  z['un_gV'][:1, :2]))
    # the backward keeps 1..4 planes per workgroup, fewer while under 512 workgroups would result: every shape above
    # runs with one. (8, 8, 33, 12, 10): 8 * 8 * ceil(33 / 4) = 576 workgroups of 4 planes, the last of each (b, v) with
    # one channel; (8, 8, 24, 64, 64): 8 * 8 * ceil(24 / 3) = 512 workgroups of 3 planes = 96 KB of dynamic LDS
    for (B, V, C, H, W, X, Y, Z), planes in (((8, 8, 33, 12, 10, 4, 4, 4), 4), ((8, 8, 24, 64, 64, 4, 4, 4), 3)):
        assert _bwd_planes(B, V, C, H, W) == planes
        proj, coord = _rig(B, V, H, W, (X, Y, Z), rng)
        cases.append((rng.normal(0, 1, (B, V, C, H, W)).astype(np.float32), proj, coord,
                      rng.uniform(0.2, 1.0, (B, V, C)).astype(np.float32),
                      rng.normal(0, 1, (B, C, X, Y, Z)).astype(np.float32)))
    for feat, proj, coord, conf, gV in cases:
        for m in METHODS:
            vol, dfeat, dconf = _unproject(feat, proj, coord, gV, m, conf)
            if feat.shape[0] == 8:                          # the multi-plane cases: the same bits on a second run
                again = _unproject(feat, proj, coord, gV, m, conf)
                assert np.array_equal(vol, again[0]) and np.array_equal(dfeat, again[1]), (feat.shape, m)
                assert dconf is None or np.array_equal(dconf, again[2])
            rv = R.unproject(feat, proj, coord, m, conf)
            rd, rc = R.unproject_bwd(feat, proj, coord, gV, m, conf)
            ev, ed = _err(vol, rv), _err(dfeat, rd)
            print(feat.shape, coord.shape[1:4], m, 'forward {:.2e} dfeatures {:.2e}'.format(ev, ed))
            assert ev <= TOL and ed <= TOL, (feat.shape, m, ev, ed)
            if m == 'conf':
                assert _err(dconf, rc) <= TOL
            if feat.shape[:3] == (1, 8, 2) and m in ('sum', 'softmax'):    # the repeated cameras
                assert np.array_equal(dfeat[:, 0], dfeat[:, 3]) and np.array_equal(dfeat[:, 0], dfeat[:, 6])
                assert np.array_equal(dfeat[:, 1], dfeat[:, 4]) and np.array_equal(dfeat[:, 2], dfeat[:, 5])
    # more views than the kernels serve is an error of the library, not a fall-back
    from hipnet import _capi as C
    t = torch.zeros(16, device='cuda')
    with pytest.raises(RuntimeError, match=r'V = 9 views \(1\.\.8\)'):
        C.call('hrnet_unproject_volume', t.data_ptr(), t.data_ptr(), t.data_ptr(), None, t.data_ptr(), 0, 1, 9, 1, 4,
               4, 2, 2, 2, C.stream_ptr())
    with pytest.raises(RuntimeError, match='H \\* W = 16900 pixels'):
        C.call('hrnet_unproject_volume_bwd', t.data_ptr(), t.data_ptr(), t.data_ptr(), None, t.data_ptr(),
               t.data_ptr(), None, 0, 1, 1, 1, 130, 130, 2, 2, 2, C.stream_ptr())


def _real_volume(rng):
    """(1, 4, 8, 64, 64) maps into 64^3 voxels of a 500 mm cuboid, four cameras that see the whole box. Each channel
    has one view that dominates the softmax (offset 2), so that the gradient of that view is of the size of S."""
    from utils.volumetric import build_coord_volumes
    B, V, C, H, W, S = 1, 4, 8, 64, 64, 64
    coord = build_coord_volumes(torch.tensor([[20.0, -10.0, 30.0]]), 500.0, S).numpy()
    proj = R.ring_cameras(V, 1500.0, 100.0, (32.0, 32.0), target=(20.0, -10.0, 30.0))[None].astype(np.float32)
    feat = rng.normal(0, 0.5, (B, V, C, H, W))
    for c in range(C):
        feat[:, c % V, c] += 2.0
    gV = rng.uniform(0.5, 1.5, (B, C, S, S, S)).astype(np.float32)
    return feat.astype(np.float32), proj, coord, gV


@spawned
def test_one_real_volume():
    feat, proj, coord, gV = _real_volume(np.random.default_rng(11))
    rv = R.unproject(feat, proj, coord, 'softmax')
    rd, _ = R.unproject_bwd(feat, proj, coord, gV, 'softmax')
    S = R.scatter_bound(feat.shape, proj, coord, gV)
    print('real volume: S.max / max|dfeatures| = {:.2f}'.format(S.max() / np.abs(rd).max()))
    assert S.max() <= 2.0 * np.abs(rd).max()
    assert (rd != 0).mean() > 0.3                           # the cameras see the box: a good part of every map is reached
    vol, dfeat, _ = _unproject(feat, proj, coord, gV, 'softmax')
    ev, ed = _err(vol, rv), _err(dfeat, rd)
    print('real volume: forward {:.2e} dfeatures {:.2e}'.format(ev, ed))
    assert ev <= TOL and ed <= TOL, (ev, ed)


@spawned
def test_reproducible_bits():
    from utils.volumetric import unproject_heatmaps
    z = np.load(GOLD)
    small = tuple(z['un_' + k] for k in ('feat', 'proj', 'coord', 'gV'))
    for feat, proj, coord, gV in (small, _real_volume(np.random.default_rng(11))):
        v1, d1, _ = _unproject(feat, proj, coord, gV, 'softmax')
        v2, d2, _ = _unproject(feat, proj, coord, gV, 'softmax')
        assert np.array_equal(v1, v2) and np.array_equal(d1, d2), feat.shape
        with torch.no_grad():
            plain = unproject_heatmaps(_dev(feat).requires_grad_(True), _dev(proj), _dev(coord), 'softmax')
        assert not plain.requires_grad and np.array_equal(plain.cpu().numpy(), v1)
    # forward + backward captured into a graph and replayed: the eager bits - on the fixture and on 64 x 64 maps with
    # three planes per workgroup (96 KB of dynamic LDS inside the capture)
    rng = np.random.default_rng(17)
    proj, coord = _rig(8, 8, 64, 64, (4, 4, 4), rng)
    assert _bwd_planes(8, 8, 24, 64, 64) == 3
    big = (rng.normal(0, 1, (8, 8, 24, 64, 64)).astype(np.float32), proj, coord,
           rng.normal(0, 1, (8, 24, 4, 4, 4)).astype(np.float32))
    for feat, proj, coord, gV in (small, big):
        v1, d1, _ = _unproject(feat, proj, coord, gV, 'softmax')
        f, P, cv, g = _dev(feat).requires_grad_(True), _dev(proj), _dev(coord), _dev(gV)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):                              # warm-up outside the capture
                torch.autograd.grad(unproject_heatmaps(f, P, cv, 'softmax'), f, g)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            vol = unproject_heatmaps(f, P, cv, 'softmax')
            df, = torch.autograd.grad(vol, f, g)
        vol.zero_()
        df.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(vol.detach().cpu().numpy(), v1) and np.array_equal(df.cpu().numpy(), d1), feat.shape


def _integrate(vols, coord, gK, gP, softmax, mult):
    from utils.volumetric import integrate_tensor_3d_with_coordinates
    v = _dev(vols).requires_grad_(True)
    kp, p = integrate_tensor_3d_with_coordinates(v, _dev(coord), softmax=softmax, multiplier=mult)
    assert kp.requires_grad and p.requires_grad and kp.dtype == p.dtype == torch.float32
    torch.autograd.backward([kp, p], [_dev(gK), _dev(gP)])
    torch.cuda.synchronize()
    return kp.detach().cpu().numpy(), p.detach().cpu().numpy(), v.grad.cpu().numpy()


def _check_integrate(got, ref, coord, what):
    """key points: 1e-6 of max|coord| - for the relu mode, which does not normalise, of the largest key point when that
    is larger (an f32 result rounds at 6e-8 of ITSELF, and a sum of relu masses is not bounded by the coordinates; under
    softmax the key points are convex combinations and the scale is max|coord|); p: 1e-6 of each map's largest p;
    dvols: 1e-5 of the largest dvols. Achieved on one MI355X: key points <= 4.9e-8, p <= 4.8e-8, dvols <= 5.4e-8"""
    (kp, p, dv), (rk, rp, rd) = got, ref
    B, J = rp.shape[:2]
    scale = max(np.abs(coord).max(), np.abs(rk).max())
    ek = np.abs(kp - rk).max() / scale
    pmax = np.abs(rp).reshape(B, J, -1).max(-1)
    ep = (np.abs(p - rp).reshape(B, J, -1).max(-1) / np.where(pmax > 0, pmax, 1.0)).max()
    ed = np.abs(dv - rd).max() / max(np.abs(rd).max(), 1e-300)
    print(what, 'keypoints {:.2e} p {:.2e} dvols {:.2e}'.format(ek, ep, ed))
    assert ek <= 1e-6 and ep <= 1e-6 and ed <= 1e-5, (what, ek, ep, ed)


@spawned
def test_integration():
    z = np.load(GOLD)
    vols, coord, gK, gP = z['in_vols'], z['un_coord'], z['in_gK'], z['in_gP']
    for mode, softmax in (('s', True), ('r', False)):
        for mult in (1, 200):
            key = 'in_{}{}_'.format(mode, mult)
            got = _integrate(vols, coord, gK, gP, softmax, float(mult))
            if key + 'p' in z.files:
                ref = (z[key + 'kp'], z[key + 'p'], z[key + 'dvols'])
            else:
                ref = (z[key + 'kp'],) + (R.integrate(vols, coord, softmax, float(mult))[1],
                                          R.integrate_bwd(vols, coord, gK, gP, softmax, float(mult)))
            _check_integrate(got, ref, coord, key)
            again = _integrate(vols, coord, gK, gP, softmax, float(mult))
            assert all(np.array_equal(a, b) for a, b in zip(got, again)), key
            if softmax:
                assert np.abs(got[1].astype(np.float64).reshape(2, 3, -1).sum(-1) - 1.0).max() <= 1e-6
            else:                                           # the all-negative map: exact zeros
                assert (got[0][1, 2] == 0).all() and (got[1][1, 2] == 0).all() and (got[2][1, 2] == 0).all()
    rng = np.random.default_rng(3)
    for B, J, X, Y, Zs in ((1, 1, 1, 1, 1), (1, 21, 64, 64, 64)):
        v = rng.uniform(-1, 1, (B, J, X, Y, Zs)).astype(np.float32)
        cv = (rng.uniform(-250, 250, (B, X, Y, Zs, 3)) + 600.0).astype(np.float32)
        k, g = rng.normal(0, 1, (B, J, 3)).astype(np.float32), rng.normal(0, 1, v.shape).astype(np.float32)
        for softmax, mult in ((True, 50.0), (False, 1.0)):
            got = _integrate(v, cv, k, g, softmax, mult)
            ref = R.integrate(v, cv, softmax, mult) + (R.integrate_bwd(v, cv, k, g, softmax, mult),)
            _check_integrate(got, ref, cv, (B, J, X, Y, Zs, softmax))
            if softmax:
                assert np.abs(got[1].astype(np.float64).reshape(B, J, -1).sum(-1) - 1.0).max() <= 1e-6
    # only one of the two outputs used: the other's gradient is taken as zero
    from utils.volumetric import integrate_tensor_3d_with_coordinates
    v = _dev(vols).requires_grad_(True)
    kp, _ = integrate_tensor_3d_with_coordinates(v, _dev(coord), multiplier=3.0)
    kp.backward(_dev(gK))
    assert _err(v.grad.cpu().numpy(), R.integrate_bwd(vols, coord, gK, None, True, 3.0)) <= 1e-5


@spawned
def test_cross_entropy():
    from core.loss import VolumetricCELoss
    z = np.load(GOLD)
    p_np = z['in_s1_p'].astype(np.float32)
    p = _dev(p_np).requires_grad_(True)
    crit = VolumetricCELoss()
    loss, idx = crit.loss_and_indices(_dev(z['un_coord']), p, _dev(z['ce_gt']), _dev(z['ce_validity']))  # B x J x 1
    assert loss.dim() == 0 and loss.dtype == torch.float32 and not idx.requires_grad
    assert idx.dtype == torch.int32 and (idx.cpu().numpy() == z['ce_idx']).all()
    assert crit(_dev(z['un_coord']), p, _dev(z['ce_gt']), _dev(z['ce_validity'])).item() == loss.item()
    el = abs(loss.item() - z['ce_loss']) / abs(z['ce_loss'])
    loss.backward()
    dp = p.grad.cpu().numpy().astype(np.float64)
    B, J = dp.shape[:2]
    valid = z['ce_validity'].reshape(B, J) != 0
    want = {(b, j, int(z['ce_idx'][b, j])) for b in range(B) for j in range(J) if valid[b, j]}
    assert set(zip(*[a.tolist() for a in np.nonzero(dp.reshape(B, J, -1))])) == want
    nz = z['ce_dp'] != 0
    ed = (np.abs(dp[nz] - z['ce_dp'][nz]) / np.abs(z['ce_dp'][nz])).max()
    print('cross-entropy: loss {:.2e} dp {:.2e}'.format(el, ed))
    assert el <= 1e-6 and ed <= 1e-6
    # an upstream factor scales dp; B x J validity is taken too
    p2 = _dev(p_np).requires_grad_(True)
    (0.25 * crit(_dev(z['un_coord']), p2, _dev(z['ce_gt']), _dev(z['ce_validity'].reshape(B, J)))).backward()
    assert np.abs(p2.grad.cpu().numpy() - 0.25 * dp).max() <= 1e-6 * np.abs(dp).max()


@spawned
def test_the_chain_the_model_will_run():
    """unproject -> integrate -> Joints3DMSELoss + 0.01 VolumetricCELoss -> backward, against the same chain through
    the restatement in float64"""
    from core.loss import Joints3DMSELoss, VolumetricCELoss
    from utils.volumetric import integrate_tensor_3d_with_coordinates, unproject_heatmaps
    z = np.load(GOLD)
    feat, proj, coord, gt, validity = z['un_feat'], z['un_proj'], z['un_coord'], z['ce_gt'], z['ce_validity']
    mult = 4.0
    f = _dev(feat).requires_grad_(True)
    cv = _dev(coord)
    vol = unproject_heatmaps(f, _dev(proj), cv, 'softmax')
    kp, p = integrate_tensor_3d_with_coordinates(vol, cv, softmax=True, multiplier=mult)
    loss = Joints3DMSELoss()(kp, _dev(gt)) + 0.01 * VolumetricCELoss()(cv, p, _dev(gt), _dev(validity))
    loss.backward()
    torch.cuda.synchronize()
    rvol = R.unproject(feat, proj, coord, 'softmax')
    rkp, rp = R.integrate(rvol, coord, True, mult)
    l3d, gK = R.joints3d_loss(rkp, gt.astype(np.float64))
    lce, _, dp = R.ce_loss(coord, rp, gt, validity)
    dvol = R.integrate_bwd(rvol, coord, gK, 0.01 * dp, True, mult)
    rd, _ = R.unproject_bwd(feat, proj, coord, dvol, 'softmax')
    el = abs(loss.item() - (l3d + 0.01 * lce)) / abs(l3d + 0.01 * lce)
    ed = _err(f.grad.cpu().numpy(), rd)
    print('chain: loss {:.2e} dfeatures {:.2e}'.format(el, ed))
    assert el <= 1e-6 and ed <= TOL, (el, ed)
