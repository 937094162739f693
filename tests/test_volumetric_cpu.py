"""The volumetric lifting operations without a device: the float64 restatement tests/volumetric_ref.py reproduces every
array of the reference's own float64 run (tests/golden/volumetric.npz, written by make_golden_volumetric.py) to 1e-12
relative; the coordinate-volume plumbing of utils/volumetric.py against the reference's two functions and a literal
transcription of the grid rule; the C ABI's six new entries; the argument errors, raised before any device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import volumetric_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'volumetric.npz')
RTOL = 1e-12
METHODS = ('sum', 'max', 'softmax', 'conf')
NEW = ('hrnet_unproject_volume', 'hrnet_unproject_volume_bwd', 'hrnet_volume_integrate', 'hrnet_volume_integrate_bwd',
       'hrnet_volumetric_ce_loss', 'hrnet_volumetric_ce_loss_bwd')


def _err(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


@pytest.fixture(scope='module')
def z():
    return np.load(GOLD)


@pytest.mark.parametrize('method', METHODS)
def test_restatement_reproduces_the_unprojection(z, method):
    feat, proj, coord, conf, gV = (z['un_' + k] for k in ('feat', 'proj', 'coord', 'conf', 'gV'))
    assert feat.dtype == proj.dtype == coord.dtype == gV.dtype == np.float32
    vol = R.unproject(feat, proj, coord, method, conf)
    assert vol.shape == (2, 3, 8, 6, 5)
    assert _err(vol, z['un_vol_' + method]) <= RTOL
    dfeat, dconf = R.unproject_bwd(feat, proj, coord, gV, method, conf)
    assert _err(dfeat, z['un_dfeat_' + method]) <= RTOL
    if method == 'conf':
        assert _err(dconf, z['un_dconf_conf']) <= RTOL
    # both zero-padding sides are hit, and some pixels are never reached
    assert (z['un_dfeat_' + method] == 0).any() and (z['un_dfeat_' + method] != 0).any()


def test_a_view_that_looks_away_contributes_exact_zeros(z):
    feat, coord, gV = z['un_feat'], z['un_coord'], z['un_gV']
    dfeat, _ = R.unproject_bwd(feat, z['un_proj_away'], coord, gV, 'softmax')
    assert _err(dfeat[0], z['un_away_dfeat_softmax']) <= RTOL
    assert (dfeat[:, 2] == 0).all() and (z['un_away_dfeat_softmax'][2] == 0).all()
    assert (dfeat[:, :2] != 0).any()
    # the softmax still counts the view's zeros: the volume differs from the two-view one
    two = R.unproject(feat[:, :2], z['un_proj_away'][:, :2], coord, 'softmax')
    assert not np.allclose(R.unproject(feat, z['un_proj_away'], coord, 'softmax'), two)


def test_scatter_bound_holds_on_the_fixture(z):
    S = R.scatter_bound(z['un_feat'].shape, z['un_proj'], z['un_coord'], z['un_gV'])
    for m in METHODS:
        assert S.max() <= 2.0 * np.abs(z['un_dfeat_' + m]).max(), m


@pytest.mark.parametrize('mode,mult', [('s', 1), ('s', 200), ('r', 1), ('r', 200)])
def test_restatement_reproduces_the_integration(z, mode, mult):
    vols, coord, gK, gP = z['in_vols'], z['un_coord'], z['in_gK'], z['in_gP']
    key = 'in_{}{}_'.format(mode, mult)
    kp, p = R.integrate(vols, coord, mode == 's', float(mult))
    assert _err(kp, z[key + 'kp']) <= RTOL
    if key + 'p' in z.files:
        assert _err(p, z[key + 'p']) <= RTOL
        assert _err(R.integrate_bwd(vols, coord, gK, gP, mode == 's', float(mult)), z[key + 'dvols']) <= RTOL
    if mode == 's':
        assert np.allclose(p.reshape(2, 3, -1).sum(-1), 1.0, rtol=0, atol=1e-12)
    else:
        assert (vols[1, 2] < 0).all() and (kp[1, 2] == 0).all() and (p[1, 2] == 0).all()
        assert (R.integrate_bwd(vols, coord, gK, gP, False, float(mult))[1, 2] == 0).all()


def test_multiplier_200_needs_the_max_subtraction(z):
    with np.errstate(over='ignore'):
        assert np.isinf(np.exp(np.float32(200.0) * z['in_vols'].max()))       # f32 exp of the raw logit overflows
    assert np.isfinite(z['in_s200_p']).all() and z['in_s200_p'].max() > 0.5


def test_restatement_reproduces_the_cross_entropy(z):
    p = z['in_s1_p'].astype(np.float32)
    loss, idx, dp = R.ce_loss(z['un_coord'], p, z['ce_gt'], z['ce_validity'])
    assert (idx == z['ce_idx']).all()
    assert abs(loss - z['ce_loss']) <= RTOL * abs(z['ce_loss'])
    assert _err(dp, z['ce_dp']) <= RTOL
    valid = z['ce_validity'].reshape(2, 3) != 0
    assert (0 < valid.sum() < 6) and ((dp.reshape(2, 3, -1) != 0).sum(-1) == valid).all()


def test_rotation_matrix_and_rotated_volume(z):
    from utils.volumetric import get_rotation_matrix, rotate_coord_volume
    for axis, theta, ref in zip(z['rot_axis'], z['rot_theta'], z['rot_matrix']):
        got = get_rotation_matrix(axis, theta)
        assert got.shape == (3, 3) and got.dtype == np.float64
        assert np.abs(got - ref).max() <= 1e-15
        assert np.abs(got @ got.T - np.eye(3)).max() <= 1e-15
    assert np.array_equal(get_rotation_matrix([0, 1, 0], 0.0), np.eye(3))
    out = rotate_coord_volume(torch.from_numpy(z['rot_in']), z['rot_theta'][1], z['rot_axis'][1])
    assert out.dtype == torch.float32 and tuple(out.shape) == z['rot_in'].shape
    # float32 products of values ~1e2 summed three at a time: 4 roundings of 6e-8 each
    assert np.abs(out.numpy() - z['rot_out']).max() <= 4 * 6e-8 * np.abs(z['rot_in']).max()


def test_build_coord_volumes_follows_the_grid_rule():
    from utils.volumetric import build_coord_volumes, get_rotation_matrix
    base = torch.tensor([[10.0, -20.0, 700.0], [-3.5, 4.25, 655.0]])
    S, side = 5, 200.0
    cv = build_coord_volumes(base, side, S)
    assert tuple(cv.shape) == (2, S, S, S, 3) and cv.dtype == torch.float32 and cv.is_contiguous()
    # a literal transcription of the rule: position = base - side / 2, voxel (i, j, k) at position + side / (S - 1) * (i, j, k)
    for b in range(2):
        position = base[b] - torch.full((3,), side) / 2
        for i, j, k in ((0, 0, 0), (4, 4, 4), (1, 3, 2), (4, 0, 2)):
            want = position + (torch.full((3,), side) / (S - 1)) * torch.tensor([i, j, k], dtype=torch.float32)
            assert torch.equal(cv[b, i, j, k], want), (b, i, j, k)
        assert torch.equal(cv[b, 0, 0, 0], base[b] - side / 2) and torch.equal(cv[b, -1, -1, -1], base[b] + side / 2)
    assert torch.equal(build_coord_volumes(base, side, S, theta=0.0), cv)          # theta = 0 is the identity
    # rotation about the base point: the centre voxel stays, every distance to the base point stays
    theta = 1.1
    rot = build_coord_volumes(base, side, S, theta=theta)
    for b in range(2):
        assert torch.allclose(rot[b, 2, 2, 2], base[b], rtol=0, atol=1e-4)
        want = (cv[b].double() - base[b].double()) @ torch.from_numpy(get_rotation_matrix([0, 1, 0], theta)).t() \
            + base[b].double()
        assert (rot[b].double() - want).abs().max() <= 4 * 6e-8 * 700.0
    assert torch.equal(rot[..., 1], cv[..., 1])                                   # the y axis is the rotation axis
    per_sample = build_coord_volumes(base, side, S, theta=[0.0, theta])
    assert torch.equal(per_sample[0], cv[0]) and torch.equal(per_sample[1], rot[1])


def test_c_abi_entry_points():
    from hipnet import _capi
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'hrnet_hip.h')).read()
    handle = _capi.lib()                                   # loads without a GPU; nothing is launched
    for name in NEW:
        assert re.search(r'^int {}\('.format(name), header, re.M), name
        assert name in _capi.EXPORTED and hasattr(handle, name), name
        assert _capi._SIGS[name][-1] == ctypes.c_void_p
    # the swapped divisors of the sample position are stated as the reference's rule
    assert "REFERENCE'S rule, not a pixel-exact one" in ' '.join(header.replace('\n *', ' ').split())
    assert _capi.ABI_VERSION == 2 and handle.hrnet_abi_version() == 2   # entries were added, nothing existing changed


def test_argument_errors_need_no_device():
    from core.loss import VolumetricCELoss
    from utils.volumetric import integrate_tensor_3d_with_coordinates, unproject_heatmaps
    feat, proj, coord = torch.zeros(1, 2, 3, 4, 5), torch.zeros(1, 2, 3, 4), torch.zeros(1, 2, 2, 2, 3)
    with pytest.raises(ValueError, match='Unknown volume_aggregation_method: mean'):
        unproject_heatmaps(feat, proj, coord, 'mean')
    with pytest.raises(ValueError, match='needs vol_confidences'):
        unproject_heatmaps(feat, proj, coord, 'conf_norm')
    with pytest.raises(ValueError, match='proj_matricies requires a gradient.*constants'):
        unproject_heatmaps(feat, proj.clone().requires_grad_(True), coord)
    with pytest.raises(ValueError, match='coord_volumes requires a gradient.*constants'):
        unproject_heatmaps(feat, proj, coord.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='coord_volumes requires a gradient'):
        integrate_tensor_3d_with_coordinates(torch.zeros(1, 3, 2, 2, 2), coord.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='proj_matricies: expected'):
        unproject_heatmaps(feat, proj[:, :1], coord)
    with pytest.raises(ValueError, match='views'):
        unproject_heatmaps(torch.zeros(1, 9, 3, 4, 5), torch.zeros(1, 9, 3, 4), coord)
    with pytest.raises(ValueError, match='coord_volumes: expected'):
        integrate_tensor_3d_with_coordinates(torch.zeros(1, 3, 2, 2, 4), coord)
    # well-formed host tensors: refused, not computed on the CPU
    with pytest.raises(RuntimeError, match='no CPU path'):
        unproject_heatmaps(feat, proj, coord)
    with pytest.raises(RuntimeError, match='no CPU path'):
        integrate_tensor_3d_with_coordinates(torch.zeros(1, 3, 2, 2, 2), coord)
    with pytest.raises(RuntimeError, match='no CPU path'):
        VolumetricCELoss()(coord, torch.zeros(1, 3, 2, 2, 2), torch.zeros(1, 3, 3), torch.ones(1, 3, 1))
