"""Volumetric lifting (reference lib/models/triangulation_model_utils/op.py:84-168 and volumetric.py:87-114, the
coordinate volumes of lib/models/triangulation.py:406-456) on the HIP kernels of csrc/volumetric.hip, with the
reference's names and argument orders.

unproject_heatmaps           every view's feature maps sampled at the projections of a world-space voxel grid and
                             aggregated over the views ('sum', 'max', 'softmax', 'conf*'): ONE hrnet_unproject_volume
                             launch for any batch and any number of views (the reference loops over both in Python);
                             backward is one hrnet_unproject_volume_bwd launch that recomputes positions and samples
                             and is bit-reproducible run to run.
integrate_tensor_3d_with_coordinates
                             softmax (or relu) over each volume and its expectation under the coordinate volume; the
                             model's `volumes * VOLUME_MULTIPLIER` is the `multiplier` argument, folded into the kernel.
                             Both outputs are differentiable.
get_rotation_matrix, rotate_coord_volume, build_coord_volumes
                             plumbing in torch, no kernel.

Deviation from the reference: proj_matricies and coord_volumes are constants. The reference's autograd would reach
them (the cuboid centre, say) through grid_sample's grid gradient; here a tensor of either kind that requires a
gradient is refused with a ValueError instead of being silently detached. The sample position keeps the reference's
normalisation as written, swapped divisors included (see include/hrnet_hip.h, hrnet_unproject_volume).

Inputs must be HIP-device tensors (no CPU path); other dtypes and non-contiguous tensors are converted."""
import numpy as np
import torch

from core.loss import _dev_f32
from hipnet import _capi as C

METHODS = {'sum': C.VALUES['HR_VOL_SUM'], 'max': C.VALUES['HR_VOL_MAX'], 'softmax': C.VALUES['HR_VOL_SOFTMAX']}
CONF = C.VALUES['HR_VOL_CONF']                       # any name beginning with 'conf'
MAX_VIEWS = 8
SPLIT = C.VALUES['HR_VOLUME_SPLIT']


def _method_id(volume_aggregation_method, vol_confidences):
    if not isinstance(volume_aggregation_method, str):
        raise ValueError('Unknown volume_aggregation_method: {}'.format(volume_aggregation_method))
    if volume_aggregation_method.startswith('conf'):
        if vol_confidences is None:
            raise ValueError("volume_aggregation_method '{}' needs vol_confidences".format(volume_aggregation_method))
        return CONF
    if volume_aggregation_method not in METHODS:
        raise ValueError('Unknown volume_aggregation_method: {}'.format(volume_aggregation_method))
    return METHODS[volume_aggregation_method]


def _constant(t, name, what):
    if t.requires_grad:
        raise ValueError('{}: {} requires a gradient, but projection matrices and coordinate volumes are constants '
                         'here (the reference would differentiate grid_sample\'s grid; this build does not) - '
                         'detach it'.format(what, name))


class _UnprojectFn(torch.autograd.Function):
    """volumes of hrnet_unproject_volume; backward: hrnet_unproject_volume_bwd on the saved inputs"""

    @staticmethod
    def forward(ctx, feat, conf, proj, coord, method):
        vol = _unproject(feat, conf, proj, coord, method)
        ctx.save_for_backward(feat, conf, proj, coord)
        ctx.method = method
        return vol

    @staticmethod
    def backward(ctx, gV):
        feat, conf, proj, coord = ctx.saved_tensors
        B, V, Cn, H, W = feat.shape
        X, Y, Z = coord.shape[1:4]
        gV = gV.contiguous().float()
        dfeat = torch.empty_like(feat)
        dconf = torch.empty_like(conf) if ctx.method == CONF and ctx.needs_input_grad[1] else None
        C.call('hrnet_unproject_volume_bwd', feat.data_ptr(), proj.data_ptr(), coord.data_ptr(), C.ptr(conf),
               gV.data_ptr(), dfeat.data_ptr(), C.ptr(dconf), ctx.method, B, V, Cn, H, W, X, Y, Z, C.stream_ptr())
        return dfeat, dconf, None, None, None


def _unproject(feat, conf, proj, coord, method):
    B, V, Cn, H, W = feat.shape
    X, Y, Z = coord.shape[1:4]
    vol = torch.empty((B, Cn, X, Y, Z), dtype=torch.float32, device=feat.device)
    C.call('hrnet_unproject_volume', feat.data_ptr(), proj.data_ptr(), coord.data_ptr(), C.ptr(conf), vol.data_ptr(),
           method, B, V, Cn, H, W, X, Y, Z, C.stream_ptr())
    return vol


def unproject_heatmaps(heatmaps, proj_matricies, coord_volumes, volume_aggregation_method='sum', vol_confidences=None):
    """heatmaps (B, V, C, H, W), proj_matricies (B, V, 3, 4), coord_volumes (B, X, Y, Z, 3), vol_confidences (B, V, C)
    for the 'conf*' methods -> volumes (B, C, X, Y, Z) float32. Differentiable in heatmaps and vol_confidences."""
    method = _method_id(volume_aggregation_method, vol_confidences)
    if heatmaps.ndim != 5:
        raise ValueError('heatmaps: expected (B, V, C, H, W), got {}'.format(tuple(heatmaps.shape)))
    B, V, Cn = heatmaps.shape[:3]
    if tuple(proj_matricies.shape) != (B, V, 3, 4):
        raise ValueError('proj_matricies: expected {}, got {}'.format((B, V, 3, 4), tuple(proj_matricies.shape)))
    if coord_volumes.ndim != 5 or coord_volumes.shape[0] != B or coord_volumes.shape[4] != 3:
        raise ValueError('coord_volumes: expected ({}, X, Y, Z, 3), got {}'.format(B, tuple(coord_volumes.shape)))
    if method == CONF and tuple(vol_confidences.shape) != (B, V, Cn):
        raise ValueError('vol_confidences: expected {}, got {}'.format((B, V, Cn), tuple(vol_confidences.shape)))
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError('heatmaps: {} views (1..{})'.format(V, MAX_VIEWS))
    _constant(proj_matricies, 'proj_matricies', 'unproject_heatmaps')
    _constant(coord_volumes, 'coord_volumes', 'unproject_heatmaps')
    conf_in = vol_confidences if method == CONF else None
    feat = _dev_f32(heatmaps, 'unproject_heatmaps')
    proj = _dev_f32(proj_matricies, 'unproject_heatmaps')
    coord = _dev_f32(coord_volumes, 'unproject_heatmaps')
    conf = None if conf_in is None else _dev_f32(conf_in, 'unproject_heatmaps')
    if torch.is_grad_enabled() and (feat.requires_grad or (conf is not None and conf.requires_grad)):
        return _UnprojectFn.apply(feat, conf, proj, coord, method)
    return _unproject(feat.detach(), None if conf is None else conf.detach(), proj, coord, method)


class _IntegrateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vols, coord, softmax, multiplier):
        kp, p = _integrate(vols, coord, softmax, multiplier)
        ctx.save_for_backward(vols, coord, p)
        ctx.softmax, ctx.multiplier = softmax, multiplier
        ctx.set_materialize_grads(False)         # an unused output's gradient stays None: no zero volume is built
        return kp, p

    @staticmethod
    def backward(ctx, gK, gP):
        vols, coord, p = ctx.saved_tensors
        B, J, X, Y, Z = vols.shape
        gK = torch.zeros((B, J, 3), dtype=torch.float32, device=vols.device) if gK is None else gK.contiguous().float()
        gP = None if gP is None else gP.contiguous().float()
        dvols = torch.empty_like(vols)
        work = torch.empty(B * J * SPLIT * 5, dtype=torch.float64, device=vols.device)
        C.call('hrnet_volume_integrate_bwd', vols.data_ptr(), p.data_ptr(), coord.data_ptr(), gK.data_ptr(), C.ptr(gP),
               ctx.multiplier, int(ctx.softmax), dvols.data_ptr(), work.data_ptr(), B, J, X, Y, Z, C.stream_ptr())
        return dvols, None, None, None


def _integrate(vols, coord, softmax, multiplier):
    B, J, X, Y, Z = vols.shape
    kp = torch.empty((B, J, 3), dtype=torch.float32, device=vols.device)
    p = torch.empty_like(vols)
    work = torch.empty(B * J * SPLIT * 5, dtype=torch.float64, device=vols.device)
    C.call('hrnet_volume_integrate', vols.data_ptr(), coord.data_ptr(), multiplier, int(softmax), kp.data_ptr(),
           p.data_ptr(), work.data_ptr(), B, J, X, Y, Z, C.stream_ptr())
    return kp, p


def integrate_tensor_3d_with_coordinates(volumes, coord_volumes, softmax=True, multiplier=1.0):
    """volumes (B, J, X, Y, Z), coord_volumes (B, X, Y, Z, 3) -> (coordinates (B, J, 3), volumes (B, J, X, Y, Z)):
    p = softmax(multiplier * volumes) over each map (softmax=False: relu(multiplier * volumes), not normalised) and its
    expectation sum p * coord. multiplier is a Python number (the model's VOLUME_MULTIPLIER)."""
    if volumes.ndim != 5:
        raise ValueError('volumes: expected (B, J, X, Y, Z), got {}'.format(tuple(volumes.shape)))
    if tuple(coord_volumes.shape) != (volumes.shape[0],) + tuple(volumes.shape[2:]) + (3,):
        raise ValueError('coord_volumes: expected {}, got {}'.format(
            (volumes.shape[0],) + tuple(volumes.shape[2:]) + (3,), tuple(coord_volumes.shape)))
    _constant(coord_volumes, 'coord_volumes', 'integrate_tensor_3d_with_coordinates')
    multiplier = float(multiplier)
    vols = _dev_f32(volumes, 'integrate_tensor_3d_with_coordinates')
    coord = _dev_f32(coord_volumes, 'integrate_tensor_3d_with_coordinates')
    if torch.is_grad_enabled() and vols.requires_grad:
        return _IntegrateFn.apply(vols, coord, bool(softmax), multiplier)
    return _integrate(vols.detach(), coord, bool(softmax), multiplier)


def get_rotation_matrix(axis, theta):
    """3 x 3 float64 numpy matrix of the reference's get_rotation_matrix (volumetric.py:87-99): with k the unit axis,
    Rodrigues' formula cos(theta) I + sin(theta) [k]x + (1 - cos(theta)) k k^T, the counterclockwise rotation by theta."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.sqrt(np.dot(k, k))
    cross = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(theta) * np.eye(3) + np.sin(theta) * cross + (1.0 - np.cos(theta)) * np.outer(k, k)


def rotate_coord_volume(coord_volume, theta, axis):
    """coord_volume (..., 3) rotated about the origin by the float32 matrix of get_rotation_matrix(axis, theta)"""
    rot = torch.from_numpy(get_rotation_matrix(axis, theta)).to(coord_volume.device, torch.float32)
    return (coord_volume.reshape(-1, 3) @ rot.t()).reshape(coord_volume.shape)


def build_coord_volumes(base_points, cuboid_side, volume_size, theta=0.0, axis=(0, 1, 0)):
    """base_points (B, 3) -> (B, S, S, S, 3) float32 on base_points' device (reference triangulation.py:406-456): voxel
    (i, j, k) of sample b sits at base_points[b] - cuboid_side / 2 + cuboid_side / (S - 1) * (i, j, k), rotated by
    theta about `axis` through the base point. theta: one angle for the batch or one per sample."""
    if base_points.ndim != 2 or base_points.shape[1] != 3:
        raise ValueError('base_points: expected (B, 3), got {}'.format(tuple(base_points.shape)))
    S = int(volume_size)
    if S < 2:
        raise ValueError('volume_size = {} (two or more voxels a side)'.format(volume_size))
    base = base_points.detach().to(torch.float32)
    dev = base.device
    B = base.shape[0]
    sides = torch.full((3,), float(cuboid_side), dtype=torch.float32, device=dev)
    position = base - sides / 2                                              # (B, 3)
    r = torch.arange(S, device=dev)
    grid = torch.stack(torch.meshgrid(r, r, r, indexing='ij'), dim=-1).to(torch.float32)   # (S, S, S, 3)
    coord = position[:, None, None, None, :] + (sides / (S - 1)) * grid[None]
    centre = base[:, None, None, None, :]
    coord = coord - centre
    thetas = np.broadcast_to(np.asarray(theta, dtype=np.float64).reshape(-1), (B,)) if np.ndim(theta) else None
    if thetas is None:
        coord = rotate_coord_volume(coord, float(theta), axis)
    else:
        coord = torch.stack([rotate_coord_volume(coord[b], float(thetas[b]), axis) for b in range(B)])
    return (coord + centre).contiguous()
