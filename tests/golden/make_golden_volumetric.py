"""Writes tests/golden/volumetric.npz: the reference's own volumetric lifting operations and their autograd in float64
on the CPU, for tests/test_volumetric_cpu.py and tests/test_volumetric_gpu.py.

    python tests/golden/make_golden_volumetric.py <reference checkout>

Imports numpy, torch, tests/volumetric_ref.py (for the camera rig only) and, by path, the reference's
lib/models/triangulation_model_utils package (op.py, volumetric.py) and lib/core/loss.py. img.py and volumetric.py import
cv2, which is not installed: an empty stand-in module sits under sys.modules['cv2'] (nothing of it is called). The
default dtype is float64, because the reference allocates its volumes with the default dtype. Every input is drawn in
float32 and widened, so that a float32 run starts from the same numbers. Only inputs and outputs are stored, no code.

unprojection, (B, V, C, H, W) = (2, 3, 3, 12, 10), (X, Y, Z) = (8, 6, 5), a 100 mm box jittered per sample, three
cameras on a 600 mm ring, focal length 60 px (positions from about -3 to 12 px: both zero-padding sides are hit;
asserted: every depth >= 500, so no voxel sits near the z <= 0 discontinuity):
- un_feat, un_proj, un_coord, un_conf (in [0.2, 1]), un_gV
- un_vol_<m>, un_dfeat_<m> for m in sum, max, softmax, conf; un_dconf_conf
- un_proj_away: the third camera looks away (asserted: every depth of that view < 0, and its reference dfeatures are
  exactly 0); un_away_dfeat_softmax (V, C, H, W): the dfeatures of sample 0
- asserted, not stored: S = the 'sum' dfeatures of |gV| has S.max() <= 2 max |dfeatures| for each method
integrate, vols (2, 3, 8, 6, 5) in +-1 with one all-negative map, on un_coord:
- in_vols, in_gK, in_gP; per mode s (softmax) / r (relu) and multiplier 1 / 200: in_<mode><mult>_kp, _p, _dvols
  (relu at 200: _kp only)
cross-entropy, on un_coord and p = the float32 rounding of in_s1_p:
- ce_gt (voxel centres displaced by 0.3 of the pitch, two joints outside the box; asserted: the runner-up voxel is
  at least 5 % farther), ce_validity (B, J, 1), ce_loss, ce_idx (flat index), ce_dp
coordinate volumes:
- rot_axis (n, 3), rot_theta (n), rot_matrix (n, 3, 3): get_rotation_matrix; rot_in, rot_out: rotate_coord_volume of
  a (2, 3, 2, 3) float32 volume by rot_theta[1] about rot_axis[1]"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import volumetric_ref as R  # noqa: E402


def f32(a):
    return np.asarray(a, dtype=np.float32)


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def main(ref_root):
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    sys.path.insert(0, os.path.join(ref_root, 'lib', 'models'))
    op = importlib.import_module('triangulation_model_utils.op')
    vm = importlib.import_module('triangulation_model_utils.volumetric')
    spec = importlib.util.spec_from_file_location('ref_loss', os.path.join(ref_root, 'lib', 'core', 'loss.py'))
    ref_loss = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_loss)
    torch.set_default_dtype(torch.float64)
    rng = np.random.default_rng(20261021)
    out = {}

    # ---- unprojection
    B, V, C, H, W, X, Y, Z = 2, 3, 3, 12, 10, 8, 6, 5
    feat = f32(rng.normal(0.0, 1.0, (B, V, C, H, W)))
    conf = f32(rng.uniform(0.2, 1.0, (B, V, C)))
    gV = f32(rng.normal(0.0, 1.0, (B, C, X, Y, Z)))
    centres = rng.uniform(-10.0, 10.0, (B, 3))
    axes = [np.linspace(-50.0, 50.0, n) for n in (X, Y, Z)]
    grid = np.stack(np.meshgrid(*axes, indexing='ij'), -1)
    coord = f32(centres[:, None, None, None, :] + grid[None])
    proj = f32(np.stack([R.ring_cameras(V, 600.0, 60.0, (4.5, 4.5)) for _ in range(B)]))
    proj_away = f32(np.stack([R.ring_cameras(V, 600.0, 60.0, (4.5, 4.5), look_away=(2,)) for _ in range(B)]))
    pts = np.concatenate([coord.reshape(B, -1, 3).astype(np.float64), np.ones((B, X * Y * Z, 1))], -1)
    depth = np.einsum('bvj,bnj->bvn', proj[:, :, 2].astype(np.float64), pts)
    assert depth.min() >= 500.0, depth.min()
    pos = np.einsum('bvij,bnj->bvni', proj.astype(np.float64), pts)
    print('projected positions', (pos[..., :2] / pos[..., 2:]).min(), (pos[..., :2] / pos[..., 2:]).max())
    depth_away = np.einsum('bvj,bnj->bvn', proj_away[:, :, 2].astype(np.float64), pts)
    assert depth_away[:, 2].max() < 0.0 and depth_away[:, :2].min() >= 500.0
    out.update(un_feat=feat, un_proj=proj, un_coord=coord, un_conf=conf, un_gV=gV, un_proj_away=proj_away)

    def run(method, P):
        f = t64(feat).requires_grad_(True)
        c = t64(conf).requires_grad_(True)
        vol = op.unproject_heatmaps(f, t64(P), t64(coord), method, c if method == 'conf' else None)
        (vol * t64(gV)).sum().backward()
        return vol.detach().numpy(), f.grad.numpy(), c.grad.numpy() if method == 'conf' else None

    S = R.scatter_bound(feat.shape, proj, coord, gV)
    for m in ('sum', 'max', 'softmax', 'conf'):
        vol, dfeat, dconf = run(m, proj)
        ratio = S.max() / np.abs(dfeat).max()
        print(m, 'S.max / max|dfeatures| = {:.2f}'.format(ratio))
        assert ratio <= 2.0, (m, ratio)
        out['un_vol_' + m], out['un_dfeat_' + m] = vol, dfeat
        if dconf is not None:
            out['un_dconf_conf'] = dconf
    vol, dfeat, _ = run('softmax', proj_away)
    assert np.all(dfeat[:, 2] == 0.0)
    out['un_away_dfeat_softmax'] = dfeat[0]                  # sample 0 only: the file stays under 200 KB

    # ---- integrate
    J = 3
    vols = f32(rng.uniform(-1.0, 1.0, (B, J, X, Y, Z)))
    vols[1, 2] = -np.abs(vols[1, 2]) - f32(0.01)            # an all-negative map
    gK = f32(rng.normal(0.0, 1.0, (B, J, 3)))
    gP = f32(rng.normal(0.0, 1.0, (B, J, X, Y, Z)))
    out.update(in_vols=vols, in_gK=gK, in_gP=gP)
    for mode, softmax in (('s', True), ('r', False)):
        for mult in (1, 200):
            v = t64(vols).requires_grad_(True)
            kp, p = op.integrate_tensor_3d_with_coordinates(v * float(mult), t64(coord), softmax=softmax)
            ((kp * t64(gK)).sum() + (p * t64(gP)).sum()).backward()
            key = 'in_{}{}_'.format(mode, mult)
            out[key + 'kp'] = kp.detach().numpy()
            if key != 'in_r200_':                            # relu at 200 is 200 times relu at 1: key points only
                out[key + 'p'], out[key + 'dvols'] = p.detach().numpy(), v.grad.numpy()

    # ---- cross-entropy
    ce_p = f32(out['in_s1_p'])
    pitch = np.array([100.0 / (X - 1), 100.0 / (Y - 1), 100.0 / (Z - 1)])
    cells = np.array([[[1, 2, 3], [7, 0, 1], [3, 5, 4]], [[0, 0, 0], [7, 4, 2], [4, 3, 0]]])
    signs = rng.choice([-1.0, 1.0], (B, J, 3))
    signs[0, 1] = [1.0, -1.0, 1.0]                           # a face and an edge voxel pushed outwards: outside the box
    signs[1, 0] = [-1.0, -1.0, -1.0]                         # a corner voxel pushed outwards on every axis
    gt = np.zeros((B, J, 3))
    for b in range(B):
        for j in range(J):
            i, k, l = cells[b, j]
            gt[b, j] = coord[b, i, k, l].astype(np.float64) + 0.3 * pitch * signs[b, j]
    lo, hi = coord.reshape(B, -1, 3).min(1), coord.reshape(B, -1, 3).max(1)
    assert np.any((gt[0, 1] < lo[0]) | (gt[0, 1] > hi[0])) and np.all(gt[1, 0] < lo[1])
    gt = f32(gt)
    validity = f32(np.array([[1, 1, 0], [1, 0, 1]]).reshape(B, J, 1))
    d = np.sqrt(((coord.reshape(B, 1, -1, 3).astype(np.float64) - gt[:, :, None].astype(np.float64)) ** 2).sum(-1))
    two = np.sort(d, axis=2)[:, :, :2]
    assert np.all(two[..., 1] >= 1.05 * two[..., 0]), two
    pt = t64(ce_p).requires_grad_(True)
    loss = ref_loss.VolumetricCELoss()(t64(coord), pt, t64(gt), t64(validity))
    loss.backward()
    out.update(ce_gt=gt, ce_validity=validity, ce_loss=np.float64(loss.item()),
               ce_idx=d.argmin(axis=2).astype(np.int32), ce_dp=pt.grad.numpy())
    assert set(zip(*np.nonzero(out['ce_dp'].reshape(B, J, -1)))) == \
        {(b, j, int(out['ce_idx'][b, j])) for b in range(B) for j in range(J) if validity[b, j, 0] != 0}

    # ---- coordinate volumes
    rot_axis = np.array([[0.0, 1.0, 0.0], [1.0, -2.0, 0.5], [0.0, 0.0, 3.0]])
    rot_theta = np.array([0.7, 2.1, -1.3])
    out.update(rot_axis=rot_axis, rot_theta=rot_theta,
               rot_matrix=np.stack([vm.get_rotation_matrix(a, t) for a, t in zip(rot_axis, rot_theta)]))
    rot_in = f32(rng.normal(0.0, 100.0, (2, 3, 2, 3)))
    out.update(rot_in=rot_in,
               rot_out=vm.rotate_coord_volume(torch.from_numpy(rot_in), rot_theta[1], rot_axis[1]).numpy())

    path = os.path.join(HERE, 'volumetric.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 200 * 1024


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '/path/to/reference')
