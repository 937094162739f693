"""float64 torch restatement of VolumetricTriangulationNet.lift (lib/models/triangulation.py) for tests/test_vol_gpu.py,
composed from pieces that are each held to the reference's own fixtures on the CPU:

    decode                oracle/hrnet_cpu.py get_final_preds (expectation)
    base point            tests/triangulate_ref.py, the DLT of joint 9 over the views
    unprojection          tests/volumetric_ref.py unproject / unproject_bwd (numpy, float64 inside), wrapped in an
                          autograd function
    V2V                   tests/v2v_ref.py Net (eval) / tests/v2v_train_ref.py TrainNet (batch statistics, autograd)
    3-D soft-argmax, the two losses: the formulas of tests/volumetric_ref.py integrate / ce_loss / joints3d_loss in torch
The new lines are the base point, the cuboid rule (coord_volumes, held to utils.volumetric.build_coord_volumes by
tests/test_vol_cpu.py) and the 1x1 convolution (F.conv2d). `dtype` is the precision of the torch graph; the numpy pieces
compute in float64 and their results are rounded to `dtype`, so a float32 run under-states the float32 error a little:
a bound derived from it is the stricter for it."""
import numpy as np
import torch
import torch.nn.functional as F

import triangulate_ref as T
import volumetric_ref as VR
from oracle import hrnet_cpu as O

BASE_JOINT = 9


def coord_volumes(base_points, cuboid_side, S, thetas):
    """(B, 3) float64, one angle per sample -> (B, S, S, S, 3) float64: voxel (i, j, k) at base - side / 2 +
    side / (S - 1) (i, j, k), turned by theta about the y axis through the base point (counterclockwise, Rodrigues)"""
    base = np.asarray(base_points, dtype=np.float64)
    r = np.arange(S, dtype=np.float64)
    grid = np.stack(np.meshgrid(r, r, r, indexing='ij'), axis=-1)
    out = []
    for b, theta in zip(base, np.broadcast_to(np.asarray(thetas, dtype=np.float64).reshape(-1), (len(base),))):
        local = -cuboid_side / 2.0 + cuboid_side / (S - 1) * grid
        c, s = np.cos(theta), np.sin(theta)
        rot = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
        out.append(local.reshape(-1, 3) @ rot.T + b)
    return np.stack(out).reshape(len(base), S, S, S, 3)


def base_points(heatmaps, proj):
    """heatmaps (B * V, K, h, w) tensor, proj (B, V, 3, 4) numpy -> (pose2d (B, V, K, 2), base (B, 3)) float64 numpy"""
    B, V = proj.shape[:2]
    pred = O.get_final_preds(heatmaps.detach().double(), True).numpy().reshape(B, V, -1, 2)
    return pred, T.triangulate_batch(proj, pred[:, :, BASE_JOINT:BASE_JOINT + 1])[:, 0]


class _Unproject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, proj, coord, method):
        ctx.save_for_backward(feat)
        ctx.rest = (proj, coord, method)
        return torch.from_numpy(VR.unproject(feat.detach().double().numpy(), proj, coord, method)).to(feat.dtype)

    @staticmethod
    def backward(ctx, gV):
        feat, = ctx.saved_tensors
        proj, coord, method = ctx.rest
        d = VR.unproject_bwd(feat.detach().double().numpy(), proj, coord, gV.double().numpy(), method)[0]
        return torch.from_numpy(d).to(feat.dtype), None, None, None


def lift(net, w, b, heatmaps, features, proj, cuboid_side, S, thetas, method='softmax', multiplier=1.0,
         dtype=torch.float64):
    """net: v2v_ref.Net or v2v_train_ref.TrainNet in `dtype`; w (32, C, 1, 1), b (32,) tensors in `dtype`; heatmaps,
    features tensors in `dtype` (features may require a gradient); proj (B, V, 3, 4) float64 numpy
    -> (key points (B, K, 3), p (B, K, S, S, S), coord (B, S, S, S, 3), base (B, 3)), the first two in the graph"""
    B, V = proj.shape[:2]
    _pred, base = base_points(heatmaps, proj)
    coord = coord_volumes(base, cuboid_side, S, thetas)
    feats = F.conv2d(features, w, b)
    feats = feats.reshape(B, V, *feats.shape[1:])
    vol = _Unproject.apply(feats, proj, coord, method)
    out = net(vol)
    K = out.shape[1]
    p = torch.softmax(multiplier * out.reshape(B, K, -1), dim=2)
    ct = torch.from_numpy(coord.reshape(B, -1, 3)).to(dtype)
    kp = torch.einsum('bjn,bnc->bjc', p, ct)
    return kp, p.reshape(out.shape), torch.from_numpy(coord), torch.from_numpy(base)


def loss(kp, p, coord, gt, ce_factor=0.01):
    """Joints3DMSELoss + ce_factor * VolumetricCELoss with every joint valid (tests/volumetric_ref.py's formulas)"""
    B, K = kp.shape[:2]
    g = torch.as_tensor(gt).to(kp.dtype)
    j3d = (kp - g).norm(dim=-1).sum() / K
    c = coord.reshape(B, 1, -1, 3).double()
    idx = ((c - torch.as_tensor(gt).double()[:, :, None, :]) ** 2).sum(-1).argmin(dim=2)      # the first of equals
    at = p.reshape(B, K, -1).gather(2, idx[..., None])[..., 0]
    ce = (-torch.log(at + VR.EPS_CE)).sum() / (B * K)
    return j3d + ce_factor * ce
