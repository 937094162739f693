"""float64 numpy restatement of the volumetric lifting operations and their gradients, vectorised over everything, for
tests/test_volumetric_cpu.py (which holds it to the reference's own float64 results, tests/golden/volumetric.npz) and
tests/test_volumetric_gpu.py (where it is the oracle at shapes too large for a fixture).

Layouts: features (B, V, C, H, W), volumes (B, C, X, Y, Z), coordinate volumes (B, X, Y, Z, 3), projections
(B, V, 3, 4). The sample position is the rule of hrnet_unproject_volume (include/hrnet_hip.h): column u (W - 1) / H, row
w (H - 1) / W, bilinear with zero padding, 0 where the depth is <= 0."""
import numpy as np

EPS_CE = 1e-6


def _positions(proj, coord, H, W):
    """-> idx (B, V, N, 4) int flat cell of the four corners (clipped), wgt (B, V, N, 4) their weights, 0 for a corner
    outside the map or an invalid view"""
    B, V = proj.shape[:2]
    pts = coord.reshape(B, -1, 3).astype(np.float64)
    P = proj.astype(np.float64)
    q = np.einsum('bvij,bnj->bvni', P[..., :3], pts) + P[:, :, None, :, 3]
    z = q[..., 2]
    invalid = z <= 0.0
    z = np.where(z == 0.0, 1.0, z)
    ix = q[..., 0] / z * (W - 1) / H
    iy = q[..., 1] / z * (H - 1) / W
    ix = np.where(np.isfinite(ix), np.clip(ix, -2.0, W + 1.0), -2.0)
    iy = np.where(np.isfinite(iy), np.clip(iy, -2.0, H + 1.0), -2.0)
    x0, y0 = np.floor(ix), np.floor(iy)
    fx, fy = ix - x0, iy - y0
    idx, wgt = [], []
    for dy, wy in ((0, 1.0 - fy), (1, fy)):
        for dx, wx in ((0, 1.0 - fx), (1, fx)):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1) & ~invalid
            idx.append((np.clip(yy, 0, H - 1) * W + np.clip(xx, 0, W - 1)).astype(np.int64))
            wgt.append(np.where(ok, wx * wy, 0.0))
    return np.stack(idx, -1), np.stack(wgt, -1)


def _samples(feat, idx, wgt):
    """-> (B, V, C, N) samples"""
    B, V, C, H, W = feat.shape
    f = feat.reshape(B, V, C, H * W).astype(np.float64)
    s = np.zeros((B, V, C, idx.shape[2]))
    for k in range(4):
        s += np.take_along_axis(f, np.broadcast_to(idx[:, :, None, :, k], s.shape), axis=3) * wgt[:, :, None, :, k]
    return s


def _method(name):
    return 'conf' if name.startswith('conf') else name


def _factors(s, method, conf):
    """d volume / d sample per view, (B, V, C, N)"""
    if method == 'sum':
        return np.ones_like(s)
    if method == 'conf':
        return np.broadcast_to(conf.astype(np.float64)[..., None], s.shape)
    if method == 'max':
        win = np.argmax(s, axis=1)                       # the first largest view
        return (np.arange(s.shape[1])[None, :, None, None] == win[:, None]).astype(np.float64)
    if method == 'softmax':
        e = np.exp(s - s.max(axis=1, keepdims=True))
        x = e / e.sum(axis=1, keepdims=True)
        return x * (1.0 + s - (s * x).sum(axis=1, keepdims=True))
    raise ValueError(method)


def unproject(feat, proj, coord, method='sum', conf=None):
    B, V, C, H, W = feat.shape
    method = _method(method)
    idx, wgt = _positions(proj, coord, H, W)
    s = _samples(feat, idx, wgt)
    if method == 'sum':
        out = s.sum(axis=1)
    elif method == 'conf':
        out = (s * conf.astype(np.float64)[..., None]).sum(axis=1)
    elif method == 'max':
        out = s.max(axis=1)
    elif method == 'softmax':
        e = np.exp(s - s.max(axis=1, keepdims=True))
        out = (s * e / e.sum(axis=1, keepdims=True)).sum(axis=1)
    else:
        raise ValueError(method)
    return out.reshape((B, C) + coord.shape[1:4])


def unproject_bwd(feat, proj, coord, gV, method='sum', conf=None):
    """-> (dfeatures (B, V, C, H, W), dconf (B, V, C) or None)"""
    B, V, C, H, W = feat.shape
    method = _method(method)
    idx, wgt = _positions(proj, coord, H, W)
    s = _samples(feat, idx, wgt)
    g = gV.reshape(B, 1, C, -1).astype(np.float64)
    gs = g * _factors(s, method, conf)                   # (B, V, C, N)
    d = np.zeros(B * V * C * H * W)
    rows = (np.arange(B * V * C) * (H * W)).reshape(B, V, C, 1)
    for k in range(4):
        cells = (rows + idx[:, :, None, :, k]).ravel()
        share = (gs * wgt[:, :, None, :, k]).ravel()
        d += np.bincount(cells, weights=share, minlength=d.size)
    dconf = (g * s).sum(axis=3) if method == 'conf' else None
    return d.reshape(B, V, C, H, W), dconf


def scatter_bound(feat_shape, proj, coord, gV):
    """S: the 'sum' input gradient of |gV|. Every bilinear weight is >= 0, so S times the method's largest per-view
    factor bounds the magnitude that reaches a pixel: the factor is 1 for 'sum' and 'max', |conf| for 'conf' and at
    most 1 + 2 max|sample| for 'softmax' (x_v (1 + s_v - sum_u s_u x_u) with x_v <= 1)"""
    return unproject_bwd(np.zeros(feat_shape), proj, coord, np.abs(gV), 'sum')[0]


def integrate(vols, coord, softmax=True, multiplier=1.0):
    """-> (keypoints (B, J, 3), p (B, J, X, Y, Z))"""
    B, J = vols.shape[:2]
    t = multiplier * vols.reshape(B, J, -1).astype(np.float64)
    if softmax:
        e = np.exp(t - t.max(axis=2, keepdims=True))
        p = e / e.sum(axis=2, keepdims=True)
    else:
        p = np.maximum(t, 0.0)
    kp = np.einsum('bjn,bnc->bjc', p, coord.reshape(B, -1, 3).astype(np.float64))
    return kp, p.reshape(vols.shape)


def integrate_bwd(vols, coord, gK, gP=None, softmax=True, multiplier=1.0):
    B, J = vols.shape[:2]
    _, p = integrate(vols, coord, softmax, multiplier)
    p = p.reshape(B, J, -1)
    t = np.einsum('bjc,bnc->bjn', gK.astype(np.float64), coord.reshape(B, -1, 3).astype(np.float64))
    if gP is not None:
        t = t + gP.reshape(B, J, -1)
    if softmax:
        d = multiplier * p * (t - (p * t).sum(axis=2, keepdims=True))
    else:
        d = multiplier * (multiplier * vols.reshape(B, J, -1) > 0) * t
    return d.reshape(vols.shape)


def ce_loss(coord, p, gt, validity):
    """-> (loss, idx (B, J) flat voxel index, dp (B, J, X, Y, Z) for d loss = 1)"""
    B, J = p.shape[:2]
    c = coord.reshape(B, 1, -1, 3).astype(np.float64)
    d = np.sqrt(((c - gt.astype(np.float64)[:, :, None, :]) ** 2).sum(-1))
    idx = d.argmin(axis=2)                               # the first of equal distances
    pf = p.reshape(B, J, -1).astype(np.float64)
    at = np.take_along_axis(pf, idx[..., None], axis=2)[..., 0]
    v = validity.reshape(B, J).astype(np.float64)
    loss = (v * -np.log(at + EPS_CE)).sum() / (B * J)
    dp = np.zeros_like(pf)
    np.put_along_axis(dp, idx[..., None], (-v / (at + EPS_CE) / (B * J))[..., None], axis=2)
    return loss, idx, dp.reshape(p.shape)


def joints3d_loss(pred, gt):
    """Joints3DMSELoss and its gradient: sum ||gt - pred|| / K"""
    diff = pred - gt
    n = np.sqrt((diff ** 2).sum(-1))
    K = pred.shape[1]
    g = np.where(n[..., None] > 0, diff / np.where(n > 0, n, 1.0)[..., None], 0.0) / K
    return n.sum() / K, g


def ring_cameras(n, radius, focal, centre, target=(0.0, 0.0, 0.0), look_away=()):
    """n pinhole cameras on a ring of `radius` about `target` in the x-z plane, looking at it, principal point
    `centre` (cx, cy): (n, 3, 4) float64 K [R|t]. A view in look_away looks the other way."""
    out = []
    for i in range(n):
        a = 2.0 * np.pi * i / n + 0.3
        pos = np.asarray(target, dtype=np.float64) + radius * np.array([np.cos(a), 0.15 * (i % 2), np.sin(a)])
        fwd = np.asarray(target, dtype=np.float64) - pos
        fwd /= np.linalg.norm(fwd)
        if i in look_away:
            fwd = -fwd
        right = np.cross(fwd, [0.0, 1.0, 0.0])
        right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        R = np.stack([right, -up, fwd])
        t = -R @ pos
        Km = np.array([[focal, 0.0, centre[0]], [0.0, focal, centre[1]], [0.0, 0.0, 1.0]])
        out.append(Km @ np.c_[R, t])
    return np.stack(out)
