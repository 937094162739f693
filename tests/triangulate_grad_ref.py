"""Float64 numpy restatement of the backward of the DLT triangulation (hrnet_triangulate_bwd, csrc/triangulate.hip) for
tests/test_triangulate_grad_cpu.py and tests/test_triangulate_grad_gpu.py.

For one point, A (2V x 4) has the rows c_v (x_v P_v[2] - P_v[0]) and c_v (y_v P_v[2] - P_v[1]), singular values
s_1 >= ... >= s_4 and right singular vectors v_1 ... v_4; h = v_4, X = h[0:3] / h[3]. With g = dL/dX:
    g^ = [g / h_3, -(g . h[0:3]) / h_3^2]                         dL/dh
    z  = -sum_{i<4} v_i (v_i . g^) / (s_i^2 - s_4^2)              first-order perturbation of the null vector
    G  = (A z) h^T + (A h) z^T                                    dL/dA
    dL/dx_v = c_v G[2v] . P_v[2],  dL/dy_v = c_v G[2v+1] . P_v[2]
    dL/dc_v = G[2v] . (x_v P_v[2] - P_v[0]) + G[2v+1] . (y_v P_v[2] - P_v[1])
The sign of h cancels. `grad_point` takes the vectors from numpy's SVD of A; `grad_point_eigh` from eigh of A^T A, the
route that squares the condition number (kept to show the gap between the two)."""
import numpy as np

from triangulate_ref import dlt_rows


def _from_basis(A, rows, proj, c, vecs, sq, g):
    """vecs (4, 4) columns v_1..v_4 with squared singular values sq descending -> (dpts (V, 2), dconf (V,))"""
    h = vecs[:, 3]
    g = np.asarray(g, np.float64)
    ghat = np.r_[g / h[3], -(g @ h[:3]) / h[3] ** 2]
    z = np.zeros(4)
    for i in range(3):
        z -= vecs[:, i] * (vecs[:, i] @ ghat) / (sq[i] - sq[3])
    G = np.outer(A @ z, h) + np.outer(A @ h, z)
    dpts = np.stack((c * (G[0::2] @ proj[:, 2].T).diagonal(), c * (G[1::2] @ proj[:, 2].T).diagonal()), 1)
    dconf = (G[0::2] * rows[0::2]).sum(1) + (G[1::2] * rows[1::2]).sum(1)
    return dpts, dconf


def _setup(proj, pts, conf):
    proj = np.asarray(proj, np.float64)
    c = np.ones(len(proj)) if conf is None else np.asarray(conf, np.float64)
    return proj, c, dlt_rows(proj, pts, conf), dlt_rows(proj, pts, None)


def grad_point(proj, pts, conf, g):
    """proj (V, 3, 4), pts (V, 2), conf (V,) or None, g (3,) -> (dL/dpts (V, 2), dL/dconf (V,))"""
    proj, c, A, rows = _setup(proj, pts, conf)
    _, s, vt = np.linalg.svd(A)
    return _from_basis(A, rows, proj, c, vt.T, s * s, g)


def grad_point_eigh(proj, pts, conf, g):
    proj, c, A, rows = _setup(proj, pts, conf)
    w, vecs = np.linalg.eigh(A.T @ A)
    return _from_basis(A, rows, proj, c, vecs[:, ::-1], w[::-1], g)


def grad_batch(proj, pts, conf, gX, point_fn=grad_point):
    """(B, V, 3, 4), (B, V, K, 2), (B, V, K) or None, (B, K, 3) -> (dpts (B, V, K, 2), dconf (B, V, K))"""
    B, V, K = pts.shape[:3]
    dpts, dconf = np.empty((B, V, K, 2)), np.empty((B, V, K))
    for b in range(B):
        for k in range(K):
            dpts[b, :, k], dconf[b, :, k] = point_fn(proj[b], pts[b, :, k], None if conf is None else conf[b, :, k],
                                                     gX[b, k])
    return dpts, dconf


def relative_gap(proj, pts, conf=None):
    """(s_3^2 - s_4^2) / s_1^2 of one point's DLT matrix: what the backward divides by"""
    s = np.linalg.svd(dlt_rows(proj, pts, conf), compute_uv=False)
    return (s[2] ** 2 - s[3] ** 2) / s[0] ** 2
