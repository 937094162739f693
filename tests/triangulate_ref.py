"""Float64 numpy restatement of csrc/triangulate.hip for the CPU tests (tests/test_triangulate_cpu.py): the DLT rows of
the reference's triangulate_point_from_multiple_views_linear(_torch) (multiview.py:120-169), streamed into a 4 x 4
triangular R by Givens rotations, then a one-sided Jacobi SVD of R, step for step as the kernel does it. Also the
float32 A^T A eigen-solve the kernel avoids, to show what the GPU tolerance rejects."""
import numpy as np

SWEEPS = 16
EPS = np.finfo(np.float64).eps


def dlt_rows(proj, pts, conf=None):
    """proj (V, 3, 4), pts (V, 2), conf (V,) or None -> A (2V, 4): w (u P[2] - P[0]), w (v P[2] - P[1]) per view"""
    proj = np.asarray(proj, np.float64)
    pts = np.asarray(pts, np.float64)
    w = np.ones(len(proj)) if conf is None else np.asarray(conf, np.float64)
    A = np.empty((2 * len(proj), 4))
    A[0::2] = w[:, None] * (pts[:, :1] * proj[:, 2] - proj[:, 0])
    A[1::2] = w[:, None] * (pts[:, 1:] * proj[:, 2] - proj[:, 1])
    return A


def givens_r(A):
    """4 x 4 upper-triangular R with A = Q R, the rows streamed in one at a time"""
    R = np.zeros((4, 4))
    for row in A:
        a = row.copy()
        for j in range(4):
            r = np.hypot(R[j, j], a[j])
            if r == 0.0:
                continue
            c, s = R[j, j] / r, a[j] / r
            R[j, j:], a[j:] = c * R[j, j:] + s * a[j:], c * a[j:] - s * R[j, j:]
    return R


def jacobi_null_vector(R):
    """right singular vector of R for its smallest singular value (one-sided Jacobi, the kernel's rotation)"""
    W, V = R.copy(), np.eye(4)
    for _ in range(SWEEPS):
        rotated = False
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            alpha, beta, gamma = W[:, p] @ W[:, p], W[:, q] @ W[:, q], W[:, p] @ W[:, q]
            if abs(gamma) <= EPS * np.sqrt(alpha * beta):
                continue
            zeta = (beta - alpha) / (2.0 * gamma)
            t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.hypot(1.0, zeta))
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = c * t
            for M in (W, V):
                mp, mq = M[:, p].copy(), M[:, q].copy()
                M[:, p], M[:, q] = c * mp - s * mq, s * mp + c * mq
            rotated = True
        if not rotated:
            break
    return V[:, int(np.argmin((W * W).sum(0)))]


def triangulate(proj, pts, conf=None):
    """proj (V, 3, 4), pts (V, 2), conf (V,) or None -> (X (3,), homogeneous v (4,)); NaN under two weighted views"""
    w = np.ones(len(proj)) if conf is None else np.asarray(conf)
    if np.count_nonzero(w) < 2:
        return np.full(3, np.nan), np.full(4, np.nan)
    v = jacobi_null_vector(givens_r(dlt_rows(proj, pts, conf)))
    return v[:3] / v[3], v


def triangulate_batch(proj, pts, conf=None):
    """(B, V, 3, 4), (B, V, K, 2), (B, V, K) or None -> (B, K, 3)"""
    B, V, K = pts.shape[:3]
    out = np.empty((B, K, 3))
    for b in range(B):
        for k in range(K):
            out[b, k] = triangulate(proj[b], pts[b, :, k], None if conf is None else conf[b, :, k])[0]
    return out


def triangulate_ata_f32(proj, pts, conf=None):
    """the shortcut the kernel does not take: eigenvector of the float32 A^T A for its smallest eigenvalue"""
    A = dlt_rows(proj, pts, conf).astype(np.float32)
    _, vecs = np.linalg.eigh(A.T @ A)
    v = vecs[:, 0].astype(np.float64)
    return v[:3] / v[3]
