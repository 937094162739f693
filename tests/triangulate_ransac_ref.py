"""Float64 numpy restatement of hrnet_triangulate_ransac (csrc/triangulate.hip) for the CPU tests
(tests/test_triangulate_ransac_cpu.py), on the Givens QR + Jacobi SVD of tests/triangulate_ref.py: the hypotheses in
table order, a two-view DLT each, HALF the pixel distance against epsilon, the candidate {i, j} + {v : err_v < epsilon}
taken only when strictly larger, and the DLT over the final set in ascending view order; a non-finite input in any
view gives NaN."""
import numpy as np

import triangulate_ref as T


def reprojection_errors(proj, pts, X):
    """proj (V, 3, 4), pts (V, 2), X (3,) -> (V,): half the pixel distance (reference multiview.py:196)"""
    h = np.asarray(proj, np.float64) @ np.r_[X, 1.0]
    with np.errstate(all='ignore'):
        return 0.5 * np.sqrt(((np.asarray(pts, np.float64) - h[:, :2] / h[:, 2:]) ** 2).sum(1))


def triangulate_ransac(proj, pts, pairs, epsilon):
    """proj (V, 3, 4), pts (V, 2), pairs (n_hyp, 2) -> (X (3,), inlier mask (V,) bool)"""
    V = len(proj)
    best = np.zeros(V, bool)
    for i, j in np.asarray(pairs).reshape(-1, 2):
        if i == j or not (0 <= i < V and 0 <= j < V):
            continue
        X2, _ = T.triangulate(proj[[i, j]], pts[[i, j]])
        with np.errstate(all='ignore'):
            cand = reprojection_errors(proj, pts, X2) < epsilon
        cand[[i, j]] = True
        if cand.sum() > best.sum():
            best = cand
    if not best.any():
        best = np.ones(V, bool)
    if not (np.isfinite(proj).all() and np.isfinite(pts).all()):         # a non-finite input is not hidden
        return np.full(3, np.nan), best
    return T.triangulate(proj[best], pts[best])[0], best


def triangulate_ransac_batch(proj, pts, pairs, epsilon):
    """(B, V, 3, 4), (B, V, K, 2), pairs (n_hyp, 2) or (B * K, n_hyp, 2) -> (X (B, K, 3), mask (B, K, V))"""
    B, V, K = pts.shape[:3]
    pairs = np.asarray(pairs)
    X, mask = np.empty((B, K, 3)), np.zeros((B, K, V), bool)
    for b in range(B):
        for k in range(K):
            table = pairs[b * K + k] if pairs.ndim == 3 else pairs
            X[b, k], mask[b, k] = triangulate_ransac(np.asarray(proj[b], np.float64),
                                                     np.asarray(pts[b, :, k], np.float64), table, epsilon)
    return X, mask
