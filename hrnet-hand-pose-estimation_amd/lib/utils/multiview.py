"""Multi-view triangulation (reference lib/models/triangulation_model_utils/multiview.py:172-187) on the HIP kernel
hrnet_triangulate (csrc/triangulate.hip): one launch per batch, no host loop over samples or joints.

The reference's tools/evaluate_3D.py lifts the pose_hrnet predictions with DLT_sii_pytorch (lib/utils/misc.py:64-97):
two shifted inverse iterations on A^T A + 1e-3 I from a torch.rand start, solved with torch.solve (which the installed
torch no longer has). Their fixed point is the eigenvector of A^T A for its smallest eigenvalue, i.e. the right
singular vector of A for its smallest singular value. This project computes that converged vector directly (in
float64, by a Givens QR and a Jacobi SVD, as triangulate_point_from_multiple_views_linear does with numpy's SVD); the
random start is not reproduced.

triangulate_ransac_batch is the reference's RANSAC over the views (lib/utils/misc.py:178-240, direct_optimization off)
on hrnet_triangulate_ransac, again one launch per batch. The host chooses the hypotheses (view pairs) and the kernel draws
nothing: by default every pair of views in lexicographic order, which is deterministic and sees every set that the
reference's ten random draws can see; sample_view_pairs gives the draws the reference would make from a seed.

triangulate_batch_of_points is differentiable in the points and the confidences (the reference trains through
torch.svd, AlgebraicTriangulationNet): when one of them requires a gradient the same hrnet_triangulate launch runs
inside an autograd function whose backward is ONE hrnet_triangulate_bwd launch, which recomputes the SVD from the saved
inputs. The projection matrices and `to_frame` are constants. triangulate_ransac_batch is not differentiable."""
import itertools
import random

import torch

from hipnet import _capi as C


class _TriangulateFn(torch.autograd.Function):
    """X of hrnet_triangulate; backward: hrnet_triangulate_bwd on the saved inputs. pts / conf are f32 contiguous,
    proj / mat f64 contiguous device tensors; conf and mat may be None."""

    @staticmethod
    def forward(ctx, pts, conf, proj, mat):
        B, V, K = pts.shape[:3]
        X = torch.empty((B, K, 3), dtype=torch.float32, device=pts.device)
        C.call('hrnet_triangulate', pts.data_ptr(), C.ptr(mat), proj.data_ptr(), C.ptr(conf), X.data_ptr(), None,
               B, V, K, C.stream_ptr())
        ctx.save_for_backward(pts, conf, proj, mat)
        return X

    @staticmethod
    def backward(ctx, gX):
        pts, conf, proj, mat = ctx.saved_tensors
        B, V, K = pts.shape[:3]
        gX = gX.contiguous().float()
        dpts = torch.empty_like(pts)
        dconf = torch.empty_like(conf) if conf is not None and ctx.needs_input_grad[1] else None
        C.call('hrnet_triangulate_bwd', pts.data_ptr(), C.ptr(mat), proj.data_ptr(), C.ptr(conf), gX.data_ptr(),
               dpts.data_ptr(), C.ptr(dconf), B, V, K, C.stream_ptr())
        return dpts, dconf, None, None


def triangulate_batch_of_points(proj_matricies_batch, points_batch, confidences_batch=None, to_frame=None,
                                return_frame_points=False):
    """proj_matricies_batch (B, V, 3, 4), points_batch (B, V, K, 2), confidences_batch (B, V, K) or None, all on the
    HIP device -> (B, K, 3) float32 points.

    to_frame (B * V, 2, 3) or None: affine from the points' pixels (heat-map pixels) to the frames of the projection
    matrices, applied first (the readers' `hm_inverse`). return_frame_points=True also returns the mapped 2-D points,
    (B, V, K, 2) float32 (never part of the graph). A point with fewer than two views of nonzero confidence is NaN.

    Differentiable in points_batch and confidences_batch: when one of them requires a gradient (and gradients are
    enabled) X carries a grad_fn whose backward is one hrnet_triangulate_bwd launch; X is the same bits either way.
    A view of zero confidence gets zero gradients, a NaN point NaN gradients in its own views only."""
    if points_batch.ndim != 4 or points_batch.shape[-1] != 2:
        raise ValueError('points_batch: expected (B, V, K, 2), got {}'.format(tuple(points_batch.shape)))
    B, V, K = points_batch.shape[:3]
    if tuple(proj_matricies_batch.shape) != (B, V, 3, 4):
        raise ValueError('proj_matricies_batch: expected {}, got {}'.format((B, V, 3, 4),
                                                                           tuple(proj_matricies_batch.shape)))
    if confidences_batch is not None and tuple(confidences_batch.shape) != (B, V, K):
        raise ValueError('confidences_batch: expected {}, got {}'.format((B, V, K), tuple(confidences_batch.shape)))
    if to_frame is not None and tuple(to_frame.shape) != (B * V, 2, 3):
        raise ValueError('to_frame: expected {}, got {}'.format((B * V, 2, 3), tuple(to_frame.shape)))
    tensors = [t for t in (proj_matricies_batch, points_batch, confidences_batch, to_frame) if t is not None]
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError('triangulate_batch_of_points: expected HIP-device tensors (no CPU path in this build)')
    dev = points_batch.device
    proj = proj_matricies_batch.detach().to(dev, torch.float64).contiguous()
    mat = None if to_frame is None else to_frame.detach().to(dev, torch.float64).contiguous()
    if torch.is_grad_enabled() and (points_batch.requires_grad or
                                    (confidences_batch is not None and confidences_batch.requires_grad)):
        pts = points_batch.to(dev, torch.float32).contiguous()
        conf = None if confidences_batch is None else confidences_batch.to(dev, torch.float32).contiguous()
        X = _TriangulateFn.apply(pts, conf, proj, mat)
        if not return_frame_points:
            return X
        # the mapped points are an extra output of the same kernel: a second, detached launch, off the training path
        return X, triangulate_batch_of_points(proj, pts.detach(), None if conf is None else conf.detach(), mat,
                                              True)[1]
    pts = points_batch.detach().to(dev, torch.float32).contiguous()
    conf = None if confidences_batch is None else confidences_batch.detach().to(dev, torch.float32).contiguous()
    X = torch.empty((B, K, 3), dtype=torch.float32, device=dev)
    frame = torch.empty((B, V, K, 2), dtype=torch.float32, device=dev) if return_frame_points else None
    C.call('hrnet_triangulate', pts.data_ptr(), C.ptr(mat), proj.data_ptr(), C.ptr(conf), X.data_ptr(), C.ptr(frame),
           B, V, K, C.stream_ptr())
    return (X, frame) if return_frame_points else X


MAX_HYPOTHESES = 64          # kRansacMaxHyp of csrc/triangulate.hip


def all_view_pairs(n_views):
    """every pair (i, j), i < j, of 0..n_views-1 in lexicographic order: (n_views (n_views - 1) / 2, 2) int32"""
    return torch.tensor(list(itertools.combinations(range(n_views), 2)), dtype=torch.int32).reshape(-1, 2)


def sample_view_pairs(n_points, n_views, n_iters, seed):
    """(n_points, n_iters, 2) int32: the pairs the reference's triangulate_ransac draws when it is called for n_points
    points in turn after one random.seed(seed): n_iters times sorted(random.sample(views, 2)) per point, the points in
    (b, k) order. seed may also be a random.Random, whose stream is continued (batch after batch)."""
    if n_views < 2:
        raise ValueError('sample_view_pairs: n_views = {} (two or more)'.format(n_views))
    rng = seed if isinstance(seed, random.Random) else random.Random(seed)
    views = range(n_views)
    draws = [sorted(rng.sample(views, 2)) for _ in range(n_points * n_iters)]
    return torch.tensor(draws, dtype=torch.int32).reshape(n_points, n_iters, 2)


def triangulate_ransac_batch(proj_matricies_batch, points_batch, pairs=None, reprojection_error_epsilon=25,
                             to_frame=None, return_frame_points=False):
    """proj_matricies_batch (B, V, 3, 4), points_batch (B, V, K, 2) on the HIP device -> (X (B, K, 3) float32,
    inliers (B, K, V) bool): per point the largest set of views that agree with a two-view solution, and the DLT over
    that set (see include/hrnet_hip.h, hrnet_triangulate_ransac).

    pairs: the hypotheses, int view-index pairs, tried in order (the first largest set wins): (n_hyp, 2) for all points
    or (B * K, n_hyp, 2) per point, n_hyp <= 64; None: every pair of views in lexicographic order. A pair with equal or
    out-of-range indices is skipped; with no usable pair every view is kept.
    reprojection_error_epsilon is in the reference's unit, HALF a frame pixel distance (its default 25 keeps views
    within 50 px). to_frame and return_frame_points as in triangulate_batch_of_points (the frame points come third)."""
    if points_batch.ndim != 4 or points_batch.shape[-1] != 2:
        raise ValueError('points_batch: expected (B, V, K, 2), got {}'.format(tuple(points_batch.shape)))
    B, V, K = points_batch.shape[:3]
    if tuple(proj_matricies_batch.shape) != (B, V, 3, 4):
        raise ValueError('proj_matricies_batch: expected {}, got {}'.format((B, V, 3, 4),
                                                                           tuple(proj_matricies_batch.shape)))
    if to_frame is not None and tuple(to_frame.shape) != (B * V, 2, 3):
        raise ValueError('to_frame: expected {}, got {}'.format((B * V, 2, 3), tuple(to_frame.shape)))
    if pairs is None:
        pairs = all_view_pairs(V)
    pairs = torch.as_tensor(pairs)
    per_point = pairs.ndim == 3
    if pairs.is_floating_point() or pairs.is_complex() or pairs.dtype == torch.bool or pairs.shape[-1:] != (2,) \
            or not (pairs.ndim == 2 or (per_point and pairs.shape[0] == B * K)):
        raise ValueError('pairs: expected integer (n_hyp, 2) or {}, got {} {}'.format(
            (B * K, 'n_hyp', 2), pairs.dtype, tuple(pairs.shape)))
    n_hyp = pairs.shape[-2]
    if n_hyp > MAX_HYPOTHESES:
        raise ValueError('pairs: {} hypotheses (at most {})'.format(n_hyp, MAX_HYPOTHESES))
    epsilon = float(reprojection_error_epsilon)
    if epsilon != epsilon:
        raise ValueError('reprojection_error_epsilon is NaN')
    tensors = [t for t in (proj_matricies_batch, points_batch, to_frame) if t is not None]
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError('triangulate_ransac_batch: expected HIP-device tensors (no CPU path in this build)')
    dev = points_batch.device
    pts = points_batch.detach().to(dev, torch.float32).contiguous()
    proj = proj_matricies_batch.detach().to(dev, torch.float64).contiguous()
    mat = None if to_frame is None else to_frame.detach().to(dev, torch.float64).contiguous()
    table = pairs.to(dev, torch.int32).contiguous() if n_hyp else None
    X = torch.empty((B, K, 3), dtype=torch.float32, device=dev)
    mask = torch.empty((B, K), dtype=torch.int32, device=dev)
    frame = torch.empty((B, V, K, 2), dtype=torch.float32, device=dev) if return_frame_points else None
    C.call('hrnet_triangulate_ransac', pts.data_ptr(), C.ptr(mat), proj.data_ptr(), C.ptr(table), n_hyp,
           int(per_point), epsilon, X.data_ptr(), mask.data_ptr(), C.ptr(frame), B, V, K, C.stream_ptr())
    inliers = (mask[..., None] >> torch.arange(V, device=dev, dtype=torch.int32) & 1).bool()
    return (X, inliers, frame) if return_frame_points else (X, inliers)
