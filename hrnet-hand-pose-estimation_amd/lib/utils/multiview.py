"""Multi-view triangulation (reference lib/models/triangulation_model_utils/multiview.py:172-187) on the HIP kernel
hrnet_triangulate (csrc/triangulate.hip): one launch per batch, no host loop over samples or joints.

The reference's tools/evaluate_3D.py lifts the pose_hrnet predictions with DLT_sii_pytorch (lib/utils/misc.py:64-97):
two shifted inverse iterations on A^T A + 1e-3 I from a torch.rand start, solved with torch.solve (which the installed
torch no longer has). Their fixed point is the eigenvector of A^T A for its smallest eigenvalue, i.e. the right
singular vector of A for its smallest singular value. This project computes that converged vector directly (in
float64, by a Givens QR and a Jacobi SVD, as triangulate_point_from_multiple_views_linear does with numpy's SVD); the
random start is not reproduced."""
import torch

from hipnet import _capi as C


def triangulate_batch_of_points(proj_matricies_batch, points_batch, confidences_batch=None, to_frame=None,
                                return_frame_points=False):
    """proj_matricies_batch (B, V, 3, 4), points_batch (B, V, K, 2), confidences_batch (B, V, K) or None, all on the
    HIP device -> (B, K, 3) float32 points.

    to_frame (B * V, 2, 3) or None: affine from the points' pixels (heat-map pixels) to the frames of the projection
    matrices, applied first (the readers' `hm_inverse`). return_frame_points=True also returns the mapped 2-D points,
    (B, V, K, 2) float32. A point with fewer than two views of nonzero confidence is NaN."""
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
    pts = points_batch.detach().to(dev, torch.float32).contiguous()
    proj = proj_matricies_batch.detach().to(dev, torch.float64).contiguous()
    conf = None if confidences_batch is None else confidences_batch.detach().to(dev, torch.float32).contiguous()
    mat = None if to_frame is None else to_frame.detach().to(dev, torch.float64).contiguous()
    X = torch.empty((B, K, 3), dtype=torch.float32, device=dev)
    frame = torch.empty((B, V, K, 2), dtype=torch.float32, device=dev) if return_frame_points else None
    C.call('hrnet_triangulate', pts.data_ptr(), C.ptr(mat), proj.data_ptr(), C.ptr(conf), X.data_ptr(), C.ptr(frame),
           B, V, K, C.stream_ptr())
    return (X, frame) if return_frame_points else X
