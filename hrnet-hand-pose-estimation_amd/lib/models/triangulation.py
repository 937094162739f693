"""VolumetricTriangulationNet, MODEL.NAME `vol` (reference lib/models/triangulation.py:277-470), end to end on HIP
kernels:

    backbone (models/pose_hrnet_volumetric.py) on (B * V, 3, H, W)    heat maps and the 480-channel concatenation
    get_final_preds(heatmaps, HEATMAP_SOFTMAX)                         (B, V, K, 2) heat-map pixels
    base point = DLT of joint 9 over the views                         ONE hrnet_triangulate launch for the batch, under
                                                                       no_grad; proj_matrices map world coordinates to
                                                                       heat-map pixels, so no `to_frame` is passed
    build_coord_volumes(base_points, CUBOID_SIZE, VOLUME_SIZE, theta)  utils/volumetric.py
    process_features, Conv2d(480, 32, 1) on NCHW float32               hrnet_pointwise_nchw (csrc/pointwise.hip) through
                                                                       ONE autograd function; the weight is read in place
    unproject_heatmaps -> volume_net (models/v2v.py) -> integrate_tensor_3d_with_coordinates

`lift(heatmaps, features, proj_matrices, theta)` is everything after the backbone; `forward` is the backbone followed
by `lift`. The children carry the reference's attribute names (`backbone`, `process_features`, `volume_net`), so a
reference `vol` checkpoint loads with strict=True. With theta=None the reference's rule applies (:438-441): one
np.random.uniform(0, 2 pi) per sample in training mode, 0 in eval mode.

Refused before any device work: a VOLUME_AGGREGATION_METHOD beginning with `conf` (NotImplementedError), a VOLUME_SIZE
that is not a multiple of 32 (V2V's five poolings), a BACKBONE_NAME other than pose_hrnet_volumetric, CPU tensors
(ValueError).

Deviations from the reference, deliberate:
- coordinate volumes and base points are constants for autograd (utils/volumetric.py says why); the reference's graph
  reaches the base point through grid_sample's grid, this one does not;
- there is no confidence head: vol_confidences is None (models/pose_hrnet_volumetric.py);
- eval mode with a gradient required is refused, by the rule of the backbone and of V2V (the backward through running
  statistics is not built): run eval mode under torch.no_grad();
- the backbone is built with the caller's is_train (the reference always passes True, which only re-draws weights that
  a checkpoint then replaces);
- MODEL.USE_GT_MIDDLEROOT is accepted and unused, as in the reference, whose use of it is commented out.
"""
import logging

import numpy as np
import torch
import torch.nn as nn

from hipnet import _capi as C
from models import pose_hrnet_volumetric
from models.v2v import V2VModel
from utils.heatmap_decoding import get_final_preds
from utils.multiview import triangulate_batch_of_points
from utils.volumetric import build_coord_volumes, integrate_tensor_3d_with_coordinates, unproject_heatmaps

logger = logging.getLogger(__name__)

BACKBONES = {'pose_hrnet_volumetric': pose_hrnet_volumetric}
BASE_JOINT = 9                 # the middle finger's root (:367)
F32 = C.HR_F32


class _PointwiseFn(torch.autograd.Function):
    """y = conv2d(x, w, b) with a 1x1 kernel on NCHW float32: hrnet_pointwise_nchw; backward: one
    hrnet_pointwise_nchw_bwd call for whichever of dx, dw, db autograd asks for"""

    @staticmethod
    def forward(ctx, x, w, b):
        y = _pointwise(x, w, b)
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        N, Cin, H, W = x.shape
        Cout, P = w.shape[0], H * W
        gy = gy.contiguous().float()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_x or need_w or need_b):
            return None, None, None
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(w) if need_w else None
        db = torch.empty(Cout, dtype=torch.float32, device=x.device) if need_b else None
        scratch, floats = None, 0
        if need_w or need_b:
            floats = C.call('hrnet_pointwise_nchw_parts', N, P) * (Cout * Cin + Cout)
            scratch = torch.empty(floats, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            C.call('hrnet_pointwise_nchw_bwd', F32, x.data_ptr(), w.data_ptr(), gy.data_ptr(), C.ptr(dx), C.ptr(dw),
                   C.ptr(db), C.ptr(scratch), floats, N, Cin, Cout, P, C.stream_ptr())
        return dx, dw, db


def _pointwise(x, w, b):
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    y = torch.empty((N, Cout, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        C.call('hrnet_pointwise_nchw', F32, x.data_ptr(), w.data_ptr(), C.ptr(b), y.data_ptr(), N, Cin, Cout, H * W,
               C.stream_ptr())
    return y


def pointwise_conv_nchw(x, weight, bias=None):
    """F.conv2d(x, weight, bias) for a 1x1 kernel: x (N, Cin, H, W), weight (Cout, Cin, 1, 1) or (Cout, Cin), bias
    (Cout,) or None, float32 on the HIP device -> (N, Cout, H, W). Differentiable in all three. The weight is read in
    place, so nothing can go stale when an optimiser updates it."""
    tensors = [t for t in (x, weight, bias) if t is not None]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
        raise ValueError('pointwise_conv_nchw: expected HIP-device tensors (there is no CPU path in this build)')
    if x.ndim != 4 or weight.ndim not in (2, 4) or tuple(weight.shape[2:]) not in ((), (1, 1)) or \
            weight.shape[1] != x.shape[1] or (bias is not None and tuple(bias.shape) != (weight.shape[0],)):
        raise ValueError('pointwise_conv_nchw: x {}, weight {}, bias {}: expected (N, Cin, H, W), (Cout, Cin, 1, 1) and '
                         '(Cout,)'.format(tuple(x.shape), tuple(weight.shape), None if bias is None else tuple(bias.shape)))
    if min(x.shape) < 1 or not C.call('hrnet_pointwise_nchw_supported', F32, x.shape[1], weight.shape[0]):
        raise ValueError('pointwise_conv_nchw: x {}, weight {}: no kernel for this shape (1 <= Cout <= 64, no empty '
                         'axis)'.format(tuple(x.shape), tuple(weight.shape)))
    x = x.contiguous().float()
    weight = weight.contiguous().float()
    bias = None if bias is None else bias.contiguous().float()
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return _PointwiseFn.apply(x, weight, bias)
    return _pointwise(x.detach(), weight.detach(), None if bias is None else bias.detach())


def check_vol_config(config):
    """what the model refuses of a config, before anything is built"""
    method = config.MODEL.VOLUME_AGGREGATION_METHOD
    if not isinstance(method, str) or method.startswith('conf'):
        raise NotImplementedError('MODEL.VOLUME_AGGREGATION_METHOD {!r}: the confidence head of pose_hrnet_volumetric is '
                                  'not built, so the conf* aggregations have nothing to weigh with (sum, max and '
                                  'softmax are built)'.format(method))
    if method not in ('sum', 'max', 'softmax'):
        raise ValueError('Unknown volume_aggregation_method: {}'.format(method))
    size = config.MODEL.VOLUME_SIZE
    if not isinstance(size, int) or size < 32 or size % 32:
        raise ValueError('MODEL.VOLUME_SIZE {}: V2V pools five times and adds the results back to the skips, so the '
                         'volume side must be a multiple of 32'.format(size))
    if config.MODEL.BACKBONE_NAME not in BACKBONES:
        raise ValueError('MODEL.BACKBONE_NAME {!r}: the volumetric model is built on {}'.format(
            config.MODEL.BACKBONE_NAME, ' / '.join(BACKBONES)))
    if config.MODEL.ALG_CONFIDENCES:
        raise NotImplementedError('MODEL.ALG_CONFIDENCES true: pose_hrnet_volumetric does not build that head')


class VolumetricTriangulationNet(nn.Module):
    def __init__(self, config, is_train=True):
        super().__init__()
        check_vol_config(config)
        self.config = config
        self.num_joints = config.DATASET.NUM_JOINTS
        self.volume_aggregation_method = config.MODEL.VOLUME_AGGREGATION_METHOD
        self.volume_softmax = config.MODEL.VOLUME_SOFTMAX
        self.volume_multiplier = config.MODEL.VOLUME_MULTIPLIER
        self.volume_size = config.MODEL.VOLUME_SIZE
        self.cuboid_side = config.MODEL.CUBOID_SIZE
        self.heatmap_softmax = config.MODEL.HEATMAP_SOFTMAX
        self.use_gt_middleroot = config.MODEL.USE_GT_MIDDLEROOT

        self.backbone = BACKBONES[config.MODEL.BACKBONE_NAME].get_pose_net(config, is_train=is_train)
        if is_train:
            path = config.MODEL.BACKBONE_MODEL_PATH
            if path:
                checkpoint = torch.load(path, map_location='cpu')
                state = checkpoint['state_dict'] if 'state_dict' in checkpoint else checkpoint
                logger.info("=> Loading pretrained {} backbone from '{}'".format(config.MODEL.BACKBONE_NAME, path))
                state = {k.replace('module.', ''): v for k, v in state.items()}
                self.backbone.load_state_dict(state, strict=False)
            # freeze the lower layers (:330-343): stage4 and the head train, the temperature does not
            for p in self.backbone.parameters():
                p.requires_grad = False
            for p in self.backbone.stage4.parameters():
                p.requires_grad = True
            for p in self.backbone.last_layer.parameters():
                p.requires_grad = True
            self.backbone.trainable_temp.requires_grad = False

        self.process_features = nn.Sequential(nn.Conv2d(sum(config.MODEL.EXTRA.STAGE4.NUM_CHANNELS), 32, 1))
        self.volume_net = V2VModel(32, self.num_joints, trainable=is_train)

    def _thetas(self, theta, B):
        if theta is None:
            return [float(np.random.uniform(0.0, 2 * np.pi)) for _ in range(B)] if self.training else 0.0
        return theta

    def lift(self, heatmaps, features, proj_matrices, theta=None):
        """heatmaps (B * V, K, h, w) and features (B * V, 480, h, w) as the backbone returns them, proj_matrices
        (B, V, 3, 4) from world coordinates to heat-map pixels, theta: None, one angle or one per sample -> the 7-tuple
        of forward"""
        tensors = (heatmaps, features, proj_matrices)
        if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
            raise ValueError('VolumetricTriangulationNet: expected HIP-device tensors (there is no CPU path in this build)')
        if proj_matrices.ndim != 4 or tuple(proj_matrices.shape[2:]) != (3, 4):
            raise ValueError('proj_matrices: expected (B, V, 3, 4), got {}'.format(tuple(proj_matrices.shape)))
        B, V = proj_matrices.shape[:2]
        if heatmaps.ndim != 4 or features.ndim != 4 or heatmaps.shape[0] != B * V or features.shape[0] != B * V or \
                heatmaps.shape[2:] != features.shape[2:]:
            raise ValueError('heatmaps {} and features {}: expected (B * V = {}, C, h, w) with one map size'.format(
                tuple(heatmaps.shape), tuple(features.shape), B * V))
        conv = self.process_features[0]
        if features.shape[1] != conv.in_channels:
            raise ValueError('features have {} channels, process_features takes {}'.format(features.shape[1],
                                                                                          conv.in_channels))
        if not self.training and torch.is_grad_enabled() and (
                heatmaps.requires_grad or features.requires_grad or
                any(p.requires_grad for m in (self.process_features, self.volume_net) for p in m.parameters())):
            raise NotImplementedError('VolumetricTriangulationNet: eval mode with a gradient required is refused - the '
                                      'backward through the running statistics is not built; call .train(), or run '
                                      'under torch.no_grad()')
        K = heatmaps.shape[1]
        pose2d_pred = get_final_preds(heatmaps, use_softmax=self.heatmap_softmax).view(B, V, K, 2)
        with torch.no_grad():
            base_points = triangulate_batch_of_points(
                proj_matrices, pose2d_pred.detach()[:, :, BASE_JOINT:BASE_JOINT + 1].contiguous())[:, 0]     # (B, 3)
            coord_volumes = build_coord_volumes(base_points, self.cuboid_side, self.volume_size, self._thetas(theta, B))
        feats = pointwise_conv_nchw(features, conv.weight, conv.bias)
        feats = feats.view(B, V, *feats.shape[1:])
        volumes = unproject_heatmaps(feats, proj_matrices.detach(), coord_volumes,
                                     volume_aggregation_method=self.volume_aggregation_method)
        volumes = self.volume_net(volumes)
        vol_keypoints_3d, volumes = integrate_tensor_3d_with_coordinates(
            volumes, coord_volumes, softmax=self.volume_softmax, multiplier=self.volume_multiplier)
        return (vol_keypoints_3d, pose2d_pred, heatmaps.view(B, V, *heatmaps.shape[1:]), volumes, None, coord_volumes,
                base_points)

    def forward(self, images, proj_matrices, batch=None, keypoints_3d=None, theta=None):
        """images (B, V, 3, H, W), proj_matrices (B, V, 3, 4) -> (vol_keypoints_3d (B, K, 3), pose2d_pred (B, V, K, 2),
        heatmaps (B, V, K, h, w), volumes (B, K, S, S, S), vol_confidences None, coord_volumes (B, S, S, S, 3),
        base_points (B, 3)); batch and keypoints_3d are accepted and unused, as in the reference"""
        if not isinstance(images, torch.Tensor) or not images.is_cuda or not isinstance(proj_matrices, torch.Tensor) \
                or not proj_matrices.is_cuda:
            raise ValueError('VolumetricTriangulationNet: expected HIP-device tensors (there is no CPU path in this build)')
        if images.ndim != 5 or tuple(proj_matrices.shape) != tuple(images.shape[:2]) + (3, 4):
            raise ValueError('images {} and proj_matrices {}: expected (B, V, 3, H, W) and (B, V, 3, 4)'.format(
                tuple(images.shape), tuple(proj_matrices.shape)))
        heatmaps, features = self.backbone(images.reshape(-1, *images.shape[2:]))[:2]
        return self.lift(heatmaps, features, proj_matrices, theta)


def get_pose_net(cfg, is_train, **kwargs):
    return VolumetricTriangulationNet(cfg, is_train=is_train)
