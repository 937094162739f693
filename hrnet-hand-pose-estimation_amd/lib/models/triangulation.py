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

VolumetricTriangulationNet_CPM, MODEL.NAME `vol_CPM` (reference :472-654), is the same model on the CPM_volumetric
backbone (models/CPM_volumetric.py). Both classes share `_VolTail._tail`: base point, coordinate volumes, unprojection,
V2V and integration. Its class docstring says what differs: the centre maps, k + 1 heat maps with the background in
channel 0, and process_features run at stride 8 on the NHWC features before ONE hrnet_upsample_slice_nchw launch lifts
its 32 channels (hipnet/upsample_slice.py). get_pose_net picks the class by MODEL.NAME.
"""
import logging

import numpy as np
import torch
import torch.nn as nn

from hipnet import _capi as C
from hipnet import conv_kxk, conv_kxk_train, upsample_slice
from models import CPM_volumetric, pose_hrnet_volumetric
from models.v2v import V2VModel
from utils.heatmap_decoding import get_final_preds
from utils.multiview import triangulate_batch_of_points
from utils.volumetric import build_coord_volumes, integrate_tensor_3d_with_coordinates, unproject_heatmaps

logger = logging.getLogger(__name__)

BACKBONES = {'pose_hrnet_volumetric': pose_hrnet_volumetric}
CPM_BACKBONES = {'CPM_volumetric': CPM_volumetric}           # of VolumetricTriangulationNet_CPM only
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
    _check_vol(config, BACKBONES, 'pose_hrnet_volumetric')


def check_vol_cpm_config(config):
    """what VolumetricTriangulationNet_CPM refuses of a config, before anything is built: check_vol_config's rules on the
    CPM backbone, and MODEL.VOL_CONFIDENCES false"""
    _check_vol(config, CPM_BACKBONES, 'CPM_volumetric')
    if not config.MODEL.VOL_CONFIDENCES:
        raise ValueError('MODEL.VOL_CONFIDENCES false: the reference then hands the stride-8 features of CPM_volumetric to '
                         'projection matrices scaled for MODEL.HEATMAP_SIZE (its CPM_volumetric.py:216-218 up-samples them '
                         'only with the head present), which is geometrically wrong; both reference yamls set it true, and '
                         'so must this one (the head\'s parameters are held, it is never run)')


def _check_vol(config, backbones, backbone):
    method = config.MODEL.VOLUME_AGGREGATION_METHOD
    if not isinstance(method, str) or method.startswith('conf'):
        raise NotImplementedError('MODEL.VOLUME_AGGREGATION_METHOD {!r}: the confidence head of {} is '
                                  'not built, so the conf* aggregations have nothing to weigh with (sum, max and '
                                  'softmax are built)'.format(method, backbone))
    if method not in ('sum', 'max', 'softmax'):
        raise ValueError('Unknown volume_aggregation_method: {}'.format(method))
    size = config.MODEL.VOLUME_SIZE
    if not isinstance(size, int) or size < 32 or size % 32:
        raise ValueError('MODEL.VOLUME_SIZE {}: V2V pools five times and adds the results back to the skips, so the '
                         'volume side must be a multiple of 32'.format(size))
    if config.MODEL.BACKBONE_NAME not in backbones:
        raise ValueError('MODEL.BACKBONE_NAME {!r}: the volumetric model is built on {}'.format(
            config.MODEL.BACKBONE_NAME, ' / '.join(backbones)))
    if config.MODEL.ALG_CONFIDENCES:
        raise NotImplementedError('MODEL.ALG_CONFIDENCES true: {} does not build that head'.format(backbone))


class _VolTail(nn.Module):
    """what the volumetric models share after the backbone: theta's rule and `_tail` (base point, coordinate volumes,
    unprojection, V2V, integration). A subclass sets process_features, volume_net and the config's fields"""

    def _thetas(self, theta, B):
        if theta is None:
            return [float(np.random.uniform(0.0, 2 * np.pi)) for _ in range(B)] if self.training else 0.0
        return theta

    def _refuse_eval_grad(self, *tensors):
        if not self.training and torch.is_grad_enabled() and (
                any(t.requires_grad for t in tensors) or
                any(p.requires_grad for m in (self.process_features, self.volume_net) for p in m.parameters())):
            raise NotImplementedError('VolumetricTriangulationNet: eval mode with a gradient required is refused - the '
                                      'backward through the running statistics is not built; call .train(), or run '
                                      'under torch.no_grad()')

    def _tail(self, heatmaps, pose2d_pred, feats, proj_matrices, theta):
        """heatmaps (B * V, C, h, w) as they leave in the 7-tuple, pose2d_pred (B, V, K, 2) decoded from them, feats
        (B * V, 32, h, w) the processed features -> the 7-tuple of forward"""
        B, V = proj_matrices.shape[:2]
        with torch.no_grad():
            base_points = triangulate_batch_of_points(
                proj_matrices, pose2d_pred.detach()[:, :, BASE_JOINT:BASE_JOINT + 1].contiguous())[:, 0]     # (B, 3)
            coord_volumes = build_coord_volumes(base_points, self.cuboid_side, self.volume_size, self._thetas(theta, B))
        feats = feats.view(B, V, *feats.shape[1:])
        volumes = unproject_heatmaps(feats, proj_matrices.detach(), coord_volumes,
                                     volume_aggregation_method=self.volume_aggregation_method)
        volumes = self.volume_net(volumes)
        vol_keypoints_3d, volumes = integrate_tensor_3d_with_coordinates(
            volumes, coord_volumes, softmax=self.volume_softmax, multiplier=self.volume_multiplier)
        return (vol_keypoints_3d, pose2d_pred, heatmaps.view(B, V, *heatmaps.shape[1:]), volumes, None, coord_volumes,
                base_points)


class VolumetricTriangulationNet(_VolTail):
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
        self._refuse_eval_grad(heatmaps, features)
        K = heatmaps.shape[1]
        pose2d_pred = get_final_preds(heatmaps, use_softmax=self.heatmap_softmax).view(B, V, K, 2)
        feats = pointwise_conv_nchw(features, conv.weight, conv.bias)
        return self._tail(heatmaps, pose2d_pred, feats, proj_matrices, theta)

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


class _ProcessFeaturesFn(torch.autograd.Function):
    """y = Conv2d(Cin, Cout, 1)(x) on f32 NHWC, x a ReLU output: hrnet_conv2d_kxk with ks = 1. Backward: the weight and
    bias gradient (hrnet_conv2d_kxk_wgrad) and the data gradient with mask = x (hrnet_conv2d_kxk_dgrad), that is the
    gradient with respect to the ReLU's INPUT: the contract of CPM_volumetric.inter_feat"""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return _process(x, w, b)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous().float()
        dw = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = conv_kxk_train.conv_kxk_wgrad(x, gy, w.shape[0], 1)
        if ctx.needs_input_grad[0]:
            dx = conv_kxk_train.conv_kxk_dgrad(gy, conv_kxk_train.pack_dgrad(w, w.shape[0]), x.shape[3], 1, mask=x)
        return dx, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None


def process_features_nhwc(x, conv):
    """conv (a Conv2d with a 1x1 kernel and a bias) on x (N, h, w, Cin) f32 NHWC, the ReLU output CPM_volumetric hands on
    -> (N, h, w, Cout). Differentiable in x, weight and bias; the weight is packed from the parameter on every call, so
    nothing can go stale when an optimiser updates it"""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or not conv.weight.is_cuda:
        raise ValueError('process_features_nhwc: expected HIP-device tensors (there is no CPU path in this build)')
    if x.ndim != 4 or tuple(conv.weight.shape[1:]) != (x.shape[3], 1, 1) or conv.bias is None or x.shape[3] % 4 or \
            conv.weight.shape[0] % 4:
        raise ValueError('process_features_nhwc: x {}, weight {}: expected (N, h, w, Cin) and (Cout, Cin, 1, 1) with a bias, '
                         'Cin and Cout multiples of 4'.format(tuple(x.shape), tuple(conv.weight.shape)))
    if torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad or conv.bias.requires_grad):
        return _ProcessFeaturesFn.apply(x, conv.weight, conv.bias)
    return _process(x, conv.weight, conv.bias)


def _process(x, w, b):
    x = x.detach().contiguous()
    return conv_kxk.conv_kxk(x, conv_kxk.pack(w.detach(), x.shape[3]), w.shape[0], 1, bias=b.detach())


class VolumetricTriangulationNet_CPM(_VolTail):
    """MODEL.NAME `vol_CPM` (reference lib/models/triangulation.py:472-654): the volumetric model on the CPM_volumetric
    backbone.

        backbone (models/CPM_volumetric.py) on (B * V, 3, H, W) and the centre maps: k + 1 heat maps at HEATMAP_SIZE
                                        (channel 0 is the background) and the stride-8 NHWC features of Mconv4_stage6
        get_final_preds(heatmaps[:, 1:], HEATMAP_SOFTMAX)      (B, V, k, 2); joint 9 is the base joint
        process_features, Conv2d(128, 32, 1), AT STRIDE 8 on the NHWC features (hipnet.conv_kxk, ks = 1), then ONE
        hrnet_upsample_slice_nchw launch lifts the 32 channels to HEATMAP_SIZE NCHW
        `_tail`: the base point, coordinate volumes, unprojection, V2V and integration of VolumetricTriangulationNet

    The reference up-samples the 128 feature channels first and convolves at HEATMAP_SIZE (CPM_volumetric.py:217,
    triangulation.py:644). A 1x1 convolution with a bias commutes with bilinear up-sampling: every output is a weighted
    mean of four inputs whose weights sum to 1, so W (sum a_i x_i) + b = sum a_i (W x_i + b). The two orders are one
    function and agree to rounding; this order has 4x fewer multiply-adds at the reference's sizes and up-samples 32
    channels instead of 128. process_features.0.weight stays an ordinary (32, 128, 1, 1) parameter.

    Refused before any device work: check_vol_cpm_config (a conf* aggregation, a VOLUME_SIZE that is no multiple of 32,
    ALG_CONFIDENCES, a BACKBONE_NAME other than CPM_volumetric, MODEL.VOL_CONFIDENCES false); eval mode with a gradient
    required. With is_train the backbone is frozen except Mconv3/4/5_stage6 (:512-527). The other deviations are those of
    VolumetricTriangulationNet (module docstring)."""

    def __init__(self, config, is_train=True):
        super().__init__()
        check_vol_cpm_config(config)
        self.config = config
        self.num_joints = config.DATASET.NUM_JOINTS
        self.volume_aggregation_method = config.MODEL.VOLUME_AGGREGATION_METHOD
        self.volume_softmax = config.MODEL.VOLUME_SOFTMAX
        self.volume_multiplier = config.MODEL.VOLUME_MULTIPLIER
        self.volume_size = config.MODEL.VOLUME_SIZE
        self.cuboid_side = config.MODEL.CUBOID_SIZE
        self.heatmap_softmax = config.MODEL.HEATMAP_SOFTMAX
        self.use_gt_middleroot = config.MODEL.USE_GT_MIDDLEROOT

        self.backbone = CPM_volumetric.get_pose_net(config, is_train=is_train, trainable=is_train)
        if is_train:
            path = config.MODEL.BACKBONE_MODEL_PATH
            if path:
                checkpoint = torch.load(path, map_location='cpu')
                state = checkpoint['state_dict'] if 'state_dict' in checkpoint else checkpoint
                logger.info("=> Loading pretrained {} backbone from '{}'".format(config.MODEL.BACKBONE_NAME, path))
                state = {k.replace('module.', ''): v for k, v in state.items()}
                self.backbone.load_state_dict(state, strict=False)
            for p in self.backbone.parameters():
                p.requires_grad = False
            for name in CPM_volumetric.TRAINED:
                for p in getattr(self.backbone, name).parameters():
                    p.requires_grad = True

        self.process_features = nn.Sequential(nn.Conv2d(CPM_volumetric.INTER, 32, 1))
        self.volume_net = V2VModel(32, self.num_joints, trainable=is_train)

    def forward(self, images, centermaps, proj_matrices, batch=None, keypoints_3d=None, theta=None):
        """images (B, V, 3, H, W), centermaps (B, V, 1, H, W), proj_matrices (B, V, 3, 4) from world coordinates to heat-map
        pixels -> the 7-tuple of VolumetricTriangulationNet with heatmaps (B, V, k + 1, h, w) and pose2d_pred (B, V, k, 2);
        batch and keypoints_3d are accepted and unused, as in the reference"""
        tensors = (images, centermaps, proj_matrices)
        if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
            raise ValueError('VolumetricTriangulationNet_CPM: expected HIP-device tensors (there is no CPU path in this '
                             'build)')
        if images.ndim != 5 or tuple(proj_matrices.shape) != tuple(images.shape[:2]) + (3, 4) or \
                tuple(centermaps.shape) != tuple(images.shape[:2]) + (1,) + tuple(images.shape[3:]):
            raise ValueError('images {}, centermaps {} and proj_matrices {}: expected (B, V, 3, H, W), (B, V, 1, H, W) and '
                             '(B, V, 3, 4)'.format(tuple(images.shape), tuple(centermaps.shape),
                                                   tuple(proj_matrices.shape)))
        self._refuse_eval_grad(images, centermaps)
        B, V = images.shape[:2]
        outs = self.backbone(images.reshape(-1, *images.shape[2:]), centermaps.reshape(-1, *centermaps.shape[2:]))
        heatmaps = outs[5]
        y = process_features_nhwc(self.backbone.inter_feat(outs), self.process_features[0])
        feats = upsample_slice.upsample_slice(y, 0, y.shape[3], heatmaps.shape[2:])
        k = heatmaps.shape[1] - 1
        pose2d_pred = get_final_preds(heatmaps[:, 1:].contiguous(), use_softmax=self.heatmap_softmax).view(B, V, k, 2)
        return self._tail(heatmaps, pose2d_pred, feats, proj_matrices, theta)


def get_pose_net(cfg, is_train, **kwargs):
    if cfg.MODEL.NAME == 'vol_CPM':
        return VolumetricTriangulationNet_CPM(cfg, is_train=is_train)
    return VolumetricTriangulationNet(cfg, is_train=is_train)
