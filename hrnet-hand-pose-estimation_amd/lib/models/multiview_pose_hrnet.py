"""MultiViewPoseNet, MODEL.NAME `multiview_pose_hrnet` (reference lib/models/multiview_pose_hrnet.py): a 2-D backbone
run once on all B * V images, then the cross-view fusion layer: every view's heat maps are corrected by the other
views' maps through one learned Linear(h * w, h * w, bias=False) per ordered view pair,

    fused[b, i, k] = 0.4 * single[b, i, k] + 0.2 * sum over j != i of  single[b, j, k] @ W[n(i, j)]^T
    n(i, j) = i * (V - 1) + (rank of j among the views other than i)          the reference's running `index` (:57-71)

The whole layer is ONE hrnet_view_fusion launch forward and ONE hrnet_view_fusion_bwd call backward (csrc/view_fusion.hip)
behind one autograd function (`view_fusion`). The weights are read in place - nothing is packed or copied, so nothing goes
stale when an optimiser updates them - and a plain torch.optim.Adam drives the step.

The children carry the reference's attribute names: `backbone`, `aggre_layer.aggre.{0..11}.weight.weight` of shape (P, P),
P = MODEL.HEATMAP_SIZE[0] ** 2, always 12 of them (the reference builds 4 * 3 whatever the number of views), with
nn.Linear's default initialisation, so a reference checkpoint loads with strict=True. With V < 4 views the first
V * (V - 1) matrices are used, as the reference's running index does, and the others get no gradient (`.grad` stays None).
The backbone is frozen as the reference freezes it (:100-106): stage4 and last_layer train, the rest does not.

forward(views): (B, V, 3, H, W), or (V, 3, H, W) for B = 1 -> (fused, single), each (B * V, K, h, w); with MODEL.AGGRE
false only `single`.

Deviations from the reference, deliberate:
- rows are in this project's slot order b * V + v (what dataset/mhp.py's MHP_mv batches and utils/multiview.py use). The
  reference concatenates view-major (torch.cat over the views) and then pairs those rows with sample-major ground truth
  (lib/core/function.py:214-216); the two orders agree only at B = 1, the one batch size its config uses;
- the backbone checkpoint is loaded only when MODEL.BACKBONE_MODEL_PATH is set; the reference crashes without one
  (`state_dict` is unbound, :98);
- CPU tensors are refused with a ValueError: there is no CPU path;
- eval mode with a gradient required is refused (the backbone has no backward through its running statistics): run eval
  mode under torch.no_grad();
- the backbone is one of the 2-D backbones this project builds (pose_hrnet, pose_hrnet_softmax, pose_hrnet_volumetric),
  called once on (B * V, 3, H, W) rather than once per view.
"""
import ctypes
import logging

import torch
import torch.nn as nn

from hipnet import _capi as C
from models import pose_hrnet, pose_hrnet_softmax, pose_hrnet_volumetric

logger = logging.getLogger(__name__)

BACKBONES = {'pose_hrnet': pose_hrnet, 'pose_hrnet_softmax': pose_hrnet_softmax,
             'pose_hrnet_volumetric': pose_hrnet_volumetric}
NUM_VIEWS = 4                  # MHP's cameras: the reference always builds 4 * 3 matrices
NUM_NETS = NUM_VIEWS * (NUM_VIEWS - 1)
F32 = C.HR_F32


def pair_index(i, j, V):
    """n(i, j): the matrix that warps view j into target view i, for V views"""
    if not (0 <= i < V and 0 <= j < V and i != j):
        raise ValueError('pair_index: i = {}, j = {} of V = {} views'.format(i, j, V))
    return i * (V - 1) + (j if j < i else j - 1)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _fusion_forward(H, Ws, w_self, w_other):
    B, V, K = H.shape[:3]
    P = H[0, 0, 0].numel()
    F = torch.empty_like(H)
    with torch.cuda.device(H.device):
        C.call('hrnet_view_fusion', F32, H.data_ptr(), _ptr_array(Ws), F.data_ptr(), B, V, K, P, w_self, w_other,
               C.stream_ptr())
    return F


class _ViewFusionFn(torch.autograd.Function):
    """F = view_fusion(H, W_0 .. W_{V(V-1)-1}): hrnet_view_fusion; backward: one hrnet_view_fusion_bwd call for
    whichever of dH and the dW autograd asks for (neither half is computed or allocated for nothing)"""

    @staticmethod
    def forward(ctx, w_self, w_other, H, *Ws):
        ctx.save_for_backward(H, *Ws)
        ctx.mix = (w_self, w_other)
        return _fusion_forward(H, Ws, w_self, w_other)

    @staticmethod
    def backward(ctx, gF):
        H, Ws = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        need_h, need_w = ctx.needs_input_grad[2], ctx.needs_input_grad[3:]
        if not (need_h or any(need_w)):
            return (None,) * (3 + len(Ws))
        B, V, K = H.shape[:3]
        P = H[0, 0, 0].numel()
        gF = gF.contiguous().float()
        dH = torch.empty_like(H) if need_h else None
        dWs = [torch.empty_like(w) if n else None for w, n in zip(Ws, need_w)]
        with torch.cuda.device(H.device):
            C.call('hrnet_view_fusion_bwd', F32, H.data_ptr(), _ptr_array(Ws) if need_h else None, gF.data_ptr(),
                   C.ptr(dH), _ptr_array(dWs) if any(need_w) else None, B, V, K, P, ctx.mix[0], ctx.mix[1],
                   C.stream_ptr())
        return (None, None, dH) + tuple(dWs)


def view_fusion(H, weights, w_self=0.4, w_other=0.2):
    """H (B, V, K, h, w) or (B, V, K, P) float32 on the HIP device, weights: V * (V - 1) tensors (P, P) in n(i, j) order
    -> the fused maps, H's shape. Differentiable in H and in every weight."""
    weights = list(weights)
    if not isinstance(H, torch.Tensor) or not H.is_cuda or not all(isinstance(w, torch.Tensor) and w.is_cuda
                                                                    for w in weights):
        raise ValueError('view_fusion: expected HIP-device tensors (there is no CPU path in this build)')
    if H.ndim not in (4, 5) or min(H.shape) < 1:
        raise ValueError('view_fusion: H {}: expected (B, V, K, h, w) or (B, V, K, P), no empty axis'.format(
            tuple(H.shape)))
    V = H.shape[1]
    P = H[0, 0, 0].numel()
    if not C.call('hrnet_view_fusion_supported', F32, V, P):
        raise ValueError('view_fusion: V = {} views, P = {}: no kernel for this shape (2 <= V <= 4)'.format(V, P))
    if len(weights) != V * (V - 1) or any(tuple(w.shape) != (P, P) for w in weights):
        raise ValueError('view_fusion: {} weights of shapes {}: expected V * (V - 1) = {} of ({}, {})'.format(
            len(weights), sorted({tuple(w.shape) for w in weights}), V * (V - 1), P, P))
    if H.dtype != torch.float32 or any(w.dtype != torch.float32 for w in weights):
        raise ValueError('view_fusion: float32 only (bf16 weights are not built)')
    H = H.contiguous()
    weights = [w if w.is_contiguous() else w.contiguous() for w in weights]
    if torch.is_grad_enabled() and (H.requires_grad or any(w.requires_grad for w in weights)):
        return _ViewFusionFn.apply(float(w_self), float(w_other), H, *weights)
    return _fusion_forward(H.detach(), [w.detach() for w in weights], float(w_self), float(w_other))


class ChannelWiseFC(nn.Module):
    """the holder of one fusion matrix (reference :15-29); its own forward is one pair of the fused layer and is not
    used by Aggregation, which launches all pairs at once"""

    def __init__(self, size):
        super(ChannelWiseFC, self).__init__()
        self.weight = nn.Linear(size, size, bias=False)

    def forward(self, input):
        raise NotImplementedError('ChannelWiseFC holds one matrix of the fusion layer; Aggregation.forward runs all of '
                                  'them in one launch (models.multiview_pose_hrnet.view_fusion)')


class Aggregation(nn.Module):
    def __init__(self, cfg, weights=[0.4, 0.2, 0.2, 0.2]):
        super(Aggregation, self).__init__()
        size = cfg.MODEL.HEATMAP_SIZE[0]
        weights = [float(w) for w in weights]
        if len(weights) < 2 or any(w != weights[1] for w in weights[2:]):
            raise ValueError('Aggregation: weights {}: one weight for the own view and ONE for every other view is what '
                             'the fused kernel mixes'.format(weights))
        self.weights = weights
        self.aggre = nn.ModuleList()
        for _ in range(NUM_NETS):
            self.aggre.append(ChannelWiseFC(size * size))

    def forward(self, inputs):
        """inputs (B, V, K, h, w) -> (B, V, K, h, w)"""
        V = inputs.shape[1]
        if not 2 <= V <= NUM_VIEWS:
            raise ValueError('Aggregation: {} views: 2 to {} are built'.format(V, NUM_VIEWS))
        mats = [self.aggre[n].weight.weight for n in range(V * (V - 1))]
        return view_fusion(inputs, mats, self.weights[0], self.weights[1])


def check_fusion_config(config):
    """what the model refuses of a config, before anything is built"""
    if config.MODEL.BACKBONE_NAME not in BACKBONES:
        raise ValueError('MODEL.BACKBONE_NAME {!r}: multiview_pose_hrnet is built on {}'.format(
            config.MODEL.BACKBONE_NAME, ' / '.join(BACKBONES)))
    hm, im = list(config.MODEL.HEATMAP_SIZE), list(config.MODEL.IMAGE_SIZE)
    if len(hm) != 2 or hm[0] != hm[1] or hm[0] < 1:
        raise ValueError('MODEL.HEATMAP_SIZE {}: the fusion matrices are (h * w, h * w) of a square map'.format(hm))
    if len(im) != 2 or im[0] != 4 * hm[0] or im[1] != 4 * hm[1]:
        raise ValueError('MODEL.HEATMAP_SIZE {} is not MODEL.IMAGE_SIZE {} / 4, the backbone\'s stride'.format(hm, im))


class MultiViewPoseNet(nn.Module):
    def __init__(self, config):
        super(MultiViewPoseNet, self).__init__()
        check_fusion_config(config)
        self.config = config
        self.backbone = BACKBONES[config.MODEL.BACKBONE_NAME].get_pose_net(config, is_train=True)
        path = config.MODEL.BACKBONE_MODEL_PATH
        if path:
            checkpoint = torch.load(path, map_location='cpu')
            state = checkpoint['state_dict'] if 'state_dict' in checkpoint else checkpoint
            logger.info("=> Loading pretrained {} backbone from '{}'".format(config.MODEL.BACKBONE_NAME, path))
            state = {k.replace('module.', ''): v for k, v in state.items()}
            self.backbone.load_state_dict(state, strict=False)
        # freeze the lower layers (:100-106)
        for p in self.backbone.parameters():
            p.requires_grad = False
        for p in self.backbone.stage4.parameters():
            p.requires_grad = True
        for p in self.backbone.last_layer.parameters():
            p.requires_grad = True
        self.aggre_layer = Aggregation(config)

    def forward(self, views):
        if not isinstance(views, torch.Tensor) or not views.is_cuda:
            raise ValueError('MultiViewPoseNet: expected HIP-device tensors (there is no CPU path in this build)')
        if views.ndim == 4:
            views = views.unsqueeze(0)
        if views.ndim != 5:
            raise ValueError('views {}: expected (B, V, 3, H, W)'.format(tuple(views.shape)))
        if not self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError('MultiViewPoseNet: eval mode with a gradient required is refused - the backbone '
                                      'has no backward through its running statistics; call .train(), or run under '
                                      'torch.no_grad()')
        B, V = views.shape[:2]
        single = self.backbone(views.reshape(B * V, *views.shape[2:]))[0]           # (B * V, K, h, w), slot b * V + v
        if not self.config.MODEL.AGGRE:
            return single
        fused = self.aggre_layer(single.view(B, V, *single.shape[1:]))
        return fused.view(B * V, *single.shape[1:]), single


def get_pose_net(cfg, is_train=None, **kwargs):
    return MultiViewPoseNet(cfg, **kwargs)
