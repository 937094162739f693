"""PoseTransformer, MODEL.NAME `pose_hrnet_transformer` (reference lib/models/pose_hrnet_transformer.py): the reference's
PoseFormer variant. A 2-D backbone gives heat maps for every frame of a window, the soft-argmax turns them into poses,
and a spatial transformer over the joints of a frame followed by a temporal transformer over the frames of a window
refines the pose of the centre frame.

Constants (reference :106-121): F = len(DATASET.SEQ_IDX) frames, J = DATASET.NUM_JOINTS joints, spatial width 32,
temporal width D = 32 J, depth 4, 8 heads, mlp_ratio 2, qkv_bias, attention scale head_dim ** -0.5, all dropouts 0,
stochastic-depth rates linspace(0, 0.2, 4) shared by spatial block i and temporal block i (:169-181); every LayerNorm has
eps 1e-6 (:119) except head.0, a plain nn.LayerNorm (:190).

forward(x): x (S, F, 3, H, W), one view's window per sequence (:224-237)
  1. backbone on the S F images -> heat maps (S F, J, h, w)                                      :227
  2. get_final_preds(use_softmax=MODEL.HEATMAP_SOFTMAX) -> p (S, F, J, 2) in heat-map pixels      :229
  3. spatial encoder on S F sequences of J tokens: Linear(2 -> 32)(p) + Spatial_pos_embed, 4 blocks, Spatial_norm, the
     J tokens of a frame concatenated joint-major -> (S, F, D)                                    :195-208
  4. temporal encoder on S sequences of F tokens: + Temporal_pos_embed, 4 blocks, Temporal_norm, weighted_mean (a
     Conv1d(F -> 1, kernel 1): out[s] = sum_f w[f] x[s, f] + b) -> (S, 1, D)                      :210-221
  5. head: LayerNorm(D), Linear(D -> 2 J) -> (S, J, 2)                                            :189-192, :235
  a block is x + dp(attn(norm1(x))), then x + dp(mlp(norm2(x)))                                   :82-85
returns (pose (S, J, 2), heatmaps (S F, J, h, w), trainable_temp).

Every arithmetic step of the head is a launch through the C ABI (hipnet.transformer over csrc/transformer.hip): 7 per
block - LayerNorm, qkv, attention, proj + residual, LayerNorm, fc1 + GELU, fc2 + residual - with the stochastic-depth
factor entering proj and fc2 as a per-row scale. The holder modules are ordinary nn.Linear / nn.LayerNorm / nn.Conv1d
under the reference's attribute names, so state_dict() has the reference's keys in the reference's order and a reference
checkpoint loads with strict=True; their own forward is never used. Torch only draws the keep flags and reshapes.

Stochastic depth (`dp`, timm's DropPath): the identity in eval mode; in training with rate r > 0 one Bernoulli(1 - r)
keep flag per sequence, drawn independently for each of the two branches of a block; a kept sequence's branch output is
divided by 1 - r, a dropped one is zero. timm is not available to this project's tests, so this follows its documented
behaviour and is UNPINNED against the library. `drop_flags=` passes the 16 flag tensors explicitly (spatial blocks then
temporal blocks, two per block: attention branch, mlp branch; S F values for a spatial block, S for a temporal one).

Inputs: (S, F, 3, H, W) as the reference, or the MHP_seq loader's frame-major batch (F S, 3, H, W) with `frames=F`
(slot f * S + s, dataset/mhp.py): the backbone then runs in the loader's order and only the (F S, J, 2) poses are
reordered - the images are never copied. In that case the returned heat maps are in the loader's order too.

Freezing when is_train (reference :126-159): the backbone checkpoint MODEL.BACKBONE_MODEL_PATH, when set, is loaded
non-strictly with `module.` stripped; the backbone is frozen except stage4 and last_layer; trainable_temp is frozen.

Deviations from the reference, deliberate:
- pose_hrnet_softmax returns a 3-tuple here (heat maps, features, temperature); the heat maps are slot 0 and the
  temperature the last slot (the reference unpacks two, :227); a backbone without a temperature gives None;
- MODEL.INIT_WEIGHTS true is refused: the reference would call an init_weights that does not exist (:243-244);
- F or J outside the attention kernel's range (1 .. 64 tokens) is refused when the model is built;
- CPU tensors are refused with a ValueError: there is no CPU path;
- eval mode with a gradient required is refused (the backbone has no backward through its running statistics): run eval
  mode under torch.no_grad();
- the backbone is one of the 2-D backbones this project builds (models.multiview_pose_hrnet.BACKBONES).
"""
import logging

import torch
import torch.nn as nn

from hipnet import transformer as T
from models.multiview_pose_hrnet import BACKBONES

logger = logging.getLogger(__name__)

EMBED_DIM_RATIO = 32
DEPTH = 4
NUM_HEADS = 8
MLP_RATIO = 2.
DROP_PATH_RATE = 0.2
NORM_EPS = 1e-6
MAX_TOKENS = 64                # hrnet_tf_supported(HR_TF_ATTENTION, N, hd): 1 <= N <= 64, hd <= 128
MAX_HEAD_DIM = 128


def _unused(name):
    def forward(self, *a, **k):
        raise NotImplementedError('{} holds parameters of the PoseFormer head; PoseTransformer.head_forward runs it '
                                  'through hipnet.transformer'.format(name))
    return forward


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features):
        super(Mlp, self).__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, in_features)

    forward = _unused('Mlp')


class Attention(nn.Module):
    def __init__(self, dim, num_heads):
        super(Attention, self).__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.proj = nn.Linear(dim, dim)

    forward = _unused('Attention')


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, drop_path):
        super(Block, self).__init__()
        self.norm1 = nn.LayerNorm(dim, eps=NORM_EPS)
        self.attn = Attention(dim, num_heads)
        self.drop_path = float(drop_path)
        self.norm2 = nn.LayerNorm(dim, eps=NORM_EPS)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    forward = _unused('Block')

    def run(self, x, scale_a, scale_m):
        """x (sequences, N, dim); scale_a / scale_m: one stochastic-depth factor per ROW (sequences * N), or None"""
        a = self.attn
        h = T.layer_norm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        h = T.attention(T.linear(h, a.qkv.weight, a.qkv.bias), a.num_heads, a.scale)
        x = T.linear(h, a.proj.weight, a.proj.bias, residual=x, row_scale=scale_a)
        h = T.layer_norm(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        h = T.linear(h, self.mlp.fc1.weight, self.mlp.fc1.bias, act='gelu')
        return T.linear(h, self.mlp.fc2.weight, self.mlp.fc2.bias, residual=x, row_scale=scale_m)


def check_config(config):
    """what the model refuses of a config, before anything is built"""
    if config.MODEL.BACKBONE_NAME not in BACKBONES:
        raise ValueError('MODEL.BACKBONE_NAME {!r}: pose_hrnet_transformer is built on {}'.format(
            config.MODEL.BACKBONE_NAME, ' / '.join(BACKBONES)))
    F, J = len(config.DATASET.SEQ_IDX), int(config.DATASET.NUM_JOINTS)
    if not 1 <= F <= MAX_TOKENS:
        raise ValueError('DATASET.SEQ_IDX has {} frames: the attention kernel takes 1 to {} tokens'.format(F, MAX_TOKENS))
    if not 1 <= J <= MAX_TOKENS:
        raise ValueError('DATASET.NUM_JOINTS {}: the attention kernel takes 1 to {} tokens'.format(J, MAX_TOKENS))
    if EMBED_DIM_RATIO * J // NUM_HEADS > MAX_HEAD_DIM:
        raise ValueError('DATASET.NUM_JOINTS {}: the temporal head dimension {} is beyond the attention kernel\'s '
                         '{}'.format(J, EMBED_DIM_RATIO * J // NUM_HEADS, MAX_HEAD_DIM))
    if int(config.MODEL.NUM_JOINTS) != J:
        raise ValueError('MODEL.NUM_JOINTS {} differs from DATASET.NUM_JOINTS {}'.format(config.MODEL.NUM_JOINTS, J))


class PoseTransformer(nn.Module):
    autograd_grads = True      # the head's gradients are autograd .grad tensors (utils.get_optimizer)

    def __init__(self, config, is_train):
        super(PoseTransformer, self).__init__()
        check_config(config)
        num_frame = len(config.DATASET.SEQ_IDX)
        num_joints = int(config.DATASET.NUM_JOINTS)
        embed_dim = EMBED_DIM_RATIO * num_joints
        self.num_frame, self.num_joints, self.embed_dim = num_frame, num_joints, embed_dim
        self.use_softmax = bool(config.MODEL.HEATMAP_SOFTMAX)
        # own parameters precede the sub-modules in a state dict: both position embeddings are registered first, as the
        # reference's state dict lists them
        self.Spatial_pos_embed = nn.Parameter(torch.zeros(1, num_joints, EMBED_DIM_RATIO))
        self.Temporal_pos_embed = nn.Parameter(torch.zeros(1, num_frame, embed_dim))
        self.backbone = BACKBONES[config.MODEL.BACKBONE_NAME].get_pose_net(config, is_train=True)
        if is_train:
            path = config.MODEL.BACKBONE_MODEL_PATH
            if path:
                checkpoint = torch.load(path, map_location='cpu')
                state = checkpoint['state_dict'] if 'state_dict' in checkpoint else checkpoint
                logger.info("=> Loading pretrained {} backbone from '{}'".format(config.MODEL.BACKBONE_NAME, path))
                state = {k.replace('module.', ''): v for k, v in state.items()}
                self.backbone.load_state_dict(state, strict=False)
            for p in self.backbone.parameters():          # freeze the lower layers (:146-159)
                p.requires_grad = False
            for p in self.backbone.stage4.parameters():
                p.requires_grad = True
            for p in self.backbone.last_layer.parameters():
                p.requires_grad = True
            if getattr(self.backbone, 'trainable_temp', None) is not None:
                self.backbone.trainable_temp.requires_grad = False
        self.Spatial_patch_to_embedding = nn.Linear(2, EMBED_DIM_RATIO)
        dpr = [x.item() for x in torch.linspace(0, DROP_PATH_RATE, DEPTH)]
        self.Spatial_blocks = nn.ModuleList([Block(EMBED_DIM_RATIO, NUM_HEADS, MLP_RATIO, dpr[i]) for i in range(DEPTH)])
        self.blocks = nn.ModuleList([Block(embed_dim, NUM_HEADS, MLP_RATIO, dpr[i]) for i in range(DEPTH)])
        self.Spatial_norm = nn.LayerNorm(EMBED_DIM_RATIO, eps=NORM_EPS)
        self.Temporal_norm = nn.LayerNorm(embed_dim, eps=NORM_EPS)
        self.weighted_mean = nn.Conv1d(in_channels=num_frame, out_channels=1, kernel_size=1)
        self.head = nn.Sequential(nn.LayerNorm(embed_dim), nn.Linear(embed_dim, num_joints * 2))

    # ---- the head ------------------------------------------------------------------------------------------------
    def draw_drop_flags(self, S, device):
        """16 keep-flag tensors, spatial then temporal, two per block, drawn on the device (a rate of 0 keeps all)"""
        flags = []
        for blocks, n in ((self.Spatial_blocks, S * self.num_frame), (self.blocks, S)):
            for blk in blocks:
                for _ in range(2):
                    flags.append(torch.empty(n, dtype=torch.float32, device=device).bernoulli_(1.0 - blk.drop_path))
        return flags

    def _row_scales(self, blk, flags, idx, tokens):
        if flags is None or blk.drop_path == 0.:          # a rate of 0 keeps every sequence (timm builds no DropPath)
            return None, None
        keep = 1.0 - blk.drop_path
        return tuple((flags[idx + k].float() / keep).repeat_interleave(tokens).contiguous() for k in range(2))

    def head_forward(self, p, drop_flags=None):
        """p (S, F, J, 2) poses in heat-map pixels on the device -> (S, J, 2): steps 3-5 of the module docstring.
        drop_flags None: the identity in eval mode, drawn in training mode"""
        if not isinstance(p, torch.Tensor) or not p.is_cuda:
            raise ValueError('PoseTransformer: expected HIP-device tensors (there is no CPU path in this build)')
        S, F, J = p.shape[:3]
        if p.ndim != 4 or p.shape[3] != 2 or F != self.num_frame or J != self.num_joints:
            raise ValueError('poses {}: expected (S, {}, {}, 2)'.format(tuple(p.shape), self.num_frame, self.num_joints))
        if drop_flags is None and self.training:
            drop_flags = self.draw_drop_flags(S, p.device)
        if drop_flags is not None:
            drop_flags = list(drop_flags)
            want = [S * F] * (2 * DEPTH) + [S] * (2 * DEPTH)
            if [int(f.numel()) for f in drop_flags] != want:
                raise ValueError('drop_flags: {} tensors of sizes {}: expected 16 of sizes {}'.format(
                    len(drop_flags), [int(f.numel()) for f in drop_flags], want))
        pe = self.Spatial_patch_to_embedding
        x = T.linear(p.reshape(S * F * J, 2).float(), pe.weight, pe.bias)
        x = T.add_rows(x, self.Spatial_pos_embed[0]).reshape(S * F, J, EMBED_DIM_RATIO)
        for i, blk in enumerate(self.Spatial_blocks):
            x = blk.run(x, *self._row_scales(blk, drop_flags, 2 * i, J))
        x = T.layer_norm(x, self.Spatial_norm.weight, self.Spatial_norm.bias, self.Spatial_norm.eps)
        # '(b f) w c -> b f (w c)': rows are already (s, f, j)-ordered, the concatenation is a view
        x = T.add_rows(x.reshape(S * F, self.embed_dim), self.Temporal_pos_embed[0]).reshape(S, F, self.embed_dim)
        for i, blk in enumerate(self.blocks):
            x = blk.run(x, *self._row_scales(blk, drop_flags, 2 * DEPTH + 2 * i, F))
        x = T.layer_norm(x, self.Temporal_norm.weight, self.Temporal_norm.bias, self.Temporal_norm.eps)
        x = T.frame_mean(x, self.weighted_mean.weight, self.weighted_mean.bias)             # (S, D)
        x = T.layer_norm(x, self.head[0].weight, self.head[0].bias, self.head[0].eps)
        return T.linear(x, self.head[1].weight, self.head[1].bias).reshape(S, J, 2)

    # ---- the model -----------------------------------------------------------------------------------------------
    def forward(self, x, frames=None, drop_flags=None):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError('PoseTransformer: expected HIP-device tensors (there is no CPU path in this build)')
        if not self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError('PoseTransformer: eval mode with a gradient required is refused - the backbone '
                                      'has no backward through its running statistics; call .train(), or run under '
                                      'torch.no_grad()')
        F = self.num_frame
        if frames is None:
            if x.ndim != 5 or x.shape[1] != F:
                raise ValueError('x {}: expected (S, {}, 3, H, W), or the frame-major batch (F * S, 3, H, W) with '
                                 'frames={}'.format(tuple(x.shape), F, F))
            S = x.shape[0]
            images = x.reshape(S * F, *x.shape[2:])
        else:
            if int(frames) != F or x.ndim != 4 or x.shape[0] % F:
                raise ValueError('x {} with frames={}: expected ({} * S, 3, H, W), frame-major'.format(
                    tuple(x.shape), frames, F))
            S = x.shape[0] // F
            images = x
        outputs = self.backbone(images)
        heatmaps = outputs[0]
        temp = outputs[-1] if len(outputs) == 3 else None
        from utils.heatmap_decoding import get_final_preds
        p = get_final_preds(heatmaps, use_softmax=self.use_softmax)                          # (S F, J, 2)
        J = p.shape[1]
        if frames is None:
            p = p.reshape(S, F, J, 2)
        else:
            p = p.reshape(F, S, J, 2).permute(1, 0, 2, 3).contiguous()                       # poses only
        return self.head_forward(p, drop_flags), heatmaps, temp


def get_pose_net(cfg, is_train, **kwargs):
    if is_train and cfg.MODEL.INIT_WEIGHTS:
        raise ValueError('MODEL.INIT_WEIGHTS true: pose_hrnet_transformer has no init_weights (the reference would fail '
                         'on the call, pose_hrnet_transformer.py:243-244); set it to false and give the backbone\'s '
                         'checkpoint as MODEL.BACKBONE_MODEL_PATH')
    return PoseTransformer(cfg, is_train, **kwargs)
