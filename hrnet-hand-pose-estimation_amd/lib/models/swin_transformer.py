"""SwinPose, MODEL.NAME `swin_transformer` (reference lib/models/swin_transformer.py:729-837): a Swin transformer over the
480-channel feature map of pose_hrnet_softmax (MODEL.BACKBONE_NAME 'pose_hrnet_softmax') or over the bare image
(BACKBONE_NAME ''), a decoder of transposed convolutions and a spatial softmax. Inference by default; SwinPose(config,
trainable=True) also trains (the last paragraph).

forward(x): x (B, 3, H, W)
  1. backbone -> features (B, 480, h, w) (slot 1 of pose_hrnet_softmax's output), or x itself                    :817-818
  2. patch embedding: Conv2d(Cin, E, p, stride p) on the map zero-padded to multiples of p, then LayerNorm(E)     :550-566
  3. four stages of DEPTHS[i] blocks at widths E 2^i with heads [3, 6, 12, 24] and 7x7 windows; block j of a stage has
     shift 0 (j even) or 3 (j odd); a block is x + proj(attn(norm1(x))), then x + fc2(gelu(fc1(norm2(x))))        :317-374
     stages 0 - 2 end in patch merging: 2x2 neighbours concatenated, LayerNorm(4 C), Linear(4 C -> 2 C, no bias)  :390-415
  4. norm3 on the last stage's output; norm0 - norm2 exist as parameters but are not computed (the reference computes
     and discards them, :820-821)                                                                                 :715-721
  5. decoder: log2(HEATMAP_SIZE / last map) steps of ConvTranspose2d(C, C / 2, 3, 2, 1, 1), Conv2d 1x1, eval-mode
     BatchNorm, ReLU; a final Conv2d 1x1 to NUM_JOINTS                                                            :784-811
  6. softmax(maps * trainable_temp) over the positions of each map                                                :824-827
returns (heatmap_pred (B, J, Hm, Wm), trainable_temp).

Every arithmetic step is a launch through the C ABI: hipnet.transformer (LayerNorm, linear with GELU / residual),
hipnet.swin (window attention in token order, the two gathers) and hipnet.nhwc (the decoder on the f32 NHWC convolution
entry). A block is
7 launches: LayerNorm, qkv, attention, proj + residual, LayerNorm, fc1 + GELU, fc2 + residual. The attention kernel finds
a window's tokens arithmetically: there is no partition, roll, pad or reverse pass, and the qkv linear runs on the unpadded
tokens only (a padded token's q, k, v are the qkv bias). The Swin output (B, H W, C) is the decoder's NHWC input as it is.
A decoder step is two launches: the transposed convolution is the zero-stuffed form of the convolution entry with the
weight packed as an input-gradient kernel, and the 1x1's bias, the BatchNorm and the ReLU are folded into a per-channel
scale and shift that the NEXT convolution applies when it loads its input. The packed decoder weights are built once and
rebuilt when a decoder parameter changes (load_state_dict, .cuda()). All other weights are read in place.

The holder modules are ordinary nn.Linear / nn.LayerNorm / nn.Conv2d / nn.BatchNorm2d under the reference's attribute
names, so state_dict() has the reference's keys in the reference's order and a reference checkpoint loads with
strict=True; their own forward is never used.

Refused when the model is built, each naming its key: MODEL.FF_TYPE other than 'mlp' (the LocalityFeedForward of the
reference's v1 / v2 yamls is not built), MODEL.ABSOLUTE_POSITION_ENCODING true, an EMB_DIM that is not a multiple of 3
(the head counts are [3, 6, 12, 24]: SwinPose does not pass NUM_HEADS, :765-773), a non-square IMAGE_SIZE / HEATMAP_SIZE
(the decoder arithmetic of :786-788 is square-only), a BACKBONE_NAME other than 'pose_hrnet_softmax' or ''.
Refused in forward: CPU tensors (ValueError); training mode, and eval mode with a gradient required (NotImplementedError:
the backward kernels and stochastic depth are not built - run model.eval() under torch.no_grad()).

MODEL.EMB_DIM may be an int, as the reference's yamls write it, or a one-element list, as the default is.

Training is opt-in: SwinPose(config, trainable=True, drop_path_rate=0.2) - get_pose_net(cfg, is_train, trainable=True) -
runs its training-mode forward on hipnet.swin_train and hipnet.transformer under autograd: the backbone in training mode
through its autograd anchor (the gradient enters on inter_feat and reaches stage4, the rest is frozen), the patch embedding,
the blocks with stochastic depth (block k has rate linspace(0, rate, sum(DEPTHS))[k]; each of its two branches draws a
per-sample keep flag and is scaled by flag / keep_prob; forward and head_forward also take the flags explicitly), patch
merging as gather, LayerNorm, linear, norm3, and the decoder on batch statistics with every activation materialised. Eval
mode under no_grad is the inference path above, on the running statistics that training left. Without trainable=True
nothing changes: training mode and eval mode with a gradient stay refused. WORLD_SIZE > 1 is refused.
"""
import logging
import math
import os

import torch
import torch.nn as nn

from hipnet import nhwc
from hipnet import swin as S
from hipnet import swin_train as ST
from hipnet import transformer as T

logger = logging.getLogger(__name__)

NUM_HEADS = (3, 6, 12, 24)
WINDOW = 7
MLP_RATIO = 4.
DROP_PATH_RATE = 0.2          # SwinTransformer's default: SwinPose does not pass it (:765-773)
NOT_BUILT = 'training of swin_transformer is not built'


def _unused(name):
    def forward(self, *a, **k):
        raise NotImplementedError('{} holds parameters of SwinPose; SwinPose.head_forward runs it through hipnet.swin and '
                                  'hipnet.transformer'.format(name))
    return forward


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features):
        super(Mlp, self).__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, in_features)

    forward = _unused('Mlp')


class WindowAttention(nn.Module):
    def __init__(self, dim, window_size, num_heads):
        super(WindowAttention, self).__init__()
        self.dim, self.window_size, self.num_heads = dim, window_size, num_heads
        self.scale = (dim // num_heads) ** -0.5
        ws = window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) * (2 * ws - 1), num_heads))
        # a buffer of the reference's state dict (:217-227); the kernel computes the same index arithmetically
        n = torch.arange(ws * ws)
        r, c = n // ws, n % ws
        self.register_buffer('relative_position_index',
                             (r[:, None] - r[None, :] + ws - 1) * (2 * ws - 1) + (c[:, None] - c[None, :] + ws - 1))
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)

    forward = _unused('WindowAttention')


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size, shift_size, drop_path=0.):
        super(SwinTransformerBlock, self).__init__()
        self.dim, self.num_heads, self.window_size, self.shift_size = dim, num_heads, window_size, shift_size
        self.drop_path = float(drop_path)
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, window_size, num_heads)
        self.norm2 = nn.LayerNorm(dim)
        self.feed_forward = Mlp(dim, int(dim * MLP_RATIO))

    forward = _unused('SwinTransformerBlock')

    def run(self, x, H, W):
        """x (B, H * W, dim) -> the same shape: 7 launches"""
        a, f = self.attn, self.feed_forward
        h = T.layer_norm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        h = T.linear(h, a.qkv.weight, a.qkv.bias)
        h = S.window_attention(h, a.qkv.bias, a.relative_position_bias_table, H, W, a.num_heads, self.window_size,
                               self.shift_size, a.scale)
        x = T.linear(h, a.proj.weight, a.proj.bias, residual=x)
        h = T.layer_norm(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        h = T.linear(h, f.fc1.weight, f.fc1.bias, act='gelu')
        return T.linear(h, f.fc2.weight, f.fc2.bias, residual=x)

    def run_train(self, x, H, W, scale_a, scale_m):
        """the same on the autograd ops; scale_a / scale_m: one stochastic-depth factor per ROW (B * H * W), or None"""
        a, f = self.attn, self.feed_forward
        h = T.layer_norm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        h = T.linear(h, a.qkv.weight, a.qkv.bias)
        h = ST.window_attention(h, a.qkv.bias, a.relative_position_bias_table, H, W, a.num_heads, self.window_size,
                                self.shift_size, a.scale)
        x = T.linear(h, a.proj.weight, a.proj.bias, residual=x, row_scale=scale_a)
        h = T.layer_norm(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        h = T.linear(h, f.fc1.weight, f.fc1.bias, act='gelu')
        return T.linear(h, f.fc2.weight, f.fc2.bias, residual=x, row_scale=scale_m)


class PatchMerging(nn.Module):
    def __init__(self, dim):
        super(PatchMerging, self).__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(4 * dim)

    forward = _unused('PatchMerging')

    def run(self, x, H, W):
        """x (B, H * W, dim) -> (B, ceil(H / 2) * ceil(W / 2), 2 dim): 2 launches"""
        return T.linear(S.merge_ln(x, H, W, self.norm.weight, self.norm.bias, self.norm.eps), self.reduction.weight)

    def run_train(self, x, H, W):
        """3 launches: the gather alone, the LayerNorm with its own backward, the linear layer"""
        h = T.layer_norm(ST.merge_gather(x, H, W), self.norm.weight, self.norm.bias, self.norm.eps)
        return T.linear(h, self.reduction.weight)


class BasicLayer(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size, downsample, drop_path=None):
        super(BasicLayer, self).__init__()
        self.window_size, self.shift_size, self.depth = window_size, window_size // 2, depth
        self.blocks = nn.ModuleList([SwinTransformerBlock(dim, num_heads, window_size,
                                                          0 if i % 2 == 0 else window_size // 2,
                                                          0. if drop_path is None else drop_path[i])
                                     for i in range(depth)])
        self.downsample = PatchMerging(dim) if downsample else None

    forward = _unused('BasicLayer')


class PatchEmbed(nn.Module):
    def __init__(self, patch_size, in_chans, embed_dim):
        super(PatchEmbed, self).__init__()
        self.patch_size, self.in_chans, self.embed_dim = patch_size, in_chans, embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = nn.LayerNorm(embed_dim)

    forward = _unused('PatchEmbed')

    def run(self, x):
        """NCHW x -> tokens (B, Hp * Wp, E), Hp, Wp: 3 launches"""
        rows, Hp, Wp = S.patch_rows(x, self.patch_size)
        t = T.linear(rows, self.proj.weight.reshape(self.embed_dim, -1), self.proj.bias)
        t = T.layer_norm(t, self.norm.weight, self.norm.bias, self.norm.eps)
        return t.reshape(x.shape[0], Hp * Wp, self.embed_dim), Hp, Wp

    def run_train(self, x):
        rows, Hp, Wp = ST.patch_rows(x, self.patch_size)
        t = T.linear(rows, self.proj.weight.reshape(self.embed_dim, -1), self.proj.bias)
        t = T.layer_norm(t, self.norm.weight, self.norm.bias, self.norm.eps)
        return t.reshape(x.shape[0], Hp * Wp, self.embed_dim), Hp, Wp


class SwinTransformer(nn.Module):
    def __init__(self, patch_size, in_chans, embed_dim, depths, drop_path_rate=0.):
        super(SwinTransformer, self).__init__()
        self.num_layers, self.embed_dim = len(depths), embed_dim
        self.patch_embed = PatchEmbed(patch_size, in_chans, embed_dim)
        self.pos_drop = nn.Dropout(p=0.)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]   # the rate of block k (:640)
        self.layers = nn.ModuleList([
            BasicLayer(embed_dim * 2 ** i, depths[i], NUM_HEADS[i], WINDOW, downsample=i < len(depths) - 1,
                       drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])])
            for i in range(len(depths))])
        self.num_features = [embed_dim * 2 ** i for i in range(len(depths))]
        for i in range(len(depths)):
            self.add_module('norm{}'.format(i), nn.LayerNorm(self.num_features[i]))

    forward = _unused('SwinTransformer')

    def run(self, x):
        """NCHW x -> the last stage's normalised output (B, H * W, C) and its H, W"""
        x, H, W = self.patch_embed.run(x)
        for i, layer in enumerate(self.layers):
            for blk in layer.blocks:
                x = blk.run(x, H, W)
            if layer.downsample is not None:
                x = layer.downsample.run(x, H, W)
                H, W = (H + 1) // 2, (W + 1) // 2
        last = getattr(self, 'norm{}'.format(self.num_layers - 1))
        return T.layer_norm(x, last.weight, last.bias, last.eps), H, W

    def blocks(self):
        return [blk for layer in self.layers for blk in layer.blocks]

    def run_train(self, x, flags):
        """run() on the autograd ops; flags: None, or two per-sample keep-flag tensors (B,) per block, attention branch
        first. A branch is scaled by flag / keep_prob (timm's DropPath); a block of rate 0 passes no row scale."""
        B = x.shape[0]
        x, H, W = self.patch_embed.run_train(x)
        k = 0
        for layer in self.layers:
            for blk in layer.blocks:
                sa = sm = None
                if flags is not None and blk.drop_path > 0.:
                    keep = 1.0 - blk.drop_path
                    sa, sm = ((flags[2 * k + t].float() / keep).repeat_interleave(H * W).contiguous() for t in range(2))
                x = blk.run_train(x, H, W, sa, sm)
                k += 1
            if layer.downsample is not None:
                x = layer.downsample.run_train(x, H, W)
                H, W = (H + 1) // 2, (W + 1) // 2
        last = getattr(self, 'norm{}'.format(self.num_layers - 1))
        return T.layer_norm(x, last.weight, last.bias, last.eps), H, W


def emb_dim(config):
    e = config.MODEL.EMB_DIM
    if isinstance(e, (list, tuple)):
        if len(e) != 1:
            raise ValueError('MODEL.EMB_DIM {}: swin_transformer takes one width (an int or a one-element list)'.format(e))
        e = e[0]
    return int(e)


def decoder_steps(config):
    """input size of the transformer, its input channels and the number of decoder steps (reference :733-739, :786-788)"""
    M = config.MODEL
    if M.BACKBONE_NAME:
        size, cin = int(M.HEATMAP_SIZE[0]), sum(M.EXTRA.STAGE4.NUM_CHANNELS)
    else:
        size, cin = int(M.IMAGE_SIZE[0]), 3
    expand = 2 ** (len(M.DEPTHS) - 1)
    last = size // int(M.PATCH_SIZE) // expand
    ratio = int(M.HEATMAP_SIZE[0]) // last if last > 0 else 0
    return size, cin, (int(math.log2(ratio)) if ratio >= 1 else 0)


def check_config(config):
    """what the model refuses of a config, before anything is built"""
    M = config.MODEL
    if M.FF_TYPE != 'mlp':
        raise ValueError('MODEL.FF_TYPE {!r}: only \'mlp\' is built (the LocalityFeedForward of FF_TYPE \'conv\' is '
                         'not)'.format(M.FF_TYPE))
    if M.ABSOLUTE_POSITION_ENCODING:
        raise ValueError('MODEL.ABSOLUTE_POSITION_ENCODING true: the absolute position embedding is not built')
    if M.BACKBONE_NAME not in ('', 'pose_hrnet_softmax'):
        raise ValueError('MODEL.BACKBONE_NAME {!r}: swin_transformer is built on \'pose_hrnet_softmax\' or on the bare '
                         'image (\'\')'.format(M.BACKBONE_NAME))
    e = emb_dim(config)
    if e < 3 or e % 3:
        raise ValueError('MODEL.EMB_DIM {}: must be a multiple of 3 (the stages have 3, 6, 12 and 24 heads)'.format(e))
    if len(M.DEPTHS) != len(NUM_HEADS) or any(int(d) < 1 for d in M.DEPTHS):
        raise ValueError('MODEL.DEPTHS {}: four stages of at least one block each'.format(list(M.DEPTHS)))
    if not S.supported(S.OP_ATTENTION, WINDOW, e // NUM_HEADS[0]):
        raise ValueError('MODEL.EMB_DIM {}: the head dimension {} is beyond the attention kernel'.format(e, e // 3))
    for key in ('IMAGE_SIZE', 'HEATMAP_SIZE'):
        v = list(M[key])
        if len(v) != 2 or v[0] != v[1]:
            raise ValueError('MODEL.{} {}: swin_transformer takes square sizes only (the decoder arithmetic is '
                             'square-only)'.format(key, v))
    if int(M.PATCH_SIZE) < 1:
        raise ValueError('MODEL.PATCH_SIZE {}: must be at least 1'.format(M.PATCH_SIZE))
    if decoder_steps(config)[2] < 1:
        raise ValueError('MODEL.PATCH_SIZE {} with MODEL.HEATMAP_SIZE {}: the decoder needs at least one upsampling '
                         'step'.format(M.PATCH_SIZE, list(M.HEATMAP_SIZE)))
    if int(M.NUM_JOINTS) != int(config.DATASET.NUM_JOINTS):
        raise ValueError('MODEL.NUM_JOINTS {} differs from DATASET.NUM_JOINTS {}'.format(M.NUM_JOINTS,
                                                                                         config.DATASET.NUM_JOINTS))


class SwinPose(nn.Module):
    autograd_grads = True      # a trainable model's gradients are autograd .grad tensors (utils.get_optimizer)

    def __init__(self, config, trainable=False, drop_path_rate=DROP_PATH_RATE):
        super(SwinPose, self).__init__()
        check_config(config)
        M = config.MODEL
        self.trainable = bool(trainable)
        if self.trainable and int(os.environ.get('WORLD_SIZE', '1')) > 1:
            raise ValueError('SwinPose(trainable=True): WORLD_SIZE = {}: data-parallel training of swin_transformer is '
                             'not built'.format(os.environ['WORLD_SIZE']))
        if not 0. <= float(drop_path_rate) < 1.:
            raise ValueError('drop_path_rate = {}: expected 0 <= rate < 1'.format(drop_path_rate))
        # own parameters precede the sub-modules in a state dict, as the reference's lists them
        self.trainable_temp = nn.Parameter(torch.tensor(1.0), requires_grad=bool(M.TRAINABLE_SOFTMAX))
        size, in_channel, steps = decoder_steps(config)
        if M.BACKBONE_NAME:
            from models import pose_hrnet_softmax
            self.backbone = pose_hrnet_softmax.get_pose_net(config, is_train=True)
            path = M.BACKBONE_MODEL_PATH
            if path:
                checkpoint = torch.load(path, map_location='cpu')
                state = checkpoint['state_dict'] if 'state_dict' in checkpoint else checkpoint
                logger.info("=> Loading pretrained {} backbone from '{}'".format(M.BACKBONE_NAME, path))
                state = {k.replace('module.', ''): v for k, v in state.items()}
                self.backbone.load_state_dict(state, strict=False)
            for p in self.backbone.parameters():              # freeze the lower layers (:760-763)
                p.requires_grad = False
            for p in self.backbone.stage4.parameters():
                p.requires_grad = True
        e = emb_dim(config)
        self.num_joints = int(config.DATASET.NUM_JOINTS)
        self.swinTransformer = SwinTransformer(int(M.PATCH_SIZE), in_channel, e, [int(d) for d in M.DEPTHS],
                                               float(drop_path_rate) if self.trainable else 0.)
        expand = 2 ** (len(M.DEPTHS) - 1)
        decoder = []
        for i in range(steps):
            cin, cout = e * expand // 2 ** i, e * expand // 2 ** (i + 1)
            decoder.extend([nn.ConvTranspose2d(cin, cout, 3, stride=2, padding=1, output_padding=1),
                            nn.Conv2d(cout, cout, kernel_size=1, stride=1, padding=0),
                            nn.BatchNorm2d(cout, momentum=0.1), nn.ReLU(inplace=False)])
        decoder.append(nn.Conv2d(decoder[-3].out_channels, self.num_joints, kernel_size=1, stride=1, padding=0))
        self.decoder = nn.Sequential(*decoder)
        self._plan, self._plan_key = None, None

    # ---- the decoder's packed weights ----------------------------------------------------------------------------
    def _decoder_plan(self):
        """packed weights and folded (scale, shift) of every decoder step; built once, rebuilt when a decoder parameter or
        buffer was written or moved"""
        tensors = list(self.decoder.parameters()) + list(self.decoder.buffers())
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        if self._plan is not None and key == self._plan_key:
            return self._plan
        mods = list(self.decoder)
        steps, cin_pad = [], mods[0].in_channels
        for i in range(0, len(mods) - 1, 4):
            up, conv, bn = mods[i], mods[i + 1], mods[i + 2]
            cop = nhwc.pad16(up.out_channels)
            scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
            shift = (conv.bias.detach().double() - bn.running_mean.detach().double()) * scale + bn.bias.detach().double()
            steps.append(dict(cout=cop, w_up=nhwc.conv_transpose_pack(up.weight, cin_pad, cop),
                              b_up=nhwc.padded(up.bias, cop), w_pw=nhwc.conv_pack(conv.weight, cop, cop),
                              affine=(nhwc.padded(scale, cop), nhwc.padded(shift, cop))))
            cin_pad = cop
        final = mods[-1]
        jp = nhwc.pad16(final.out_channels)
        self._plan = dict(steps=steps, jp=jp, w_final=nhwc.conv_pack(final.weight, cin_pad, jp),
                          b_final=nhwc.padded(final.bias, jp))
        self._plan_key = key
        return self._plan

    def decoder_forward(self, x, H, W):
        """x (B, H * W, C), the Swin output, read as NHWC -> heat maps (B, J, H 2^steps, W 2^steps)"""
        plan = self._decoder_plan()
        y = x.reshape(x.shape[0], H, W, x.shape[2])
        affine = None                 # the step before's folded BatchNorm, applied with its ReLU when the next one loads
        for st in plan['steps']:
            y = nhwc.conv_nhwc(y, st['w_up'], st['cout'], 3, up=True, bias=st['b_up'], in_affine=affine,
                               in_relu=affine is not None)
            y = nhwc.conv_nhwc(y, st['w_pw'], st['cout'], 1)
            affine = st['affine']
        y = nhwc.conv_nhwc(y, plan['w_final'], plan['jp'], 1, bias=plan['b_final'], in_affine=affine, in_relu=True)
        return nhwc.heatmap_softmax(y, self.num_joints, self.trainable_temp)

    # ---- the model -----------------------------------------------------------------------------------------------
    def _refuse(self, x):
        if self.training and not self.trainable:
            raise NotImplementedError('SwinPose: {} (the window-attention backward and stochastic depth are the next '
                                      'step): call .eval() and run under torch.no_grad()'.format(NOT_BUILT))
        if not self.training and torch.is_grad_enabled() and (getattr(x, 'requires_grad', False) or
                                                              any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('SwinPose: eval mode with a gradient required is refused - {}: run under '
                                      'torch.no_grad()'.format(NOT_BUILT))
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError('SwinPose: expected HIP-device tensors (there is no CPU path in this build)')

    # ---- training (trainable=True) -------------------------------------------------------------------------------
    def draw_drop_flags(self, B, device):
        """two keep-flag tensors (B,) per block, attention branch first, drawn on the device from torch's generator"""
        return [torch.empty(B, dtype=torch.float32, device=device).bernoulli_(1.0 - blk.drop_path)
                for blk in self.swinTransformer.blocks() for _ in range(2)]

    def decoder_train(self, x, H, W):
        """decoder_forward in training mode: every step's activation is materialised, the BatchNorms run on batch
        statistics and update their running ones, the packed weights are rebuilt from the parameters every call"""
        from models.pose_hrnet_softmax import _SpatialSoftmax
        mods = list(self.decoder)
        y = x.reshape(x.shape[0], H, W, x.shape[2])
        for i in range(0, len(mods) - 1, 4):
            y = ST.decoder_step(y, mods[i], mods[i + 1], mods[i + 2])
        self._plan = None                 # the running statistics were written through their pointers, not their version
        y = nhwc.to_nchw(nhwc.conv1x1_train(y, mods[-1]), self.num_joints)
        return _SpatialSoftmax.apply(y, self.trainable_temp)

    def _check_flags(self, drop_flags, B):
        n = 2 * len(self.swinTransformer.blocks())
        drop_flags = list(drop_flags)
        if len(drop_flags) != n or any(int(f.numel()) != B for f in drop_flags):
            raise ValueError('drop_flags: {} tensors of sizes {}: expected {} of size {}'.format(
                len(drop_flags), sorted({int(f.numel()) for f in drop_flags}), n, B))
        return drop_flags

    def head_forward(self, features, drop_flags=None):
        """features (B, Cin, H, W) NCHW on the device -> heat maps: everything after the backbone. In training mode of a
        trainable model drop_flags are the per-sample keep flags of draw_drop_flags (None: drawn here)"""
        self._refuse(features)
        pe = self.swinTransformer.patch_embed
        if features.ndim != 4 or features.shape[1] != pe.in_chans:
            raise ValueError('features {}: expected (B, {}, H, W)'.format(tuple(features.shape), pe.in_chans))
        if self.training:
            B = features.shape[0]
            flags = self.draw_drop_flags(B, features.device) if drop_flags is None else self._check_flags(drop_flags, B)
            x, H, W = self.swinTransformer.run_train(features.float(), flags)
            return self.decoder_train(x, H, W)
        if drop_flags is not None:
            raise ValueError('drop_flags are for training mode')
        with torch.no_grad():
            x, H, W = self.swinTransformer.run(features.float())
            return self.decoder_forward(x, H, W)

    def forward(self, x, drop_flags=None):
        self._refuse(x)
        if self.training:
            if hasattr(self, 'backbone'):
                # the backbone runs in training mode through its autograd anchor; the gradient enters on inter_feat and
                # reaches stage4 only (the rest is frozen)
                x = self.backbone(x)[1]
            return self.head_forward(x, drop_flags), self.trainable_temp
        with torch.no_grad():
            if hasattr(self, 'backbone'):
                x = self.backbone(x)[1]
        return self.head_forward(x), self.trainable_temp


def get_pose_net(cfg, is_train, **kwargs):
    return SwinPose(cfg, **kwargs)
