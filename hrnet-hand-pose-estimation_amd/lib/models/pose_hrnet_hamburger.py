"""HamNet, MODEL.NAME `pose_hrnet_hamburger` (reference lib/models/pose_hrnet_hamburger.py:17-84 with
lib/models/hamburger/burger.py:123-201 HamburgerV2Plus, ham.py:14-117, :227-269 NMF2D and bread.py:20-49): a Hamburger
block - a non-negative matrix factorisation of the feature map between two 1x1 convolutions - on the 480-channel features
of pose_hrnet_softmax, and a spatial softmax. HamNet(cfg) is inference only; HamNet(cfg, is_train, trainable=True) also
trains its head (TRAINING below).

forward(x): x (B, 3, H, W)
  1. backbone -> features (B, 480, h, w) (slot 1 of pose_hrnet_softmax's output)                         hamburger.py:69
  2. squeeze: Conv2d 3x3 480 -> E (no bias), BatchNorm on running statistics, ReLU; E = MODEL.EMB_DIM            :56, :73
  3. hamburger (V2+): lower_bread Conv2d 1x1 E -> C (bias) + ReLU, C = S E (2 S E with DUAL_HAM); the ham(s): with
     DUAL_HAM the first C / 2 channels go through ham_1 (spatial), the last through ham_2 (not), else all C through ham
     (MODEL.SPATIAL); cheese Conv2d 1x1 C -> C / f (no bias) + BatchNorm + ReLU, f = CHEESE_FACTOR (doubled when dual);
     upper_bread Conv2d 1x1 C / f -> E (no bias); out = relu(coef_ham * x + coef_shortcut * shortcut)       burger.py:183-201
  4. align: Conv2d 3x3 E -> 256 (no bias), BatchNorm, ReLU; fc: Dropout2d (identity here), Conv2d 1x1 256 -> J   :61-63
  5. softmax(maps * trainable_temp) over the positions of each map                                               :79-82
returns (heatmap_pred (B, J, h, w), trainable_temp).

A ham (NMF2D in eval mode) reads its channels as G = B S matrices X (D, N) - spatial: D = channels / S, N = h w; not
spatial: D = h w, N = channels / S - draws bases (G, D, R) with torch.rand on the HOST from the global CPU generator (ham_1
before ham_2), normalises them along D, and runs
    coef = softmax_R(X^T bases); EVAL_STEPS times {coef *= X^T bases / (coef bases^T bases + 1e-6);
    bases *= X coef / (bases coef^T coef + 1e-6)}; one more coef update; out = bases coef^T.
MODEL.INV_T has no effect (NMF2D sets its inv_t to 1, ham.py:231).

Every product is a launch through the C ABI. The head runs NHWC: the features are turned once (hrnet_nchw_to_nhwc), and
the hams are hipnet.nmf on views of lower_bread's output - the spatial ham reads its channel half as X^T, the other as X,
nothing is copied - and write their reconstructions straight into their channels of the cheese input (no cat). The
convolutions, all f32 on existing entries:
  squeeze, align   the 3x3 as nine 1x1 launches over displaced windows that accumulate (hrnet_conv2d_dilated3x3, dilation
                   1): nine sums of 480 / 512 terms in place of hrnet_conv2d's single chain of 4320 / 4608, whose error
                   alone was 2.5e-6 / 2.0e-6 of max|.| at full size against 6.6e-7 / 5.4e-7 this way
  lower_bread, upper_bread, fc   hrnet_conv2d 1x1 on packed weights, bias in the launch
  cheese           a plain product of the NMF engine, pixels x (C, C / f), the ham outputs read in place (a 1024-term sum
                   in chunks of 256; hrnet_conv2d's chain gave 1.7e-6)
An eval-mode BatchNorm is a folded (scale, shift) that the CONSUMER applies with the ReLU when it loads its input
(hrnet_conv2d's in_scale / in_shift / in_relu). What stays in torch, small element-wise launches: the ReLU of lower_bread's
output (the hams read it thirteen times, the convolution entry has no output activation); coef_shortcut *
relu(bn(squeeze)) (addcmul, relu_, mul_; upper_bread, its weight scaled by coef_ham when it is packed, then ACCUMULATES
into that buffer) and the block's closing relu_ (the tap-wise align has no prologue); and the L2-normalisation of the fresh
bases. The packed weights are built once and rebuilt when a head parameter or buffer changes (load_state_dict, .cuda()).

The holder modules are ordinary nn.Conv2d / nn.BatchNorm2d under the reference's attribute names, so state_dict() has
the reference's keys in the reference's order and a reference checkpoint loads with strict=True; their own forward is never
used.

Refused when the model is built, each naming its key: MODEL.HAM_TYPE other than 'NMF' (VQ and CD are not built),
MODEL.VERSION other than 'V2+', MODEL.RAND_INIT false (the persistent bases buffer and its online update), a
MODEL.BACKBONE_NAME without 'hrnet' (the ResNet backbone), MODEL.COMPUTE_DTYPE other than fp32, an S, R, EMB_DIM,
CHEESE_FACTOR or EVAL_STEPS that does not fit. Refused in forward: CPU tensors (ValueError); without trainable=True training
mode, and in every model eval mode with a gradient required (NotImplementedError - run model.eval() under
torch.no_grad()).

TRAINING (trainable=True; tools/train_hamburger.py). In training mode head_forward(features, bases=None, drop_keep=None)
runs under autograd on hipnet.burger_train and hipnet.nmf_train: squeeze, lower_bread, the hams on MODEL.TRAIN_STEPS with
the bases drawn as above, cheese, upper_bread, the mix relu(coef_ham x + coef_shortcut shortcut) (hrnet_burger_mix: its
backward forms both map gradients and the two scalar ones in one pass, the sums in double in a fixed order), align,
Dropout2d(0.1) on the keep mask of draw_drop_keep (hrnet_dropout2d), fc and the spatial softmax. Every activation is
materialised; the BatchNorms run on batch statistics and move their running ones with momentum 3e-4 through their
pointers (so the packed plan is dropped after a training forward; num_batches_tracked is NOT incremented: the
reference's SyncBN calls F.batch_norm directly and its counter stays 0); the packed weights are rebuilt on every call.
  The ham's gradient needs no kernel of its own: the reference runs the TRAIN_STEPS updates under torch.no_grad()
(ham.py:48-58), so only compute_coef and the closing bmm carry one (ham.py:90-93, :261-269). With bases_T, coef_T the
factors after TRAIN_STEPS updates and Gm = bases_T^T bases_T: dnum = coef_T * (dY^T bases_T) / (coef_T Gm + 1e-6) is
hrnet_nmf_update with dY where X sits, dX = bases_T dnum^T is hrnet_nmf_reconstruct into the gradient's own strided view
(1.4e-16 of max|dX| against autograd through the reference's NMF2D in float64). A single fused launch would save one
(G, N, R) round trip, 8 MB at full size, against about 6 GFLOP of products, and was not built. The bases get no gradient.
  The backbone keeps every parameter frozen and runs under torch.no_grad() in whatever mode the module is in: no
gradient enters it and its parameters never get a .grad, but model.train() puts its BatchNorms on batch statistics, as
in the reference (which freezes the parameters and leaves the mode alone). features.requires_grad is honoured by
head_forward: squeeze then forms its input gradient. Eval mode under no_grad is the inference path above, on EVAL_STEPS
and on the statistics that training left. WORLD_SIZE > 1 is refused when the trainable model is built.
"""
import logging
import os

import torch
import torch.nn as nn

from hipnet import burger_train as BT
from hipnet import nhwc
from hipnet import nmf as N
from hipnet import nmf_train as NT

logger = logging.getLogger(__name__)

NOT_BUILT = 'training of pose_hrnet_hamburger is not built'
ALIGN_CHANNELS = 256
BN_MOMENTUM = 3e-4            # bread.py:17


def _unused(name):
    def forward(self, *a, **k):
        raise NotImplementedError('{} holds parameters of HamNet; HamNet.head_forward runs it through hipnet.nmf and the '
                                  'convolution entry'.format(name))
    return forward


class ConvBNReLU(nn.Module):
    def __init__(self, in_c, out_c, kernel_size=1):
        super(ConvBNReLU, self).__init__()
        self.conv = nn.Conv2d(in_c, out_c, kernel_size=kernel_size, stride=1, padding=kernel_size // 2, bias=False)
        self.bn = nn.BatchNorm2d(out_c, momentum=BN_MOMENTUM)
        self.act = nn.ReLU(inplace=True)

    forward = _unused('ConvBNReLU')


class NMF2D(nn.Module):
    """holds the sizes of one ham; no parameters, and with RAND_INIT no buffers"""

    def __init__(self, spatial, S_, R, steps):
        super(NMF2D, self).__init__()
        self.spatial, self.S, self.R, self.eval_steps = bool(spatial), int(S_), int(R), int(steps)

    forward = _unused('NMF2D')

    def sizes(self, B, channels, hw):
        """(G, D, N) of this ham on `channels` channels of an hw-pixel map"""
        per = channels // self.S
        return (B * self.S, per, hw) if self.spatial else (B * self.S, hw, per)


class HamburgerV2Plus(nn.Module):
    def __init__(self, config, in_c):
        super(HamburgerV2Plus, self).__init__()
        M = config.MODEL
        S_, D, R, steps = int(M.S), emb_dim(config), int(M.R), int(M.EVAL_STEPS)
        self.dual = bool(M.DUAL_HAM)
        C_ = S_ * D * (2 if self.dual else 1)
        # own parameters precede the sub-modules in a state dict, as the reference's lists them
        self.coef_shortcut = nn.Parameter(torch.tensor([1.]))
        self.coef_ham = nn.Parameter(torch.tensor([0. if M.ZERO_HAM else 1.]))
        self.lower_bread = nn.Sequential(nn.Conv2d(in_c, C_, 1), nn.ReLU(inplace=True))
        if self.dual:
            self.ham_1 = NMF2D(True, S_, R, steps)
            self.ham_2 = NMF2D(False, S_, R, steps)
        else:
            self.ham = NMF2D(M.SPATIAL, S_, R, steps)
        factor = int(M.CHEESE_FACTOR) * (2 if self.dual else 1)
        self.channels, self.mid = C_, C_ // factor
        self.cheese = ConvBNReLU(C_, C_ // factor)
        self.upper_bread = nn.Conv2d(C_ // factor, in_c, 1, bias=False)
        self.shortcut = nn.Sequential()
        for m in self.modules():                       # burger.py:173-181
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, (2. / n) ** 0.5)

    forward = _unused('HamburgerV2Plus')

    def hams(self):
        """[(ham, first channel, channels)] in the reference's drawing order"""
        if self.dual:
            return [(self.ham_1, 0, self.channels // 2), (self.ham_2, self.channels // 2, self.channels // 2)]
        return [(self.ham, 0, self.channels)]


def emb_dim(config):
    e = config.MODEL.EMB_DIM
    if isinstance(e, (list, tuple)):
        if len(e) != 1:
            raise ValueError('MODEL.EMB_DIM {}: pose_hrnet_hamburger takes one width (an int or a one-element '
                             'list)'.format(e))
        e = e[0]
    return int(e)


def check_config(config):
    """what the model refuses of a config, before anything is built"""
    M = config.MODEL
    if M.HAM_TYPE != 'NMF':
        raise ValueError('MODEL.HAM_TYPE {!r}: only \'NMF\' is built (the VQ and CD hams are not)'.format(M.HAM_TYPE))
    if M.VERSION != 'V2+':
        raise ValueError('MODEL.VERSION {!r}: only the \'V2+\' burger is built (V1 and V2 are not)'.format(M.VERSION))
    if not M.RAND_INIT:
        raise ValueError('MODEL.RAND_INIT false: the persistent bases buffer and its online update are not built')
    if 'hrnet' not in M.BACKBONE_NAME:
        raise ValueError('MODEL.BACKBONE_NAME {!r}: pose_hrnet_hamburger is built on \'pose_hrnet_softmax\' (the ResNet '
                         'backbone is not built)'.format(M.BACKBONE_NAME))
    if M.BACKBONE_NAME != 'pose_hrnet_softmax':
        raise ValueError('MODEL.BACKBONE_NAME {!r}: the HRNet backbone that hands out its features is '
                         '\'pose_hrnet_softmax\''.format(M.BACKBONE_NAME))
    if str(M.COMPUTE_DTYPE).lower() not in ('fp32', 'float32'):
        raise ValueError('MODEL.COMPUTE_DTYPE {!r}: pose_hrnet_hamburger runs in fp32 only (bf16 is not built)'.format(
            M.COMPUTE_DTYPE))
    e, s, r, f = emb_dim(config), int(M.S), int(M.R), int(M.CHEESE_FACTOR)
    if e < 1 or s < 1 or r < 1:
        raise ValueError('MODEL.EMB_DIM {}, MODEL.S {}, MODEL.R {}: each must be at least 1'.format(e, s, r))
    if f < 1 or (s * e) % f:
        raise ValueError('MODEL.CHEESE_FACTOR {}: must divide the S * EMB_DIM = {} channels of a ham'.format(f, s * e))
    if int(M.EVAL_STEPS) < 0:
        raise ValueError('MODEL.EVAL_STEPS {}: must be at least 0'.format(M.EVAL_STEPS))
    if not N.supported(N.OP_UPDATE, s * e, r):
        raise ValueError('MODEL.EMB_DIM {} with MODEL.R {}: beyond the NMF kernels'.format(e, r))
    if int(M.NUM_JOINTS) != int(config.DATASET.NUM_JOINTS):
        raise ValueError('MODEL.NUM_JOINTS {} differs from DATASET.NUM_JOINTS {}'.format(M.NUM_JOINTS,
                                                                                         config.DATASET.NUM_JOINTS))


def _fold(bn):
    """eval-mode BatchNorm as (scale, shift), float64"""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.detach().double() * scale


class HamNet(nn.Module):
    autograd_grads = True      # a trainable model's gradients are autograd .grad tensors (utils.get_optimizer)

    def __init__(self, config, is_train=False, trainable=False):
        super(HamNet, self).__init__()
        check_config(config)
        M = config.MODEL
        self.trainable = bool(trainable)
        if self.trainable and int(os.environ.get('WORLD_SIZE', '1')) > 1:
            raise ValueError('HamNet(trainable=True): WORLD_SIZE = {}: data-parallel training of pose_hrnet_hamburger is '
                             'not built'.format(os.environ['WORLD_SIZE']))
        if self.trainable and int(M.TRAIN_STEPS) < 0:
            raise ValueError('MODEL.TRAIN_STEPS {}: must be at least 0'.format(M.TRAIN_STEPS))
        self.train_steps = int(M.TRAIN_STEPS)
        # own parameters precede the sub-modules in a state dict, as the reference's lists them
        self.trainable_temp = nn.Parameter(torch.tensor(1.0), requires_grad=bool(M.TRAINABLE_SOFTMAX))
        from models import pose_hrnet_softmax
        self.in_channel = sum(M.EXTRA.STAGE4.NUM_CHANNELS)
        self.backbone = pose_hrnet_softmax.get_pose_net(config, is_train=True)
        path = M.BACKBONE_MODEL_PATH
        if path and is_train:                                   # the reference loads it when training only (:29)
            checkpoint = torch.load(path, map_location='cpu')
            state = checkpoint['state_dict'] if 'state_dict' in checkpoint else checkpoint
            logger.info("=> Loading pretrained {} backbone from '{}'".format(M.BACKBONE_NAME, path))
            self.backbone.load_state_dict({k.replace('module.', ''): v for k, v in state.items()}, strict=False)
        for p in self.backbone.parameters():
            p.requires_grad = False
        e = emb_dim(config)
        self.embed_dim, self.num_joints = e, int(config.DATASET.NUM_JOINTS)
        self.squeeze = ConvBNReLU(self.in_channel, e, 3)
        self.hamburger = HamburgerV2Plus(config, in_c=e)
        self.align = ConvBNReLU(e, ALIGN_CHANNELS, 3)
        self.fc = nn.Sequential(nn.Dropout2d(p=0.1), nn.Conv2d(ALIGN_CHANNELS, self.num_joints, 1))
        self._plan, self._plan_key = None, None

    # ---- the packed weights ----------------------------------------------------------------------------------------
    def _head_tensors(self):
        return [t for m in (self.squeeze, self.hamburger, self.align, self.fc) for t in
                list(m.parameters()) + list(m.buffers())]

    def _head_plan(self):
        """packed weights of the convolutions and the folded BatchNorms (scale, shift) their consumers apply; built once,
        rebuilt when a head parameter or buffer was written or moved"""
        key = tuple((t.data_ptr(), t._version) for t in self._head_tensors())
        if self._plan is not None and key == self._plan_key:
            return self._plan
        h = self.hamburger
        pad16, padded, pack = nhwc.pad16, nhwc.padded, nhwc.conv_pack
        cin, e = pad16(self.in_channel), pad16(self.embed_dim)
        cp, mp, ap, jp = pad16(h.channels), pad16(h.mid), pad16(ALIGN_CHANNELS), pad16(self.num_joints)
        affine = lambda bn, n: tuple(padded(v, n) for v in _fold(bn))
        # a 3x3 as the nine [cout_pad][cin_pad] matrices of its taps, tap t = 3 r + s
        taps = lambda conv, ip, op: nhwc.pack_taps(conv.weight.detach().float().contiguous(), conv.out_channels,
                                                   conv.in_channels, op, ip, 0)
        # the cheese as the (C, mid) matrix of a plain NMF-engine product, zero columns up to the padded width
        w_cheese = torch.zeros((h.channels, mp), dtype=torch.float32, device=h.cheese.conv.weight.device)
        w_cheese[:, :h.mid] = h.cheese.conv.weight.detach().float().reshape(h.mid, h.channels).t()
        self._plan = dict(
            cin=cin, e=e, cp=cp, mp=mp, ap=ap, jp=jp,
            w_squeeze=taps(self.squeeze.conv, cin, e), bn_squeeze=affine(self.squeeze.bn, e),
            w_lower=pack(h.lower_bread[0].weight, e, cp), b_lower=padded(h.lower_bread[0].bias, cp),
            w_cheese=w_cheese, bn_cheese=affine(h.cheese.bn, mp),
            w_upper=pack(h.upper_bread.weight, mp, e, h.coef_ham.detach().double().expand(self.embed_dim)),
            w_align=taps(self.align.conv, e, ap), bn_align=affine(self.align.bn, ap),
            w_fc=pack(self.fc[1].weight, ap, jp), b_fc=padded(self.fc[1].bias, jp))
        self._plan_key = key
        return self._plan

    # ---- the bases -------------------------------------------------------------------------------------------------
    def bases_shapes(self, B, h, w):
        """the (G, D, R) of every ham's bases for B images of h x w features, in drawing order"""
        return [(g, d, ham.R) for ham, _, ch in self.hamburger.hams() for g, d, _ in [ham.sizes(B, ch, h * w)]]

    def draw_bases(self, B, h, w):
        """the reference's draw, on the host: torch.rand((B * S, D, R)) from the global CPU generator, ham_1 before ham_2;
        float32 CPU tensors, not yet normalised"""
        return [N.draw_bases(*shape) for shape in self.bases_shapes(B, h, w)]

    # ---- the model -------------------------------------------------------------------------------------------------
    def _refuse(self, x):
        if self.training and self.trainable:
            if not isinstance(x, torch.Tensor) or not x.is_cuda:
                raise ValueError('HamNet: expected HIP-device tensors (there is no CPU path in this build)')
            if self.trainable_temp.device != x.device:
                raise ValueError('HamNet: the model is on {} and the input on {}: move the model with .cuda()'.format(
                    self.trainable_temp.device, x.device))
            return
        if self.training:
            raise NotImplementedError('HamNet: {} (SyncBN batch statistics, the backward through the last coefficient '
                                      'update and Dropout2d are a later step): call .eval() and run under '
                                      'torch.no_grad()'.format(NOT_BUILT))
        if torch.is_grad_enabled() and (getattr(x, 'requires_grad', False) or
                                        any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('HamNet: eval mode with a gradient required is refused - {}: run under '
                                      'torch.no_grad()'.format(NOT_BUILT))
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError('HamNet: expected HIP-device tensors (there is no CPU path in this build)')
        if self.trainable_temp.device != x.device:
            raise ValueError('HamNet: the model is on {} and the input on {}: move the model with .cuda()'.format(
                self.trainable_temp.device, x.device))

    # ---- training (trainable=True) ---------------------------------------------------------------------------------
    def draw_drop_keep(self, B, device):
        """the keep mask of fc's Dropout2d(0.1): (B, 256) values in {0, 1 / 0.9}, drawn on the device from torch's
        generator"""
        p = float(self.fc[0].p)
        return torch.empty((B, ALIGN_CHANNELS), dtype=torch.float32, device=device).bernoulli_(1.0 - p).div_(1.0 - p)

    def _head_train(self, features, bases, drop_keep):
        """head_forward in training mode under autograd, on hipnet.burger_train and hipnet.nmf_train: every activation is
        materialised, the BatchNorms run on batch statistics and update their running ones (num_batches_tracked stays),
        the packed weights are rebuilt from the parameters on every call"""
        from models.pose_hrnet_softmax import _SpatialSoftmax
        B, _, hh, ww = features.shape
        dev = features.device
        if drop_keep is None:
            drop_keep = self.draw_drop_keep(B, dev)
        if not isinstance(drop_keep, torch.Tensor) or tuple(drop_keep.shape) != (B, ALIGN_CHANNELS):
            raise ValueError('drop_keep {}: expected ({}, {})'.format(tuple(getattr(drop_keep, 'shape', ())), B,
                                                                      ALIGN_CHANNELS))
        h = self.hamburger
        keep = torch.zeros((B, nhwc.pad16(ALIGN_CHANNELS)), dtype=torch.float32, device=dev)
        keep[:, :ALIGN_CHANNELS] = drop_keep.to(device=dev, dtype=torch.float32)
        with torch.no_grad():
            nb = [N.normalise_bases(b.to(device=dev, dtype=torch.float32)) for b in bases]
        specs = [(ham.spatial, c0, ch, ham.S) for ham, c0, ch in h.hams()]
        x = nhwc.to_nhwc(features.float(), nhwc.pad16(self.in_channel))
        sq = BT.conv_bn_relu_train(x, self.squeeze.conv, self.squeeze.bn, 3)
        low = nhwc.conv1x1_train(sq, h.lower_bread[0], relu_out=True)
        y = NT.hams_train(low, specs, nb, self.train_steps)
        y = BT.conv_bn_relu_train(y, h.cheese.conv, h.cheese.bn, 1)
        y = nhwc.conv1x1_train(y, h.upper_bread)
        y = BT.burger_mix(y, sq, h.coef_ham, h.coef_shortcut)
        y = BT.conv_bn_relu_train(y, self.align.conv, self.align.bn, 3)
        y = nhwc.conv1x1_train(BT.dropout2d(y, keep), self.fc[1])
        self._plan = None                 # the running statistics were written through their pointers, not their version
        return _SpatialSoftmax.apply(nhwc.to_nchw(y, self.num_joints), self.trainable_temp)

    def head_forward(self, features, bases=None, drop_keep=None):
        """features (B, 480, h, w) NCHW on the device -> heat maps: everything after the backbone. bases: None (drawn here
        as the reference draws them), or a list of one tensor per ham, (B * S, D, R), NOT yet normalised (CPU or device).
        In training mode of a trainable model the hams run MODEL.TRAIN_STEPS steps and drop_keep is the (B, 256) keep mask
        of draw_drop_keep (None: drawn here); features.requires_grad is honoured"""
        self._refuse(features)
        if features.ndim != 4 or features.shape[1] != self.in_channel or features.numel() == 0:
            raise ValueError('features {}: expected (B, {}, h, w)'.format(tuple(features.shape), self.in_channel))
        B, _, hh, ww = features.shape
        shapes = self.bases_shapes(B, hh, ww)
        if bases is None:
            bases = self.draw_bases(B, hh, ww)
        bases = list(bases) if isinstance(bases, (list, tuple)) else [bases]
        if len(bases) != len(shapes) or any(tuple(b.shape) != s for b, s in zip(bases, shapes)):
            raise ValueError('bases {}: expected {}'.format([tuple(b.shape) for b in bases], shapes))
        if self.training:
            return self._head_train(features, bases, drop_keep)
        if drop_keep is not None:
            raise ValueError('drop_keep is for training mode')
        with torch.no_grad():
            p = self._head_plan()
            dev = features.device
            x = nhwc.to_nhwc(features.detach().float(), p['cin'])
            z = nhwc.conv3x3_taps(x, p['w_squeeze'], p['e'])                          # squeeze before its BatchNorm
            low = nhwc.conv_nhwc(z, p['w_lower'], p['cp'], 1, bias=p['b_lower'], in_affine=p['bn_squeeze'],
                                 in_relu=True).relu_()
            h = self.hamburger
            cheese_in = torch.empty_like(low)             # the hams write every real channel; no other is read
            for (ham, c0, ch), b in zip(h.hams(), bases):
                b = N.normalise_bases(b.to(device=dev, dtype=torch.float32))
                xin = low.permute(0, 3, 1, 2)[:, c0:c0 + ch]                          # (B, ch, h, w) view of the NHWC map
                N.nmf2d(xin, b, ham.eval_steps, ham.spatial, ham.S, out=cheese_in.permute(0, 3, 1, 2)[:, c0:c0 + ch])
            # cheese before its BatchNorm: rows of pixels times the (C, mid) matrix, the channels read as X^T in place
            # (one matrix over the pixels of all images)
            mid = N.product(cheese_in.reshape(1, B * hh * ww, p['cp']).transpose(1, 2)[:, :h.channels],
                            p['w_cheese'].unsqueeze(0)).reshape(B, hh, ww, p['mp'])
            scale, shift = p['bn_squeeze']
            block = torch.addcmul(shift, z, scale).relu_().mul_(h.coef_shortcut.detach())
            # + coef_ham * upper_bread(relu(bn(mid))); the block's own ReLU, then align before its BatchNorm
            nhwc.conv_nhwc(mid, p['w_upper'], p['e'], 1, in_affine=p['bn_cheese'], in_relu=True, into=block)
            y = nhwc.conv3x3_taps(block.relu_(), p['w_align'], p['ap'])
            y = nhwc.conv_nhwc(y, p['w_fc'], p['jp'], 1, bias=p['b_fc'], in_affine=p['bn_align'], in_relu=True)
            return nhwc.heatmap_softmax(y, self.num_joints, self.trainable_temp)

    def forward(self, x, bases=None, drop_keep=None):
        self._refuse(x)
        with torch.no_grad():            # frozen: no parameter of the backbone requires a gradient, in any mode
            features = self.backbone(x)[1]
        return self.head_forward(features, bases, drop_keep), self.trainable_temp


def get_pose_net(cfg, is_train, **kwargs):
    return HamNet(cfg, is_train, **kwargs)
