"""FTLMultiviewNet, MODEL.NAME `FTL` (reference lib/models/FTL_encoder_decoder.py:83-214): a multi-view encoder-decoder
on the 480-channel features of the frozen pose_hrnet_softmax backbone. The encoded map of every view is read as 3-vectors,
carried into a common world frame by that view's camera (the feature transform layer), fused over the views, carried back
into every view's frame and decoded to heat maps; the decoded 2-D points are lifted by DLT. Inference by default; the
head trains when the model is built with trainable=True (the backbone stays frozen, as in the reference's train3D.py).

forward(images (B, V, 3, H, W), extrinsic_matrices (B, V, 3, 4) = [R | t], intrinsic_matrices (3, 3) or (B, 3, 3),
        to_frame=None, orig_img_size=(640, 480))
  1. backbone per view-image -> features (B V, C, h, w), C = sum(STAGE4.NUM_CHANNELS) = 480 (slot 1 of its output)    :155
  2. encoder_head: two [Conv2d(3, stride 2, padding 2, bias) + BatchNorm + ReLU], C -> C -> C / 2; 64 -> 33 -> 18       :111
  3. each (C / 2, h2, w2) map, flat in NCHW order, as (C / 2, h2 w2 / 3, 3) - triplets of consecutive pixels in row-major
     order, across row ends when w2 % 3 != 0 - and per view x -> (x K^-T - t^T) R^-T; the V results concatenated on the
     channel axis in view order                                                                                    :159-176
  4. fuse_after_FTL: two [Conv2d 1x1 + BatchNorm + ReLU], V C / 2 -> C / 2 -> C / 2                                     :179
  5. per view f -> (f R^T + t^T) K^T                                                                               :183-188
  6. channel_expansion: [Conv2d 1x1 + BatchNorm + ReLU], C / 2 -> C                                                    :191
  7. decoder: [ConvTranspose2d(C -> 256, 3, stride 2, padding 2) + BatchNorm + ReLU] 18 -> 33, [ConvTranspose2d(256 -> 256,
     3, stride 2, padding 2, output_padding 1) + BatchNorm + ReLU] 33 -> 64, Conv2d(256 -> 256, 3, padding 1)           :198
  8. final_layer Conv2d(256 -> K, 1); softmax over the positions of each map (temperature 1)                       :201-206
  9. expectation decode -> pose2d_pred; DLT of every joint with P = K [R | t] -> pose3d_pred                       :208-212
returns (heatmaps_pred (B V, K, h, w), pose2d_pred (B, V, K, 2) in heat-map pixels, pose3d_pred (B, K, 3)), every row with
views in slot order b V + v. head_forward(features, ...) is everything after the backbone.

Every product is a launch through the C ABI, on NHWC maps; no map is padded, cropped or concatenated through torch:
  encoder_head     hrnet_conv2d_3x3g (stride 2, pad_lo 2, explicit 33 / 18), BatchNorm folded into the packed weights
                   and the bias, ReLU in the epilogue
  steps 3, 5       hrnet_ftl_gather writes view v's transformed channels into slice v of the concatenated map (slice width
                   C / 2: the reference's channel order, so fuse_after_FTL.0's weight is packed as it is); hrnet_ftl_scatter
                   writes all V views from one read of the fused map. Both evaluate the composed x A + c, whose 12
                   coefficients per (b, v) hipnet.ftl.affines computes in float64 on the host
  1x1 layers       hrnet_conv2d_kxk with ks 1 (bias and ReLU in the launch)
  decoder          the transposed layers as hrnet_conv2d_3x3g on the input read zero-stuffed (z 2, stride 1, pad_lo 0, Ho =
                   2 H - 3 + output_padding) with the flipped, transposed weights of nhwc.conv_transpose_pack: only the taps
                   of a parity class that meet no stuffed zero are issued. decoder.layer_lst.2 and final_layer have nothing
                   between them and are ONE 3x3 convolution 256 -> K whose weights are multiplied in float64 on the host
                   (4.8 of the head's GFLOP per image less); the maps of 256 channels at 64 x 64 are never formed
  step 8, 9        hrnet_spatial_softmax_fwd, the expectation decode, one hrnet_triangulate launch
The packed weights are built once and rebuilt when a head parameter or buffer changes (load_state_dict, .cuda()).

The holder modules are ordinary nn.Conv2d / nn.ConvTranspose2d / nn.BatchNorm2d under the reference's attribute names, so
state_dict() has the reference's keys in the reference's order and a reference checkpoint loads with strict=True after
'module.' is stripped; their own forward is never used.

Reference defects not reproduced:
- Batch order after step 5: the reference stacks the views view-major (row v B + b) and then reads the rows as batch-major
  (.view(B, V, ...), :208), which pairs predictions with the wrong views whenever B > 1. Here every stage after the
  distribution is in slot order b V + v, the order of tools/evaluate_3D.py's heatmaps_of; the two agree at B = 1.
- `heatmaps, inter_feat = self.backbone(images)` (:155) unpacks two values from pose_hrnet_softmax, which returns three;
  the features are slot [1].
- `DLT_sii_pytorch(proj_matrices, pose2d)` (:212) has its arguments swapped and cannot run, and its points are in heat-map
  pixels while K is the frame's. Here utils.multiview.triangulate_batch_of_points lifts the points after mapping them to
  frame pixels through `to_frame` (the batch's hm_inverse) when given, else by orig_img_size / heatmap size.
  pose2d_pred is returned in heat-map pixels, as the reference's losses expect.
- The reference uses intrinsic_matrices[0] for the whole batch; here (3, 3) or (B, 3, 3) is taken and a batch whose
  matrices differ is refused.
- The encoder's output width is hard-coded as 240 (:112) while everything behind it uses C // 2; here it is C // 2.

Refused when the model is built: a MODEL.BACKBONE_NAME other than 'pose_hrnet_softmax', MODEL.COMPUTE_DTYPE other than
fp32, a C with C / 2 no multiple of 4, DATASET.NUM_VIEWS < 1. Refused in forward: CPU tensors (ValueError), a number of
views other than DATASET.NUM_VIEWS, features whose encoded h2 w2 is no multiple of 3, and - for a model built without
trainable=True - training mode and eval mode with a gradient required (NotImplementedError - run model.eval() under
torch.no_grad()).

Training (FTLMultiviewNet(config, is_train, trainable=True), model.train(), gradients enabled): the head runs on batch
statistics as ONE autograd node (hipnet.ftl_train.HeadFn), from the features and cameras to the heat maps and from the
heat maps' gradient to .grad of every head parameter, with no torch convolution in between:
  conv + BatchNorm + ReLU   the raw-weight convolution with its bias and no ReLU (the kernels above), then
                            nhwc.bn_batch_forward, which updates the running statistics with the module's momentum;
                            backward nhwc.bn_batch_backward (gamma, beta and the convolution's bias), then
  weight gradients          hrnet_conv2d_3x3g_wgrad for the strided layers and - with the roles of input and gradient
                            swapped - the transposed ones; hrnet_conv2d_kxk_wgrad (ks 1, and ks 3 for the output layer)
  data gradients            the forward kernel hrnet_conv2d_3x3g itself on repacked weights (hipnet.ftl_train states the
                            two identities), hrnet_conv2d_kxk_dgrad for the 1x1 layers and the output layer,
                            hrnet_ftl_scatter_bwd / hrnet_ftl_gather_bwd for the transforms; encoder_head.0 needs none
  output layer              decoder.layer_lst.2 and final_layer stay folded (nothing lies between them, so the fold is exact
                            in training): W_out = Wf W_last and b_out are formed on the device each step, dW_out / db_out
                            come from hrnet_conv2d_kxk_wgrad and go back through the product: dWf = <dW_out, W_last>,
                            dW_last = Wf^T dW_out, db_last = Wf^T db_out, db_fin = db_out
pose2d_pred and pose3d_pred then come from the differentiable expectation decode and DLT. The backbone runs in eval mode
under no_grad. model.hip() hands hipnet.optim.FlatAdam the flat parameters and gradients of the head; a backward pass
overwrites the gradients. Under torch.no_grad(), or in .eval(), a trainable model runs the inference path bit for bit.
"""
import logging

import torch
import torch.nn as nn

from hipnet import conv_kxk as KX
from hipnet import ftl as FT
from hipnet import ftl_train as FTT
from hipnet import nhwc
from utils.heatmap_decoding import get_final_preds
from utils.multiview import triangulate_batch_of_points

logger = logging.getLogger(__name__)

NOT_BUILT = 'training of FTL is not built'
BN_MOMENTUM = 0.1
DECODER_CHANNELS = 256


def _unused(name):
    def forward(self, *a, **k):
        raise NotImplementedError('{} holds parameters of FTLMultiviewNet; FTLMultiviewNet.head_forward runs it through '
                                  'hipnet.ftl and hipnet.conv_kxk'.format(name))
    return forward


class conv_block(nn.Module):
    def __init__(self, n_layers, channel_lst, kernel_size_lst, stride_lst, padding_lst):
        super(conv_block, self).__init__()
        self.layer_lst = nn.ModuleList([
            nn.Sequential(nn.Conv2d(channel_lst[i], channel_lst[i + 1], kernel_size_lst[i], stride_lst[i], padding_lst[i]),
                          nn.BatchNorm2d(channel_lst[i + 1], momentum=BN_MOMENTUM), nn.ReLU(inplace=False))
            for i in range(n_layers)])

    forward = _unused('conv_block')


class Decoder(nn.Module):
    """(n_layers - 1) transposed convolutions with BatchNorm and ReLU, and one bare convolution"""

    def __init__(self, n_layers, channel_lst, kernel_size_lst, stride_lst, padding_lst, output_padding_lst):
        super(Decoder, self).__init__()
        layers = [nn.Sequential(nn.ConvTranspose2d(channel_lst[i], channel_lst[i + 1], kernel_size_lst[i], stride_lst[i],
                                                   padding_lst[i], output_padding_lst[i]),
                                nn.BatchNorm2d(channel_lst[i + 1], momentum=BN_MOMENTUM), nn.ReLU(inplace=False))
                  for i in range(n_layers - 1)]
        layers.append(nn.Conv2d(channel_lst[-2], channel_lst[-1], kernel_size_lst[-1], stride_lst[-1], padding_lst[-1]))
        self.layer_lst = nn.ModuleList(layers)

    forward = _unused('Decoder')


def check_config(config):
    """what the model refuses of a config, before anything is built"""
    M = config.MODEL
    if M.BACKBONE_NAME != 'pose_hrnet_softmax':
        raise ValueError('MODEL.BACKBONE_NAME {!r}: FTL is built on \'pose_hrnet_softmax\', the HRNet backbone that hands '
                         'out its features'.format(M.BACKBONE_NAME))
    if str(M.COMPUTE_DTYPE).lower() not in ('fp32', 'float32'):
        raise ValueError('MODEL.COMPUTE_DTYPE {!r}: FTL runs in fp32 only (bf16 is not built)'.format(M.COMPUTE_DTYPE))
    C = sum(M.EXTRA.STAGE4.NUM_CHANNELS)
    if C < 8 or C % 8:
        raise ValueError('MODEL.EXTRA.STAGE4.NUM_CHANNELS {}: their sum {} must be a multiple of 8 (the transform moves the '
                         'C / 2 encoded channels four at a time)'.format(list(M.EXTRA.STAGE4.NUM_CHANNELS), C))
    if int(config.DATASET.NUM_VIEWS) < 1:
        raise ValueError('DATASET.NUM_VIEWS {}: must be at least 1'.format(config.DATASET.NUM_VIEWS))


def _fold(bn):
    """eval-mode BatchNorm as (scale, shift), float64"""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.detach().double() * scale


class FTLMultiviewNet(nn.Module):
    def __init__(self, config, is_train=False, trainable=False):
        super(FTLMultiviewNet, self).__init__()
        check_config(config)
        self.trainable = bool(trainable)
        self._flat, self._dirty, self.tape = None, 0, None
        M = config.MODEL
        from models import pose_hrnet_softmax
        self.backbone = pose_hrnet_softmax.get_pose_net(config, is_train=True)
        path = M.BACKBONE_MODEL_PATH
        if path and is_train:                                   # as HamNet: the backbone's own file when training only
            checkpoint = torch.load(path, map_location='cpu')
            state = checkpoint['state_dict'] if 'state_dict' in checkpoint else checkpoint
            logger.info("=> Loading pretrained {} backbone from '{}'".format(M.BACKBONE_NAME, path))
            self.backbone.load_state_dict({k.replace('module.', ''): v for k, v in state.items()}, strict=False)
        for p in self.backbone.parameters():
            p.requires_grad = False
        C = sum(M.EXTRA.STAGE4.NUM_CHANNELS)
        self.in_channel, self.mid = C, C // 2
        self.num_views, self.num_joints = int(config.DATASET.NUM_VIEWS), int(config.DATASET.NUM_JOINTS)
        self.encoder_head = conv_block(2, [C, C, C // 2], [3, 3], [2, 2], [2, 2])
        self.fuse_after_FTL = conv_block(2, [C // 2 * self.num_views, C // 2, C // 2], [1, 1], [1, 1], [0, 0])
        self.channel_expansion = conv_block(1, [C // 2, C], [1], [1], [0])
        D = DECODER_CHANNELS
        self.decoder = Decoder(3, [C, D, D, D], [3, 3, 3], [2, 2, 1], [2, 2, 1], [0, 1])
        self.final_layer = nn.Conv2d(D, self.num_joints, 1)
        self._plan, self._plan_key = None, None

    # ---- the packed weights ----------------------------------------------------------------------------------------
    def _head_tensors(self):
        return [t for m in (self.encoder_head, self.fuse_after_FTL, self.channel_expansion, self.decoder, self.final_layer)
                for t in list(m.parameters()) + list(m.buffers())]

    def _head_plan(self):
        """per layer (packed weights with the BatchNorm scale folded in, bias with its shift); built once, rebuilt when a
        head parameter or buffer was written or moved"""
        key = tuple((t.data_ptr(), t._version) for t in self._head_tensors()) + (self._dirty,)
        if self._plan is not None and key == self._plan_key:
            return self._plan

        def conv_bn(seq, cin_pad):
            scale, shift = _fold(seq[1])
            bias = (seq[0].bias.detach().double() * scale + shift).float().contiguous()
            return nhwc.conv_pack(seq[0].weight.detach().float(), cin_pad, None, scale), bias

        def tconv_bn(seq, cin_pad):
            # ConvTranspose2d weight (Cin, Cout, 3, 3): the scale goes on its SECOND axis
            scale, shift = _fold(seq[1])
            w = (seq[0].weight.detach().double() * scale.reshape(1, -1, 1, 1)).float().contiguous()
            bias = (seq[0].bias.detach().double() * scale + shift).float().contiguous()
            return nhwc.conv_transpose_pack(w, cin_pad, None), bias

        C, C2, D, K = self.in_channel, self.mid, DECODER_CHANNELS, self.num_joints
        cin = nhwc.pad16(C)
        last, fin = self.decoder.layer_lst[2], self.final_layer
        wf = fin.weight.detach().double().reshape(K, D)
        w_out = torch.einsum('km,mcrs->kcrs', wf, last.weight.detach().double()).float().contiguous()
        b_out = (wf @ last.bias.detach().double() + fin.bias.detach().double()).float().contiguous()
        self._plan = dict(
            cin=cin,
            enc0=conv_bn(self.encoder_head.layer_lst[0], cin), enc1=conv_bn(self.encoder_head.layer_lst[1], C),
            fuse0=conv_bn(self.fuse_after_FTL.layer_lst[0], C2 * self.num_views),
            fuse1=conv_bn(self.fuse_after_FTL.layer_lst[1], C2),
            expand=conv_bn(self.channel_expansion.layer_lst[0], C2),
            dec0=tconv_bn(self.decoder.layer_lst[0], C), dec1=tconv_bn(self.decoder.layer_lst[1], D),
            out=(nhwc.conv_pack(w_out, D, None), b_out),
            temp=torch.ones(1, dtype=torch.float32, device=fin.weight.device))
        self._plan_key = key
        return self._plan

    # ---- training --------------------------------------------------------------------------------------------------
    def hip(self):
        """the flat f32 parameter and gradient buffers of the head (what hipnet.optim.FlatAdam steps): built on first use
        on the parameters' device; every head parameter becomes a view of flat_p and its .grad a view of flat_g"""
        if not self.trainable:
            raise NotImplementedError('FTLMultiviewNet: {}: build the model with trainable=True'.format(NOT_BUILT))
        if self._flat is None or self._flat.flat_p.device != self.final_layer.weight.device:
            self._flat = FTT.HeadFlat(self)
        return self._flat

    def head_parameters(self):
        return [p for m in FTT.HEAD_MODULES for p in getattr(self, m).parameters()]

    def train(self, mode=True):
        super(FTLMultiviewNet, self).train(mode)
        if self.trainable:
            self.backbone.eval()           # frozen: its BatchNorms keep their running statistics
        return self

    def _training_pass(self):
        return self.trainable and self.training and torch.is_grad_enabled()

    # ---- the model -------------------------------------------------------------------------------------------------
    def _refuse(self, x):
        if self.trainable:
            if not isinstance(x, torch.Tensor) or not x.is_cuda:
                raise ValueError('FTLMultiviewNet: expected HIP-device tensors (there is no CPU path in this build)')
            if self.final_layer.weight.device != x.device:
                raise ValueError('FTLMultiviewNet: the model is on {} and the input on {}: move the model with '
                                 '.cuda()'.format(self.final_layer.weight.device, x.device))
            return
        if self.training:
            raise NotImplementedError('FTLMultiviewNet: {} (the backward of the transforms and of the general 3x3 '
                                      'convolution is the next step): call .eval() and run under '
                                      'torch.no_grad()'.format(NOT_BUILT))
        head = [p for m in (self.encoder_head, self.fuse_after_FTL, self.channel_expansion, self.decoder, self.final_layer)
                for p in m.parameters()]
        if torch.is_grad_enabled() and (getattr(x, 'requires_grad', False) or any(p.requires_grad for p in head)):
            raise NotImplementedError('FTLMultiviewNet: eval mode with a gradient required is refused - {}: run under '
                                      'torch.no_grad()'.format(NOT_BUILT))
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError('FTLMultiviewNet: expected HIP-device tensors (there is no CPU path in this build)')
        if self.final_layer.weight.device != x.device:
            raise ValueError('FTLMultiviewNet: the model is on {} and the input on {}: move the model with .cuda()'.format(
                self.final_layer.weight.device, x.device))

    def _cameras(self, extrinsic, BV):
        V = self.num_views
        if not isinstance(extrinsic, torch.Tensor) or extrinsic.ndim != 4 or tuple(extrinsic.shape[2:]) != (3, 4):
            raise ValueError('extrinsic_matrices {}: expected (B, V, 3, 4)'.format(tuple(getattr(extrinsic, 'shape', ()))))
        if extrinsic.shape[1] != V:
            raise ValueError('extrinsic_matrices {}: {} views, the model was built for DATASET.NUM_VIEWS = {}'.format(
                tuple(extrinsic.shape), extrinsic.shape[1], V))
        if BV != extrinsic.shape[0] * V:
            raise ValueError('{} view-images for extrinsic_matrices {}: expected {}'.format(BV, tuple(extrinsic.shape),
                                                                                            extrinsic.shape[0] * V))
        return extrinsic.shape[0]

    def encoded_size(self, h, w):
        """(h2, w2) of the encoded map of h x w features: two Conv2d(3, stride 2, padding 2)"""
        step = lambda n: FT.out_size(n, 2, 2)
        return step(step(h)), step(step(w))

    def head_stages(self, features, extrinsic_matrices, intrinsic_matrices):
        """head_forward's maps before the decode, NHWC: dict of 'encoder_head' (B V, h2, w2, C / 2), 'fuse_after_FTL'
        (B, h2, w2, C / 2), 'channel_expansion' (B V, h2, w2, C), 'logits' (B V, h, w, pad16(K)) and 'heatmaps' NCHW"""
        self._refuse(features)
        if features.ndim != 4 or features.shape[1] != self.in_channel or features.numel() == 0:
            raise ValueError('features {}: expected (B * V, {}, h, w)'.format(tuple(features.shape), self.in_channel))
        BV, _, h, w = features.shape
        B, V = self._cameras(extrinsic_matrices, BV), self.num_views
        h1, w1 = FT.out_size(h, 2, 2), FT.out_size(w, 2, 2)
        h2, w2 = self.encoded_size(h, w)
        if (h2 * w2) % 3:
            raise ValueError('features {}: the encoded map is {} x {} = {} pixels, no whole number of triplets'.format(
                tuple(features.shape), h2, w2, h2 * w2))
        with torch.no_grad():
            p = self._head_plan()
            dev = features.device
            C, C2, D, K = self.in_channel, self.mid, DECODER_CHANNELS, self.num_joints
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
            x = nhwc.to_nhwc(features.detach().float(), p['cin'])
            x = FT.conv(x, p['enc0'][0], p['enc0'][1], new(BV, h1, w1, C), p['cin'], 0, C, 0, 2, 2, 1, True)
            enc = FT.conv(x, p['enc1'][0], p['enc1'][1], new(BV, h2, w2, C2), C, 0, C2, 0, 2, 2, 1, True)
            # the 12 coefficients per (b, v), float64 on the host while the device runs the encoder
            coef_g, coef_s = FT.affines(extrinsic_matrices.to(dev), intrinsic_matrices)
            cat = FT.gather_raw(enc, coef_g, new(B, h2, w2, V * C2), B, V, C2, 0, 0, C2)
            x = KX.conv(cat, p['fuse0'][0], p['fuse0'][1], new(B, h2, w2, C2), V * C2, 0, C2, 0, 1, True)
            fused = KX.conv(x, p['fuse1'][0], p['fuse1'][1], new(B, h2, w2, C2), C2, 0, C2, 0, 1, True)
            x = FT.scatter_raw(fused, coef_s, new(BV, h2, w2, C2), B, V, C2, 0, 0)
            exp = KX.conv(x, p['expand'][0], p['expand'][1], new(BV, h2, w2, C), C2, 0, C, 0, 1, True)
            ha, wa = FT.out_size(h2, 1, 0, 2, 0), FT.out_size(w2, 1, 0, 2, 0)
            x = FT.conv(exp, p['dec0'][0], p['dec0'][1], new(BV, ha, wa, D), C, 0, D, 0, 1, 0, 2, True)
            hb, wb = FT.out_size(ha, 1, 0, 2, 1), FT.out_size(wa, 1, 0, 2, 1)
            x = FT.conv(x, p['dec1'][0], p['dec1'][1], new(BV, hb, wb, D), D, 0, D, 0, 1, 0, 2, True)
            logits = FT.conv(x, p['out'][0], p['out'][1], new(BV, hb, wb, nhwc.pad16(K)), D, 0, K, 0, 1, 1, 1, False)
            hm = nhwc.heatmap_softmax(logits, K, p['temp'])
        return {'encoder_head': enc, 'fuse_after_FTL': fused, 'channel_expansion': exp, 'logits': logits, 'heatmaps': hm}

    def _head_train(self, features, extrinsic_matrices, intrinsic_matrices):
        """the training forward of the head on batch statistics: heat maps (B V, K, h, w) that carry the head's backward"""
        self._refuse(features)
        if features.ndim != 4 or features.shape[1] != self.in_channel or features.numel() == 0:
            raise ValueError('features {}: expected (B * V, {}, h, w)'.format(tuple(features.shape), self.in_channel))
        self._cameras(extrinsic_matrices, features.shape[0])
        h2, w2 = self.encoded_size(features.shape[2], features.shape[3])
        if (h2 * w2) % 3:
            raise ValueError('features {}: the encoded map is {} x {} = {} pixels, no whole number of triplets'.format(
                tuple(features.shape), h2, w2, h2 * w2))
        return FTT.head_forward_train(self, features, extrinsic_matrices, intrinsic_matrices)

    def head_forward(self, features, extrinsic_matrices, intrinsic_matrices, to_frame=None, orig_img_size=(640, 480)):
        """features (B * V, C, h, w) NCHW on the device, slot order b V + v -> (heatmaps_pred, pose2d_pred, pose3d_pred):
        everything after the backbone"""
        train = self._training_pass()
        if train:
            hm = self._head_train(features, extrinsic_matrices, intrinsic_matrices)
        else:
            hm = self.head_stages(features, extrinsic_matrices, intrinsic_matrices)['heatmaps']
        B, V, K = extrinsic_matrices.shape[0], self.num_views, self.num_joints
        dev = hm.device
        with torch.enable_grad() if train else torch.no_grad():
            pose2d = get_final_preds(hm, True).view(B, V, K, 2)
            Kmat = intrinsic_matrices.to(dev).double()
            Kmat = Kmat[0] if Kmat.ndim == 3 else Kmat
            proj = Kmat @ extrinsic_matrices.to(dev).double()                       # (B, V, 3, 4)
            if to_frame is None:
                sx, sy = orig_img_size[0] / float(hm.shape[3]), orig_img_size[1] / float(hm.shape[2])
                to_frame = torch.tensor([[sx, 0., 0.], [0., sy, 0.]], dtype=torch.float64, device=dev).expand(B * V, 2, 3)
            pose3d = triangulate_batch_of_points(proj, pose2d, to_frame=to_frame.to(dev).contiguous())
        return hm, pose2d, pose3d

    def forward(self, images, extrinsic_matrices, intrinsic_matrices, to_frame=None, orig_img_size=(640, 480)):
        self._refuse(images)
        if images.ndim != 5 or images.shape[1] != self.num_views:
            raise ValueError('images {}: expected (B, V, 3, H, W) with V = DATASET.NUM_VIEWS = {}'.format(
                tuple(images.shape), self.num_views))
        with torch.no_grad():            # frozen: no parameter of the backbone requires a gradient
            features = self.backbone(images.reshape(-1, *images.shape[2:]))[1]
        return self.head_forward(features, extrinsic_matrices, intrinsic_matrices, to_frame, orig_img_size)


def get_pose_net(cfg, is_train=False, **kwargs):
    return FTLMultiviewNet(cfg, is_train, **kwargs)
