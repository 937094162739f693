"""V2V, the 3-D encoder-decoder of the volumetric models (reference lib/models/v2v.py, called from
lib/models/triangulation.py:349,467), as an eval-mode f32 forward on the HIP kernels of csrc/conv3d.hip.

The parameters live in ordinary nn.Conv3d / nn.BatchNorm3d / nn.ConvTranspose3d children under the reference's
attribute names, so state_dict() has the reference's keys and shapes and a reference checkpoint's `volume_net.*`
entries load with strict=True. None of these children is ever called: V2VModel.forward walks the tree once per input
shape into a flat list of launches (hrnet_conv3d, hrnet_maxpool3d, hrnet_deconv3d_k2s2 between two layout
transposes), and replays the list - one linear chain on the current stream, capturable after one warm-up call.

  weights      packed once by hrnet_pack_weights3d to [tap][Cout_pad][Cin_pad]; BatchNorm is NOT folded into them:
               scale = gamma / sqrt(var + eps) and shift = beta + (bias - mean) * scale are computed on the host in
               float64 from the running statistics and applied to the f32 accumulator. They are rebuilt when any
               parameter or buffer changes (its version counter or its storage), so after load_state_dict, after an
               optimiser step, after .to(); .train() drops them.
  activations  NDHWC f32 buffers, channels padded to 4 (input) and 16 (everything a kernel writes), cached per input
               shape: a second call with the same shape allocates only the tensor it returns.

Not built: the training-mode forward (batch statistics) and the whole backward. forward() refuses instead of
returning something detached: in training mode, and when gradients are enabled and the input or any parameter
requires one (wrap the call in torch.no_grad(), or freeze the parameters)."""
import torch
import torch.nn as nn

from hipnet import _capi as C

F32 = C.HR_F32
LEVELS = 5                                   # 2x2x2 poolings of the encoder: extents must be multiples of 2 ** 5


def _pad(c, to):
    return (c + to - 1) // to * to


class Basic3DBlock(nn.Module):
    """conv(ks) + BatchNorm + ReLU (v2v.py:7-17): one hrnet_conv3d launch"""

    def __init__(self, in_planes, out_planes, kernel_size):
        super().__init__()
        self.block = nn.Sequential(nn.Conv3d(in_planes, out_planes, kernel_size, 1, (kernel_size - 1) // 2),
                                   nn.BatchNorm3d(out_planes), nn.ReLU(True))

    def _emit(self, plan, x):
        return plan.conv(self.block[0], self.block[1], x, relu=True)


class Res3DBlock(nn.Module):
    """relu(bn(conv3(relu(bn(conv3(x))))) + skip(x)), skip = identity or bn(conv1(x)) (v2v.py:20-42): two or three
    hrnet_conv3d launches, the sum and the last ReLU in the epilogue of the last one"""

    def __init__(self, in_planes, out_planes):
        super().__init__()
        self.res_branch = nn.Sequential(nn.Conv3d(in_planes, out_planes, 3, 1, 1), nn.BatchNorm3d(out_planes),
                                        nn.ReLU(True), nn.Conv3d(out_planes, out_planes, 3, 1, 1),
                                        nn.BatchNorm3d(out_planes))
        self.skip_con = nn.Sequential() if in_planes == out_planes else nn.Sequential(
            nn.Conv3d(in_planes, out_planes, 1, 1, 0), nn.BatchNorm3d(out_planes))

    def _emit(self, plan, x):
        skip = x if len(self.skip_con) == 0 else plan.conv(self.skip_con[0], self.skip_con[1], x, relu=False)
        mid = plan.conv(self.res_branch[0], self.res_branch[1], x, relu=True)
        return plan.conv(self.res_branch[3], self.res_branch[4], mid, relu=True, res=skip)


class Pool3DBlock(nn.Module):
    """F.max_pool3d(x, pool_size, pool_size) (v2v.py:45-51); the kernel is the 2x2x2 one"""

    def __init__(self, pool_size):
        super().__init__()
        if pool_size != 2:
            raise NotImplementedError('Pool3DBlock: pool_size = {} (hrnet_maxpool3d is 2x2x2)'.format(pool_size))
        self.pool_size = pool_size

    def _emit(self, plan, x):
        return plan.pool(x)


class Upsample3DBlock(nn.Module):
    """ConvTranspose3d(k = 2, s = 2) + BatchNorm + ReLU (v2v.py:54-66): one hrnet_deconv3d_k2s2 launch, which also
    adds the decoder's skip tensor after the ReLU"""

    def __init__(self, in_planes, out_planes, kernel_size, stride):
        super().__init__()
        if kernel_size != 2 or stride != 2:
            raise NotImplementedError('Upsample3DBlock: kernel_size = {}, stride = {} (hrnet_deconv3d_k2s2 is 2 / 2)'
                                      .format(kernel_size, stride))
        self.block = nn.Sequential(nn.ConvTranspose3d(in_planes, out_planes, kernel_size, stride, 0, 0),
                                   nn.BatchNorm3d(out_planes), nn.ReLU(True))

    def _emit(self, plan, x, add=None):
        return plan.deconv(self.block[0], self.block[1], x, add)


class EncoderDecorder(nn.Module):
    """five levels of pool + Res3DBlock down, a middle block, five of Res3DBlock + upsample up, each level's skip
    block added after its upsample (v2v.py:69-138; the class name is the reference's spelling)"""

    WIDTHS = (32, 64, 128, 128, 128, 128)    # channels at level 0 .. 5

    def __init__(self):
        super().__init__()
        w = self.WIDTHS
        for k in range(1, LEVELS + 1):
            setattr(self, 'encoder_pool{}'.format(k), Pool3DBlock(2))
            setattr(self, 'encoder_res{}'.format(k), Res3DBlock(w[k - 1], w[k]))
        self.mid_res = Res3DBlock(w[LEVELS], w[LEVELS])
        for k in range(LEVELS, 0, -1):
            setattr(self, 'decoder_res{}'.format(k), Res3DBlock(w[k], w[k]))
            setattr(self, 'decoder_upsample{}'.format(k), Upsample3DBlock(w[k], w[k - 1], 2, 2))
        for k in range(1, LEVELS + 1):
            setattr(self, 'skip_res{}'.format(k), Res3DBlock(w[k - 1], w[k - 1]))

    def _emit(self, plan, x):
        skips = []
        for k in range(1, LEVELS + 1):
            skips.append(getattr(self, 'skip_res{}'.format(k))._emit(plan, x))
            x = getattr(self, 'encoder_pool{}'.format(k))._emit(plan, x)
            x = getattr(self, 'encoder_res{}'.format(k))._emit(plan, x)
        x = self.mid_res._emit(plan, x)
        for k in range(LEVELS, 0, -1):
            x = getattr(self, 'decoder_res{}'.format(k))._emit(plan, x)
            x = getattr(self, 'decoder_upsample{}'.format(k))._emit(plan, x, add=skips[k - 1])
        return x


class _Packed:
    """device copies the kernels read, per layer (keyed by the conv module): packed weight, scale, shift"""

    def __init__(self, model, device):
        self.key = model._param_key()
        self.device = device
        self.layers = {}
        stream = C.stream_ptr()
        mods = dict(model.named_modules())
        for name, m in mods.items():
            if not isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)):
                continue
            transposed = isinstance(m, nn.ConvTranspose3d)
            cin, cout, ks = m.in_channels, m.out_channels, m.kernel_size[0]
            cin_p, cout_p = _pad(cin, 4), _pad(cout, 16)
            if not transposed and not C.call('hrnet_conv3d_supported', F32, cin_p, cout_p, ks):
                raise RuntimeError('V2VModel: no HIP kernel for {} ({} -> {}, ks {})'.format(name, cin, cout, ks))
            w = m.weight.detach().to(device, torch.float32).contiguous()
            packed = torch.empty(ks ** 3 * cout_p * cin_p, dtype=torch.float32, device=device)
            C.call('hrnet_pack_weights3d', F32, w.data_ptr(), packed.data_ptr(), cout, cin, ks, cout_p, cin_p,
                   int(transposed), stream)
            self.layers[m] = [packed, None, None, cin_p, cout_p, ks, w]
        # the BatchNorm that follows a conv inside its nn.Sequential; the output layer has none
        for seq in (m for m in mods.values() if isinstance(m, nn.Sequential)):
            kids = list(seq)
            for conv, bn in zip(kids, kids[1:] + [None]):
                if conv in self.layers:
                    self._affine(conv, bn if isinstance(bn, nn.BatchNorm3d) else None)
        self._affine(model.output_layer, None)
        for ent in self.layers.values():
            ent.pop()                        # the f32 copy of the raw weight: the pack launch is ordered before its reuse

    def _affine(self, conv, bn):
        ent = self.layers[conv]
        cout_p = ent[4]
        bias = (conv.bias.detach().double().cpu() if conv.bias is not None
                else torch.zeros(conv.out_channels, dtype=torch.float64))
        scale = None
        shift = bias
        if bn is not None:
            gamma = bn.weight.detach().double().cpu() if bn.affine else torch.ones_like(bias)
            beta = bn.bias.detach().double().cpu() if bn.affine else torch.zeros_like(bias)
            scale = gamma / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
            shift = beta + (bias - bn.running_mean.detach().double().cpu()) * scale
        pad = torch.zeros(cout_p, dtype=torch.float64)

        def dev(v):
            out = pad.clone()
            out[:v.numel()] = v
            return out.to(torch.float32).to(self.device)
        ent[1] = None if scale is None else dev(scale)
        ent[2] = dev(shift)


class _Plan:
    """the launches of one input shape and the buffers they write; run() replays them on the current stream"""

    def __init__(self, model, packed, shape, device):
        B, Cn, D, H, W = shape
        self.packed, self.device, self.B = packed, device, B
        self.calls, self.buffers = [], []
        cin_p = _pad(Cn, 4)
        self.x_in = self._buf((D, H, W), cin_p)
        t = self.x_in
        for blk in model.front_layers:
            t = blk._emit(self, t)
        t = model.encoder_decoder._emit(self, t)
        for blk in model.back_layers:
            t = blk._emit(self, t)
        self.y_out = self.conv(model.output_layer, None, t, relu=False)
        self.shape, self.cin_p = shape, cin_p
        self.J, self.j_p = model.output_layer.out_channels, self.y_out[2]

    def _buf(self, ext, ch):
        D, H, W = ext
        t = torch.empty(self.B * D * H * W * ch, dtype=torch.float32, device=self.device)
        self.buffers.append(t)
        return (t, ext, ch)

    def conv(self, conv, bn, x, relu, res=None):
        packed, scale, shift, cin_p, cout_p, ks = self.packed.layers[conv]
        xt, (D, H, W), ch = x
        assert ch == cin_p and (res is None or (res[1], res[2]) == ((D, H, W), cout_p))
        y = self._buf((D, H, W), cout_p)
        self.calls.append(('hrnet_conv3d', (F32, xt.data_ptr(), packed.data_ptr(), C.ptr(scale), shift.data_ptr(),
                                            None if res is None else res[0].data_ptr(), y[0].data_ptr(), self.B, D, H,
                                            W, cin_p, cout_p, ks, int(relu))))
        return y

    def pool(self, x):
        xt, (D, H, W), ch = x
        y = self._buf((D // 2, H // 2, W // 2), ch)
        self.calls.append(('hrnet_maxpool3d', (F32, xt.data_ptr(), y[0].data_ptr(), self.B, D, H, W, ch)))
        return y

    def deconv(self, conv, bn, x, add):
        packed, scale, shift, cin_p, cout_p, ks = self.packed.layers[conv]
        xt, (D, H, W), ch = x
        ext = (2 * D, 2 * H, 2 * W)
        assert ch == cin_p and ks == 2 and (add is None or (add[1], add[2]) == (ext, cout_p))
        y = self._buf(ext, cout_p)
        self.calls.append(('hrnet_deconv3d_k2s2', (F32, xt.data_ptr(), packed.data_ptr(), C.ptr(scale),
                                                   shift.data_ptr(), None if add is None else add[0].data_ptr(),
                                                   y[0].data_ptr(), self.B, D, H, W, cin_p, cout_p, 1)))
        return y

    def run(self, x):
        B, Cn, D, H, W = self.shape
        stream = C.stream_ptr()
        out = torch.empty((B, self.J, D, H, W), dtype=torch.float32, device=self.device)
        # NCDHW <-> NDHWC are the 2-D layout kernels with H := D * H; they zero the pad channels
        C.call('hrnet_nchw_to_nhwc', F32, x.data_ptr(), self.x_in[0].data_ptr(), B, D * H, W, self.cin_p, Cn, stream)
        for name, args in self.calls:
            C.call(name, *args, stream)
        C.call('hrnet_nhwc_to_nchw', F32, self.y_out[0].data_ptr(), out.data_ptr(), B, D * H, W, self.j_p, self.J,
               stream)
        return out


class V2VModel(nn.Module):
    """(B, input_channels, D, H, W) -> (B, output_channels, D, H, W) float32 (v2v.py:141-180); D, H and W multiples
    of 32. Eval mode, no gradients: see the module docstring."""

    def __init__(self, input_channels, output_channels):
        super().__init__()
        self.front_layers = nn.Sequential(Basic3DBlock(input_channels, 16, 7), Res3DBlock(16, 32), Res3DBlock(32, 32),
                                          Res3DBlock(32, 32))
        self.encoder_decoder = EncoderDecorder()
        self.back_layers = nn.Sequential(Res3DBlock(32, 32), Basic3DBlock(32, 32, 1), Basic3DBlock(32, 32, 1))
        self.output_layer = nn.Conv3d(32, output_channels, 1, 1, 0)
        self._packed = None
        self._plans = {}
        self._initialize_weights()

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)):
                nn.init.xavier_normal_(m.weight)
                nn.init.constant_(m.bias, 0)

    def train(self, mode=True):
        self._packed = None
        self._plans = {}
        return super().train(mode)

    def _param_key(self):
        return tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def _refuse(self, x):
        """every refusal, before any device call"""
        if self.training:
            raise NotImplementedError('V2VModel: the training-mode forward (batch statistics) is not built; call '
                                      '.eval() - BatchNorm then uses its running statistics')
        if torch.is_grad_enabled() and (getattr(x, 'requires_grad', False) or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('V2VModel: the training forward and the backward are not built, and the input or '
                                      'a parameter requires a gradient; run under torch.no_grad() (or freeze the '
                                      'parameters) - nothing is detached silently')
        cin = self.front_layers[0].block[0].in_channels
        if not isinstance(x, torch.Tensor) or x.ndim != 5:
            raise ValueError('V2VModel: expected a (B, {}, D, H, W) tensor, got {}'.format(
                cin, tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__))
        if x.shape[1] != cin:
            raise ValueError('V2VModel: input has {} channels, the model takes {}'.format(x.shape[1], cin))
        if x.shape[0] < 1 or any(s < 1 or s % (1 << LEVELS) for s in x.shape[2:]):
            raise ValueError('V2VModel: D, H, W = {} must be multiples of {} (five 2x2x2 poolings whose outputs are '
                             'added back to the skips), B = {} at least 1'.format(tuple(x.shape[2:]), 1 << LEVELS,
                                                                                 x.shape[0]))
        if not x.is_cuda:
            raise ValueError('V2VModel: expected a HIP-device tensor (there is no CPU path in this build)')

    def forward(self, x):
        self._refuse(x)
        from core.loss import _dev_f32
        x = _dev_f32(x.detach(), 'V2VModel')
        if any(t.device != x.device for t in list(self.parameters()) + list(self.buffers())):
            raise ValueError('V2VModel: the parameters are not on the input\'s device {}'.format(x.device))
        with torch.cuda.device(x.device):
            if self._packed is None or self._packed.key != self._param_key():
                self._packed = _Packed(self, x.device)
                self._plans = {}
            shape = tuple(x.shape)
            if shape not in self._plans:
                self._plans[shape] = _Plan(self, self._packed, shape, x.device)
            return self._plans[shape].run(x)
