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

Training is opt-in: V2VModel(..., trainable=True). In training mode such a model runs one torch.autograd.Function over the
whole network (_TrainFn): the forward normalises every BatchNorm3d with the statistics of the batch and updates the
running ones on the device, the backward gives the input's gradient and one for every parameter that requires it, all on
the kernels of csrc/conv3d_train.hip. Per input shape the forward and the backward launches are recorded once
(_TrainPlan) together with everything the backward needs: per layer the raw convolution output z AND the layer's output
y ("V2V training", says what that costs). A plan's buffers are shared by every call of its shape, so a
backward must follow its own forward before the next forward of that shape; anything else is refused.

Without trainable=True (the default) nothing of this exists: forward() refuses in training mode, and when gradients are
enabled and the input or any parameter requires one (wrap the call in torch.no_grad(), or freeze the parameters). Eval
mode with a gradient required is refused with trainable=True as well: the backward through the running statistics is
not built."""
import ctypes

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


class _Act:
    """an activation of the training plan: t NDHWC f32 [B, *ext, ch], of which `real` channels are not padding; needs:
    a gradient must reach it (its producer has a parameter that requires one, or an input that needs one); grad: the
    buffer that holds (so far) d loss / d t"""

    def __init__(self, t, ext, ch, real, needs):
        self.t, self.ext, self.ch, self.real, self.needs = t, ext, ch, real, needs
        self.grad, self.shared = None, False


class _TrainPacked:
    """device copies the training kernels read, in buffers that live as long as the trainer (the recorded launches
    hold their addresses): per conv the packed weight, the weight packed for the input gradient, the padded bias and
    the padded gamma / beta of its BatchNorm. refresh() fills them again after the parameters changed."""

    def __init__(self, modules, device):
        self.device, self.key, self.layers = device, None, {}
        mods = []
        for root in modules:
            mods += [m for m in root.modules()]
        self.bn_of = {}
        for seq in (m for m in mods if isinstance(m, nn.Sequential)):
            kids = list(seq)
            for conv, bn in zip(kids, kids[1:]):
                if isinstance(conv, (nn.Conv3d, nn.ConvTranspose3d)) and isinstance(bn, nn.BatchNorm3d):
                    self.bn_of[conv] = bn
        for m in mods:
            if not isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)) or m in self.layers:
                continue
            transposed = isinstance(m, nn.ConvTranspose3d)
            cin, cout, ks = m.in_channels, m.out_channels, m.kernel_size[0]
            cin_p, cout_p = _pad(cin, 4), _pad(cout, 16)
            if not transposed and not C.call('hrnet_conv3d_supported', F32, cin_p, cout_p, ks):
                raise RuntimeError('V2V training: no HIP kernel for a convolution {} -> {}, ks {}'.format(cin, cout, ks))
            bn = self.bn_of.get(m)
            if bn is not None and (not bn.affine or bn.momentum is None):
                raise NotImplementedError('V2V training: BatchNorm3d without affine parameters or with momentum=None')
            if m.bias is None:
                raise NotImplementedError('V2V training: a convolution without bias')
            gin_p = _pad(cin_p, 16)                      # channels of the input gradient this layer writes

            def buf(n):
                return torch.zeros(n, dtype=torch.float32, device=device)
            self.layers[m] = dict(conv=m, bn=bn, transposed=transposed, cin=cin, cout=cout, ks=ks, cin_p=cin_p,
                                  cout_p=cout_p, gin_p=gin_p, w=buf(ks ** 3 * cout_p * cin_p),
                                  wd=buf(ks ** 3 * (cin_p if transposed else gin_p) * cout_p), bias=buf(cout_p),
                                  gamma=buf(cout_p) if bn is not None else None,
                                  beta=buf(cout_p) if bn is not None else None)

    @staticmethod
    def param_key(params):
        return tuple((p.data_ptr(), p._version) for p in params)

    def refresh(self, key):
        stream = C.stream_ptr()
        for L in self.layers.values():
            m, bn = L['conv'], L['bn']
            w = m.weight.detach().to(self.device, torch.float32).contiguous()
            C.call('hrnet_pack_weights3d', F32, w.data_ptr(), L['w'].data_ptr(), L['cout'], L['cin'], L['ks'], L['cout_p'],
                   L['cin_p'], int(L['transposed']), stream)
            if L['transposed']:                          # [8][Cin][Cout]: IODHW read with the channel roles exchanged
                C.call('hrnet_pack_weights3d', F32, w.data_ptr(), L['wd'].data_ptr(), L['cin'], L['cout'], 2, L['cin_p'],
                       L['cout_p'], 0, stream)
            else:
                C.call('hrnet_pack_weights3d_dgrad', F32, w.data_ptr(), L['wd'].data_ptr(), L['cout'], L['cin'], L['ks'],
                       L['cout_p'], L['gin_p'], stream)
            L['bias'][:L['cout']].copy_(m.bias.detach())
            if bn is not None:
                L['gamma'][:L['cout']].copy_(bn.weight.detach())
                L['beta'][:L['cout']].copy_(bn.bias.detach())
        self.key = key


class _TrainPlan:
    """the forward and the backward launches of one input shape, recorded once, and every buffer they use. The blocks'
    _emit methods drive conv / pool / deconv exactly as they drive _Plan; each call also leaves a tape entry, and the
    backward is recorded by walking the tape in reverse. Gradients of an activation with several consumers are
    summed without extra passes: an input-gradient convolution adds the sum so far through hrnet_conv3d's `res` (into a
    fresh buffer), the other kernels add in place."""

    def __init__(self, trainer, shape, add_shape, device, needs_x, needs_add, req):
        B, Cn, D, H, W = shape
        self.packed, self.device, self.B, self.shape, self.add_shape = trainer.packed, device, B, shape, add_shape
        self.req = req                               # parameter -> it requires a gradient
        self.fwd, self.bwd, self.tape, self.buffers = [], [], [], []
        self.stats, self.bn_floats, self.dz_floats, self.wg_bytes = [], 0, 0, 0
        self.generation = 0
        self.slots, self.gtotal = {}, 0              # parameter -> (offset, numel) in the flat gradient buffer
        for prm in trainer.params:
            if req[prm]:
                self.slots[prm] = (self.gtotal, prm.numel())
                self.gtotal += _pad(prm.numel(), 4)
        self.gflat = torch.zeros(max(self.gtotal, 1), dtype=torch.float32, device=device)
        self.cin_p = _pad(Cn, 4)
        self.x_in = self._buf((D, H, W), self.cin_p, Cn, needs_x)
        self.add_in = None
        if add_shape is not None:
            self.add_in = self._buf(tuple(add_shape[2:]), _pad(add_shape[1], 16), add_shape[1], needs_add)
        self.y_out = trainer.emit(self, self.x_in, self.add_in)
        self.J = self.y_out.real                     # the real output channels, from the layer that wrote y_out
        if self.y_out.needs:                         # else nothing requires a gradient: no backward is recorded
            self.y_out.grad = self._raw(self.y_out.ext, self.y_out.ch)
            for entry in reversed(self.tape):
                entry()
        self.tape = None
        # shared scratch, sized by the largest user: the launches are stream-ordered, one user at a time
        self.zeros = torch.zeros(4096, dtype=torch.float32, device=device)
        self.bn_scratch = torch.empty(max(self.bn_floats, 1), dtype=torch.float32, device=device)
        self.dz = torch.empty(max(self.dz_floats, 1), dtype=torch.float32, device=device)
        self.wg_scratch = torch.empty(max(self.wg_bytes // 4, 1), dtype=torch.float32, device=device)

    def _raw(self, ext, ch):
        D, H, W = ext
        t = torch.empty(self.B * D * H * W * ch, dtype=torch.float32, device=self.device)
        self.buffers.append(t)
        return t

    def _buf(self, ext, ch, real, needs):
        return _Act(self._raw(ext, ch), ext, ch, real, needs)

    def _wants(self, L):
        """a parameter of layer L (or of its BatchNorm) requires a gradient"""
        prms = [L['conv'].weight, L['conv'].bias] + ([L['bn'].weight, L['bn'].bias] if L['bn'] is not None else [])
        return any(self._gptr(prm) is not None for prm in prms)

    def _gptr(self, prm):
        if prm is None or prm not in self.slots:
            return None
        return self.gflat.data_ptr() + 4 * self.slots[prm][0]

    def _inplace(self, act):
        """(gradient buffer of act, accumulate flag) for a kernel that writes or adds in place"""
        if act.ch % 16:
            raise NotImplementedError('V2V training: an in-place gradient for {} channels'.format(act.ch))
        if act.grad is None:
            act.grad = self._raw(act.ext, act.ch)
            return act.grad, 0
        if act.shared:
            raise NotImplementedError('V2V training: a second consumer of a tensor whose gradient is passed through')
        return act.grad, 1

    def _norm(self, L, z, y, ext, relu, other, after):
        """batch statistics of z, then y = apply(z); returns the saved per-channel vectors"""
        bn, cout_p = L['bn'], L['cout_p']
        D, H, W = ext
        rows = self.B * D * H * W
        if rows < 2:
            raise ValueError('Expected more than 1 value per channel when training, got input size {}'.format(
                torch.Size([self.B, L['cout'], D, H, W])))
        vec = torch.empty(4 * cout_p, dtype=torch.float32, device=self.device)
        self.stats.append(vec)
        mean, invstd, scale, shift = (vec.data_ptr() + 4 * k * cout_p for k in range(4))
        parts = C.call('hrnet_bn3d_parts', rows)
        self.bn_floats = max(self.bn_floats, (2 * parts + 2) * cout_p)
        track = bn.track_running_stats and bn.running_mean is not None
        self.fwd.append(('hrnet_bn3d_stats', lambda: (
            F32, z.t.data_ptr(), L['gamma'].data_ptr(), L['beta'].data_ptr(), self.bn_scratch.data_ptr(), mean, invstd,
            scale, shift, bn.running_mean.data_ptr() if track else None, bn.running_var.data_ptr() if track else None,
            bn.num_batches_tracked.data_ptr() if track else None, self.B, D, H, W, cout_p, L['cout'],
            float(bn.momentum), float(bn.eps))))
        self.fwd.append(('hrnet_bn3d_apply', lambda: (
            F32, z.t.data_ptr(), scale, shift, None if other is None else other.t.data_ptr(), y.t.data_ptr(), self.B, D,
            H, W, cout_p, int(relu), int(after))))
        return mean, invstd, scale, shift

    def _bn_bwd(self, L, y, z, ext, saved, relu, recompute, res):
        """records dz (into self.dz) and the BatchNorm / bias gradients of layer L; routes g to a residual input"""
        m, bn, cout_p = L['conv'], L['bn'], L['cout_p']
        D, H, W = ext
        mean, invstd, scale, shift = saved
        dother, acc = (None, 0)
        if res is not None and res.needs:
            dother, acc = self._inplace(res)
        dy = y.grad
        self.dz_floats = max(self.dz_floats, self.B * D * H * W * cout_p)
        self.bwd.append(('hrnet_bn3d_bwd', lambda: (
            F32, dy.data_ptr(), z.t.data_ptr(), y.t.data_ptr() if relu and not recompute else None, scale, shift, mean,
            invstd, self.bn_scratch.data_ptr(), self.dz.data_ptr(), None if dother is None else dother.data_ptr(),
            self._gptr(bn.weight), self._gptr(bn.bias), self._gptr(m.bias), self.B, D, H, W, cout_p, L['cout'],
            int(recompute), acc, 0)))

    def conv(self, conv, bn, x, relu, res=None):
        L = self.packed.layers[conv]
        D, H, W = x.ext
        cin_p, cout_p, ks = L['cin_p'], L['cout_p'], L['ks']
        assert x.ch == cin_p and (res is None or (res.ext, res.ch) == (x.ext, cout_p)) and bn is L['bn']
        needs = x.needs or (res is not None and res.needs) or self._wants(L)
        z = self._buf(x.ext, cout_p, L['cout'], needs)
        self.fwd.append(('hrnet_conv3d', lambda: (F32, x.t.data_ptr(), L['w'].data_ptr(), None, L['bias'].data_ptr(),
                                                  None, z.t.data_ptr(), self.B, D, H, W, cin_p, cout_p, ks, 0)))
        if bn is None:
            assert not relu and res is None
            y, saved = z, None
        else:
            y = self._buf(x.ext, cout_p, L['cout'], needs)
            saved = self._norm(L, z, y, x.ext, relu, res, 0)

        def backward():
            if not y.needs:                          # nothing behind this layer requires a gradient
                return
            if y.grad is None:
                raise RuntimeError('V2V training: an output of the plan receives no gradient')
            if bn is None:
                parts = C.call('hrnet_bn3d_parts', self.B * D * H * W)
                self.bn_floats = max(self.bn_floats, (2 * parts + 2) * cout_p)
                dz = y.grad
                if self._gptr(conv.bias) is not None:
                    self.bwd.append(('hrnet_bn3d_bwd', lambda: (
                        F32, dz.data_ptr(), None, None, None, None, None, None, self.bn_scratch.data_ptr(), None, None,
                        None, None, self._gptr(conv.bias), self.B, D, H, W, cout_p, L['cout'], 0, 0, 0)))
                dzp = lambda: dz.data_ptr()
            else:
                self._bn_bwd(L, y, z, x.ext, saved, relu, False, res)
                dzp = lambda: self.dz.data_ptr()
            if self._gptr(conv.weight) is not None:
                self._wgrad_from(L, x, x.ext, dzp)
            if x.needs:
                prev = x.grad
                if prev is not None and x.ch != L['gin_p']:
                    raise NotImplementedError('V2V training: summing gradients of a {}-channel input'.format(x.ch))
                out = self._raw(x.ext, L['gin_p'])
                self.bwd.append(('hrnet_conv3d', lambda: (
                    F32, dzp(), L['wd'].data_ptr(), None, self.zeros.data_ptr(), None if prev is None else prev.data_ptr(),
                    out.data_ptr(), self.B, D, H, W, cout_p, L['gin_p'], ks, 0)))
                x.grad, x.shared = out, False
        self.tape.append(backward)
        return y

    def _wgrad_from(self, L, x, ext, dzp):
        m = L['conv']
        D, H, W = ext
        nbytes, nsplit = ctypes.c_int64(0), ctypes.c_int(0)
        deconv = int(L['transposed'])
        C.call('hrnet_conv3d_wgrad_scratch', F32, self.B, D, H, W, L['cin_p'], L['cout_p'], L['ks'], deconv,
               ctypes.byref(nbytes), ctypes.byref(nsplit), None)
        self.wg_bytes = max(self.wg_bytes, nbytes.value)
        self.bwd.append(('hrnet_conv3d_wgrad', lambda: (
            F32, x.t.data_ptr(), dzp(), self.wg_scratch.data_ptr(), self.wg_scratch.numel() * 4, self._gptr(m.weight),
            self.B, D, H, W, L['cin_p'], L['cout_p'], L['cin'], L['cout'], L['ks'], deconv, 0)))

    def pool(self, x):
        D, H, W = x.ext
        y = self._buf((D // 2, H // 2, W // 2), x.ch, x.real, x.needs)
        self.fwd.append(('hrnet_maxpool3d', lambda: (F32, x.t.data_ptr(), y.t.data_ptr(), self.B, D, H, W, x.ch)))

        def backward():
            if x.needs:
                dx, acc = self._inplace(x)
                dy = y.grad
                self.bwd.append(('hrnet_maxpool3d_bwd', lambda: (F32, x.t.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                                                                 self.B, D, H, W, x.ch, acc)))
        self.tape.append(backward)
        return y

    def deconv(self, conv, bn, x, add):
        L = self.packed.layers[conv]
        D, H, W = x.ext
        ext = (2 * D, 2 * H, 2 * W)
        cin_p, cout_p = L['cin_p'], L['cout_p']
        assert x.ch == cin_p and L['ks'] == 2 and bn is L['bn'] and bn is not None
        assert add is None or (add.ext, add.ch) == (ext, cout_p)
        needs = x.needs or (add is not None and add.needs) or self._wants(L)
        z, y = self._buf(ext, cout_p, L['cout'], needs), self._buf(ext, cout_p, L['cout'], needs)
        self.fwd.append(('hrnet_deconv3d_k2s2', lambda: (F32, x.t.data_ptr(), L['w'].data_ptr(), None,
                                                         L['bias'].data_ptr(), None, z.t.data_ptr(), self.B, D, H, W,
                                                         cin_p, cout_p, 0)))
        saved = self._norm(L, z, y, ext, True, add, 1)

        def backward():
            if not y.needs:
                return
            if add is not None and add.needs:        # d (relu(..) + add) / d add = 1: the incoming gradient itself
                if add.grad is not None:
                    raise NotImplementedError('V2V training: a second consumer of the tensor added after an upsample')
                add.grad, add.shared = y.grad, True
            self._bn_bwd(L, y, z, ext, saved, True, add is not None, None)
            if self._gptr(conv.weight) is not None:
                self._wgrad_from(L, x, x.ext, lambda: self.dz.data_ptr())
            if x.needs:
                dx, acc = self._inplace(x)
                self.bwd.append(('hrnet_deconv3d_k2s2_dgrad', lambda: (F32, self.dz.data_ptr(), L['wd'].data_ptr(),
                                                                       dx.data_ptr(), self.B, D, H, W, cin_p, cout_p,
                                                                       acc)))
        self.tape.append(backward)
        return y

    def freeze(self):
        """the argument tuples, built once every buffer exists"""
        self.fwd = [(name, args()) for name, args in self.fwd]
        self.bwd = [(name, args()) for name, args in self.bwd]

    def run_forward(self, x, add):
        B, Cn, D, H, W = self.shape
        stream = C.stream_ptr()
        self.generation += 1
        C.call('hrnet_nchw_to_nhwc', F32, x.data_ptr(), self.x_in.t.data_ptr(), B, D * H, W, self.cin_p, Cn, stream)
        if add is not None:
            a = self.add_in
            C.call('hrnet_nchw_to_nhwc', F32, add.data_ptr(), a.t.data_ptr(), B, a.ext[0] * a.ext[1], a.ext[2], a.ch,
                   self.add_shape[1], stream)
        for name, args in self.fwd:
            C.call(name, *args, stream)
        o = self.y_out
        out = torch.empty((B, self.J) + tuple(o.ext), dtype=torch.float32, device=self.device)
        C.call('hrnet_nhwc_to_nchw', F32, o.t.data_ptr(), out.data_ptr(), B, o.ext[0] * o.ext[1], o.ext[2], o.ch, self.J,
               stream)
        return out

    def run_backward(self, gout):
        B, Cn, D, H, W = self.shape
        stream = C.stream_ptr()
        o = self.y_out
        C.call('hrnet_nchw_to_nhwc', F32, gout.data_ptr(), o.grad.data_ptr(), B, o.ext[0] * o.ext[1], o.ext[2], o.ch,
               self.J, stream)
        for name, args in self.bwd:
            C.call(name, *args, stream)
        dx = dadd = None
        if self.x_in.needs:
            dx = torch.empty(self.shape, dtype=torch.float32, device=self.device)
            C.call('hrnet_nhwc_to_nchw', F32, self.x_in.grad.data_ptr(), dx.data_ptr(), B, D * H, W,
                   _pad(self.cin_p, 16), Cn, stream)
        a = self.add_in
        if a is not None and a.needs:
            dadd = torch.empty(self.add_shape, dtype=torch.float32, device=self.device)
            C.call('hrnet_nhwc_to_nchw', F32, a.grad.data_ptr(), dadd.data_ptr(), B, a.ext[0] * a.ext[1], a.ext[2], a.ch,
                   self.add_shape[1], stream)
        return dx, dadd, self.gflat.clone()          # a fresh tensor: autograd may keep it as .grad


class _TrainFn(torch.autograd.Function):
    """the whole network as one autograd node: forward(plan, x, add, *parameters) -> y"""

    @staticmethod
    def forward(ctx, plan, x, add, *params):
        ctx.plan = plan
        out = plan.run_forward(x, add)
        ctx.generation, ctx.key = plan.generation, plan.packed.key
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        plan = ctx.plan
        if plan.generation != ctx.generation:
            raise RuntimeError('V2V training: a later forward of the same input shape has overwritten what this backward '
                               'needs (the saved activations belong to the shape\'s plan); call backward() before the '
                               'next forward')
        if plan.packed.key != ctx.key or _TrainPacked.param_key(plan.params) != ctx.key:
            raise RuntimeError('V2V training: a parameter was modified (or the weights were packed again for another '
                               'forward) between this forward and its backward; the backward would use weights the '
                               'forward did not')
        with torch.cuda.device(plan.device):
            dx, dadd, flat = plan.run_backward(gout.contiguous().float())
        grads = []
        for prm in plan.params:
            slot = plan.slots.get(prm)
            grads.append(None if slot is None else flat[slot[0]:slot[0] + slot[1]].view(prm.shape))
        return (None, dx, dadd) + tuple(grads)


class _Trainer:
    """the training path of a list of modules: emit(plan, x, add) walks them. Owns the packed copies and the plans."""

    def __init__(self, modules, emit, what):
        self.modules, self.emit, self.what = modules, emit, what
        self.params, seen = [], set()
        for root in modules:
            for prm in root.parameters():
                if id(prm) not in seen:
                    seen.add(id(prm))
                    self.params.append(prm)
        self.packed, self.plans = None, {}

    def __call__(self, x, add=None):
        from core.loss import _dev_f32
        x = _dev_f32(x, self.what)
        if add is not None:
            add = _dev_f32(add, self.what)
        tensors = self.params + [b for root in self.modules for b in root.buffers()]
        if any(t.device != x.device for t in tensors):
            raise ValueError('{}: the parameters are not on the input\'s device {}'.format(self.what, x.device))
        with torch.cuda.device(x.device):
            if self.packed is None or self.packed.device != x.device:
                self.packed, self.plans = _TrainPacked(self.modules, x.device), {}
            key = _TrainPacked.param_key(self.params)
            if self.packed.key != key:
                self.packed.refresh(key)
            grad = torch.is_grad_enabled()
            req = {prm: grad and prm.requires_grad for prm in self.params}
            pkey = (tuple(x.shape), None if add is None else tuple(add.shape), grad and x.requires_grad,
                    grad and add is not None and add.requires_grad, tuple(req[prm] for prm in self.params),
                    tuple(t.data_ptr() for t in tensors))
            plan = self.plans.get(pkey)
            if plan is None:
                if len(self.plans) >= 8:
                    self.plans.clear()
                plan = _TrainPlan(self, tuple(x.shape), None if add is None else tuple(add.shape), x.device, pkey[2],
                                  pkey[3], req)
                plan.params = self.params
                plan.freeze()
                self.plans[pkey] = plan
            return _TrainFn.apply(plan, x, add, *self.params)


def train_blocks(blocks, x, add=None):
    """the training path (batch statistics, autograd) over V2V blocks in sequence - what V2VModel(trainable=True) does
    for the whole network, for one or a few blocks; `add` is the tensor an Upsample3DBlock at the end adds after its
    ReLU. The blocks must be in training mode and on x's device."""
    blocks = list(blocks)
    if not all(b.training for b in blocks):
        raise NotImplementedError('train_blocks: eval mode (the backward through running statistics is not built)')
    trainer = getattr(blocks[0], '_block_trainer', None)
    if trainer is None or trainer.modules != blocks:
        def emit(plan, t, a):
            for b in blocks[:-1]:
                t = b._emit(plan, t)
            return blocks[-1]._emit(plan, t, a) if a is not None else blocks[-1]._emit(plan, t)
        trainer = _Trainer(blocks, emit, 'train_blocks')
        object.__setattr__(blocks[0], '_block_trainer', trainer)
    return trainer(x, add)


class V2VModel(nn.Module):
    """(B, input_channels, D, H, W) -> (B, output_channels, D, H, W) float32 (v2v.py:141-180); D, H and W multiples
    of 32. Eval mode under torch.no_grad() is the inference path. trainable=True adds the training-mode forward (batch
    statistics, running statistics updated on the device) and the backward; eval mode with a gradient required stays
    refused either way, because the backward through the running statistics is not built. See the module docstring."""

    def __init__(self, input_channels, output_channels, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self._trainer = None
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
        if self.training and not self.trainable:
            raise NotImplementedError('V2VModel: the training-mode forward (batch statistics) is not built; call '
                                      '.eval() - BatchNorm then uses its running statistics')
        wants = torch.is_grad_enabled() and (getattr(x, 'requires_grad', False) or
                                             any(p.requires_grad for p in self.parameters()))
        if wants and not self.training and self.trainable:
            raise NotImplementedError('V2VModel(trainable=True): eval mode with a gradient required is refused - the '
                                      'backward through the running statistics is not built; call .train(), or run '
                                      'under torch.no_grad()')
        if wants and not self.training:
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
        if self.training and x.shape[0] * (x.shape[2] >> LEVELS) * (x.shape[3] >> LEVELS) * (x.shape[4] >> LEVELS) == 1:
            # torch's own refusal, for the BatchNorm3d of the bottom level
            raise ValueError('Expected more than 1 value per channel when training, got input size {}'.format(
                torch.Size([1, EncoderDecorder.WIDTHS[LEVELS], 1, 1, 1])))
        if not x.is_cuda:
            raise ValueError('V2VModel: expected a HIP-device tensor (there is no CPU path in this build)')

    def _emit(self, plan, t, add=None):
        for blk in self.front_layers:
            t = blk._emit(plan, t)
        t = self.encoder_decoder._emit(plan, t)
        for blk in self.back_layers:
            t = blk._emit(plan, t)
        return plan.conv(self.output_layer, None, t, relu=False)

    def forward(self, x):
        self._refuse(x)
        if self.training:
            if self._trainer is None:
                self._trainer = _Trainer([self], self._emit, 'V2VModel')
            # the kernels update the running statistics through their addresses, which moves no version counter: drop
            # what the inference path folded from them (train() does so too; this also covers a bare `training = True`)
            self._packed, self._plans = None, {}
            return self._trainer(x)
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
