"""The NHWC convolution, BatchNorm and layout layer ops of the heads (SwinPose's decoder, HamNet, the aggregation head of
pose_hrnet_PoseAggr) over the C ABI, f32 and, where an op says so, bf16: the one home of every launch of

    hrnet_pack_weights, hrnet_conv2d (eager.ConvBN's, which also writes BatchNorm row sums, aside),
    hrnet_conv2d_dilated3x3, hrnet_conv2d_wgrad + hrnet_wgrad_reduce (eager.DilatedConv's tap-by-tap one aside),
    hrnet_bias_grad,
    hrnet_bn3d_stats / _apply / _bwd on a 2-D map, hrnet_nchw_to_nhwc, hrnet_nhwc_to_nchw

in lib/hipnet. Three layers:

  guards and small helpers, used by every op module
    check(name, **tensors)   HIP-device float32 tensors only (a CPU tensor is a ValueError: there is no CPU path)
    check_nhwc(name, x)  pad16(c)  padded(v, n)  contiguous(t)  wants_grad(*ts)

  raw launchers: no argument checks, no autograd; the autograd Functions and plan builders of the op modules call them.
  `dtype` is the C ABI's id (F32, BF16). Each runs under torch.cuda.device of its input.
    pack(w, o, i, ks, op, ip, mode, dtype)      pack_taps(w, o, i, op, ip, mode, dtype)
    conv(x, packed, cout, ks, ...)              conv3x3_taps(x, taps, cout, dilation)
    wgrad(x, dy, ks, stride, o_real, i_real)    bias_grad(dy, real)
    bn_batch_forward(z, gamma, beta, bn, real, count_batches)    bn_batch_backward(gy, z, y, vec, scratch, real, ...)
    nchw_to_nhwc(x, cp, dtype)                  nhwc_to_nchw(y, c)

  checked public ops: shapes are checked before any device call
    conv_pack(weight, cin_pad, cout_pad, scale)   conv_transpose_pack(weight, cin_pad, cout_pad)
    conv_nhwc(x, packed, cout, ks, ...)           heatmap_softmax(y, joints, temp)        inference: a required gradient
                                                                                          is a NotImplementedError
    conv1x1_train(x, conv, relu_out)              Conv2d 1x1 (+ bias) (+ ReLU) under autograd; the ReLU's backward is
                                                  hrnet_grad_term with coef NULL
    to_nhwc(x, cp, dtype)   to_nchw(y, joints)    the layout ops under autograd, f32 or bf16 maps: the backward of each is
                                                  the other (ToNHWC and ToNCHW are their Functions, unchecked)

The maps are NHWC (B, H, W, Cp) with the real channels first and the pad channels zero, in and out.
"""
import torch

from hipnet import _capi as C

F32, BF16 = C.HR_F32, C.HR_BF16
_TORCH = {F32: torch.float32, BF16: torch.bfloat16}


# ----------------------------------------------------------------------------------------- guards and small helpers
def _on_device(name, k, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError('{}: {} must be a HIP-device tensor (there is no CPU path in this build)'.format(name, k))


def check(name, **tensors):
    for k, t in tensors.items():
        if t is None:
            continue
        _on_device(name, k, t)
        if t.dtype != torch.float32:
            raise ValueError('{}: {} is {}: float32 only'.format(name, k, t.dtype))


def check_nhwc(name, x):
    if x.ndim != 4 or x.numel() == 0 or x.shape[3] % 16:
        raise ValueError('{}: x {}: expected NHWC (B, H, W, C) with C a multiple of 16, nothing empty'.format(
            name, tuple(x.shape)))


def pad16(c):
    return (int(c) + 15) // 16 * 16


def padded(v, n):
    out = torch.zeros(n, dtype=torch.float32, device=v.device)
    out[:v.numel()] = v.detach().float().reshape(-1)
    return out


def contiguous(t):
    return None if t is None else t.contiguous()


def wants_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _no_grad(name, *ts):
    if wants_grad(*ts):
        raise NotImplementedError('{}: backward is not built (this op is inference only; conv1x1_train is the training '
                                  'one): run under torch.no_grad()'.format(name))


def _d(t):
    return None if t is None else t.detach().contiguous()


# --------------------------------------------------------------------------------------------------- raw launchers
def pack(w, o, i, ks, op, ip, mode, dtype=F32):
    """hrnet_pack_weights of the f32 w read as OIHW (o, i, ks, ks), into `dtype`; mode 0: [op][ks ks][ip], mode 1:
    [ip][ks ks flipped][op]"""
    out = torch.empty(op * ks * ks * ip, dtype=_TORCH[dtype], device=w.device)
    with torch.cuda.device(w.device):
        C.call('hrnet_pack_weights', dtype, w.data_ptr(), out.data_ptr(), o, i, ks, op, ip, mode, C.stream_ptr())
    return out


def pack_taps(w, o, i, op, ip, mode, dtype=F32):
    """3x3 OIHW weight -> nine packed 1x1 matrices, one pack and a permute. mode 0: [9][op][ip], tap t = 3 r + s (the
    forward); mode 1: [9][ip][op], the transposed weights in reversed tap order (the input gradient)"""
    rows, cols = (op, ip) if mode == 0 else (ip, op)
    return pack(w, o, i, 3, op, ip, mode, dtype).reshape(rows, 9, cols).permute(1, 0, 2).contiguous()


def conv(x, packed, cout, ks, stride=1, upz=False, bias=None, in_affine=None, in_relu=False, into=None, dtype=F32):
    """hrnet_conv2d on an NHWC map: ks 1; ks 3 (padding 1) at stride 1 or 2; ks 3 with upz (the input read zero-stuffed,
    output 2 H x 2 W). bias (cout,); in_affine: a per-input-channel (scale, shift), applied with in_relu when x is loaded;
    into: accumulate into this (B, Ho, Wo, cout) tensor instead of writing a new one"""
    B, H, W, cin = x.shape
    Ho, Wo = (2 * H, 2 * W) if upz else (H // stride, W // stride)
    y = torch.empty((B, Ho, Wo, cout), dtype=_TORCH[dtype], device=x.device) if into is None else into
    scale, shift = (None, None) if in_affine is None else in_affine
    with torch.cuda.device(x.device):
        C.call('hrnet_conv2d', dtype, x.data_ptr(), packed.data_ptr(), C.ptr(scale), C.ptr(shift), C.ptr(bias), y.data_ptr(),
               None, B, H, W, cin, Ho, Wo, cout, ks, 2 if upz else stride, 1 if upz else 0, 1 if in_relu else 0,
               0 if into is None else 1, C.stream_ptr())
    return y


def conv3x3_taps(x, taps, cout, dilation=1):
    """a 3x3 convolution (padding = dilation, no bias) as nine 1x1 launches over displaced windows that accumulate into y
    (hrnet_conv2d_dilated3x3): nine sums of Cin terms in place of one of 9 Cin. x (B, H, W, Cin) as it is (no prologue),
    taps [9][>= cout][Cin] of pack_taps in x's dtype"""
    B, H, W, cin = x.shape
    y = torch.empty((B, H, W, cout), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        C.call('hrnet_conv2d_dilated3x3', C.dtype_id(x.dtype), x.data_ptr(), taps.data_ptr(),
               taps.stride(0) * taps.element_size(), y.data_ptr(), B, H, W, cin, cout, dilation, C.stream_ptr())
    return y


def wgrad(x, dy, ks, stride, o_real, i_real):
    """weight gradient (o_real, i_real, ks, ks) f32 of dy = conv(x): x (B, H, W, Cin), dy (B, Ho, Wo, Cout) in x's dtype;
    slabs + reduce"""
    B, H, W, cin = x.shape
    _, Ho, Wo, cout = dy.shape
    dt = C.dtype_id(x.dtype)
    with torch.cuda.device(x.device):
        ns = C.call('hrnet_wgrad_splits', dt, B, Ho, Wo, cout, cin, ks, stride)
        slabs = torch.empty(ns * cout * ks * ks * cin, dtype=torch.float32, device=x.device)
        C.call('hrnet_conv2d_wgrad', dt, x.data_ptr(), dy.data_ptr(), None, None, slabs.data_ptr(), B, H, W, cin, Ho, Wo,
               cout, ks, stride, 0, ns, C.stream_ptr())
        gw = torch.empty((o_real, i_real, ks, ks), dtype=torch.float32, device=x.device)
        C.call('hrnet_wgrad_reduce', slabs.data_ptr(), gw.data_ptr(), ns, cout, cin, ks, o_real, i_real, 0, 0,
               C.stream_ptr())
    return gw


def bias_grad(dy, real):
    """the sum of the f32 dy (..., Cp) over its pixels, first `real` channels"""
    pixels, cp = dy.numel() // dy.shape[-1], dy.shape[-1]
    blocks = C.call('hrnet_reduce_blocks', 1, 1, pixels, cp)
    scratch = torch.empty(blocks * cp, dtype=torch.float32, device=dy.device)
    db = torch.empty(real, dtype=torch.float32, device=dy.device)
    with torch.cuda.device(dy.device):
        C.call('hrnet_bias_grad', F32, dy.data_ptr(), db.data_ptr(), scratch.data_ptr(), pixels, cp, real, 0, C.stream_ptr())
    return db


def bn_batch_forward(z, gamma, beta, bn, real, count_batches):
    """relu(BatchNorm2d(z)) on the batch statistics of the f32 map z (B, H, W, cp), `real` channels: (y, vec, scratch).
    vec (4, cp) holds mean, invstd, scale and shift; scratch is what bn_batch_backward reads. bn's running statistics are
    updated through their pointers with bn.momentum; num_batches_tracked is incremented only with count_batches"""
    B, H, W, cp = z.shape
    parts = C.call('hrnet_bn3d_parts', B * H * W)
    scratch = torch.empty((2 * parts + 2) * cp, dtype=torch.float32, device=z.device)
    vec = torch.empty((4, cp), dtype=torch.float32, device=z.device)
    track = bn.track_running_stats and bn.running_mean is not None
    gamma_p, beta_p = padded(gamma, cp), padded(beta, cp)              # zero in the pad channels: they stay zero
    y = torch.empty_like(z)
    with torch.cuda.device(z.device):
        C.call('hrnet_bn3d_stats', F32, z.data_ptr(), gamma_p.data_ptr(), beta_p.data_ptr(), scratch.data_ptr(),
               vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(),
               bn.running_mean.data_ptr() if track else None, bn.running_var.data_ptr() if track else None,
               bn.num_batches_tracked.data_ptr() if track and count_batches else None, B, 1, H, W, cp, real,
               float(bn.momentum if bn.momentum is not None else 0.1), float(bn.eps), C.stream_ptr())
        C.call('hrnet_bn3d_apply', F32, z.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), None, y.data_ptr(), B, 1, H, W,
               cp, 1, 0, C.stream_ptr())
    return y, vec, scratch


def bn_batch_backward(gy, z, y, vec, scratch, real, want_gamma, want_beta, want_conv_bias):
    """the backward of bn_batch_forward: (dz, dgamma, dbeta, dbias), None for what is not wanted; dbias is the gradient
    of a bias added to z by the convolution in front (the sum of dz)"""
    B, H, W, cp = z.shape
    new = lambda want: torch.empty(real, dtype=torch.float32, device=z.device) if want else None
    dgamma, dbeta, dbias = new(want_gamma), new(want_beta), new(want_conv_bias)
    dz = torch.empty_like(z)
    with torch.cuda.device(z.device):
        C.call('hrnet_bn3d_bwd', F32, gy.data_ptr(), z.data_ptr(), y.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(),
               vec[0].data_ptr(), vec[1].data_ptr(), scratch.data_ptr(), dz.data_ptr(), None, C.ptr(dgamma), C.ptr(dbeta),
               C.ptr(dbias), B, 1, H, W, cp, real, 0, 0, 0, C.stream_ptr())
    return dz, dgamma, dbeta, dbias


def nchw_to_nhwc(x, cp, dtype):
    """f32 NCHW x (B, C, H, W) -> NHWC (B, H, W, cp) in `dtype`, zero pad channels"""
    B, Cc, H, W = x.shape
    y = torch.empty((B, H, W, cp), dtype=_TORCH[dtype], device=x.device)
    with torch.cuda.device(x.device):
        C.call('hrnet_nchw_to_nhwc', dtype, x.data_ptr(), y.data_ptr(), B, H, W, cp, Cc, C.stream_ptr())
    return y


def nhwc_to_nchw(y, c):
    """NHWC y (B, H, W, Cp), f32 or bf16 -> its first c channels as f32 NCHW (B, c, H, W)"""
    B, H, W, cp = y.shape
    x = torch.empty((B, c, H, W), dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        C.call('hrnet_nhwc_to_nchw', C.dtype_id(y.dtype), y.data_ptr(), x.data_ptr(), B, H, W, cp, c, C.stream_ptr())
    return x


# ---------------------------------------------------------------------------------------------- checked public ops
def _pads(name, ci, co, cin_pad, cout_pad):
    cip = ci if cin_pad is None else int(cin_pad)
    cop = pad16(co) if cout_pad is None else int(cout_pad)
    if cip < ci or cip % 4 or cop < co or cop % 16:
        raise ValueError('{}: Cin = {} in {}, Cout = {} in {}: the padded counts must hold the real ones and be multiples '
                         'of 4 (in) and 16 (out)'.format(name, ci, cip, co, cop))
    return cip, cop


def conv_pack(weight, cin_pad=None, cout_pad=None, scale=None):
    """a Conv2d weight (Cout, Cin, ks, ks), optionally scaled per output channel (in float64), packed to
    [cout_pad][ks ks][cin_pad] (hrnet_pack_weights mode 0), zeros in the padding"""
    check('conv_pack', weight=weight)
    if scale is not None:
        _on_device('conv_pack', 'scale', scale)
    if weight.ndim != 4 or weight.shape[2] != weight.shape[3] or (scale is not None and scale.numel() != weight.shape[0]):
        raise ValueError('conv_pack: weight {}: expected (Cout, Cin, ks, ks), and a scale of Cout values if one is '
                         'given'.format(tuple(weight.shape)))
    co, ci, ks, _ = weight.shape
    cip, cop = _pads('conv_pack', ci, co, cin_pad, cout_pad)
    w = _d(weight)
    if scale is not None:
        w = (w.double() * scale.detach().double().reshape(-1, 1, 1, 1)).float()
    return pack(w, co, ci, ks, cop, cip, 0)


def conv_transpose_pack(weight, cin_pad=None, cout_pad=None):
    """a ConvTranspose2d(Cin, Cout, 3, 2, 1, 1) weight (Cin, Cout, 3, 3) is the OIHW weight of the stride-2 convolution
    whose input gradient the layer is: packed by hrnet_pack_weights mode 1 to [cout_pad][9 flipped][cin_pad], zeros in the
    padding"""
    check('conv_transpose_pack', weight=weight)
    if weight.ndim != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError('conv_transpose_pack: weight {}: expected (Cin, Cout, 3, 3)'.format(tuple(weight.shape)))
    ci, co = weight.shape[:2]
    cip, cop = _pads('conv_transpose_pack', ci, co, cin_pad, cout_pad)
    return pack(_d(weight), ci, co, 3, cip, cop, 1)


def conv_nhwc(x, packed, cout, ks, up=False, bias=None, in_affine=None, in_relu=False, into=None):
    """f32 NHWC convolution on hrnet_conv2d: x (B, H, W, Cin), packed weights of conv_pack (ks 1) or conv_transpose_pack
    (ks 3 with up=True: the input is read zero-stuffed, the output is (B, 2 H, 2 W, cout)); bias (cout,); in_affine: a
    per-input-channel (scale, shift) applied with in_relu to x on load (the producer's folded BatchNorm); into: accumulate
    into this (B, Ho, Wo, cout) tensor instead of writing a new one"""
    in_scale, in_shift = (None, None) if in_affine is None else in_affine
    check('conv_nhwc', x=x, packed=packed, bias=bias, in_scale=in_scale, in_shift=in_shift, into=into)
    if x.ndim != 4 or x.numel() == 0 or x.shape[3] % 4 or cout % 16 or (ks, bool(up)) not in ((1, False), (3, True)):
        raise ValueError('conv_nhwc: x {}, cout = {}, ks = {}, up = {}: expected (B, H, W, Cin) with Cin a multiple of 4, '
                         'cout a multiple of 16, and a 1x1 or a transposed 3x3'.format(tuple(x.shape), cout, ks, up))
    B, H, W, cin = x.shape
    if packed.numel() != cout * ks * ks * cin:
        raise ValueError('conv_nhwc: {} packed weights for cout = {}, ks = {}, Cin = {}'.format(
            packed.numel(), cout, ks, cin))
    if (in_scale is None) != (in_shift is None) or (
            in_scale is not None and (in_scale.numel() != cin or in_shift.numel() != cin)):
        raise ValueError('conv_nhwc: in_affine: expected None or a (scale, shift) of ({},) each'.format(cin))
    if bias is not None and bias.numel() != cout:
        raise ValueError('conv_nhwc: bias has {} values for cout = {}'.format(bias.numel(), cout))
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    if into is not None and (tuple(into.shape) != (B, Ho, Wo, cout) or not into.is_contiguous()):
        raise ValueError('conv_nhwc: into {}: expected a contiguous ({}, {}, {}, {})'.format(
            tuple(into.shape), B, Ho, Wo, cout))
    _no_grad('conv_nhwc', x, bias, in_scale, in_shift, into)
    return conv(_d(x), packed, cout, ks, upz=bool(up), bias=_d(bias), in_affine=(_d(in_scale), _d(in_shift)),
                in_relu=in_relu, into=into)


def heatmap_softmax(y, joints, temp):
    """y (B, H, W, Cp) NHWC with the joints in the first channels -> NCHW (B, joints, H, W) softmax(y * temp) per map"""
    check('heatmap_softmax', y=y, temp=temp)
    if y.ndim != 4 or y.numel() == 0 or not 1 <= joints <= y.shape[3] or temp.numel() != 1:
        raise ValueError('heatmap_softmax: y {}, joints = {}, temp {}: expected (B, H, W, Cp >= joints) and one '
                         'temperature'.format(tuple(y.shape), joints, tuple(temp.shape)))
    _no_grad('heatmap_softmax', y, temp)
    temp = _d(temp)
    z = nhwc_to_nchw(_d(y), joints)
    out = torch.empty_like(z)
    with torch.cuda.device(z.device):
        C.call('hrnet_spatial_softmax_fwd', z.data_ptr(), temp.data_ptr(), out.data_ptr(), z.shape[0] * joints,
               z.shape[2] * z.shape[3], C.stream_ptr())
    return out


class _Conv1x1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, relu, cop):
        o, i = w.shape[:2]
        y = conv(x, pack(w, o, i, 1, cop, x.shape[3], 0), cop, 1, bias=None if b is None else padded(b, cop))
        if relu:
            y.relu_()
        ctx.save_for_backward(x, w, y if relu else None)
        ctx.relu, ctx.has_bias = relu, b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        nx, nw, nb = ctx.needs_input_grad[:3]
        nb = nb and ctx.has_bias
        o, i = w.shape[:2]
        gy = gy.contiguous().float()
        B, H, W, cop = gy.shape
        if ctx.relu:
            dz = torch.empty_like(gy)
            with torch.cuda.device(x.device):
                C.call('hrnet_grad_term', F32, dz.data_ptr(), gy.data_ptr(), y.data_ptr(), None, None, None, None, B, H, W,
                       cop, 0, 0, 0, C.stream_ptr())
            gy = dz
        dx = conv(gy, pack(w, o, i, 1, cop, x.shape[3], 1), x.shape[3], 1) if nx else None
        dw = wgrad(x, gy, 1, 1, o, i) if nw else None
        db = bias_grad(gy, o) if nb else None
        return dx, dw, db, None, None


def conv1x1_train(x, conv, relu_out=False):
    """Conv2d(ci, co, 1) with or without bias, then ReLU if relu_out, on x (B, H, W, cip) f32 NHWC -> (B, H, W, pad16(co)),
    pad channels zero"""
    check('conv1x1_train', x=x, weight=conv.weight, bias=conv.bias)
    check_nhwc('conv1x1_train', x)
    co, ci = conv.weight.shape[:2]
    if tuple(conv.weight.shape[2:]) != (1, 1) or x.shape[3] < ci:
        raise ValueError('conv1x1_train: x {}, weight {}: expected Cin <= C and (Cout, Cin, 1, 1)'.format(
            tuple(x.shape), tuple(conv.weight.shape)))
    return _Conv1x1Fn.apply(contiguous(x), contiguous(conv.weight), contiguous(conv.bias), bool(relu_out), pad16(co))


class ToNHWC(torch.autograd.Function):
    """f32 NCHW -> NHWC in the torch dtype `dtype`, channels zero-padded to cp; no argument checks"""

    @staticmethod
    def forward(ctx, x, cp, dtype):
        ctx.channels = x.shape[1]
        return nchw_to_nhwc(x.contiguous(), cp, C.dtype_id(dtype))

    @staticmethod
    def backward(ctx, gy):
        return (nhwc_to_nchw(gy.contiguous(), ctx.channels) if ctx.needs_input_grad[0] else None), None, None


class ToNCHW(torch.autograd.Function):
    """NHWC, f32 or bf16 -> its first c channels as f32 NCHW; the backward zeroes the pad channels; no argument checks"""

    @staticmethod
    def forward(ctx, y, c):
        ctx.cp, ctx.dtype = y.shape[3], y.dtype
        return nhwc_to_nchw(y.contiguous(), c)

    @staticmethod
    def backward(ctx, gx):
        return nchw_to_nhwc(gx.contiguous().float(), ctx.cp, C.dtype_id(ctx.dtype)), None


def to_nhwc(x, cp, dtype=torch.float32):
    """x (B, C, H, W) f32 NCHW -> (B, H, W, cp) NHWC in `dtype` (float32 or bfloat16), cp >= C a multiple of 16, zero pad
    channels"""
    check('to_nhwc', x=x)
    if x.ndim != 4 or x.numel() == 0 or cp % 16 or cp < x.shape[1]:
        raise ValueError('to_nhwc: x {}, cp = {}: expected (B, C, H, W), nothing empty, cp >= C a multiple of 16'.format(
            tuple(x.shape), cp))
    if wants_grad(x):
        return ToNHWC.apply(x, int(cp), dtype)
    return nchw_to_nhwc(x.detach().contiguous(), int(cp), C.dtype_id(dtype))


def to_nchw(y, joints):
    """y (B, H, W, Cp) NHWC, float32 or bfloat16 -> its first `joints` channels as f32 NCHW (B, joints, H, W); the backward
    zeroes the pad channels"""
    if isinstance(y, torch.Tensor) and y.dtype == torch.bfloat16:
        _on_device('to_nchw', 'y', y)
    else:
        check('to_nchw', y=y)
    if y.ndim != 4 or y.numel() == 0 or not 1 <= joints <= y.shape[3]:
        raise ValueError('to_nchw: y {}, joints = {}: expected (B, H, W, Cp >= joints)'.format(tuple(y.shape), joints))
    return ToNCHW.apply(y, int(joints))
