"""Swin ops of swin_transformer over the C ABI (csrc/swin.hip), forward only,

    window_attention(qkv, qkv_bias, bias_table, H, W, heads, ws, shift, scale)   hrnet_swin_attention
    merge_ln(x, H, W, weight, bias, eps)                                         hrnet_swin_merge_ln
    patch_rows(x, p)                                                             hrnet_swin_patch_rows
    conv_transpose_pack(weight) / conv_pack(weight, cout_pad) / conv_nhwc(...)   hrnet_pack_weights, hrnet_conv2d (f32)
    heatmap_softmax(y, joints, temp)                                             hrnet_nhwc_to_nchw, hrnet_spatial_softmax_fwd

HIP-device float32 tensors only (a CPU tensor is a ValueError: there is no CPU path). Shapes are checked before any device
call. There is no autograd here: an input that requires grad while grad is enabled raises NotImplementedError.
"""
import torch

from hipnet import _capi as C

OP_ATTENTION, OP_MERGE, OP_EMBED = (C.VALUES['HR_SWIN_' + n] for n in ('ATTENTION', 'MERGE', 'EMBED'))


def _check(name, **tensors):
    for k, t in tensors.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError('{}: {} must be a HIP-device tensor (there is no CPU path in this build)'.format(name, k))
        if t.dtype != torch.float32:
            raise ValueError('{}: {} is {}: float32 only'.format(name, k, t.dtype))


def _no_grad(name, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise NotImplementedError('{}: backward is not built (swin_transformer is inference only): run under '
                                  'torch.no_grad()'.format(name))


def _d(t):
    return None if t is None else t.detach().contiguous()


def supported(op, a, b=0):
    return bool(C.call('hrnet_swin_supported', int(op), int(a), int(b)))


def window_attention(qkv, qkv_bias, bias_table, H, W, heads, ws, shift, scale):
    """qkv (B, H * W, 3 * heads * hd) of the unpadded tokens, qkv_bias (3 * heads * hd,), bias_table ((2 ws - 1)^2, heads)
    -> (B, H * W, heads * hd): shifted-window attention in token order (padding, roll, mask and bias inside the kernel)"""
    _check('window_attention', qkv=qkv, qkv_bias=qkv_bias, bias_table=bias_table)
    H, W, heads, ws, shift = int(H), int(W), int(heads), int(ws), int(shift)
    if qkv.ndim == 5:
        qkv = qkv.reshape(qkv.shape[0], qkv.shape[1], -1)
    if qkv.ndim != 3 or qkv.numel() == 0 or heads < 1 or H < 1 or W < 1 or qkv.shape[1] != H * W \
            or qkv.shape[2] % (3 * heads):
        raise ValueError('window_attention: qkv {} with H = {}, W = {}, {} heads: expected (B, H * W, 3 * heads * hd), '
                         'nothing empty'.format(tuple(qkv.shape), H, W, heads))
    hd = qkv.shape[2] // (3 * heads)
    if ws < 1 or not supported(OP_ATTENTION, ws, hd):
        raise ValueError('window_attention: ws = {}, hd = {}: no kernel for this shape (ws * ws <= 64, hd <= 128)'.format(
            ws, hd))
    if not 0 <= shift < ws:
        raise ValueError('window_attention: shift = {}: expected 0 <= shift < ws = {}'.format(shift, ws))
    if tuple(qkv_bias.shape) != (qkv.shape[2],) or tuple(bias_table.shape) != ((2 * ws - 1) ** 2, heads):
        raise ValueError('window_attention: qkv_bias {}, bias_table {}: expected ({},) and ({}, {})'.format(
            tuple(qkv_bias.shape), tuple(bias_table.shape), qkv.shape[2], (2 * ws - 1) ** 2, heads))
    _no_grad('window_attention', qkv, qkv_bias, bias_table)
    qkv, qkv_bias, bias_table = _d(qkv), _d(qkv_bias), _d(bias_table)
    B = qkv.shape[0]
    out = torch.empty((B, H * W, heads * hd), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        C.call('hrnet_swin_attention', qkv.data_ptr(), qkv_bias.data_ptr(), bias_table.data_ptr(), out.data_ptr(), B, H, W,
               heads, hd, ws, shift, float(scale), C.stream_ptr())
    return out


def merge_ln(x, H, W, weight=None, bias=None, eps=1e-5):
    """patch merging + LayerNorm: x (B, H * W, C) or (B, H, W, C) -> (B, ceil(H / 2) * ceil(W / 2), 4 C), the channel
    blocks [x(0,0), x(1,0), x(0,1), x(1,1)], zeros beyond an odd H or W; weight, bias (4 C,), or both None for the gather
    alone"""
    _check('merge_ln', x=x, weight=weight, bias=bias)
    H, W = int(H), int(W)
    if x.ndim == 4:
        x = x.reshape(x.shape[0], -1, x.shape[3])
    if x.ndim != 3 or x.numel() == 0 or H < 1 or W < 1 or x.shape[1] != H * W:
        raise ValueError('merge_ln: x {} with H = {}, W = {}: expected (B, H * W, C), nothing empty'.format(
            tuple(x.shape), H, W))
    B, _, Cc = x.shape
    if not supported(OP_MERGE, Cc):
        raise ValueError('merge_ln: C = {}: no kernel for this width'.format(Cc))
    if (weight is None) != (bias is None) or (weight is not None and (
            tuple(weight.shape) != (4 * Cc,) or tuple(bias.shape) != (4 * Cc,))):
        raise ValueError('merge_ln: weight and bias: expected both None or both ({},)'.format(4 * Cc))
    _no_grad('merge_ln', x, weight, bias)
    x, weight, bias = _d(x), _d(weight), _d(bias)
    y = torch.empty((B, ((H + 1) // 2) * ((W + 1) // 2), 4 * Cc), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        C.call('hrnet_swin_merge_ln', x.data_ptr(), C.ptr(weight), C.ptr(bias), y.data_ptr(), B, H, W, Cc, float(eps),
               C.stream_ptr())
    return y


def patch_rows(x, p):
    """NCHW x (B, Cin, H, W) -> (B * Hp * Wp, Cin * p * p) with Hp, Wp = ceil(H / p), ceil(W / p): column
    c * p * p + kh * p + kw, zeros right of W and below H; returns (rows, Hp, Wp)"""
    _check('patch_rows', x=x)
    p = int(p)
    if x.ndim != 4 or x.numel() == 0 or p < 1:
        raise ValueError('patch_rows: x {} with p = {}: expected (B, Cin, H, W), nothing empty, p >= 1'.format(
            tuple(x.shape), p))
    B, Cin, H, W = x.shape
    if not supported(OP_EMBED, Cin, p):
        raise ValueError('patch_rows: Cin = {}, p = {}: no kernel for this shape (Cin * p * p <= 65536)'.format(Cin, p))
    _no_grad('patch_rows', x)
    x = _d(x)
    Hp, Wp = (H + p - 1) // p, (W + p - 1) // p
    rows = torch.empty((B * Hp * Wp, Cin * p * p), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        C.call('hrnet_swin_patch_rows', x.data_ptr(), rows.data_ptr(), B, Cin, H, W, p, C.stream_ptr())
    return rows, Hp, Wp


# --------------------------------------------------------------------------------------------- the decoder's convolutions
def _pad16(c):
    return (c + 15) // 16 * 16


def pad16(c):
    return _pad16(int(c))


def _pads(name, ci, co, cin_pad, cout_pad):
    cip = ci if cin_pad is None else int(cin_pad)
    cop = _pad16(co) if cout_pad is None else int(cout_pad)
    if cip < ci or cip % 4 or cop < co or cop % 16:
        raise ValueError('{}: Cin = {} in {}, Cout = {} in {}: the padded counts must hold the real ones and be multiples '
                         'of 4 (in) and 16 (out)'.format(name, ci, cip, co, cop))
    return cip, cop


def conv_transpose_pack(weight, cin_pad=None, cout_pad=None):
    """a ConvTranspose2d(Cin, Cout, 3, 2, 1, 1) weight (Cin, Cout, 3, 3) is the OIHW weight of the stride-2 convolution
    whose input gradient the layer is: packed by hrnet_pack_weights mode 1 to [cout_pad][9 flipped][cin_pad], zeros in the
    padding"""
    _check('conv_transpose_pack', weight=weight)
    if weight.ndim != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError('conv_transpose_pack: weight {}: expected (Cin, Cout, 3, 3)'.format(tuple(weight.shape)))
    ci, co = weight.shape[:2]
    cip, cop = _pads('conv_transpose_pack', ci, co, cin_pad, cout_pad)
    w = _d(weight)
    out = torch.empty(cop * 9 * cip, dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        C.call('hrnet_pack_weights', C.HR_F32, w.data_ptr(), out.data_ptr(), ci, co, 3, cip, cop, 1, C.stream_ptr())
    return out


def conv_pack(weight, cin_pad=None, cout_pad=None):
    """a 1x1 Conv2d weight (Cout, Cin, 1, 1) packed to [cout_pad][cin_pad] (hrnet_pack_weights mode 0), zeros in the
    padding"""
    _check('conv_pack', weight=weight)
    if weight.ndim != 4 or tuple(weight.shape[2:]) != (1, 1):
        raise ValueError('conv_pack: weight {}: expected (Cout, Cin, 1, 1)'.format(tuple(weight.shape)))
    co, ci = weight.shape[:2]
    cip, cop = _pads('conv_pack', ci, co, cin_pad, cout_pad)
    w = _d(weight)
    out = torch.empty(cop * cip, dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        C.call('hrnet_pack_weights', C.HR_F32, w.data_ptr(), out.data_ptr(), co, ci, 1, cop, cip, 0, C.stream_ptr())
    return out


def conv_nhwc(x, packed, cout, ks, up=False, bias=None, in_scale=None, in_shift=None, in_relu=False):
    """f32 NHWC convolution on hrnet_conv2d: x (B, H, W, Cin), packed weights of conv_pack (ks 1) or conv_transpose_pack
    (ks 3 with up=True: the input is read zero-stuffed, the output is (B, 2 H, 2 W, cout)); bias (cout,), and an optional
    per-input-channel affine + ReLU applied to x on load (the producer's folded BatchNorm)"""
    _check('conv_nhwc', x=x, packed=packed, bias=bias, in_scale=in_scale, in_shift=in_shift)
    if x.ndim != 4 or x.numel() == 0 or x.shape[3] % 4 or cout % 16 or (ks, bool(up)) not in ((1, False), (3, True)):
        raise ValueError('conv_nhwc: x {}, cout = {}, ks = {}, up = {}: expected (B, H, W, Cin) with Cin a multiple of 4, '
                         'cout a multiple of 16, and a 1x1 or a transposed 3x3'.format(tuple(x.shape), cout, ks, up))
    B, H, W, cin = x.shape
    if packed.numel() != cout * ks * ks * cin:
        raise ValueError('conv_nhwc: {} packed weights for cout = {}, ks = {}, Cin = {}'.format(packed.numel(), cout, ks, cin))
    if (in_scale is None) != (in_shift is None) or (in_scale is not None and (in_scale.numel() != cin or in_shift.numel() != cin)):
        raise ValueError('conv_nhwc: in_scale and in_shift: expected both None or both ({},)'.format(cin))
    if bias is not None and bias.numel() != cout:
        raise ValueError('conv_nhwc: bias has {} values for cout = {}'.format(bias.numel(), cout))
    _no_grad('conv_nhwc', x, bias, in_scale, in_shift)
    x, bias, in_scale, in_shift = _d(x), _d(bias), _d(in_scale), _d(in_shift)
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    y = torch.empty((B, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        C.call('hrnet_conv2d', C.HR_F32, x.data_ptr(), packed.data_ptr(), C.ptr(in_scale), C.ptr(in_shift), C.ptr(bias),
               y.data_ptr(), None, B, H, W, cin, Ho, Wo, cout, ks, 2 if up else 1, 1 if up else 0, 1 if in_relu else 0, 0,
               C.stream_ptr())
    return y


def heatmap_softmax(y, joints, temp):
    """y (B, H, W, Cp) NHWC with the joints in the first channels -> NCHW (B, joints, H, W) softmax(y * temp) per map"""
    _check('heatmap_softmax', y=y, temp=temp)
    if y.ndim != 4 or y.numel() == 0 or not 1 <= joints <= y.shape[3] or temp.numel() != 1:
        raise ValueError('heatmap_softmax: y {}, joints = {}, temp {}: expected (B, H, W, Cp >= joints) and one '
                         'temperature'.format(tuple(y.shape), joints, tuple(temp.shape)))
    _no_grad('heatmap_softmax', y, temp)
    y, temp = _d(y), _d(temp)
    B, H, W, cp = y.shape
    z = torch.empty((B, joints, H, W), dtype=torch.float32, device=y.device)
    out = torch.empty_like(z)
    with torch.cuda.device(y.device):
        C.call('hrnet_nhwc_to_nchw', C.HR_F32, y.data_ptr(), z.data_ptr(), B, H, W, cp, joints, C.stream_ptr())
        C.call('hrnet_spatial_softmax_fwd', z.data_ptr(), temp.data_ptr(), out.data_ptr(), B * joints, H * W, C.stream_ptr())
    return out
