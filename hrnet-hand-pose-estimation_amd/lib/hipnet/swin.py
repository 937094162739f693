"""Swin ops of swin_transformer over the C ABI (csrc/swin.hip), forward only,

    window_attention(qkv, qkv_bias, bias_table, H, W, heads, ws, shift, scale)   hrnet_swin_attention
    merge_ln(x, H, W, weight, bias, eps)                                         hrnet_swin_merge_ln
    patch_rows(x, p)                                                             hrnet_swin_patch_rows

The decoder's convolutions and the heat maps' softmax are hipnet.nhwc's (conv_pack, conv_transpose_pack, conv_nhwc,
heatmap_softmax). HIP-device float32 tensors only (a CPU tensor is a ValueError: there is no CPU path). Shapes are checked
before any device call. There is no autograd here: an input that requires grad while grad is enabled raises
NotImplementedError.
"""
import torch

from hipnet import _capi as C
from hipnet.nhwc import check

OP_ATTENTION, OP_MERGE, OP_EMBED = (C.VALUES['HR_SWIN_' + n] for n in ('ATTENTION', 'MERGE', 'EMBED'))


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
    check('window_attention', qkv=qkv, qkv_bias=qkv_bias, bias_table=bias_table)
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
    check('merge_ln', x=x, weight=weight, bias=bias)
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
    check('patch_rows', x=x)
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
