"""Autograd ops of swin_transformer's training path over the C ABI (csrc/swin.hip, and the f32 NHWC convolution, BatchNorm
and weight-gradient launchers of hipnet.nhwc): one torch.autograd.Function per kernel group behind plain functions, as
hipnet.transformer,

    window_attention(qkv, qkv_bias, bias_table, H, W, heads, ws, shift, scale)   hrnet_swin_attention[_bwd]
    merge_gather(x, H, W)                                                        hrnet_swin_merge_ln (gather alone) /
                                                                                 hrnet_swin_merge_scatter
    patch_rows(x, p)                                                             hrnet_swin_patch_rows[_bwd]
    decoder_step(x, up, conv, bn)       ConvTranspose2d, Conv2d 1x1, BatchNorm2d on batch statistics, ReLU: nhwc.pack (every
                                        call: the weights change every step), conv, bn_batch_forward / _backward, wgrad,
                                        bias_grad, and hrnet_swin_deconv_dgrad

The decoder's last 1x1 convolution and the way back to NCHW are nhwc.conv1x1_train and nhwc.to_nchw. HIP-device float32
tensors only (a CPU tensor is a ValueError: there is no CPU path). Shapes are checked before any device call. Without a
gradient required the Functions are bypassed; each backward computes only what needs_input_grad asks for. hipnet.swin
stays the inference module and keeps refusing gradients.

window_attention saves qkv, the qkv bias and the table; its backward recomputes the softmax. The gradient it returns for
qkv_bias is the attention's own (the padded keys' dk and dv); the qkv linear adds its column sums through autograd.
"""
import torch

from hipnet import _capi as C
from hipnet import nhwc
from hipnet import swin as S
from hipnet.nhwc import check, check_nhwc, contiguous, wants_grad


# ------------------------------------------------------------------------------------------------- window attention
def _attn_forward(qkv, qkv_bias, table, cfg):
    H, W, heads, hd, ws, shift, scale = cfg
    B = qkv.shape[0]
    out = torch.empty((B, H * W, heads * hd), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        C.call('hrnet_swin_attention', qkv.data_ptr(), qkv_bias.data_ptr(), table.data_ptr(), out.data_ptr(), B, H, W,
               heads, hd, ws, shift, scale, C.stream_ptr())
    return out


class _WindowAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, qkv_bias, table, cfg):
        ctx.save_for_backward(qkv, qkv_bias, table)
        ctx.cfg = cfg
        return _attn_forward(qkv, qkv_bias, table, cfg)

    @staticmethod
    def backward(ctx, gout):
        nq, nb, nt = ctx.needs_input_grad[:3]
        if not (nq or nb or nt):
            return None, None, None, None
        qkv, qkv_bias, table = ctx.saved_tensors
        H, W, heads, hd, ws, shift, scale = ctx.cfg
        B = qkv.shape[0]
        gout = gout.contiguous().float()
        dqkv = torch.empty_like(qkv)
        dbias = torch.empty_like(qkv_bias) if nb else None
        dtable = torch.empty_like(table) if nt else None
        scratch, need = None, 0
        if nb or nt:
            need = C.call('hrnet_swin_attention_bwd_scratch', B, H, W, heads, hd, ws)
            scratch = torch.empty(need, dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            C.call('hrnet_swin_attention_bwd', qkv.data_ptr(), qkv_bias.data_ptr(), table.data_ptr(), gout.data_ptr(),
                   dqkv.data_ptr(), C.ptr(dbias), C.ptr(dtable), C.ptr(scratch), need, B, H, W, heads, hd, ws, shift, scale,
                   C.stream_ptr())
        return (dqkv if nq else None), dbias, dtable, None


def window_attention(qkv, qkv_bias, bias_table, H, W, heads, ws, shift, scale):
    """hipnet.swin.window_attention with a backward: qkv (B, H * W, 3 * heads * hd), qkv_bias (3 * heads * hd,), bias_table
    ((2 ws - 1)^2, heads) -> (B, H * W, heads * hd)"""
    check('window_attention', qkv=qkv, qkv_bias=qkv_bias, bias_table=bias_table)
    H, W, heads, ws, shift = int(H), int(W), int(heads), int(ws), int(shift)
    if qkv.ndim == 5:
        qkv = qkv.reshape(qkv.shape[0], qkv.shape[1], -1)
    if qkv.ndim != 3 or qkv.numel() == 0 or heads < 1 or H < 1 or W < 1 or qkv.shape[1] != H * W \
            or qkv.shape[2] % (3 * heads):
        raise ValueError('window_attention: qkv {} with H = {}, W = {}, {} heads: expected (B, H * W, 3 * heads * hd), '
                         'nothing empty'.format(tuple(qkv.shape), H, W, heads))
    hd = qkv.shape[2] // (3 * heads)
    if ws < 1 or not S.supported(S.OP_ATTENTION, ws, hd):
        raise ValueError('window_attention: ws = {}, hd = {}: no kernel for this shape (ws * ws <= 64, hd <= 128)'.format(
            ws, hd))
    if not 0 <= shift < ws:
        raise ValueError('window_attention: shift = {}: expected 0 <= shift < ws = {}'.format(shift, ws))
    if tuple(qkv_bias.shape) != (qkv.shape[2],) or tuple(bias_table.shape) != ((2 * ws - 1) ** 2, heads):
        raise ValueError('window_attention: qkv_bias {}, bias_table {}: expected ({},) and ({}, {})'.format(
            tuple(qkv_bias.shape), tuple(bias_table.shape), qkv.shape[2], (2 * ws - 1) ** 2, heads))
    qkv, qkv_bias, bias_table = contiguous(qkv), contiguous(qkv_bias), contiguous(bias_table)
    cfg = (H, W, heads, hd, ws, shift, float(scale))
    if wants_grad(qkv, qkv_bias, bias_table):
        return _WindowAttentionFn.apply(qkv, qkv_bias, bias_table, cfg)
    return _attn_forward(qkv.detach(), qkv_bias.detach(), bias_table.detach(), cfg)


# ------------------------------------------------------------------------------------------------------ the gathers
def _merge_forward(x, H, W):
    B, _, Cc = x.shape
    y = torch.empty((B, ((H + 1) // 2) * ((W + 1) // 2), 4 * Cc), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        C.call('hrnet_swin_merge_ln', x.data_ptr(), None, None, y.data_ptr(), B, H, W, Cc, 1e-5, C.stream_ptr())
    return y


class _MergeGatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, H, W):
        ctx.shape = (tuple(x.shape), H, W)
        return _merge_forward(x, H, W)

    @staticmethod
    def backward(ctx, gy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (B, L, Cc), H, W = ctx.shape
        gy = gy.contiguous().float()
        dx = torch.empty((B, L, Cc), dtype=torch.float32, device=gy.device)
        with torch.cuda.device(gy.device):
            C.call('hrnet_swin_merge_scatter', gy.data_ptr(), dx.data_ptr(), B, H, W, Cc, C.stream_ptr())
        return dx, None, None


def merge_gather(x, H, W):
    """patch merging's gather alone: x (B, H * W, C) or (B, H, W, C) -> (B, ceil(H / 2) * ceil(W / 2), 4 C), the channel
    blocks [x(0,0), x(1,0), x(0,1), x(1,1)], zeros beyond an odd H or W (their gradient is dropped)"""
    check('merge_gather', x=x)
    H, W = int(H), int(W)
    if x.ndim == 4:
        x = x.reshape(x.shape[0], -1, x.shape[3])
    if x.ndim != 3 or x.numel() == 0 or H < 1 or W < 1 or x.shape[1] != H * W:
        raise ValueError('merge_gather: x {} with H = {}, W = {}: expected (B, H * W, C), nothing empty'.format(
            tuple(x.shape), H, W))
    if not S.supported(S.OP_MERGE, x.shape[2]):
        raise ValueError('merge_gather: C = {}: no kernel for this width'.format(x.shape[2]))
    x = contiguous(x)
    if wants_grad(x):
        return _MergeGatherFn.apply(x, H, W)
    return _merge_forward(x.detach(), H, W)


def _rows_forward(x, p):
    B, Cin, H, W = x.shape
    Hp, Wp = (H + p - 1) // p, (W + p - 1) // p
    rows = torch.empty((B * Hp * Wp, Cin * p * p), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        C.call('hrnet_swin_patch_rows', x.data_ptr(), rows.data_ptr(), B, Cin, H, W, p, C.stream_ptr())
    return rows


class _PatchRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        ctx.shape, ctx.p = tuple(x.shape), p
        return _rows_forward(x, p)

    @staticmethod
    def backward(ctx, grows):
        if not ctx.needs_input_grad[0]:
            return None, None
        B, Cin, H, W = ctx.shape
        grows = grows.contiguous().float()
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=grows.device)
        with torch.cuda.device(grows.device):
            C.call('hrnet_swin_patch_rows_bwd', grows.data_ptr(), dx.data_ptr(), B, Cin, H, W, ctx.p, C.stream_ptr())
        return dx, None


def patch_rows(x, p):
    """NCHW x (B, Cin, H, W) -> (rows (B * Hp * Wp, Cin * p * p), Hp, Wp), as hipnet.swin.patch_rows, with a backward"""
    check('patch_rows', x=x)
    p = int(p)
    if x.ndim != 4 or x.numel() == 0 or p < 1:
        raise ValueError('patch_rows: x {} with p = {}: expected (B, Cin, H, W), nothing empty, p >= 1'.format(
            tuple(x.shape), p))
    B, Cin, H, W = x.shape
    if not S.supported(S.OP_EMBED, Cin, p):
        raise ValueError('patch_rows: Cin = {}, p = {}: no kernel for this shape (Cin * p * p <= 65536)'.format(Cin, p))
    x = contiguous(x)
    rows = _PatchRowsFn.apply(x, p) if wants_grad(x) else _rows_forward(x.detach(), p)
    return rows, (H + p - 1) // p, (W + p - 1) // p


# ------------------------------------------------------------------------------------------- the decoder, training mode
class _DecoderStepFn(torch.autograd.Function):
    """ConvTranspose2d(ci, co, 3, 2, 1, 1) + bias, Conv2d 1x1 + bias, BatchNorm2d on batch statistics, ReLU, f32 NHWC with
    the channels padded to cip / cop. Every activation is materialised: the weight gradient of the transposed convolution
    reads the step's input in the dy role, where the entry applies no transform on load."""

    @staticmethod
    def forward(ctx, x, up_w, up_b, pw_w, pw_b, gamma, beta, bn, cop):
        cip = x.shape[3]
        ci, co = up_w.shape[:2]
        u = nhwc.conv(x, nhwc.pack(up_w, ci, co, 3, cip, cop, 1), cop, 3, upz=True, bias=nhwc.padded(up_b, cop))
        z = nhwc.conv(u, nhwc.pack(pw_w, co, co, 1, cop, cop, 0), cop, 1, bias=nhwc.padded(pw_b, cop))
        y, vec, scratch = nhwc.bn_batch_forward(z, gamma, beta, bn, co, count_batches=True)
        ctx.save_for_backward(x, up_w, pw_w, u, z, y, vec, scratch)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, up_w, pw_w, u, z, y, vec, scratch = ctx.saved_tensors
        nx, nuw, nub, npw, npb, ng, nb = ctx.needs_input_grad[:7]
        B, H, W, cip = x.shape
        ci, co = up_w.shape[:2]
        cop = y.shape[3]
        dz, dgamma, dbeta, dpb = nhwc.bn_batch_backward(gy.contiguous().float(), z, y, vec, scratch, co, ng, nb, npb)
        dpw = nhwc.wgrad(u, dz, 1, 1, co, co) if npw else None
        dx = duw = dub = None
        if nx or nuw or nub:
            du = nhwc.conv(dz, nhwc.pack(pw_w, co, co, 1, cop, cop, 1), cop, 1)
            if nub:
                dub = nhwc.bias_grad(du, co)
            if nuw:
                # the transposed convolution is the input gradient of the stride-2 convolution du -> x with W read
                # as OIHW (ci, co, 3, 3): its weight gradient takes du as the input and the step's input as dy
                duw = nhwc.wgrad(du, x, 3, 2, ci, co)
            if nx:
                # hrnet_conv2d's stride-2 form computes the same sum in one f32 chain of 9 cop terms; this entry adds
                # 32-term chunks in f64 (the error rule of the tests at 768 -> 384 channels needs it)
                dx, packed = torch.empty_like(x), nhwc.pack(up_w, ci, co, 3, cip, cop, 0)
                with torch.cuda.device(x.device):
                    C.call('hrnet_swin_deconv_dgrad', du.data_ptr(), packed.data_ptr(), dx.data_ptr(), B, H, W, cop, cip,
                           C.stream_ptr())
        return dx, duw, dub, dpw, dpb, dgamma, dbeta, None, None


def decoder_step(x, up, conv, bn):
    """one training-mode decoder step on x (B, H, W, cip) f32 NHWC, pad channels zero: up = ConvTranspose2d(ci, co, 3, 2, 1,
    1), conv = Conv2d(co, co, 1), bn = BatchNorm2d(co) (its running statistics are updated) -> (B, 2 H, 2 W, pad16(co)),
    pad channels zero"""
    check('decoder_step', x=x, up_weight=up.weight, up_bias=up.bias, conv_weight=conv.weight, conv_bias=conv.bias,
          bn_weight=bn.weight, bn_bias=bn.bias, running_mean=bn.running_mean, running_var=bn.running_var)
    check_nhwc('decoder_step', x)
    ci, co = up.weight.shape[:2]
    if tuple(up.weight.shape[2:]) != (3, 3) or x.shape[3] < ci or tuple(conv.weight.shape) != (co, co, 1, 1) \
            or bn.num_features != co or up.bias is None or conv.bias is None or co > 1024:
        raise ValueError('decoder_step: x {}, transposed weight {}, 1x1 weight {}, BatchNorm({}): expected Cin <= C, '
                         '(Cin, Cout, 3, 3), (Cout, Cout, 1, 1), Cout <= 1024 and both biases'.format(
                             tuple(x.shape), tuple(up.weight.shape), tuple(conv.weight.shape), bn.num_features))
    if x.shape[0] * 4 * x.shape[1] * x.shape[2] < 2:
        raise ValueError('Expected more than 1 value per channel when training, got input size {}'.format(
            torch.Size([x.shape[0], co, 2 * x.shape[1], 2 * x.shape[2]])))
    return _DecoderStepFn.apply(contiguous(x), contiguous(up.weight), contiguous(up.bias), contiguous(conv.weight),
                                contiguous(conv.bias), contiguous(bn.weight), contiguous(bn.bias), bn, nhwc.pad16(co))

