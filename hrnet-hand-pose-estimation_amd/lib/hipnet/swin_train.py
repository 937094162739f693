"""Autograd ops of swin_transformer's training path over the C ABI (csrc/swin.hip and the f32 NHWC convolution, BatchNorm
and weight-gradient entries): one torch.autograd.Function per kernel group behind plain functions, as hipnet.transformer,

    window_attention(qkv, qkv_bias, bias_table, H, W, heads, ws, shift, scale)   hrnet_swin_attention[_bwd]
    merge_gather(x, H, W)                                                        hrnet_swin_merge_ln (gather alone) /
                                                                                 hrnet_swin_merge_scatter
    patch_rows(x, p)                                                             hrnet_swin_patch_rows[_bwd]
    decoder_step(x, up, conv, bn)       ConvTranspose2d, Conv2d 1x1, BatchNorm2d on batch statistics, ReLU: hrnet_conv2d,
                                        hrnet_bn3d_stats / _apply / _bwd, hrnet_conv2d_wgrad + hrnet_wgrad_reduce,
                                        hrnet_bias_grad, hrnet_pack_weights (every call: the weights change every step)
    decoder_final(x, conv)              the last 1x1 convolution, the same entries
    to_nchw(y, joints)                  hrnet_nhwc_to_nchw / hrnet_nchw_to_nhwc

HIP-device float32 tensors only (a CPU tensor is a ValueError: there is no CPU path). Shapes are checked before any device
call. Without a gradient required the Functions are bypassed; each backward computes only what needs_input_grad asks for.
hipnet.swin stays the inference module and keeps refusing gradients.

window_attention saves qkv, the qkv bias and the table; its backward recomputes the softmax. The gradient it returns for
qkv_bias is the attention's own (the padded keys' dk and dv); the qkv linear adds its column sums through autograd.
"""
import torch

from hipnet import _capi as C
from hipnet import swin as S
from hipnet.swin import _check


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _c(t):
    return None if t is None else t.contiguous()


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
    _check('window_attention', qkv=qkv, qkv_bias=qkv_bias, bias_table=bias_table)
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
    qkv, qkv_bias, bias_table = _c(qkv), _c(qkv_bias), _c(bias_table)
    cfg = (H, W, heads, hd, ws, shift, float(scale))
    if _wants_grad(qkv, qkv_bias, bias_table):
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
    _check('merge_gather', x=x)
    H, W = int(H), int(W)
    if x.ndim == 4:
        x = x.reshape(x.shape[0], -1, x.shape[3])
    if x.ndim != 3 or x.numel() == 0 or H < 1 or W < 1 or x.shape[1] != H * W:
        raise ValueError('merge_gather: x {} with H = {}, W = {}: expected (B, H * W, C), nothing empty'.format(
            tuple(x.shape), H, W))
    if not S.supported(S.OP_MERGE, x.shape[2]):
        raise ValueError('merge_gather: C = {}: no kernel for this width'.format(x.shape[2]))
    x = _c(x)
    if _wants_grad(x):
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
    _check('patch_rows', x=x)
    p = int(p)
    if x.ndim != 4 or x.numel() == 0 or p < 1:
        raise ValueError('patch_rows: x {} with p = {}: expected (B, Cin, H, W), nothing empty, p >= 1'.format(
            tuple(x.shape), p))
    B, Cin, H, W = x.shape
    if not S.supported(S.OP_EMBED, Cin, p):
        raise ValueError('patch_rows: Cin = {}, p = {}: no kernel for this shape (Cin * p * p <= 65536)'.format(Cin, p))
    x = _c(x)
    rows = _PatchRowsFn.apply(x, p) if _wants_grad(x) else _rows_forward(x.detach(), p)
    return rows, (H + p - 1) // p, (W + p - 1) // p


# ------------------------------------------------------------------------------------------- the decoder, training mode
F32 = C.HR_F32


def _padded(v, n):
    out = torch.zeros(n, dtype=torch.float32, device=v.device)
    out[:v.numel()] = v.detach().float().reshape(-1)
    return out


def _conv(x, packed, bias, cout, ks, stride=1, upz=0):
    """hrnet_conv2d, f32 NHWC: ks 1; ks 3 with upz (zero-stuffed input, output 2 H x 2 W); ks 3 stride 2 (output H / 2)"""
    B, H, W, cin = x.shape
    Ho, Wo = (2 * H, 2 * W) if upz else (H // stride, W // stride)
    y = torch.empty((B, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    C.call('hrnet_conv2d', F32, x.data_ptr(), packed.data_ptr(), None, None, C.ptr(bias), y.data_ptr(), None, B, H, W, cin,
           Ho, Wo, cout, ks, 2 if upz else stride, 1 if upz else 0, 0, 0, C.stream_ptr())
    return y


def _pack(w, o, i, ks, op, ip, mode):
    """hrnet_pack_weights of w read as OIHW (o, i, ks, ks); mode 0: [op][ks ks][ip], mode 1: [ip][ks ks flipped][op]"""
    out = torch.empty(op * ks * ks * ip, dtype=torch.float32, device=w.device)
    C.call('hrnet_pack_weights', F32, w.data_ptr(), out.data_ptr(), o, i, ks, op, ip, mode, C.stream_ptr())
    return out


def _wgrad(x, dy, ks, stride, o_real, i_real):
    """weight gradient (o_real, i_real, ks, ks) of dy = conv(x): x (B, H, W, Cin), dy (B, Ho, Wo, Cout); slabs + reduce"""
    B, H, W, cin = x.shape
    _, Ho, Wo, cout = dy.shape
    ns = C.call('hrnet_wgrad_splits', F32, B, Ho, Wo, cout, cin, ks, stride)
    slabs = torch.empty(ns * cout * ks * ks * cin, dtype=torch.float32, device=x.device)
    C.call('hrnet_conv2d_wgrad', F32, x.data_ptr(), dy.data_ptr(), None, None, slabs.data_ptr(), B, H, W, cin, Ho, Wo, cout,
           ks, stride, 0, ns, C.stream_ptr())
    gw = torch.empty((o_real, i_real, ks, ks), dtype=torch.float32, device=x.device)
    C.call('hrnet_wgrad_reduce', slabs.data_ptr(), gw.data_ptr(), ns, cout, cin, ks, o_real, i_real, 0, 0, C.stream_ptr())
    return gw


def _bias_grad(dy, real):
    pixels, cp = dy.numel() // dy.shape[-1], dy.shape[-1]
    blocks = C.call('hrnet_reduce_blocks', 1, 1, pixels, cp)
    scratch = torch.empty(blocks * cp, dtype=torch.float32, device=dy.device)
    db = torch.empty(real, dtype=torch.float32, device=dy.device)
    C.call('hrnet_bias_grad', F32, dy.data_ptr(), db.data_ptr(), scratch.data_ptr(), pixels, cp, real, 0, C.stream_ptr())
    return db


class _DecoderStepFn(torch.autograd.Function):
    """ConvTranspose2d(ci, co, 3, 2, 1, 1) + bias, Conv2d 1x1 + bias, BatchNorm2d on batch statistics, ReLU, f32 NHWC with
    the channels padded to cip / cop. Every activation is materialised: the weight gradient of the transposed convolution
    reads the step's input in the dy role, where the entry applies no transform on load."""

    @staticmethod
    def forward(ctx, x, up_w, up_b, pw_w, pw_b, gamma, beta, bn, cop):
        B, H, W, cip = x.shape
        ci, co = up_w.shape[:2]
        with torch.cuda.device(x.device):
            u = _conv(x, _pack(up_w, ci, co, 3, cip, cop, 1), _padded(up_b, cop), cop, 3, upz=1)
            z = _conv(u, _pack(pw_w, co, co, 1, cop, cop, 0), _padded(pw_b, cop), cop, 1)
            rows = B * 4 * H * W
            parts = C.call('hrnet_bn3d_parts', rows)
            scratch = torch.empty((2 * parts + 2) * cop, dtype=torch.float32, device=x.device)
            vec = torch.empty((4, cop), dtype=torch.float32, device=x.device)
            track = bn.track_running_stats and bn.running_mean is not None
            gamma_p, beta_p = _padded(gamma, cop), _padded(beta, cop)      # zero in the pad channels: they stay zero
            C.call('hrnet_bn3d_stats', F32, z.data_ptr(), gamma_p.data_ptr(), beta_p.data_ptr(),
                   scratch.data_ptr(), vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(),
                   bn.running_mean.data_ptr() if track else None, bn.running_var.data_ptr() if track else None,
                   bn.num_batches_tracked.data_ptr() if track else None, B, 1, 2 * H, 2 * W, cop, co,
                   float(bn.momentum if bn.momentum is not None else 0.1), float(bn.eps), C.stream_ptr())
            y = torch.empty_like(z)
            C.call('hrnet_bn3d_apply', F32, z.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), None, y.data_ptr(), B, 1,
                   2 * H, 2 * W, cop, 1, 0, C.stream_ptr())
        ctx.save_for_backward(x, up_w, pw_w, u, z, y, vec, scratch)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, up_w, pw_w, u, z, y, vec, scratch = ctx.saved_tensors
        nx, nuw, nub, npw, npb, ng, nb = ctx.needs_input_grad[:7]
        B, H, W, cip = x.shape
        ci, co = up_w.shape[:2]
        cop = y.shape[3]
        gy = gy.contiguous().float()
        dev = x.device
        new = lambda n: torch.empty(n, dtype=torch.float32, device=dev)
        dgamma, dbeta, dpb = (new(co) if ng else None), (new(co) if nb else None), (new(co) if npb else None)
        with torch.cuda.device(dev):
            dz = torch.empty_like(z)
            C.call('hrnet_bn3d_bwd', F32, gy.data_ptr(), z.data_ptr(), y.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(),
                   vec[0].data_ptr(), vec[1].data_ptr(), scratch.data_ptr(), dz.data_ptr(), None, C.ptr(dgamma),
                   C.ptr(dbeta), C.ptr(dpb), B, 1, 2 * H, 2 * W, cop, co, 0, 0, 0, C.stream_ptr())
            dpw = _wgrad(u, dz, 1, 1, co, co) if npw else None
            dx = duw = dub = None
            if nx or nuw or nub:
                du = _conv(dz, _pack(pw_w, co, co, 1, cop, cop, 1), None, cop, 1)
                if nub:
                    dub = _bias_grad(du, co)
                if nuw:
                    # the transposed convolution is the input gradient of the stride-2 convolution du -> x with W read
                    # as OIHW (ci, co, 3, 3): its weight gradient takes du as the input and the step's input as dy
                    duw = _wgrad(du, x, 3, 2, ci, co)
                if nx:
                    # hrnet_conv2d's stride-2 form computes the same sum in one f32 chain of 9 cop terms; this entry adds
                    # 32-term chunks in f64 (the error rule of the tests at 768 -> 384 channels needs it)
                    dx, packed = torch.empty_like(x), _pack(up_w, ci, co, 3, cip, cop, 0)
                    C.call('hrnet_swin_deconv_dgrad', du.data_ptr(), packed.data_ptr(), dx.data_ptr(), B, H, W, cop, cip,
                           C.stream_ptr())
        return dx, duw, dub, dpw, dpb, dgamma, dbeta, None, None


def _check_nhwc(name, x):
    if x.ndim != 4 or x.numel() == 0 or x.shape[3] % 16:
        raise ValueError('{}: x {}: expected NHWC (B, H, W, C) with C a multiple of 16, nothing empty'.format(
            name, tuple(x.shape)))


def decoder_step(x, up, conv, bn):
    """one training-mode decoder step on x (B, H, W, cip) f32 NHWC, pad channels zero: up = ConvTranspose2d(ci, co, 3, 2, 1,
    1), conv = Conv2d(co, co, 1), bn = BatchNorm2d(co) (its running statistics are updated) -> (B, 2 H, 2 W, pad16(co)),
    pad channels zero"""
    _check('decoder_step', x=x, up_weight=up.weight, up_bias=up.bias, conv_weight=conv.weight, conv_bias=conv.bias,
           bn_weight=bn.weight, bn_bias=bn.bias, running_mean=bn.running_mean, running_var=bn.running_var)
    _check_nhwc('decoder_step', x)
    ci, co = up.weight.shape[:2]
    if tuple(up.weight.shape[2:]) != (3, 3) or x.shape[3] < ci or tuple(conv.weight.shape) != (co, co, 1, 1) \
            or bn.num_features != co or up.bias is None or conv.bias is None or co > 1024:
        raise ValueError('decoder_step: x {}, transposed weight {}, 1x1 weight {}, BatchNorm({}): expected Cin <= C, '
                         '(Cin, Cout, 3, 3), (Cout, Cout, 1, 1), Cout <= 1024 and both biases'.format(
                             tuple(x.shape), tuple(up.weight.shape), tuple(conv.weight.shape), bn.num_features))
    if x.shape[0] * 4 * x.shape[1] * x.shape[2] < 2:
        raise ValueError('Expected more than 1 value per channel when training, got input size {}'.format(
            torch.Size([x.shape[0], co, 2 * x.shape[1], 2 * x.shape[2]])))
    return _DecoderStepFn.apply(_c(x), _c(up.weight), _c(up.bias), _c(conv.weight), _c(conv.bias), _c(bn.weight),
                                _c(bn.bias), bn, S.pad16(co))


class _DecoderFinalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, jp):
        j, ci = w.shape[:2]
        with torch.cuda.device(x.device):
            y = _conv(x, _pack(w, j, ci, 1, jp, x.shape[3], 0), _padded(b, jp), jp, 1)
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        nx, nw, nb = ctx.needs_input_grad[:3]
        j, ci = w.shape[:2]
        gy = gy.contiguous().float()
        with torch.cuda.device(x.device):
            dx = _conv(gy, _pack(w, j, ci, 1, gy.shape[3], x.shape[3], 1), None, x.shape[3], 1) if nx else None
            dw = _wgrad(x, gy, 1, 1, j, ci) if nw else None
            db = _bias_grad(gy, j) if nb else None
        return dx, dw, db, None


def decoder_final(x, conv):
    """the last Conv2d(ci, joints, 1) on x (B, H, W, cip) -> (B, H, W, pad16(joints)), pad channels zero"""
    _check('decoder_final', x=x, weight=conv.weight, bias=conv.bias)
    _check_nhwc('decoder_final', x)
    j, ci = conv.weight.shape[:2]
    if tuple(conv.weight.shape[2:]) != (1, 1) or x.shape[3] < ci or conv.bias is None:
        raise ValueError('decoder_final: x {}, weight {}: expected Cin <= C, (J, Cin, 1, 1) and a bias'.format(
            tuple(x.shape), tuple(conv.weight.shape)))
    return _DecoderFinalFn.apply(_c(x), _c(conv.weight), _c(conv.bias), S.pad16(j))


class _ToNCHWFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, joints):
        B, H, W, cp = y.shape
        ctx.cp = cp
        z = torch.empty((B, joints, H, W), dtype=torch.float32, device=y.device)
        with torch.cuda.device(y.device):
            C.call('hrnet_nhwc_to_nchw', F32, y.data_ptr(), z.data_ptr(), B, H, W, cp, joints, C.stream_ptr())
        return z

    @staticmethod
    def backward(ctx, gz):
        gz = gz.contiguous().float()
        B, J, H, W = gz.shape
        gy = torch.empty((B, H, W, ctx.cp), dtype=torch.float32, device=gz.device)
        with torch.cuda.device(gz.device):
            C.call('hrnet_nchw_to_nhwc', F32, gz.data_ptr(), gy.data_ptr(), B, H, W, ctx.cp, J, C.stream_ptr())
        return gy, None


def to_nchw(y, joints):
    """y (B, H, W, Cp) NHWC -> its first `joints` channels as NCHW (B, joints, H, W); the backward zeroes the pad channels"""
    _check('to_nchw', y=y)
    if y.ndim != 4 or y.numel() == 0 or not 1 <= joints <= y.shape[3]:
        raise ValueError('to_nchw: y {}, joints = {}: expected (B, H, W, Cp >= joints)'.format(tuple(y.shape), joints))
    return _ToNCHWFn.apply(_c(y), int(joints))
