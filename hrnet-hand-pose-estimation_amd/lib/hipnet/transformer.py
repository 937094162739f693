"""Transformer ops of pose_hrnet_transformer over the C ABI (csrc/transformer.hip): one torch.autograd.Function per
kernel group behind plain functions,

    layer_norm(x, weight, bias, eps)                                         hrnet_tf_layernorm[_bwd]
    linear(x, weight, bias, act=None, residual=None, row_scale=None)         hrnet_tf_linear[_bwd]
    attention(qkv, heads, scale)                                             hrnet_tf_attention[_bwd]
    frame_mean(x, weight, bias)                                              hrnet_tf_frame_mean[_bwd]
    add_rows(x, pos)                                                         hrnet_tf_add_rows (+ frame mean backward)

HIP-device float32 tensors only (a CPU tensor is a ValueError: there is no CPU path). Without a gradient required the
Functions are bypassed; each backward computes only what needs_input_grad asks for. `linear` with act='gelu' keeps the
pre-activation the forward kernel stores and hands it to the backward kernel (nothing is recomputed); `attention` saves
qkv alone and its backward recomputes the softmax.
"""
import torch

from hipnet import _capi as C
from hipnet.nhwc import check, contiguous, wants_grad

OP_LAYERNORM, OP_LINEAR, OP_ATTENTION, OP_FRAME_MEAN = (
    C.VALUES['HR_TF_' + n] for n in ('LAYERNORM', 'LINEAR', 'ATTENTION', 'FRAME_MEAN'))
ACT_NONE, ACT_GELU = C.VALUES['HR_TF_ACT_NONE'], C.VALUES['HR_TF_ACT_GELU']
_ACTS = {None: ACT_NONE, 'none': ACT_NONE, 'gelu': ACT_GELU}


def supported(op, a, b=0):
    return bool(C.call('hrnet_tf_supported', int(op), int(a), int(b)))


# ------------------------------------------------------------------------------------------------------- layer norm
def _ln_forward(x, w, b, eps):
    rows, Cc = x.numel() // x.shape[-1], x.shape[-1]
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        C.call('hrnet_tf_layernorm', x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), rows, Cc, eps,
               C.stream_ptr())
    return y


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        ctx.save_for_backward(x, w)
        ctx.eps = eps
        return _ln_forward(x, w, b, eps)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        nx, nw, nb = ctx.needs_input_grad[:3]
        if not (nx or nw or nb):
            return None, None, None, None
        rows, Cc = x.numel() // x.shape[-1], x.shape[-1]
        gy = gy.contiguous().float()
        dx = torch.empty_like(x) if nx else None
        dw = torch.empty_like(w) if nw else None
        db = torch.empty_like(w) if nb else None
        scratch, need = None, 0
        if nw or nb:
            need = C.call('hrnet_tf_layernorm_scratch', rows, Cc)
            scratch = torch.empty(need, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            C.call('hrnet_tf_layernorm_bwd', x.data_ptr(), w.data_ptr(), gy.data_ptr(), C.ptr(dx), C.ptr(dw), C.ptr(db),
                   C.ptr(scratch), need, rows, Cc, ctx.eps, C.stream_ptr())
        return dx, dw, db, None


def layer_norm(x, weight, bias, eps=1e-5):
    """LayerNorm over the last axis of x (..., C); weight, bias (C,)"""
    check('layer_norm', x=x, weight=weight, bias=bias)
    Cc = x.shape[-1] if x.ndim else 0
    if x.ndim < 1 or x.numel() == 0 or tuple(weight.shape) != (Cc,) or tuple(bias.shape) != (Cc,):
        raise ValueError('layer_norm: x {}, weight {}, bias {}: expected (..., C), (C,), (C,), nothing empty'.format(
            tuple(x.shape), tuple(weight.shape), tuple(bias.shape)))
    if not supported(OP_LAYERNORM, Cc):
        raise ValueError('layer_norm: C = {}: no kernel for this width'.format(Cc))
    x, weight, bias = contiguous(x), contiguous(weight), contiguous(bias)
    if wants_grad(x, weight, bias):
        return _LayerNormFn.apply(x, weight, bias, float(eps))
    return _ln_forward(x.detach(), weight.detach(), bias.detach(), float(eps))


# ----------------------------------------------------------------------------------------------------------- linear
def _linear_forward(x, w, b, res, rs, act, keep_pre):
    Cout, Cin = w.shape
    rows = x.numel() // Cin
    y = torch.empty(x.shape[:-1] + (Cout,), dtype=torch.float32, device=x.device)
    pre = torch.empty_like(y) if (keep_pre and act == ACT_GELU) else None
    with torch.cuda.device(x.device):
        C.call('hrnet_tf_linear', x.data_ptr(), w.data_ptr(), C.ptr(b), C.ptr(res), C.ptr(rs), y.data_ptr(), C.ptr(pre),
               rows, Cin, Cout, act, C.stream_ptr())
    return y, pre


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, res, rs, act):
        y, pre = _linear_forward(x, w, b, res, rs, act, True)
        ctx.save_for_backward(x, w, pre, rs)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, pre, rs = ctx.saved_tensors
        nx, nw, nb, nres = ctx.needs_input_grad[:4]
        gy = gy.contiguous().float()
        dx = dw = db = None
        if nx or nw or nb:
            Cout, Cin = w.shape
            rows = x.numel() // Cin
            dx = torch.empty_like(x) if nx else None
            dw = torch.empty_like(w) if nw else None
            db = torch.empty(Cout, dtype=torch.float32, device=x.device) if nb else None
            with torch.cuda.device(x.device):
                C.call('hrnet_tf_linear_bwd', x.data_ptr(), w.data_ptr(), gy.data_ptr(), C.ptr(pre), C.ptr(rs),
                       C.ptr(dx), C.ptr(dw), C.ptr(db), rows, Cin, Cout, ctx.act, C.stream_ptr())
        return dx, dw, db, (gy if nres else None), None, None


def linear(x, weight, bias=None, act=None, residual=None, row_scale=None):
    """y = [residual +] row_scale[row] * act(x weight^T + bias): x (..., Cin), weight (Cout, Cin), bias (Cout,) or None,
    act None or 'gelu' (exact), residual y's shape, row_scale one value per row (no gradient: it carries the
    stochastic-depth keep flags)"""
    check('linear', x=x, weight=weight, bias=bias, residual=residual, row_scale=row_scale)
    if act not in _ACTS:
        raise ValueError('linear: act {!r}: None or \'gelu\''.format(act))
    if x.ndim < 1 or weight.ndim != 2 or x.numel() == 0 or weight.numel() == 0 or x.shape[-1] != weight.shape[1]:
        raise ValueError('linear: x {}, weight {}: expected (..., Cin) and (Cout, Cin), nothing empty'.format(
            tuple(x.shape), tuple(weight.shape)))
    Cout, Cin = weight.shape
    rows = x.numel() // Cin
    if not supported(OP_LINEAR, Cin, Cout):
        raise ValueError('linear: Cin = {}, Cout = {}: no kernel for this shape'.format(Cin, Cout))
    if bias is not None and tuple(bias.shape) != (Cout,):
        raise ValueError('linear: bias {}: expected ({},)'.format(tuple(bias.shape), Cout))
    if residual is not None and tuple(residual.shape) != tuple(x.shape[:-1]) + (Cout,):
        raise ValueError('linear: residual {}: expected {}'.format(tuple(residual.shape), tuple(x.shape[:-1]) + (Cout,)))
    if row_scale is not None and row_scale.numel() != rows:
        raise ValueError('linear: row_scale has {} values for {} rows'.format(row_scale.numel(), rows))
    x, weight, bias, residual = contiguous(x), contiguous(weight), contiguous(bias), contiguous(residual)
    rs = None if row_scale is None else row_scale.detach().contiguous()
    a = _ACTS[act]
    if wants_grad(x, weight, bias, residual):
        return _LinearFn.apply(x, weight, bias, residual, rs, a)
    det = lambda t: None if t is None else t.detach()
    return _linear_forward(x.detach(), weight.detach(), det(bias), det(residual), rs, a, False)[0]


# -------------------------------------------------------------------------------------------------------- attention
def _attn_forward(qkv, heads, hd, scale):
    S, N = qkv.shape[:2]
    out = torch.empty((S, N, heads * hd), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        C.call('hrnet_tf_attention', qkv.data_ptr(), out.data_ptr(), S, N, heads, hd, scale, C.stream_ptr())
    return out


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads, hd, scale):
        ctx.save_for_backward(qkv)
        ctx.cfg = (heads, hd, scale)
        return _attn_forward(qkv, heads, hd, scale)

    @staticmethod
    def backward(ctx, gout):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        qkv, = ctx.saved_tensors
        heads, hd, scale = ctx.cfg
        S, N = qkv.shape[:2]
        gout = gout.contiguous().float()
        dqkv = torch.empty_like(qkv)
        with torch.cuda.device(qkv.device):
            C.call('hrnet_tf_attention_bwd', qkv.data_ptr(), gout.data_ptr(), dqkv.data_ptr(), S, N, heads, hd, scale,
                   C.stream_ptr())
        return dqkv, None, None, None


def attention(qkv, heads, scale):
    """qkv (S, N, 3 * C) or (S, N, 3, heads, hd), packed [q | k | v] as nn.Linear(C, 3 C) leaves it -> (S, N, C):
    softmax(q k^T * scale) v per (sequence, head)"""
    check('attention', qkv=qkv)
    heads = int(heads)
    if qkv.ndim == 5:
        qkv = qkv.reshape(qkv.shape[0], qkv.shape[1], -1)
    if qkv.ndim != 3 or qkv.numel() == 0 or heads < 1 or qkv.shape[2] % (3 * heads):
        raise ValueError('attention: qkv {} with {} heads: expected (S, N, 3 * heads * hd), nothing empty'.format(
            tuple(qkv.shape), heads))
    N, hd = qkv.shape[1], qkv.shape[2] // (3 * heads)
    if not supported(OP_ATTENTION, N, hd):
        raise ValueError('attention: N = {} tokens, hd = {}: no kernel for this shape (1 <= N <= 64, hd <= 128)'.format(
            N, hd))
    qkv = contiguous(qkv)
    if wants_grad(qkv):
        return _AttentionFn.apply(qkv, heads, hd, float(scale))
    return _attn_forward(qkv.detach(), heads, hd, float(scale))


# ------------------------------------------------------------------------------------------- frame mean and add rows
def _fmean_forward(x, w, b):
    S, F = x.shape[:2]
    D = x.numel() // (S * F)
    y = torch.empty((S,) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        C.call('hrnet_tf_frame_mean', x.data_ptr(), w.data_ptr(), C.ptr(b), y.data_ptr(), S, F, D, C.stream_ptr())
    return y


class _FrameMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return _fmean_forward(x, w, b)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        nx, nw = ctx.needs_input_grad[:2]
        nb = len(ctx.needs_input_grad) > 2 and ctx.needs_input_grad[2]
        if not (nx or nw or nb):
            return None, None, None
        S, F = x.shape[:2]
        D = x.numel() // (S * F)
        gy = gy.contiguous().float()
        dx = torch.empty_like(x) if nx else None
        dw = torch.empty_like(w) if nw else None
        db = torch.empty(1, dtype=torch.float32, device=x.device) if nb else None
        with torch.cuda.device(x.device):
            C.call('hrnet_tf_frame_mean_bwd', x.data_ptr(), w.data_ptr(), gy.data_ptr(), C.ptr(dx), C.ptr(dw), C.ptr(db),
                   S, F, D, C.stream_ptr())
        return dx, dw, db


def frame_mean(x, weight, bias=None):
    """out[s] = sum_f weight[f] * x[s, f] + bias: x (S, F, ...), weight F values (a Conv1d(F, 1, 1) weight (1, F, 1) is
    taken as it is), bias one value or None -> (S, ...)"""
    check('frame_mean', x=x, weight=weight, bias=bias)
    if x.ndim < 3 or x.numel() == 0 or weight.numel() != x.shape[1] or (bias is not None and bias.numel() != 1):
        raise ValueError('frame_mean: x {}, weight {}: expected (S, F, ...), F weights and one bias'.format(
            tuple(x.shape), tuple(weight.shape)))
    if not supported(OP_FRAME_MEAN, x.shape[1]):
        raise ValueError('frame_mean: F = {}: no kernel for this many frames'.format(x.shape[1]))
    x, weight, bias = contiguous(x), contiguous(weight), contiguous(bias)
    if wants_grad(x, weight, bias):
        return _FrameMeanFn.apply(x, weight.reshape(-1), None if bias is None else bias.reshape(1))
    return _fmean_forward(x.detach(), weight.detach(), None if bias is None else bias.detach())


class _AddRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos):
        ctx.reps = x.shape[0] // pos.shape[0]
        return _add_rows_forward(x, pos)

    @staticmethod
    def backward(ctx, gy):
        nx, npos = ctx.needs_input_grad
        gy = gy.contiguous().float()
        dpos = None
        if npos:
            # the sum over the repeats is the frame mean with unit weights: (1, reps, period * C) -> (1, period * C)
            ones = torch.ones(ctx.reps, dtype=torch.float32, device=gy.device)
            dpos = _fmean_forward(gy.reshape(1, ctx.reps, -1), ones, None).reshape(-1, gy.shape[-1])
        return (gy if nx else None), dpos


def _add_rows_forward(x, pos):
    rows, Cc = x.shape
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        C.call('hrnet_tf_add_rows', x.data_ptr(), pos.data_ptr(), y.data_ptr(), rows, Cc, pos.shape[0], C.stream_ptr())
    return y


def add_rows(x, pos):
    """y[r] = x[r] + pos[r % period]: x (rows, C), pos (period, C), period divides rows (a position embedding added to
    every sequence)"""
    check('add_rows', x=x, pos=pos)
    if x.ndim != 2 or pos.ndim != 2 or x.numel() == 0 or pos.numel() == 0 or x.shape[1] != pos.shape[1] \
            or x.shape[0] % pos.shape[0]:
        raise ValueError('add_rows: x {}, pos {}: expected (rows, C) and (period, C), period dividing rows'.format(
            tuple(x.shape), tuple(pos.shape)))
    x, pos = contiguous(x), contiguous(pos)
    if wants_grad(x, pos):
        return _AddRowsFn.apply(x, pos)
    return _add_rows_forward(x.detach(), pos.detach())
