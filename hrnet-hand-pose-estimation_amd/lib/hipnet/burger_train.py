"""Autograd ops of pose_hrnet_hamburger's training path over the C ABI (csrc/burger_train.hip and the f32 NHWC
convolution, BatchNorm and weight-gradient entries): one torch.autograd.Function per kernel group behind plain functions,
as hipnet.swin_train,

    conv_bn_relu_train(x, conv, bn, ks)   Conv2d ks x ks (no bias), BatchNorm2d on batch statistics, ReLU: squeeze, cheese,
                                          align. hrnet_conv2d (1x1) / hrnet_conv2d_dilated3x3 (3x3: nine taps, nine sums
                                          of Cin terms in place of one of 9 Cin), hrnet_bn3d_stats / _apply / _bwd,
                                          hrnet_conv2d_wgrad + hrnet_wgrad_reduce, hrnet_pack_weights (every call)
    conv1x1_train(x, conv, relu_out)      Conv2d 1x1 (+ bias) (+ ReLU): lower_bread, upper_bread, fc. The ReLU's backward
                                          is hrnet_grad_term with coef NULL
    burger_mix(u, s, coef_ham, coef_shortcut)   relu(coef_ham * u + coef_shortcut * s): hrnet_burger_mix[_bwd]
    dropout2d(x, keep)                    Dropout2d on a given keep mask (B, C): hrnet_dropout2d, its own backward
    to_nhwc(x, cp)                        NCHW -> NHWC with zero pad channels: hrnet_nchw_to_nhwc / hrnet_nhwc_to_nchw

The maps are f32 NHWC (B, H, W, Cp), Cp a multiple of 16, pad channels zero in and out. HIP-device float32 tensors only
(a CPU tensor is a ValueError: there is no CPU path). Shapes are checked before any device call. Each backward computes
only what needs_input_grad asks for. A BatchNorm's running statistics are updated through their pointers with
bn.momentum; num_batches_tracked is NOT incremented (the reference's SyncBN calls F.batch_norm directly: the counter
stays 0 after a reference training forward).
"""
import torch

from hipnet import _capi as C
from hipnet import swin as S
from hipnet.swin import _check
from hipnet.swin_train import F32, _bias_grad, _c, _check_nhwc, _conv, _pack, _padded, _wgrad


def _taps(w, o, i, op, ip, mode):
    """3x3 OIHW weight -> nine packed 1x1 matrices. mode 0: [9][op][ip], tap t = 3 r + s (the forward); mode 1:
    [9][ip][op], the transposed weights in reversed tap order (the input gradient)"""
    packed = _pack(w, o, i, 3, op, ip, mode)
    rows, cols = (op, ip) if mode == 0 else (ip, op)
    return packed.reshape(rows, 9, cols).permute(1, 0, 2).contiguous()


def _conv3x3(x, taps, cout):
    B, H, W, cin = x.shape
    y = torch.empty((B, H, W, cout), dtype=torch.float32, device=x.device)
    C.call('hrnet_conv2d_dilated3x3', F32, x.data_ptr(), taps.data_ptr(), 4 * cout * cin, y.data_ptr(), B, H, W, cin, cout, 1,
           C.stream_ptr())
    return y


# ------------------------------------------------------------------------------------------ Conv2d, BatchNorm2d, ReLU
class _ConvBNReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, gamma, beta, bn, cop):
        B, H, W, cip = x.shape
        o, i, ks = w.shape[0], w.shape[1], w.shape[2]
        with torch.cuda.device(x.device):
            if ks == 3:
                z = _conv3x3(x, _taps(w, o, i, cop, cip, 0), cop)
            else:
                z = _conv(x, _pack(w, o, i, 1, cop, cip, 0), None, cop, 1)
            parts = C.call('hrnet_bn3d_parts', B * H * W)
            scratch = torch.empty((2 * parts + 2) * cop, dtype=torch.float32, device=x.device)
            vec = torch.empty((4, cop), dtype=torch.float32, device=x.device)
            track = bn.track_running_stats and bn.running_mean is not None
            gamma_p, beta_p = _padded(gamma, cop), _padded(beta, cop)      # zero in the pad channels: they stay zero
            C.call('hrnet_bn3d_stats', F32, z.data_ptr(), gamma_p.data_ptr(), beta_p.data_ptr(), scratch.data_ptr(),
                   vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(),
                   bn.running_mean.data_ptr() if track else None, bn.running_var.data_ptr() if track else None, None,
                   B, 1, H, W, cop, o, float(bn.momentum if bn.momentum is not None else 0.1), float(bn.eps),
                   C.stream_ptr())
            y = torch.empty_like(z)
            C.call('hrnet_bn3d_apply', F32, z.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), None, y.data_ptr(), B, 1,
                   H, W, cop, 1, 0, C.stream_ptr())
        ctx.save_for_backward(x, w, z, y, vec, scratch)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, z, y, vec, scratch = ctx.saved_tensors
        nx, nw, ng, nb = ctx.needs_input_grad[:4]
        B, H, W, cip = x.shape
        o, i, ks = w.shape[0], w.shape[1], w.shape[2]
        cop = y.shape[3]
        gy = gy.contiguous().float()
        new = lambda n: torch.empty(n, dtype=torch.float32, device=x.device)
        dgamma, dbeta = (new(o) if ng else None), (new(o) if nb else None)
        dx = dw = None
        with torch.cuda.device(x.device):
            dz = torch.empty_like(z)
            C.call('hrnet_bn3d_bwd', F32, gy.data_ptr(), z.data_ptr(), y.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(),
                   vec[0].data_ptr(), vec[1].data_ptr(), scratch.data_ptr(), dz.data_ptr(), None, C.ptr(dgamma),
                   C.ptr(dbeta), None, B, 1, H, W, cop, o, 0, 0, 0, C.stream_ptr())
            if nw:
                dw = _wgrad(x, dz, ks, 1, o, i)
            if nx and ks == 3:
                dx = _conv3x3(dz, _taps(w, o, i, cop, cip, 1), cip)
            elif nx:
                dx = _conv(dz, _pack(w, o, i, 1, cop, cip, 1), None, cip, 1)
        return dx, dw, dgamma, dbeta, None, None


def conv_bn_relu_train(x, conv, bn, ks):
    """training-mode ConvBNReLU (bread.py:20-49) on x (B, H, W, cip) f32 NHWC, pad channels zero: conv = Conv2d(ci, co, ks,
    padding ks // 2, no bias), ks 1 or 3; bn = BatchNorm2d(co) on batch statistics (its running statistics are updated)
    -> (B, H, W, pad16(co)), pad channels zero. The input gradient is formed only when x needs one."""
    _check('conv_bn_relu_train', x=x, conv_weight=conv.weight, bn_weight=bn.weight, bn_bias=bn.bias,
           running_mean=bn.running_mean, running_var=bn.running_var)
    _check_nhwc('conv_bn_relu_train', x)
    ks = int(ks)
    co, ci = conv.weight.shape[:2]
    if ks not in (1, 3) or tuple(conv.weight.shape[2:]) != (ks, ks) or x.shape[3] < ci or bn.num_features != co \
            or conv.bias is not None or co > 1024:
        raise ValueError('conv_bn_relu_train: x {}, weight {}, ks = {}, BatchNorm({}): expected ks 1 or 3, (Cout, Cin <= C, '
                         'ks, ks), Cout <= 1024 and no bias'.format(tuple(x.shape), tuple(conv.weight.shape), ks,
                                                                    bn.num_features))
    if x.shape[0] * x.shape[1] * x.shape[2] < 2:
        raise ValueError('Expected more than 1 value per channel when training, got input size {}'.format(
            torch.Size([x.shape[0], co, x.shape[1], x.shape[2]])))
    return _ConvBNReLUFn.apply(_c(x), _c(conv.weight), _c(bn.weight), _c(bn.bias), bn, S.pad16(co))


# ------------------------------------------------------------------------------------------------------- Conv2d 1x1
class _Conv1x1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, relu, cop):
        o, i = w.shape[:2]
        with torch.cuda.device(x.device):
            y = _conv(x, _pack(w, o, i, 1, cop, x.shape[3], 0), None if b is None else _padded(b, cop), cop, 1)
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
        with torch.cuda.device(x.device):
            if ctx.relu:
                dz = torch.empty_like(gy)
                C.call('hrnet_grad_term', F32, dz.data_ptr(), gy.data_ptr(), y.data_ptr(), None, None, None, None, B, H, W,
                       cop, 0, 0, 0, C.stream_ptr())
                gy = dz
            dx = _conv(gy, _pack(w, o, i, 1, cop, x.shape[3], 1), None, x.shape[3], 1) if nx else None
            dw = _wgrad(x, gy, 1, 1, o, i) if nw else None
            db = _bias_grad(gy, o) if nb else None
        return dx, dw, db, None, None


def conv1x1_train(x, conv, relu_out=False):
    """Conv2d(ci, co, 1) with or without bias, then ReLU if relu_out, on x (B, H, W, cip) f32 NHWC -> (B, H, W, pad16(co)),
    pad channels zero"""
    _check('conv1x1_train', x=x, weight=conv.weight, bias=conv.bias)
    _check_nhwc('conv1x1_train', x)
    co, ci = conv.weight.shape[:2]
    if tuple(conv.weight.shape[2:]) != (1, 1) or x.shape[3] < ci:
        raise ValueError('conv1x1_train: x {}, weight {}: expected Cin <= C and (Cout, Cin, 1, 1)'.format(
            tuple(x.shape), tuple(conv.weight.shape)))
    return _Conv1x1Fn.apply(_c(x), _c(conv.weight), _c(conv.bias), bool(relu_out), S.pad16(co))


# ---------------------------------------------------------------------------------------------------------- the mix
def mix_scratch(rows, Cc):
    return int(C.call('hrnet_burger_mix_scratch', int(rows), int(Cc)))


def _mix_forward(u, s, ch, cs, out=None):
    out = torch.empty_like(u) if out is None else out
    with torch.cuda.device(u.device):
        C.call('hrnet_burger_mix', u.data_ptr(), s.data_ptr(), ch.data_ptr(), cs.data_ptr(), out.data_ptr(),
               u.numel() // u.shape[-1], u.shape[-1], C.stream_ptr())
    return out


def mix_backward(g, out, u, s, ch, cs, want_du=True, want_ds=True, want_dcoef=True, du=None, scratch=None):
    """hrnet_burger_mix_bwd on dense maps: (du, ds, dcoef (2,)), None for what is not wanted. du: the tensor to write du to
    (g itself is allowed); scratch: None (allocated here) or a float64 tensor of mix_scratch(rows, C) values"""
    rows, Cc = g.numel() // g.shape[-1], g.shape[-1]
    du = (torch.empty_like(g) if du is None else du) if want_du else None
    ds = torch.empty_like(g) if want_ds else None
    dcoef = torch.empty(2, dtype=torch.float32, device=g.device) if want_dcoef else None
    if want_dcoef and scratch is None:
        scratch = torch.empty(mix_scratch(rows, Cc), dtype=torch.float64, device=g.device)
    with torch.cuda.device(g.device):
        C.call('hrnet_burger_mix_bwd', g.data_ptr(), out.data_ptr(), u.data_ptr(), s.data_ptr(), ch.data_ptr(),
               cs.data_ptr(), C.ptr(du), C.ptr(ds), C.ptr(dcoef), C.ptr(scratch) if want_dcoef else None,
               scratch.numel() if want_dcoef else 0, rows, Cc, C.stream_ptr())
    return du, ds, dcoef


class _BurgerMixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, s, ch, cs):
        out = _mix_forward(u, s, ch, cs)
        ctx.save_for_backward(u, s, ch, cs, out)
        return out

    @staticmethod
    def backward(ctx, g):
        u, s, ch, cs, out = ctx.saved_tensors
        nu, ns, nh, nc = ctx.needs_input_grad
        if not (nu or ns or nh or nc):
            return None, None, None, None
        du, ds, dcoef = mix_backward(g.contiguous().float(), out, u, s, ch, cs, nu, ns, nh or nc)
        return du, ds, (dcoef[0:1].reshape(ch.shape) if nh else None), (dcoef[1:2].reshape(cs.shape) if nc else None)


def _check_mix(name, u, s, coef_ham, coef_shortcut):
    _check(name, u=u, s=s, coef_ham=coef_ham, coef_shortcut=coef_shortcut)
    if u.ndim < 2 or u.numel() == 0 or u.shape[-1] % 16 or tuple(u.shape) != tuple(s.shape):
        raise ValueError('{}: u {}, s {}: expected two maps of one shape (..., C) with C a multiple of 16, nothing '
                         'empty'.format(name, tuple(u.shape), tuple(s.shape)))
    if coef_ham.numel() != 1 or coef_shortcut.numel() != 1:
        raise ValueError('{}: coef_ham {}, coef_shortcut {}: expected one value each'.format(
            name, tuple(coef_ham.shape), tuple(coef_shortcut.shape)))


def burger_mix(u, s, coef_ham, coef_shortcut):
    """relu(coef_ham * u + coef_shortcut * s) (burger.py:198-199) on two f32 NHWC maps of one shape; the coefficients are
    one-element device tensors and are never read on the host"""
    _check_mix('burger_mix', u, s, coef_ham, coef_shortcut)
    u, s, ch, cs = _c(u), _c(s), _c(coef_ham), _c(coef_shortcut)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (u, s, ch, cs)):
        return _BurgerMixFn.apply(u, s, ch, cs)
    return _mix_forward(u.detach(), s.detach(), ch.detach(), cs.detach())


# ------------------------------------------------------------------------------------------------------- Dropout2d
def _dropout(x, keep):
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        C.call('hrnet_dropout2d', x.data_ptr(), keep.data_ptr(), y.data_ptr(), x.shape[0], x.numel() // (x.shape[0] *
               x.shape[-1]), x.shape[-1], C.stream_ptr())
    return y


class _Dropout2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, keep):
        ctx.save_for_backward(keep)
        return _dropout(x, keep)

    @staticmethod
    def backward(ctx, gy):
        if not ctx.needs_input_grad[0]:
            return None, None
        return _dropout(gy.contiguous().float(), ctx.saved_tensors[0]), None


def dropout2d(x, keep):
    """Dropout2d with the mask given: x (B, ..., C) f32 NHWC, keep (B, C) holding 0 or 1 / (1 - p) (zero in pad channels
    or not: they are zero in x) -> x * keep[b, c]"""
    _check('dropout2d', x=x, keep=keep)
    if x.ndim < 3 or x.numel() == 0 or x.shape[-1] % 16 or tuple(keep.shape) != (x.shape[0], x.shape[-1]):
        raise ValueError('dropout2d: x {}, keep {}: expected (B, ..., C) with C a multiple of 16, nothing empty, and '
                         '(B, C)'.format(tuple(x.shape), tuple(keep.shape)))
    x, keep = _c(x), keep.detach().contiguous()
    if torch.is_grad_enabled() and x.requires_grad:
        return _Dropout2dFn.apply(x, keep)
    return _dropout(x.detach(), keep)


# ----------------------------------------------------------------------------------------------------------- layout
def _nhwc(x, cp):
    B, Cc, H, W = x.shape
    y = torch.empty((B, H, W, cp), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        C.call('hrnet_nchw_to_nhwc', F32, x.data_ptr(), y.data_ptr(), B, H, W, cp, Cc, C.stream_ptr())
    return y


class _ToNHWCFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cp):
        ctx.channels = x.shape[1]
        return _nhwc(x, cp)

    @staticmethod
    def backward(ctx, gy):
        if not ctx.needs_input_grad[0]:
            return None, None
        gy = gy.contiguous().float()
        B, H, W, cp = gy.shape
        Cc = ctx.channels
        dx = torch.empty((B, Cc, H, W), dtype=torch.float32, device=gy.device)
        with torch.cuda.device(gy.device):
            C.call('hrnet_nhwc_to_nchw', F32, gy.data_ptr(), dx.data_ptr(), B, H, W, cp, Cc, C.stream_ptr())
        return dx, None


def to_nhwc(x, cp):
    """x (B, C, H, W) NCHW -> (B, H, W, cp) NHWC, cp >= C a multiple of 16, zero pad channels"""
    _check('to_nhwc', x=x)
    if x.ndim != 4 or x.numel() == 0 or cp % 16 or cp < x.shape[1]:
        raise ValueError('to_nhwc: x {}, cp = {}: expected (B, C, H, W), nothing empty, cp >= C a multiple of 16'.format(
            tuple(x.shape), cp))
    x = _c(x)
    if torch.is_grad_enabled() and x.requires_grad:
        return _ToNHWCFn.apply(x, int(cp))
    return _nhwc(x.detach(), int(cp))
