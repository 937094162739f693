"""Autograd ops of pose_hrnet_hamburger's training path over the C ABI (csrc/burger_train.hip, and the f32 NHWC
convolution, BatchNorm and weight-gradient launchers of hipnet.nhwc): one torch.autograd.Function per kernel group behind
plain functions, as hipnet.swin_train,

    conv_bn_relu_train(x, conv, bn, ks)   Conv2d ks x ks (no bias), BatchNorm2d on batch statistics, ReLU: squeeze, cheese,
                                          align. nhwc.conv (1x1) / conv3x3_taps (3x3: nine taps, nine sums of Cin terms in
                                          place of one of 9 Cin), bn_batch_forward / _backward, wgrad, pack / pack_taps
                                          (every call)
    burger_mix(u, s, coef_ham, coef_shortcut)   relu(coef_ham * u + coef_shortcut * s): hrnet_burger_mix[_bwd]
    dropout2d(x, keep)                    Dropout2d on a given keep mask (B, C): hrnet_dropout2d, its own backward

lower_bread, upper_bread and fc are nhwc.conv1x1_train, the layout ops nhwc.to_nhwc and nhwc.to_nchw. The maps are f32
NHWC (B, H, W, Cp), Cp a multiple of 16, pad channels zero in and out. HIP-device float32 tensors only
(a CPU tensor is a ValueError: there is no CPU path). Shapes are checked before any device call. Each backward computes
only what needs_input_grad asks for. A BatchNorm's running statistics are updated through their pointers with
bn.momentum; num_batches_tracked is NOT incremented (the reference's SyncBN calls F.batch_norm directly: the counter
stays 0 after a reference training forward).
"""
import torch

from hipnet import _capi as C
from hipnet import nhwc
from hipnet.nhwc import check, check_nhwc, contiguous


# ------------------------------------------------------------------------------------------ Conv2d, BatchNorm2d, ReLU
def _conv(x, w, cin_pad, cout_pad, mode):
    """the bias-free convolution (mode 0: cin_pad -> cout_pad channels) or its input gradient (mode 1: cout_pad -> cin_pad)
    on freshly packed weights: a 1x1 on nhwc.conv, a 3x3 as nine taps"""
    o, i, ks = w.shape[:3]
    cout = cout_pad if mode == 0 else cin_pad
    if ks == 3:
        return nhwc.conv3x3_taps(x, nhwc.pack_taps(w, o, i, cout_pad, cin_pad, mode), cout)
    return nhwc.conv(x, nhwc.pack(w, o, i, 1, cout_pad, cin_pad, mode), cout, 1)


class _ConvBNReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, gamma, beta, bn, cop):
        z = _conv(x, w, x.shape[3], cop, 0)
        # num_batches_tracked stays: the reference's SyncBN calls F.batch_norm directly
        y, vec, scratch = nhwc.bn_batch_forward(z, gamma, beta, bn, w.shape[0], count_batches=False)
        ctx.save_for_backward(x, w, z, y, vec, scratch)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, z, y, vec, scratch = ctx.saved_tensors
        nx, nw, ng, nb = ctx.needs_input_grad[:4]
        o, i, ks = w.shape[:3]
        dz, dgamma, dbeta, _ = nhwc.bn_batch_backward(gy.contiguous().float(), z, y, vec, scratch, o, ng, nb, False)
        dw = nhwc.wgrad(x, dz, ks, 1, o, i) if nw else None
        dx = _conv(dz, w, x.shape[3], y.shape[3], 1) if nx else None
        return dx, dw, dgamma, dbeta, None, None


def conv_bn_relu_train(x, conv, bn, ks):
    """training-mode ConvBNReLU (bread.py:20-49) on x (B, H, W, cip) f32 NHWC, pad channels zero: conv = Conv2d(ci, co, ks,
    padding ks // 2, no bias), ks 1 or 3; bn = BatchNorm2d(co) on batch statistics (its running statistics are updated)
    -> (B, H, W, pad16(co)), pad channels zero. The input gradient is formed only when x needs one."""
    check('conv_bn_relu_train', x=x, conv_weight=conv.weight, bn_weight=bn.weight, bn_bias=bn.bias,
          running_mean=bn.running_mean, running_var=bn.running_var)
    check_nhwc('conv_bn_relu_train', x)
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
    return _ConvBNReLUFn.apply(contiguous(x), contiguous(conv.weight), contiguous(bn.weight), contiguous(bn.bias), bn,
                               nhwc.pad16(co))


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
    check(name, u=u, s=s, coef_ham=coef_ham, coef_shortcut=coef_shortcut)
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
    u, s, ch, cs = contiguous(u), contiguous(s), contiguous(coef_ham), contiguous(coef_shortcut)
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
    check('dropout2d', x=x, keep=keep)
    if x.ndim < 3 or x.numel() == 0 or x.shape[-1] % 16 or tuple(keep.shape) != (x.shape[0], x.shape[-1]):
        raise ValueError('dropout2d: x {}, keep {}: expected (B, ..., C) with C a multiple of 16, nothing empty, and '
                         '(B, C)'.format(tuple(x.shape), tuple(keep.shape)))
    x, keep = contiguous(x), keep.detach().contiguous()
    if torch.is_grad_enabled() and x.requires_grad:
        return _Dropout2dFn.apply(x, keep)
    return _dropout(x.detach(), keep)
