"""Op-by-op autograd layers over the C ABI (one HIP launch per step, no recorded program): the building blocks of
the parts of the reference that sit outside the recorded HRNet programs - today the aggregation head of
pose_hrnet_PoseAggr in TRAINING mode (reference lib/models/pose_hrnet_PoseAggr.py:612-646 and its autograd).

Activations are NHWC tensors in the compute dtype (channel counts padded as the kernels need: multiples of 8 in,
16 out); parameters stay the module's f32 OIHW tensors and are packed per call (these paths are small and not
performance critical). Every forward / backward below is a hrnet_* launch; torch supplies memory, views and the
autograd graph only. Weight packing, the plain convolution, the whole-kernel weight gradient and the nine-tap 3x3 go
through the launchers of hipnet.nhwc, whose ToNHWC / ToNCHW are the layout Functions of these paths too; what stays here
runs on the recorded kernels' row-sum BatchNorm (ConvBN), or is this head's own (AddReLU, the tap-by-tap weight gradient
of DilatedConv, LinComb).
"""
import ctypes

import torch

from . import _capi as C
from . import nhwc
from . import ops


def _dt(t):
    return C.dtype_id(t.dtype)


def _pads(w):
    """the padded (Cout, Cin) of an OIHW weight here: multiples of 16 and of 8"""
    return (w.shape[0] + 15) // 16 * 16, (w.shape[1] + 7) // 8 * 8


def _pack(w, dtype, mode, ks):
    """OIHW f32 -> packed kernel layout (mode 0 forward / 1 transposed input-gradient copy)"""
    cop, cip = _pads(w)
    wf = w.detach().float().contiguous()
    return nhwc.pack(wf, w.shape[0], w.shape[1], ks, cop, cip, mode, C.dtype_id(dtype)), cop, cip


def _conv_backward(x, gy, weight, ks, need_gx):
    """input gradient (conv with the transposed packed kernel) and weight gradient (slabs + reduce) of y = conv(x)"""
    gx = nhwc.conv(gy, _pack(weight, x.dtype, 1, ks)[0], x.shape[3], ks, dtype=_dt(x)) if need_gx else None
    return gx, nhwc.wgrad(x, gy, ks, 1, weight.shape[0], weight.shape[1])


class ConvBN(torch.autograd.Function):
    """z = relu?(BatchNorm_train(conv(x))): conv with batch statistics, finalize (running statistics updated),
    apply; backward: BatchNorm backward (reduce, finalize, apply) then the conv's two gradients."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, bn_module, relu):
        N, H, W, cin = x.shape
        ks = weight.shape[2]
        dt = _dt(x)
        wf, cop, cip = _pack(weight, x.dtype, 0, ks)
        assert cip == cin and cop == gamma.numel(), (cip, cin, cop, gamma.numel())
        y = torch.empty((N, H, W, cop), dtype=x.dtype, device=x.device)
        tiles = C.call('hrnet_conv_tiles', N, H, W, cop, ks, 1)
        rows = torch.empty(tiles * 2 * cop, dtype=torch.float32, device=x.device)
        C.call('hrnet_conv2d', dt, x.data_ptr(), wf.data_ptr(), None, None, None, y.data_ptr(), rows.data_ptr(), N, H, W,
               cin, H, W, cop, ks, 1, 0, 0, 0, C.stream_ptr())
        scale, shift, mean, invstd = (torch.empty(cop, dtype=torch.float32, device=x.device) for _ in range(4))
        m = bn_module
        C.call('hrnet_bn_finalize', rows.data_ptr(), tiles, cop, float(N * H * W), gamma.data_ptr(), beta.data_ptr(),
               m.running_mean.data_ptr(), m.running_var.data_ptr(), m.num_batches_tracked.data_ptr(),
               m.momentum if m.momentum is not None else 0.1, m.eps, 1, scale.data_ptr(), shift.data_ptr(),
               mean.data_ptr(), invstd.data_ptr(), C.stream_ptr())
        z = torch.empty_like(y)
        C.call('hrnet_sum_terms', dt, z.data_ptr(), N, H, W, cop, 1, (ctypes.c_void_p * 1)(y.data_ptr()),
               (ctypes.c_void_p * 1)(scale.data_ptr()), (ctypes.c_void_p * 1)(shift.data_ptr()), (ctypes.c_int * 1)(0),
               (ctypes.c_int * 1)(1 if relu else 0), 0, C.stream_ptr())
        ctx.save_for_backward(x, weight, gamma, y, scale, shift, mean, invstd)
        ctx.relu = bool(relu)
        return z

    @staticmethod
    def backward(ctx, gz):
        x, weight, gamma, y, scale, shift, mean, invstd = ctx.saved_tensors
        N, H, W, cop = y.shape
        dt = _dt(x)
        gz = gz.contiguous()
        blocks = C.call('hrnet_reduce_blocks', N, H, W, cop)
        part = torch.empty(blocks * 2 * cop, dtype=torch.float32, device=x.device)
        C.call('hrnet_bn_bwd_reduce', dt, part.data_ptr(), gz.data_ptr(), None, y.data_ptr(), scale.data_ptr(),
               shift.data_ptr(), N, H, W, cop, 0, 1 if ctx.relu else 0, C.stream_ptr())
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        coef = torch.empty(3 * cop, dtype=torch.float32, device=x.device)
        C.call('hrnet_bn_bwd_finalize', part.data_ptr(), blocks, cop, float(N * H * W), gamma.data_ptr(), mean.data_ptr(),
               invstd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), coef.data_ptr(), 0, C.stream_ptr())
        gy = torch.empty_like(y)
        C.call('hrnet_grad_term', dt, gy.data_ptr(), gz.data_ptr(), None, y.data_ptr(), scale.data_ptr(), shift.data_ptr(),
               coef.data_ptr(), N, H, W, cop, 0, 1 if ctx.relu else 0, 0, C.stream_ptr())
        gx, gw = _conv_backward(x, gy, weight, weight.shape[2], ctx.needs_input_grad[0])
        return gx, gw, dgamma, dbeta, None, None


class AddReLU(torch.autograd.Function):
    """out = relu(a + b) (the residual add that closes a BasicBlock, pose_hrnet.py:54-55)"""

    @staticmethod
    def forward(ctx, a, b):
        N, H, W, c = a.shape
        out = torch.empty_like(a)
        C.call('hrnet_sum_terms', _dt(a), out.data_ptr(), N, H, W, c, 2, (ctypes.c_void_p * 2)(a.data_ptr(), b.data_ptr()),
               (ctypes.c_void_p * 2)(None, None), (ctypes.c_void_p * 2)(None, None), (ctypes.c_int * 2)(0, 0),
               (ctypes.c_int * 2)(0, 0), 1, C.stream_ptr())
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        out, = ctx.saved_tensors
        N, H, W, c = out.shape
        g = g.contiguous()
        d = torch.empty_like(out)
        C.call('hrnet_grad_term', _dt(out), d.data_ptr(), g.data_ptr(), out.data_ptr(), None, None, None, None, N, H, W, c,
               0, 0, 0, C.stream_ptr())
        return d, d


class DilatedConv(torch.autograd.Function):
    """y = conv3x3(x, dilation d, padding d), no bias (the offset convs, pose_hrnet_PoseAggr.py:497-506).
    backward: the input gradient is the same op with the transposed, mirrored taps; the weight gradient of tap t
    is a 1x1 weight gradient against the input displaced by that tap (a displaced copy made by a 1x1 identity conv)."""

    @staticmethod
    def forward(ctx, x, weight, dilation):
        co, ci = weight.shape[:2]
        cop, cip = _pads(weight)
        assert cip == x.shape[3]
        y = nhwc.conv3x3_taps(x, nhwc.pack_taps(weight.detach().float().contiguous(), co, ci, cop, cip, 0, _dt(x)), cop,
                              dilation)
        ctx.save_for_backward(x, weight)
        ctx.d = dilation
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        N, H, W, cin = x.shape
        cop = gy.shape[3]
        dt, d = _dt(x), ctx.d
        gy = gy.contiguous()
        gx = None
        if ctx.needs_input_grad[0]:
            # (padded output channels of y carry zero weights: the transposed matrices' K is cop; their rows are padded to
            # a multiple of 16 as a packed Cout is)
            taps_t = nhwc.pack_taps(weight.detach().float().contiguous(), weight.shape[0], weight.shape[1], cop,
                                    nhwc.pad16(cin), 1, dt)
            gx = nhwc.conv3x3_taps(gy, taps_t, cin, d)
        # weight gradient, tap by tap
        eye = torch.eye(cin, dtype=torch.float32, device=x.device).reshape(cin, cin, 1, 1)
        ident, _, _ = _pack(eye, x.dtype, 0, 1)
        gw = torch.zeros(weight.shape, dtype=torch.float32, device=x.device)
        co, ci = weight.shape[0], weight.shape[1]
        ns = C.call('hrnet_wgrad_splits', dt, N, H, W, cop, cin, 1, 1)
        slabs = torch.empty(ns * cop * cin, dtype=torch.float32, device=x.device)
        xs = torch.empty_like(x)
        g1 = torch.empty((co, ci, 1, 1), dtype=torch.float32, device=x.device)
        for t in range(9):
            # xs[p] = x[p + shift_t] (zero outside): one 1x1 identity conv over the displaced window
            op = ops.make(C.OP_CONV, dtype=dt, n=N, h=H, w=W, cin=cin, ho=H, wo=W, cout=cin, ks=1, stride=1,
                          in_dy=(t // 3 - 1) * d, in_dx=(t % 3 - 1) * d, x=x.data_ptr(), wgt=ident.data_ptr(),
                          y=xs.data_ptr())
            C.call('hrnet_program_run', ctypes.byref(op), 1, C.stream_ptr())
            C.call('hrnet_conv2d_wgrad', dt, xs.data_ptr(), gy.data_ptr(), None, None, slabs.data_ptr(), N, H, W, cin, H, W,
                   cop, 1, 1, 0, ns, C.stream_ptr())
            C.call('hrnet_wgrad_reduce', slabs.data_ptr(), g1.data_ptr(), ns, cop, cin, 1, co, ci, 0, 0, C.stream_ptr())
            gw[:, :, t // 3, t % 3] = g1[:, :, 0, 0]
        return gx, gw, None


class LinComb(torch.autograd.Function):
    """out = sum_j coef_j * src_j over f32 tensors of one shape"""

    @staticmethod
    def forward(ctx, coefs, *srcs):
        srcs = [s.contiguous() for s in srcs]
        out = torch.empty_like(srcs[0])
        C.call('hrnet_lincomb_f32', out.data_ptr(), out.numel(), len(srcs),
               (ctypes.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs]), (ctypes.c_float * len(srcs))(*coefs),
               C.stream_ptr())
        ctx.coefs = list(coefs)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        outs = []
        for j, c in enumerate(ctx.coefs):
            if ctx.needs_input_grad[1 + j]:
                o = torch.empty_like(g)
                C.call('hrnet_lincomb_f32', o.data_ptr(), o.numel(), 1, (ctypes.c_void_p * 1)(g.data_ptr()),
                       (ctypes.c_float * 1)(c), C.stream_ptr())
                outs.append(o)
            else:
                outs.append(None)
        return (None,) + tuple(outs)


def basic_block(x, unit):
    """BasicBlock forward in training mode (pose_hrnet.py:41-57) over the container module `unit`"""
    z1 = ConvBN.apply(x, unit.conv1.weight, unit.bn1.weight, unit.bn1.bias, unit.bn1, True)
    z2 = ConvBN.apply(z1, unit.conv2.weight, unit.bn2.weight, unit.bn2.bias, unit.bn2, False)
    res = x
    if hasattr(unit, 'downsample'):
        ds = unit.downsample
        res = ConvBN.apply(x, ds[0].weight, ds[1].weight, ds[1].bias, ds[1], False)
    return AddReLU.apply(z2, res)
