"""The backward of the Convolutional Pose Machine's K x K convolution and max pool over the C ABI, f32 NHWC
(csrc/conv_kxk_train.hip): the one home of every launch of

    hrnet_conv2d_kxk_wgrad_scratch, hrnet_conv2d_kxk_wgrad, hrnet_conv2d_kxk_dgrad, hrnet_maxpool2d_3x3s2_bwd

The forward ops stay in hipnet.conv_kxk (inference only, refusals included); this module adds the gradients beside them.
Every op reads and writes channel slices (ld, off, C) of wider maps, stores only the real channels, uses no atomics and
sums in a fixed order: two runs from the same state give equal bits. Two layers, as hipnet.conv_kxk:

  raw launchers: no argument checks beyond the C entry's own (anything it cannot serve is a RuntimeError)
    wgrad_plan(B, H, W, cin, cout, ks)          (scratch bytes, pixel-tile splits, tiles per split): a host query
    wgrad(x, dy, scratch, dw, db, cin, cin_real, x_off, cout, y_off, ks)
    dgrad(dy, packed_t, dx, mask, cout, y_off, cin, x_off, m_off, ks, accumulate)
    maxpool_bwd(x, dy, dx, c, x_off, dy_off, dx_off, relu_mask)

  checked public ops: shapes are checked before any device call, a CPU tensor is a ValueError
    pack_dgrad(weight, cout_pad, ci_lo, ci_hi)  the flipped, transposed weight of input channels [ci_lo, ci_hi)
    conv_kxk_wgrad(x, dy, cout, ks, ...)        -> (dW (cout, cin_real, ks, ks), db (cout,) or None)
    conv_kxk_dgrad(dy, packed_t, cin, ks, ...)  -> the map written
    maxpool3x3s2_bwd(x, dy, ...)                -> the map written
"""
import ctypes

import torch

from hipnet import _capi as C
from hipnet import conv_kxk as K
from hipnet import nhwc

F32 = C.HR_F32


# --------------------------------------------------------------------------------------------------- raw launchers
def wgrad_plan(B, H, W, cin, cout, ks):
    """(bytes of scratch, pixel-tile splits, 8 x 16 pixel tiles per split) of hrnet_conv2d_kxk_wgrad for this shape"""
    nbytes, nsplit, per = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)
    C.call('hrnet_conv2d_kxk_wgrad_scratch', F32, B, H, W, cin, cout, ks, ctypes.byref(nbytes), ctypes.byref(nsplit),
           ctypes.byref(per))
    return nbytes.value, nsplit.value, per.value


def wgrad(x, dy, scratch, dw, db, cin, cin_real, x_off, cout, y_off, ks):
    B, H, W, ldx = x.shape
    with torch.cuda.device(x.device):
        C.call('hrnet_conv2d_kxk_wgrad', F32, x.data_ptr(), dy.data_ptr(), scratch.data_ptr(),
               scratch.numel() * scratch.element_size(), dw.data_ptr(), C.ptr(db), B, H, W, cin, cin_real, ldx, x_off, cout,
               dy.shape[3], y_off, ks, C.stream_ptr())
    return dw, db


def dgrad(dy, packed_t, dx, mask, cout, y_off, cin, x_off, m_off, ks, accumulate):
    B, H, W, ldy = dy.shape
    with torch.cuda.device(dy.device):
        C.call('hrnet_conv2d_kxk_dgrad', F32, dy.data_ptr(), packed_t.data_ptr(), dx.data_ptr(), C.ptr(mask), B, H, W, cout,
               ldy, y_off, cin, dx.shape[3], x_off, 0 if mask is None else mask.shape[3], m_off, ks, 1 if accumulate else 0,
               C.stream_ptr())
    return dx


def maxpool_bwd(x, dy, dx, c, x_off, dy_off, dx_off, relu_mask):
    B, H, W, ldx = x.shape
    with torch.cuda.device(x.device):
        C.call('hrnet_maxpool2d_3x3s2_bwd', x.data_ptr(), dy.data_ptr(), dx.data_ptr(), B, H, W, c, ldx, x_off, dy.shape[3],
               dy_off, dx.shape[3], dx_off, 1 if relu_mask else 0, C.stream_ptr())
    return dx


# ---------------------------------------------------------------------------------------------- checked public ops
def _f32(name, **ts):
    for k, t in ts.items():
        if t is not None and t.dtype != torch.float32:
            raise ValueError('{}: {} is {}: float32 only'.format(name, k, t.dtype))


def _ks(name, ks):
    ks = int(ks)
    if not ks % 2 or not 1 <= ks <= K.tile()[3]:
        raise ValueError('{}: ks = {}: expected an odd size <= {}'.format(name, ks, K.tile()[3]))
    return ks


def pack_dgrad(weight, cout_pad=None, ci_lo=0, ci_hi=None):
    """the weights of conv_kxk_dgrad for the input channels [ci_lo, ci_hi) of a Conv2d weight (Cout, Cin, ks, ks): permuted
    to (Cin', Cout, ks, ks), flipped in both kernel axes and packed by hrnet_pack_weights mode 0 to
    [pad16(Cin')][ks ks][cout_pad]; cout_pad (default: Cout rounded up to 4) is the width of the dy slice the layer reads,
    zeros in the padding"""
    nhwc.check('conv_kxk_train.pack_dgrad', weight=weight)
    if weight.ndim != 4:
        raise ValueError('conv_kxk_train.pack_dgrad: weight {}: expected (Cout, Cin, ks, ks)'.format(tuple(weight.shape)))
    ci_hi = weight.shape[1] if ci_hi is None else int(ci_hi)
    if not 0 <= ci_lo < ci_hi <= weight.shape[1]:
        raise ValueError('conv_kxk_train.pack_dgrad: input channels [{}, {}) of {}'.format(ci_lo, ci_hi, weight.shape[1]))
    wt = weight.detach()[:, ci_lo:ci_hi].permute(1, 0, 2, 3).flip(2, 3).contiguous()
    return K.pack(wt, cout_pad)


def conv_kxk_wgrad(x, dy, cout, ks, cin=None, cin_real=None, x_off=0, y_off=0, want_bias=True, scratch=None, dw=None,
                   db=None):
    """the weight and bias gradients of y = Conv2d(cin_real, cout, ks, padding=ks // 2)(x): x (B, H, W, ldx) read at
    channels [x_off, x_off + cin) (cin, ldx, x_off multiples of 4; default: the whole row) of which the first cin_real
    (default cin) are real, dy (B, H, W, ldy) read at [y_off, y_off + cout). Returns (dW (cout, cin_real, ks, ks),
    db (cout,) or None), new tensors unless dw / db are given (overwritten). scratch: a float32 tensor of at least
    wgrad_plan(...)[0] bytes, None for a new one"""
    name = 'conv_kxk_wgrad'
    nhwc.check(name, x=x, dy=dy, scratch=scratch, dw=dw, db=db)
    _f32(name, x=x, dy=dy, scratch=scratch, dw=dw, db=db)
    K._map(name, 'x', x)
    K._map(name, 'dy', dy)
    B, H, W, ldx = x.shape
    ks, cout, x_off, y_off = _ks(name, ks), int(cout), int(x_off), int(y_off)
    cin = ldx - x_off if cin is None else int(cin)
    cin_real = cin if cin_real is None else int(cin_real)
    K._slice(name, 'input', x_off, cin, ldx)
    if cin % 4 or ldx % 4 or x_off % 4:
        raise ValueError('{}: cin = {}, ldx = {}, x_off = {}: expected multiples of 4'.format(name, cin, ldx, x_off))
    if not 1 <= cin_real <= cin:
        raise ValueError('{}: {} real input channels of {}'.format(name, cin_real, cin))
    if tuple(dy.shape[:3]) != (B, H, W):
        raise ValueError('{}: dy {}: expected ({}, {}, {}, ld)'.format(name, tuple(dy.shape), B, H, W))
    K._slice(name, 'gradient', y_off, cout, dy.shape[3])
    nbytes = wgrad_plan(B, H, W, cin, cout, ks)[0]
    if scratch is None:
        scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    elif not scratch.is_contiguous() or scratch.numel() * 4 < nbytes:
        raise ValueError('{}: scratch of {} bytes, {} needed'.format(name, scratch.numel() * 4, nbytes))
    if dw is None:
        dw = torch.empty((cout, cin_real, ks, ks), dtype=torch.float32, device=x.device)
    elif tuple(dw.shape) != (cout, cin_real, ks, ks) or not dw.is_contiguous():
        raise ValueError('{}: dw {}: expected a contiguous ({}, {}, {}, {})'.format(name, tuple(dw.shape), cout, cin_real, ks,
                                                                                 ks))
    if db is None:
        db = torch.empty(cout, dtype=torch.float32, device=x.device) if want_bias else None
    elif db.numel() != cout or not db.is_contiguous():
        raise ValueError('{}: db has {} values for cout = {}'.format(name, db.numel(), cout))
    return wgrad(x.detach(), dy.detach(), scratch, dw, db, cin, cin_real, x_off, cout, y_off, ks)


def conv_kxk_dgrad(dy, packed_t, cin, ks, cout=None, y_off=0, out=None, x_off=0, mask=None, m_off=0, accumulate=False):
    """the input gradient of y = Conv2d(cin, cout, ks, padding=ks // 2)(x): dy (B, H, W, ldy) read at channels
    [y_off, y_off + cout) (cout, ldy, y_off multiples of 4, zeros in dy's pad channels; default: the whole row), packed_t
    of pack_dgrad(weight, cout). out: None for a new (B, H, W, cin) map, or a (B, H, W, ldx) map whose channels
    [x_off, x_off + cin) are written and no others. mask (B, H, W, ldm) read at [m_off, m_off + cin): the result is zeroed
    where mask <= 0 (the ReLU whose output the convolution read). accumulate: add onto what out holds. Returns out"""
    name = 'conv_kxk_dgrad'
    nhwc.check(name, dy=dy, packed_t=packed_t, out=out, mask=mask)
    _f32(name, dy=dy, packed_t=packed_t, out=out, mask=mask)
    K._map(name, 'dy', dy)
    B, H, W, ldy = dy.shape
    ks, cin, x_off, y_off, m_off = _ks(name, ks), int(cin), int(x_off), int(y_off), int(m_off)
    cout = ldy - y_off if cout is None else int(cout)
    K._slice(name, 'gradient', y_off, cout, ldy)
    if cout % 4 or ldy % 4 or y_off % 4:
        raise ValueError('{}: cout = {}, ldy = {}, y_off = {}: expected multiples of 4'.format(name, cout, ldy, y_off))
    if cin < 1 or packed_t.numel() != nhwc.pad16(cin) * ks * ks * cout:
        raise ValueError('{}: {} packed weights for cin = {} (in {}), ks = {}, cout = {}'.format(
            name, packed_t.numel(), cin, nhwc.pad16(cin), ks, cout))
    if out is None:
        if x_off or accumulate:
            raise ValueError('{}: x_off = {}, accumulate = {} without a map to write into'.format(name, x_off, accumulate))
        out = torch.empty((B, H, W, cin), dtype=torch.float32, device=dy.device)
    else:
        K._map(name, 'out', out)
        if tuple(out.shape[:3]) != (B, H, W):
            raise ValueError('{}: out {}: expected ({}, {}, {}, ld)'.format(name, tuple(out.shape), B, H, W))
        K._slice(name, 'output', x_off, cin, out.shape[3])
        if out.data_ptr() == dy.data_ptr():
            raise ValueError('{}: out is dy'.format(name))
    if mask is not None:
        K._map(name, 'mask', mask)
        if tuple(mask.shape[:3]) != (B, H, W):
            raise ValueError('{}: mask {}: expected ({}, {}, {}, ld)'.format(name, tuple(mask.shape), B, H, W))
        K._slice(name, 'mask', m_off, cin, mask.shape[3])
    return dgrad(dy.detach(), packed_t, out, None if mask is None else mask.detach(), cout, y_off, cin, x_off, m_off, ks,
                 accumulate)


def maxpool3x3s2_bwd(x, dy, c=None, x_off=0, dy_off=0, out=None, dx_off=0, relu_mask=False):
    """the backward of MaxPool2d(3, 2, 1): x (B, H, W, ldx) the pool's input read at [x_off, x_off + c), dy
    (B, (H-1)//2 + 1, (W-1)//2 + 1, lddy) read at [dy_off, dy_off + c) -> channels [dx_off, dx_off + c) of out (B, H, W, lddx)
    (None: a new map of c channels), overwritten. The arg-max is the forward's (first maximum in scan order).
    relu_mask: times (x > 0), the backward of the ReLU that produced x"""
    name = 'maxpool3x3s2_bwd'
    nhwc.check(name, x=x, dy=dy, out=out)
    _f32(name, x=x, dy=dy, out=out)
    K._map(name, 'x', x)
    K._map(name, 'dy', dy)
    B, H, W, ldx = x.shape
    c = ldx - int(x_off) if c is None else int(c)
    K._slice(name, 'input', int(x_off), c, ldx)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if tuple(dy.shape[:3]) != (B, Ho, Wo):
        raise ValueError('{}: dy {}: expected ({}, {}, {}, ld)'.format(name, tuple(dy.shape), B, Ho, Wo))
    K._slice(name, 'gradient', int(dy_off), c, dy.shape[3])
    if out is None:
        if dx_off:
            raise ValueError('{}: dx_off = {} without a map to write into'.format(name, dx_off))
        out = torch.empty((B, H, W, c), dtype=torch.float32, device=x.device)
    else:
        K._map(name, 'out', out)
        if tuple(out.shape[:3]) != (B, H, W):
            raise ValueError('{}: out {}: expected ({}, {}, {}, ld)'.format(name, tuple(out.shape), B, H, W))
        K._slice(name, 'output', int(dx_off), c, out.shape[3])
        if out.data_ptr() in (x.data_ptr(), dy.data_ptr()):
            raise ValueError('{}: out is x or dy'.format(name))
    return maxpool_bwd(x.detach(), dy.detach(), out, c, int(x_off), int(dy_off), int(dx_off), relu_mask)
