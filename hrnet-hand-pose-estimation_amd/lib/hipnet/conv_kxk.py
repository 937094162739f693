"""The K x K convolution and the two pools of the Convolutional Pose Machine (models.CPM) over the C ABI, f32 NHWC,
inference only: the one home of every launch of

    hrnet_conv2d_kxk, hrnet_conv_kxk_tile, hrnet_maxpool2d_3x3s2, hrnet_avgpool2d_9s8

Every op reads a channel slice [x_off, x_off + C) of a map (B, H, W, ldx) and writes a slice [y_off, y_off + C) of a map
(B, Ho, Wo, ldy), so the producers of a concatenated map write their parts in place and the concat is never a copy.
Two layers, as hipnet.nhwc (whose guards and layout ops - check, to_nhwc / nhwc_to_nchw - serve here too):

  raw launchers: no argument checks beyond the C entry's own (anything it cannot serve is a RuntimeError)
    conv(x, packed, bias, y, cin, x_off, cout, y_off, ks, relu)    maxpool(x, y, c, x_off, y_off)
    avgpool_center(center, y, y_off)

  checked public ops: shapes are checked before any device call, a CPU tensor is a ValueError, a required gradient a
  NotImplementedError
    tile()                          (Th, Tw, channels per pass, largest ks) of the convolution kernel
    pack(weight, cin_pad)           Conv2d weight (Cout, Cin, ks, ks) -> [pad16(Cout)][ks ks][cin_pad]
    conv_kxk(x, packed, cout, ks, bias, relu, cin, x_off, out, y_off)
    maxpool3x3s2(x, c, x_off, out, y_off)
    avgpool9s8(center, out, y_off)
"""
import torch

from hipnet import _capi as C
from hipnet import nhwc

F32 = C.HR_F32


def tile():
    """(pixel-tile height, pixel-tile width, input channels staged per pass, largest ks) of hrnet_conv2d_kxk"""
    return tuple(C.call('hrnet_conv_kxk_tile', i) for i in range(4))


# --------------------------------------------------------------------------------------------------- raw launchers
def conv(x, packed, bias, y, cin, x_off, cout, y_off, ks, relu):
    B, H, W, ldx = x.shape
    with torch.cuda.device(x.device):
        C.call('hrnet_conv2d_kxk', F32, x.data_ptr(), packed.data_ptr(), C.ptr(bias), y.data_ptr(), B, H, W, cin, ldx,
               x_off, cout, y.shape[3], y_off, ks, 1 if relu else 0, C.stream_ptr())
    return y


def maxpool(x, y, c, x_off, y_off):
    B, H, W, ldx = x.shape
    with torch.cuda.device(x.device):
        C.call('hrnet_maxpool2d_3x3s2', x.data_ptr(), y.data_ptr(), B, H, W, c, ldx, x_off, y.shape[3], y_off,
               C.stream_ptr())
    return y


def avgpool_center(center, y, y_off):
    B, _, H, W = center.shape
    with torch.cuda.device(center.device):
        C.call('hrnet_avgpool2d_9s8', center.data_ptr(), y.data_ptr(), B, H, W, y.shape[3], y_off, C.stream_ptr())
    return y


# ---------------------------------------------------------------------------------------------- checked public ops
def _no_grad(name, *ts):
    if nhwc.wants_grad(*ts):
        raise NotImplementedError('{}: backward is not built (this op is inference only): run under '
                                  'torch.no_grad()'.format(name))


def _map(name, key, t):
    if t.ndim != 4 or t.numel() == 0 or not t.is_contiguous():
        raise ValueError('{}: {} {}: expected a contiguous NHWC (B, H, W, ld), nothing empty'.format(
            name, key, tuple(t.shape)))


def _slice(name, key, off, c, ld):
    if off < 0 or c < 1 or off + c > ld:
        raise ValueError('{}: {} channels [{}, {} + {}) do not lie in a row of {}'.format(name, key, off, off, c, ld))


def pack(weight, cin_pad=None):
    """a Conv2d weight (Cout, Cin, ks, ks), odd ks <= 11 -> [pad16(Cout)][ks ks][cin_pad] (hrnet_pack_weights mode 0),
    zeros in the padding; cin_pad (default: Cin rounded up to 4) is the width of the slice the layer reads"""
    nhwc.check('conv_kxk.pack', weight=weight)
    if weight.ndim != 4 or weight.shape[2] != weight.shape[3] or not weight.shape[2] % 2 or weight.shape[2] > tile()[3]:
        raise ValueError('conv_kxk.pack: weight {}: expected (Cout, Cin, ks, ks) with an odd ks <= {}'.format(
            tuple(weight.shape), tile()[3]))
    co, ci, ks, _ = weight.shape
    cip = (ci + 3) // 4 * 4 if cin_pad is None else int(cin_pad)
    if cip < ci or cip % 4:
        raise ValueError('conv_kxk.pack: Cin = {} in {}: the padded count must hold the real one and be a multiple of '
                         '4'.format(ci, cip))
    return nhwc.pack(weight.detach().contiguous(), co, ci, ks, nhwc.pad16(co), cip, 0)


def conv_kxk(x, packed, cout, ks, bias=None, relu=False, cin=None, x_off=0, out=None, y_off=0):
    """Conv2d(cin, cout, ks, padding=ks // 2) (+ bias) (+ ReLU) on hrnet_conv2d_kxk: x (B, H, W, ldx) read at channels
    [x_off, x_off + cin) (cin, ldx, x_off multiples of 4; default: the whole row); packed weights of pack(weight, cin);
    bias (cout,). out: None for a new (B, H, W, cout) map, or a (B, H, W, ldy) map whose channels [y_off, y_off + cout)
    are written and no others. Returns the map written"""
    nhwc.check('conv_kxk', x=x, packed=packed, bias=bias, out=out)
    _map('conv_kxk', 'x', x)
    B, H, W, ldx = x.shape
    cin = ldx - x_off if cin is None else int(cin)
    ks, cout, x_off, y_off = int(ks), int(cout), int(x_off), int(y_off)
    if not ks % 2 or not 1 <= ks <= tile()[3]:
        raise ValueError('conv_kxk: ks = {}: expected an odd size <= {}'.format(ks, tile()[3]))
    _slice('conv_kxk', 'input', x_off, cin, ldx)
    if cin % 4 or ldx % 4 or x_off % 4:
        raise ValueError('conv_kxk: cin = {}, ldx = {}, x_off = {}: expected multiples of 4'.format(cin, ldx, x_off))
    if cout < 1 or packed.numel() != nhwc.pad16(cout) * ks * ks * cin:
        raise ValueError('conv_kxk: {} packed weights for cout = {} (in {}), ks = {}, cin = {}'.format(
            packed.numel(), cout, nhwc.pad16(cout), ks, cin))
    if bias is not None and bias.numel() != cout:
        raise ValueError('conv_kxk: bias has {} values for cout = {}'.format(bias.numel(), cout))
    if out is None:
        if y_off:
            raise ValueError('conv_kxk: y_off = {} without a map to write into'.format(y_off))
    else:
        _map('conv_kxk', 'out', out)
        if tuple(out.shape[:3]) != (B, H, W):
            raise ValueError('conv_kxk: out {}: expected ({}, {}, {}, ld)'.format(tuple(out.shape), B, H, W))
        _slice('conv_kxk', 'output', y_off, cout, out.shape[3])
    _no_grad('conv_kxk', x, packed, bias, out)
    if out is None:
        out = torch.empty((B, H, W, cout), dtype=torch.float32, device=x.device)
    return conv(x.detach(), packed, nhwc.contiguous(None if bias is None else bias.detach()), out, cin, x_off, cout, y_off,
                ks, relu)


def maxpool3x3s2(x, c=None, x_off=0, out=None, y_off=0):
    """MaxPool2d(3, 2, 1) of channels [x_off, x_off + c) of x (B, H, W, ldx) -> channels [y_off, y_off + c) of out
    (B, (H-1)//2 + 1, (W-1)//2 + 1, ldy) (None: a new map of c channels); the padding never wins"""
    nhwc.check('maxpool3x3s2', x=x, out=out)
    _map('maxpool3x3s2', 'x', x)
    B, H, W, ldx = x.shape
    c = ldx - x_off if c is None else int(c)
    _slice('maxpool3x3s2', 'input', int(x_off), c, ldx)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is not None:
        _map('maxpool3x3s2', 'out', out)
        if tuple(out.shape[:3]) != (B, Ho, Wo):
            raise ValueError('maxpool3x3s2: out {}: expected ({}, {}, {}, ld)'.format(tuple(out.shape), B, Ho, Wo))
        _slice('maxpool3x3s2', 'output', int(y_off), c, out.shape[3])
    elif y_off:
        raise ValueError('maxpool3x3s2: y_off = {} without a map to write into'.format(y_off))
    _no_grad('maxpool3x3s2', x, out)
    if out is None:
        out = torch.empty((B, Ho, Wo, c), dtype=torch.float32, device=x.device)
    return maxpool(x.detach(), out, c, int(x_off), int(y_off))


def avgpool9s8(center, out=None, y_off=0):
    """AvgPool2d(9, 8, 1) (count_include_pad) of center (B, 1, H, W) NCHW, H and W >= 7, into channel y_off of out
    (B, (H-7)//8 + 1, (W-7)//8 + 1, ldy) (None: a new one-channel map)"""
    nhwc.check('avgpool9s8', center=center, out=out)
    if center.ndim != 4 or center.shape[1] != 1 or center.numel() == 0 or min(center.shape[2:]) < 7:
        raise ValueError('avgpool9s8: center {}: expected (B, 1, H, W) with H, W >= 7'.format(tuple(center.shape)))
    B, _, H, W = center.shape
    Ho, Wo = (H - 7) // 8 + 1, (W - 7) // 8 + 1
    if out is not None:
        _map('avgpool9s8', 'out', out)
        if tuple(out.shape[:3]) != (B, Ho, Wo):
            raise ValueError('avgpool9s8: out {}: expected ({}, {}, {}, ld)'.format(tuple(out.shape), B, Ho, Wo))
        _slice('avgpool9s8', 'output', int(y_off), 1, out.shape[3])
    elif y_off:
        raise ValueError('avgpool9s8: y_off = {} without a map to write into'.format(y_off))
    _no_grad('avgpool9s8', center, out)
    if out is None:
        out = torch.empty((B, Ho, Wo, 1), dtype=torch.float32, device=center.device)
    return avgpool_center(center.detach().contiguous(), out, int(y_off))
