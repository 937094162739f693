"""The feature transform layer and the general 3x3 convolution of FTLMultiviewNet's head (models.FTL_encoder_decoder)
over the C ABI, f32 NHWC, inference only: the one home of every launch of

    hrnet_ftl_gather, hrnet_ftl_scatter, hrnet_conv2d_3x3g

Every op reads a channel slice [x_off, x_off + C) of a map (N, H, W, ldx) and writes a slice of a map (N, Ho, Wo, ldy), as
hipnet.conv_kxk (whose hrnet_conv2d_kxk with ks 1 is the head's 1x1 convolution). Two layers, as hipnet.conv_kxk:

  raw launchers: no argument checks beyond the C entry's own (anything it cannot serve is a RuntimeError)
    gather_raw(x, coef, y, B, V, c, x_off, y_off, slice)    scatter_raw(f, coef, y, B, V, c, f_off, y_off)
    conv(x, packed, bias, y, cin, x_off, cout, y_off, stride, pad_lo, z, relu)

  checked public ops: shapes are checked before any device call, a CPU tensor is a ValueError, a required gradient a
  NotImplementedError
    affines(extrinsic, intrinsic)       the gather and scatter coefficients (B, V, 12) each: float64 on the host, float32
                                        on the device of `extrinsic`
    gather(x, coef, V, c, x_off, out, y_off, slice)      (B V, h, w, ldx) -> view v into slice v of (B, h, w, ldy)
    scatter(f, coef, V, c, f_off, out, y_off)            (B, h, w, ldf) -> (B V, h, w, ldy), slot b V + v
    out_size(n, stride, pad_lo, z, pad_hi)               the output size of conv3x3g along one axis
    conv3x3g(x, packed, cout, stride, pad_lo, z, out_hw, bias, relu, cin, x_off, out, y_off)
    counts(...)                                          MACs issued and useful of one conv3x3g launch (host arithmetic)

Both transforms read a map per channel as 3-vectors - triplets of consecutive pixels in row-major order - and map each by
x -> x A + c: gather A = K^-T R^-T, c = -t^T R^-T (pixels -> camera -> world), scatter A = R^T K^T, c = t^T K^T (back).
"""
import torch

from hipnet import _capi as C
from hipnet import conv_kxk as KX
from hipnet import nhwc

F32 = C.HR_F32


# --------------------------------------------------------------------------------------------------- raw launchers
def gather_raw(x, coef, y, B, V, c, x_off, y_off, slice_):
    _, H, W, ldx = x.shape
    with torch.cuda.device(x.device):
        C.call('hrnet_ftl_gather', x.data_ptr(), coef.data_ptr(), y.data_ptr(), B, V, H, W, c, ldx, x_off, y.shape[3], y_off,
               slice_, C.stream_ptr())
    return y


def scatter_raw(f, coef, y, B, V, c, f_off, y_off):
    _, H, W, ldf = f.shape
    with torch.cuda.device(f.device):
        C.call('hrnet_ftl_scatter', f.data_ptr(), coef.data_ptr(), y.data_ptr(), B, V, H, W, c, ldf, f_off, y.shape[3], y_off,
               C.stream_ptr())
    return y


def conv(x, packed, bias, y, cin, x_off, cout, y_off, stride, pad_lo, z, relu):
    N, H, W, ldx = x.shape
    with torch.cuda.device(x.device):
        C.call('hrnet_conv2d_3x3g', F32, x.data_ptr(), packed.data_ptr(), C.ptr(bias), y.data_ptr(), N, H, W, cin, ldx, x_off,
               cout, y.shape[3], y_off, y.shape[1], y.shape[2], stride, pad_lo, z, 1 if relu else 0, C.stream_ptr())
    return y


# ---------------------------------------------------------------------------------------------- checked public ops
def _no_grad(name, *ts):
    if nhwc.wants_grad(*ts):
        raise NotImplementedError('{}: backward is not built (this op is inference only): run under '
                                  'torch.no_grad()'.format(name))


def affines(extrinsic, intrinsic):
    """extrinsic (B, V, 3, 4) = [R | t], intrinsic (3, 3) or (B, 3, 3) (a batch whose matrices differ is refused: the
    reference uses the first for all) -> (gather, scatter) coefficients, (B, V, 12) float32 each on extrinsic's device: A
    row-major, then c. Computed in float64 on the host (two 3x3 inverses per batch)."""
    if not isinstance(extrinsic, torch.Tensor) or not isinstance(intrinsic, torch.Tensor):
        raise ValueError('ftl.affines: expected tensors')
    if extrinsic.ndim != 4 or tuple(extrinsic.shape[2:]) != (3, 4) or extrinsic.numel() == 0:
        raise ValueError('ftl.affines: extrinsic {}: expected (B, V, 3, 4)'.format(tuple(extrinsic.shape)))
    B, V = extrinsic.shape[:2]
    K = intrinsic.detach().double().cpu()
    if K.ndim == 3 and K.shape[0] in (1, B) and tuple(K.shape[1:]) == (3, 3):
        if not bool((K == K[:1]).all()):
            raise ValueError('ftl.affines: the intrinsic matrices of the batch differ: the transform takes one for all views '
                             'and frames')
        K = K[0]
    if tuple(K.shape) != (3, 3):
        raise ValueError('ftl.affines: intrinsic {}: expected (3, 3) or ({}, 3, 3)'.format(tuple(intrinsic.shape), B))
    E = extrinsic.detach().double().cpu()
    Rt, tt, Kt = E[..., :3].transpose(2, 3), E[..., 3:].transpose(2, 3), K.t()
    Ri = torch.inverse(Rt)
    Ag, cg = torch.inverse(Kt) @ Ri, -(tt @ Ri)
    As, cs = Rt @ Kt, tt @ Kt
    pack = lambda A, c: torch.cat([A.reshape(B, V, 9), c.reshape(B, V, 3)], -1).float().contiguous().to(extrinsic.device)
    return pack(Ag, cg), pack(As, cs)


def _transform_args(name, x, coef, V, c, off, rows):
    nhwc.check(name, x=x, coef=coef)
    KX._map(name, 'x', x)
    N, H, W, ld = x.shape
    V = int(V)
    c = ld - off if c is None else int(c)
    if V < 1 or N % rows(V):
        raise ValueError('{}: {} maps for V = {}'.format(name, N, V))
    B = N // rows(V)
    if (H * W) % 3:
        raise ValueError('{}: a {} x {} map has {} pixels: no whole number of triplets'.format(name, H, W, H * W))
    KX._slice(name, 'input', off, c, ld)
    if c % 4 or ld % 4 or off % 4:
        raise ValueError('{}: c = {}, ld = {}, offset = {}: expected multiples of 4'.format(name, c, ld, off))
    if tuple(coef.shape) != (B, V, 12) or not coef.is_contiguous():
        raise ValueError('{}: coef {}: expected a contiguous ({}, {}, 12)'.format(name, tuple(coef.shape), B, V))
    return B, V, H, W, c


def _transform_out(name, out, shape, off, width):
    if out is None:
        if off:
            raise ValueError('{}: y_off = {} without a map to write into'.format(name, off))
        return
    KX._map(name, 'out', out)
    if tuple(out.shape[:3]) != shape:
        raise ValueError('{}: out {}: expected {} + (ld,)'.format(name, tuple(out.shape), shape))
    KX._slice(name, 'output', off, width, out.shape[3])
    if out.shape[3] % 4 or off % 4:
        raise ValueError('{}: out ld = {}, y_off = {}: expected multiples of 4'.format(name, out.shape[3], off))


def gather(x, coef, V, c=None, x_off=0, out=None, y_off=0, slice=None):
    """x (B V, h, w, ldx) in slot order b V + v, channels [x_off, x_off + c) -> (B, h, w, ldy) with view v's transformed
    channels at [y_off + v slice, y_off + v slice + c) (slice: default c; out: default a new (B, h, w, V c) map). coef: the
    gather coefficients of affines()"""
    x_off, y_off = int(x_off), int(y_off)
    B, V, H, W, c = _transform_args('ftl.gather', x, coef, V, c, x_off, lambda v: v)
    slice_ = c if slice is None else int(slice)
    if slice_ < c or slice_ % 4:
        raise ValueError('ftl.gather: slice = {}: expected a multiple of 4 that holds c = {}'.format(slice_, c))
    nhwc.check('ftl.gather', out=out)
    _transform_out('ftl.gather', out, (B, H, W), y_off, (V - 1) * slice_ + c)
    _no_grad('ftl.gather', x, coef, out)
    if out is None:
        make = torch.empty if slice_ == c else torch.zeros
        out = make((B, H, W, V * slice_), dtype=torch.float32, device=x.device)
    return gather_raw(x.detach(), coef.detach(), out, B, V, c, x_off, y_off, slice_)


def scatter(f, coef, V, c=None, f_off=0, out=None, y_off=0):
    """f (B, h, w, ldf), channels [f_off, f_off + c) -> (B V, h, w, ldy) in slot order b V + v, view v's transform of f at
    channels [y_off, y_off + c) (out: default a new (B V, h, w, c) map). coef: the scatter coefficients of affines()"""
    f_off, y_off = int(f_off), int(y_off)
    B, V, H, W, c = _transform_args('ftl.scatter', f, coef, V, c, f_off, lambda v: 1)
    nhwc.check('ftl.scatter', out=out)
    _transform_out('ftl.scatter', out, (B * V, H, W), y_off, c)
    _no_grad('ftl.scatter', f, coef, out)
    if out is None:
        out = torch.empty((B * V, H, W, c), dtype=torch.float32, device=f.device)
    return scatter_raw(f.detach(), coef.detach(), out, B, V, c, f_off, y_off)


def _geometry(name, stride, pad_lo, z):
    stride, pad_lo, z = int(stride), int(pad_lo), int(z)
    if stride not in (1, 2) or pad_lo not in (0, 1, 2) or (z, stride) not in ((1, 1), (1, 2), (2, 1)):
        raise ValueError('{}: stride = {}, pad_lo = {}, z = {}: expected stride 1 or 2, pad_lo 0 .. 2, z 1 or (with stride 1) '
                         '2'.format(name, stride, pad_lo, z))
    return stride, pad_lo, z


def out_size(n, stride, pad_lo, z=1, pad_hi=None):
    """the output size along an axis of n inputs: ((n - 1) z + 1 + pad_lo + pad_hi - 3) // stride + 1; pad_hi defaults to
    pad_lo. Conv2d(3, 2, 2): out_size(n, 2, 2); ConvTranspose2d(3, 2, 2, output_padding op): out_size(n, 1, 0, 2, op)"""
    pad_hi = pad_lo if pad_hi is None else pad_hi
    return ((n - 1) * z + 1 + pad_lo + pad_hi - 3) // stride + 1


def size_range(n, stride, pad_lo, z=1):
    """(smallest, largest) output size hrnet_conv2d_3x3g takes: no padding behind the map, and two rows of it"""
    return max(out_size(n, stride, pad_lo, z, 0), 1), out_size(n, stride, pad_lo, z, 2)


def conv3x3g(x, packed, cout, stride, pad_lo, z=1, out_hw=None, bias=None, relu=False, cin=None, x_off=0, out=None, y_off=0):
    """a 3x3 convolution (+ bias) (+ ReLU) on hrnet_conv2d_3x3g: the input x (N, H, W, ldx), read at channels
    [x_off, x_off + cin), is taken zero-stuffed by z, padded by pad_lo in front, and convolved at `stride` into
    out_hw = (Ho, Wo) outputs (default: padding pad_lo behind as well). packed: conv_kxk.pack / nhwc.conv_pack of the
    Conv2d weight, or nhwc.conv_transpose_pack of a ConvTranspose2d one (z = 2, stride 1, pad_lo = 2 - padding).
    out: None for a new (N, Ho, Wo, cout) map, or a (N, Ho, Wo, ldy) map whose channels [y_off, y_off + cout) are written
    and no others. Returns the map written"""
    nhwc.check('conv3x3g', x=x, packed=packed, bias=bias, out=out)
    KX._map('conv3x3g', 'x', x)
    N, H, W, ldx = x.shape
    stride, pad_lo, z = _geometry('conv3x3g', stride, pad_lo, z)
    cin = ldx - x_off if cin is None else int(cin)
    cout, x_off, y_off = int(cout), int(x_off), int(y_off)
    KX._slice('conv3x3g', 'input', x_off, cin, ldx)
    if cin % 4 or ldx % 4 or x_off % 4:
        raise ValueError('conv3x3g: cin = {}, ldx = {}, x_off = {}: expected multiples of 4'.format(cin, ldx, x_off))
    if cout < 1 or packed.numel() != nhwc.pad16(cout) * 9 * cin:
        raise ValueError('conv3x3g: {} packed weights for cout = {} (in {}), cin = {}'.format(
            packed.numel(), cout, nhwc.pad16(cout), cin))
    if bias is not None and bias.numel() != cout:
        raise ValueError('conv3x3g: bias has {} values for cout = {}'.format(bias.numel(), cout))
    if out_hw is None:
        out_hw = (out_size(H, stride, pad_lo, z), out_size(W, stride, pad_lo, z)) if out is None else tuple(out.shape[1:3])
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    for key, n, o in (('Ho', H, Ho), ('Wo', W, Wo)):
        lo, hi = size_range(n, stride, pad_lo, z)
        if not lo <= o <= hi:
            raise ValueError('conv3x3g: {} = {}: {} inputs with z = {}, stride = {}, pad_lo = {} give {} .. {}'.format(
                key, o, n, z, stride, pad_lo, lo, hi))
    if out is None:
        if y_off:
            raise ValueError('conv3x3g: y_off = {} without a map to write into'.format(y_off))
    else:
        KX._map('conv3x3g', 'out', out)
        if tuple(out.shape[:3]) != (N, Ho, Wo):
            raise ValueError('conv3x3g: out {}: expected ({}, {}, {}, ld)'.format(tuple(out.shape), N, Ho, Wo))
        KX._slice('conv3x3g', 'output', y_off, cout, out.shape[3])
    _no_grad('conv3x3g', x, packed, bias, out)
    if out is None:
        out = torch.empty((N, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    return conv(x.detach(), packed, nhwc.contiguous(None if bias is None else bias.detach()), out, cin, x_off, cout, y_off,
                stride, pad_lo, z, relu)


def counts(N, H, W, cin, cout, Ho, Wo, stride, pad_lo, z, tile=(8, 16, 16)):
    """(launch grid, MACs issued, MACs useful) of one hrnet_conv2d_3x3g launch; host arithmetic that mirrors the entry's
    dispatch. Issued: every MFMA of every workgroup, the masked pixels of its 128-pixel tiles and the padded channels
    included; the taps of a transposed layer that meet stuffed zeros are not issued. Useful: the products of a real weight with a real input. tile: (Th, Tw, channels per
    pass) of the kernel, conv_kxk.tile()[:3]"""
    th, tw, kc = tile
    cout_pad, cin_pad = nhwc.pad16(cout), (cin + kc - 1) // kc * kc
    ha, wa, step = -(-Ho // z), -(-Wo // z), stride if z == 1 else 1
    tiles, strips = (ha + th - 1) // th * ((wa + tw - 1) // tw), -(-ha * wa // (th * tw))
    # strips of 128 consecutive pixels where they need fewer tiles and their window of whole rows fits 48 KB of LDS
    if strips < tiles and (((th * tw - 1) // wa + 1) * step + 3) * ((wa - 1) * step + 3) <= 768:
        tiles = strips
    ptiles = N * z * z * tiles
    if cout_pad % 64 == 0 and ptiles * (cout_pad // 64) >= 512:
        cb = 64
    elif ptiles * ((cout_pad + 31) // 32) >= 256:
        cb = 32
    else:
        cb = 16
    blocks = -(-cout_pad // cb)
    issued = 0
    for ph in range(z):
        for pw in range(z):
            live = sum(1 for r in range(3) if z == 1 or (ph + r - pad_lo) % 2 == 0) * \
                sum(1 for s in range(3) if z == 1 or (pw + s - pad_lo) % 2 == 0)
            issued += N * tiles * th * tw * blocks * cb * live * cin_pad

    def real(n_out, n_in):
        k = 0
        for o in range(n_out):
            for r in range(3):
                i = o * stride + r - pad_lo
                k += i % z == 0 and 0 <= i // z < n_in
        return k
    useful = N * real(Ho, H) * real(Wo, W) * cin * cout
    return (ptiles, blocks), issued, useful
