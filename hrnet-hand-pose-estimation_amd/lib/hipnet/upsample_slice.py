"""A channel slice of an f32 NHWC map, resampled bilinearly with align_corners and written as NCHW
(csrc/upsample_slice.hip): the one home of every launch of

    hrnet_upsample_slice_nchw, hrnet_upsample_slice_nchw_bwd

It is the joint between the CPM backbone (f32 NHWC, heat maps inside a concatenated map, stride 8) and the volumetric half
(f32 NCHW at MODEL.HEATMAP_SIZE). hipnet.nhwc's hrnet_bilinear_cat / hrnet_upsample_bilinear_t work on whole NHWC maps
and serve the HRNet head; they are not touched. Two layers, as hipnet.conv_kxk:

  raw launchers: no argument checks beyond the C entry's own (anything it cannot serve is a RuntimeError)
    forward(src, dst, c0, C)                     dst (N, C, H, W) <- src (N, h, w, Cp)[..., c0 : c0 + C]
    backward(ddst, dsrc, c0, C, accumulate)      the slice of dsrc (N, h, w, Cp) <- ddst (N, C, H, W)

  checked public ops: shapes are checked before any device call, a CPU tensor is a ValueError
    upsample_slice(x, c0, C, size)               differentiable in x (ONE torch.autograd.Function)
    upsample_slice_bwd(g, size_in, Cp, c0, C, out=None, accumulate=False)

The backward is a gather without atomics in a fixed order: two runs give equal bits.
"""
import torch

from hipnet import _capi as C
from hipnet import nhwc


# --------------------------------------------------------------------------------------------------- raw launchers
def forward(src, dst, c0, c):
    N, h, w, Cp = src.shape
    with torch.cuda.device(src.device):
        C.call('hrnet_upsample_slice_nchw', src.data_ptr(), dst.data_ptr(), N, h, w, Cp, c0, c, dst.shape[2], dst.shape[3],
               C.stream_ptr())
    return dst


def backward(ddst, dsrc, c0, c, accumulate):
    N, h, w, Cp = dsrc.shape
    with torch.cuda.device(ddst.device):
        C.call('hrnet_upsample_slice_nchw_bwd', ddst.data_ptr(), dsrc.data_ptr(), N, h, w, Cp, c0, c, ddst.shape[2],
               ddst.shape[3], 1 if accumulate else 0, C.stream_ptr())
    return dsrc


# ---------------------------------------------------------------------------------------------- checked public ops
def _size(name, size):
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('{}: size {!r}: expected (H, W)'.format(name, size)) from None
    if H < 1 or W < 1:
        raise ValueError('{}: size ({}, {}): expected H, W >= 1'.format(name, H, W))
    return H, W


def _slice(name, c0, c, Cp):
    c0, c = int(c0), int(c)
    if not C.call('hrnet_upsample_slice_nchw_supported', int(Cp), c0, c):
        raise ValueError('{}: channels [{}, {} + {}) do not lie in a row of {}'.format(name, c0, c0, c, Cp))
    return c0, c


class _UpsampleSliceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c0, c, H, W):
        ctx.meta = (tuple(x.shape), c0, c)
        out = torch.empty((x.shape[0], c, H, W), dtype=torch.float32, device=x.device)
        return forward(x.detach(), out, c0, c)

    @staticmethod
    def backward(ctx, g):
        shape, c0, c = ctx.meta
        # the gradient of the whole map: zeros outside the slice
        dx = torch.zeros(shape, dtype=torch.float32, device=g.device)
        backward(g.detach().contiguous().float(), dx, c0, c, False)
        return dx, None, None, None, None


def upsample_slice(x, c0, c, size):
    """F.interpolate(x[..., c0 : c0 + c].permute(0, 3, 1, 2), size, mode='bilinear', align_corners=True): x (N, h, w, Cp)
    contiguous f32 NHWC on the HIP device -> (N, c, H, W) NCHW. Differentiable in x: the gradient is zero outside the
    slice"""
    name = 'upsample_slice'
    nhwc.check(name, x=x)
    if x.ndim != 4 or x.numel() == 0 or not x.is_contiguous():
        raise ValueError('{}: x {}: expected a contiguous NHWC (N, h, w, Cp), nothing empty'.format(name, tuple(x.shape)))
    c0, c = _slice(name, c0, c, x.shape[3])
    H, W = _size(name, size)
    if nhwc.wants_grad(x):
        return _UpsampleSliceFn.apply(x, c0, c, H, W)
    out = torch.empty((x.shape[0], c, H, W), dtype=torch.float32, device=x.device)
    return forward(x.detach(), out, c0, c)


def upsample_slice_bwd(g, size_in, Cp, c0, c, out=None, accumulate=False):
    """the transpose of upsample_slice: g (N, c, H, W) contiguous f32 NCHW -> channels [c0, c0 + c) of out (N, h, w, Cp)
    (None: a new map of zeros), written, or added onto when accumulate; the other channels keep their bits"""
    name = 'upsample_slice_bwd'
    nhwc.check(name, g=g, out=out)
    if g.ndim != 4 or g.numel() == 0 or not g.is_contiguous():
        raise ValueError('{}: g {}: expected a contiguous NCHW (N, C, H, W), nothing empty'.format(name, tuple(g.shape)))
    h, w = _size(name, size_in)
    c0, c = _slice(name, c0, c, Cp)
    if g.shape[1] != c:
        raise ValueError('{}: g {} for a slice of {} channels'.format(name, tuple(g.shape), c))
    if out is None:
        if accumulate:
            raise ValueError('{}: accumulate without a map to add onto'.format(name))
        out = torch.zeros((g.shape[0], h, w, int(Cp)), dtype=torch.float32, device=g.device)
    elif tuple(out.shape) != (g.shape[0], h, w, int(Cp)) or not out.is_contiguous():
        raise ValueError('{}: out {}: expected a contiguous ({}, {}, {}, {})'.format(name, tuple(out.shape), g.shape[0], h, w,
                                                                                  int(Cp)))
    return backward(g.detach(), out.detach(), c0, c, accumulate)
