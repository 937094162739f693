"""float64 reference and per-element bounds of hipnet.upsample_slice (csrc/upsample_slice.hip): a channel slice of an NHWC
map resampled bilinearly with align_corners and written as NCHW, and its transpose.

The reference is torch's own F.interpolate in float64 on the sliced, permuted tensor, and its autograd.

Bounds (f32 kernel against the float64 reference, per element), and where they come from.

Position. The kernel's position is fl(fl((in-1)/(out-1)) * index): two f32 roundings of a number <= in - 1, so it differs
from the exact one by |dpos| <= 2^-23 (in - 1) per axis.

Forward. The blend is continuous and piecewise linear in the position, with slope (lower row/column blend minus upper)
at most 2 M in magnitude, so the position costs at most |dpos_y| 2 M + |dpos_x| 2 M = 2^-22 ((h-1) + (w-1)) M. The three
lerps (two in x, one in y) round 1 - lambda, two products and a sum each: a few 2^-24 M, bounded by 2^-21 M. So

    |out - ref| <= [2^-22 ((h-1) + (w-1)) + 2^-21] M.

M is the largest magnitude among the element's four neighbours AND the source pixels next to them (the neighbour set
dilated by one pixel): a position within |dpos| of an integer may round to the other side, and the cell it then blends
in has one row or column outside the four neighbours; by continuity the value still moves by at most |dpos| times that
cell's slope, which the dilated M covers. On dyadic size pairs nothing rounds at all (exact()).

Backward. dsrc[y][x] = sum over the footprint of wy(Y) wx(X) g[Y][X]. Each weight is 1-Lipschitz in its position and at
most 1, so |d(wy wx)| <= |dpos_y| + |dpos_x| = 2^-23 ((h-1) + (w-1)); an output that enters or leaves the footprint through
rounding does so with a weight <= |dpos|, which the same term covers once S is taken over the footprint dilated by one
output row and column. The f32 sum of n terms by fma, with 1 - lambda and wy wx rounded, costs at most (n + 3) 2^-24 S. So

    |dsrc - ref| <= [2^-23 ((h-1) + (w-1)) + (n + 3) 2^-24] S,   S = sum |g| over the dilated footprint, n its length.
"""
import numpy as np
import torch
import torch.nn.functional as F

# (N, h, w, Cp, c0, C, H, W)
CASES = ((2, 4, 4, 56, 32, 22, 8, 8),          # the model's slice at a non-dyadic ratio
         (1, 32, 32, 56, 32, 22, 64, 64),      # the real map size
         (1, 1, 1, 4, 0, 1, 5, 3),             # one source pixel
         (1, 3, 5, 8, 3, 5, 3, 5),             # equal sizes, odd c0, slice ending at Cp
         (1, 5, 2, 4, 1, 2, 1, 7),             # H = 1
         (3, 7, 9, 36, 0, 32, 4, 5),           # down-sampling: some sources get no weight
         (1, 2, 70, 4, 0, 3, 3, 139),          # rows wider than a wave: column-tile seams
         (1, 3, 3, 132, 100, 32, 5, 5))        # Cp > 128
# dyadic size pairs 2->3, 3->5, 2->5, 5->9, 3->9, 4->4, 1->k: every position and weight is a short dyadic fraction, so with
# integer inputs in [-8, 8] the float64 result is a float32 number and the kernel must match it bit for bit
DYADIC = ((1, 2, 3, 8, 1, 5, 3, 5), (1, 2, 5, 8, 3, 5, 5, 9), (1, 3, 4, 8, 0, 3, 9, 4), (1, 1, 1, 4, 0, 3, 4, 6),
          (2, 3, 2, 40, 3, 34, 5, 3), (1, 5, 3, 4, 1, 2, 9, 9), (1, 1, 4, 5, 2, 3, 7, 4))


def inputs(case, seed=0, integer=False):
    """(src (N, h, w, Cp), g (N, C, H, W)) float32 numpy"""
    N, h, w, Cp, c0, C, H, W = case
    rng = np.random.RandomState(1000 + seed + sum(case))
    if integer:
        return (rng.randint(-8, 9, (N, h, w, Cp)).astype(np.float32), rng.randint(-8, 9, (N, C, H, W)).astype(np.float32))
    return rng.randn(N, h, w, Cp).astype(np.float32), rng.randn(N, C, H, W).astype(np.float32)


def forward(src, case, dtype=torch.float64, align_corners=True, shift=0):
    N, h, w, Cp, c0, C, H, W = case
    x = torch.as_tensor(src).to(dtype)[..., c0 + shift:c0 + shift + C].permute(0, 3, 1, 2)
    return F.interpolate(x, size=(H, W), mode='bilinear', align_corners=align_corners)


def backward(g, case, dtype=torch.float64, align_corners=True):
    """the gradient of the slice, (N, h, w, C)"""
    N, h, w, Cp, c0, C, H, W = case
    x = torch.zeros((N, h, w, C), dtype=dtype, requires_grad=True)
    y = F.interpolate(x.permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=align_corners)
    y.backward(torch.as_tensor(g).to(dtype))
    return x.grad


def _pos(n_in, n_out):
    return np.arange(n_out, dtype=np.float64) * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)


def forward_bound(src, case):
    """(N, C, H, W) float64: the bound of the module docstring"""
    N, h, w, Cp, c0, C, H, W = case
    a = torch.as_tensor(src).double()[..., c0:c0 + C].permute(0, 3, 1, 2).abs()
    a = F.max_pool2d(a, 3, stride=1, padding=1)
    y0 = np.minimum(np.floor(_pos(h, H)).astype(np.int64), h - 1)
    x0 = np.minimum(np.floor(_pos(w, W)).astype(np.int64), w - 1)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    m = None
    for ys in (y0, y1):
        for xs in (x0, x1):
            v = a[:, :, torch.as_tensor(ys)][:, :, :, torch.as_tensor(xs)]
            m = v if m is None else torch.maximum(m, v)
    return (2.0 ** -22 * ((h - 1) + (w - 1)) + 2.0 ** -21) * m


def _footprint(n_in, n_out):
    """(n_out, n_in) 0/1: output index in the footprint of the source index, dilated by one output index"""
    f = np.abs(_pos(n_in, n_out)[:, None] - np.arange(n_in)[None, :]) <= 1.0
    d = f.copy()
    d[1:] |= f[:-1]
    d[:-1] |= f[1:]
    return d.astype(np.float64)


def backward_bound(g, case):
    """(N, h, w, C) float64: the bound of the module docstring"""
    N, h, w, Cp, c0, C, H, W = case
    fy, fx = torch.as_tensor(_footprint(h, H)), torch.as_tensor(_footprint(w, W))
    s = torch.einsum('Yy,ncYX,Xx->nyxc', fy, torch.as_tensor(g).double().abs(), fx)
    n = torch.einsum('y,x->yx', fy.sum(0), fx.sum(0))[None, :, :, None]
    return (2.0 ** -23 * ((h - 1) + (w - 1)) + (n + 3) * 2.0 ** -24) * s


def exact(t):
    """every value of the float64 tensor is a float32 number"""
    return bool(torch.equal(t.float().double(), t))
