"""Error bounds for the per-channel BatchNorm statistic sums the kernel epilogues gather (no GPU needed).

A statistics producer leaves, per channel c, S = sum_p t_p with t one of y, y^2 (forward batch sums) or dz, dz*y
(backward-statistics rows), summed in f32 on the device. The reference is the same sum in f64 over exactly the
operands the device saw (inputs and weights rounded to the device dtype, staged operands rounded the way the kernel
rounds them). The allowed per-channel error is

    sum_p e_p  +  2 * D * u * sum_p (|t_p| + e_p)

  * e_p bounds the f32 error of one term. A contraction result carries 2 * K * u * (|a| * |w|)_p (K products and
    additions, u = 2^-24, the factor 2 for a matrix-core adder that need not round to nearest), plus the convolution of
    |w| with the one-ulp uncertainty of a staged operand that lies on a rounding tie; e_p is carried through y^2 and
    dz * y. A term whose ReLU mask lies within rounding of 0 is allowed whole.
  * D is the longest chain of f32 additions one term passes through on its way into the sum: read from the kernel
    source and the launch geometry (walk_chain / ring_chain below), plus the float-atomic adds per copy.

Nothing in it is fitted to an observed error. The data the tests feed are of one sign per channel, so |S| is about
sum |t| and one tile's share of a sum is far above the bound: `tile_sums` gives those shares, and every case asserts
that the bound is at most half of the smallest one."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24   # unit roundoff of f32


def q(t, dtype):
    """t rounded to the device dtype, as f64"""
    return t.to(dtype).double()


def stage(v, dtype, relu=False, addend=None, slack=None):
    """The operand a kernel stages from v = x * scale + shift (an f64 tensor, exact up to f64 rounding): one f32
    rounding (fmaf), + addend in f32 when given (the residual-sum prologue), ReLU, rounding to the dtype.
    Returns (a, da) in f64; da is nonzero where one f32 ulp of the pre-rounding value changes the staged operand
    (a rounding tie, or a second rounding the device may place differently): its size there. `slack`: the f32 value
    is only known to within this much of v (several f32 roundings before the staging): probed at v -/+ slack."""
    def finish(v32):
        if addend is not None:
            v32 = v32 + addend.float()
        if relu:
            v32 = torch.relu(v32)
        return v32.to(dtype).double()
    a = finish(v.float())
    # (finish is monotone: the extremes lie one f32 ulp beyond the ends of the window)
    lo_v, hi_v = (v, v) if slack is None else (v - slack, v + slack)
    lo = finish(torch.nextafter(lo_v.float(), torch.full_like(a, -math.inf, dtype=torch.float32)))
    hi = finish(torch.nextafter(hi_v.float(), torch.full_like(a, math.inf, dtype=torch.float32)))
    return a, torch.maximum((lo - a).abs(), (hi - a).abs())


def contraction(y, m, K, extra_adds=0):
    """e_p of a contraction result y (f64) whose absolute-value contraction is m = (|a| * |w|)_p (+ |addends|):
    K products accumulated, plus `extra_adds` f32 additions after the accumulator (bias, the old value of an
    accumulating store)"""
    return 2.0 * (K + extra_adds) * U * m


def conv_fwd(a, da, w, bias, stride, pad, extra_adds=0):
    """f64 forward conv of staged operands: (y, e) with e the per-output error bound (bias is an extra add)"""
    y = F.conv2d(a, w, bias, stride=stride, padding=pad)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    if (a < 0).any() or (w < 0).any():
        m = F.conv2d(a.abs(), w.abs(), None, stride=stride, padding=pad)
    else:
        m = y - (bias.view(1, -1, 1, 1) if bias is not None else 0)
    if bias is not None:
        m = m + bias.abs().view(1, -1, 1, 1)
    e = contraction(y, m, K, extra_adds + (1 if bias is not None else 0))
    if bool((da != 0).any()):
        e = e + F.conv2d(da, w.abs(), None, stride=stride, padding=pad)
    return y, e


def conv_dgrad(dy, w, in_hw, stride, pad):
    """f64 input gradient of a conv (dy, w exact device operands): (v, e)"""
    N, Co, Ho, Wo = dy.shape
    size = (N, w.shape[1], in_hw[0], in_hw[1])
    v = torch.nn.grad.conv2d_input(size, w, dy, stride=stride, padding=pad)
    if (dy < 0).any() or (w < 0).any():
        m = torch.nn.grad.conv2d_input(size, w.abs(), dy.abs(), stride=stride, padding=pad)
    else:
        m = v
    K = Co * w.shape[2] * w.shape[3]
    return v, m, K


def square(y, e):
    """(y^2, its bound) for a device value within e of y: |v^2 - y^2| <= 2|y|e + e^2, plus the product's rounding"""
    ay = y.abs()
    return y * y, 2 * ay * e + e * e + U * (ay + e) ** 2


def product(d, ed, y):
    """(d * y, its bound) for a device value within ed of d and an exact operand y (the fma may round the product)"""
    t = d * y
    return t, ed * y.abs() + U * (t.abs() + ed * y.abs())


def mask_terms(t, e, keep, edge):
    """apply a ReLU mask: masked-out terms are exact zeros; where the mask's argument lies within rounding of 0
    (`edge`) the device may take either side, so the whole term is allowed there"""
    tm = t * keep
    em = e * keep + edge * (t.abs() + e)
    return tm, em


def channel_bound(t, e, D):
    """per-channel bound of the f32 sum of t [N, C, H, W] (term bounds e, addition chains <= D)"""
    dims = (0, 2, 3)
    return e.sum(dims) + 2.0 * D * U * (t.abs() + e).sum(dims)


def walk_chain(th, tw, tpw, atomic_walks=0, wp_max=4):
    """longest f32 addition chain of the tile-walking body's statistics epilogue (conv_body.h): a lane adds every
    pixel it owns in each of the walk's tpw tiles (a tile's th*tw pixels are spread over 16 lanes of a wave, and
    over WP >= 1 waves), a 4-level shuffle tree over those 16 lanes (wave_sum16), WP partials added in LDS; with
    float atomics, each of the walks that share a copy adds once more (`atomic_walks` = walks per copy)"""
    return tpw * -(-(th * tw) // 16) + 4 + wp_max + atomic_walks


def ring_chain(ti, th, tw, tpw, atomic_walks=0, waves=8):
    """the same for the LDS-ring pipeline (conv_ring.hip), counted as the pixels of one row (every pixel of the
    walk in one chain) + a shuffle tree and a sum over the waves"""
    return tpw * ti * th * tw + 6 + waves + atomic_walks


def tile_view(t, th, tw, ti=1):
    """t [N, C, H, W] as [tiles, ti*th*tw, C]: the pixels of each tile (ti images x th x tw; edge tiles padded with
    zeros) in the kernels' walk order (image group, tile row, tile column)"""
    N, C, H, W = t.shape
    ty, tx, tn = -(-H // th), -(-W // tw), -(-N // ti)
    p = F.pad(t, (0, tx * tw - W, 0, ty * th - H))
    if tn * ti != N:
        p = torch.cat([p, p.new_zeros(tn * ti - N, C, ty * th, tx * tw)])
    p = p.view(tn, ti, C, ty, th, tx, tw).permute(0, 3, 5, 1, 4, 6, 2)     # [tn, ty, tx, ti, th, tw, C]
    return p.reshape(tn * ty * tx, ti * th * tw, C)


def tile_sums(t, th, tw, ti=1):
    """per-tile partial sums [tiles, C] of t [N, C, H, W] (see tile_view)"""
    return tile_view(t, th, tw, ti).sum(1)


def check(label, got, want, bound, tiles):
    """assert the device sums `got` [C] within `bound` of the f64 reference `want`, and that the bound could see one
    tile: per channel it is at most half of the smallest one-tile contribution (`tiles` = tile_sums of the terms)"""
    got, want, bound = got.double(), want.double(), bound.double()
    tmin = tiles.abs().min(0).values
    err = (got - want).abs()
    print('{}: bound max {:.3e}  smallest tile min {:.3e}  (tile / bound >= {:.1f})  err / bound max {:.3f}'.format(
        label, float(bound.max()), float(tmin.min()), float((tmin / bound).min()), float((err / bound).max())))
    assert bool((2 * bound <= tmin).all()), '{}: the bound cannot see one tile (bound {} vs tile {})'.format(
        label, bound.tolist(), tmin.tolist())
    bad = (err > bound) | torch.isnan(got)
    assert not bool(bad.any()), '{}: channels {} outside the bound: got {} want {} bound {}'.format(
        label, bad.nonzero().flatten().tolist()[:8], got[bad][:8].tolist(), want[bad][:8].tolist(), bound[bad][:8].tolist())


# ---- the cases' data and their f64 references (shared by test_bn_sums_gpu.py and test_bn_bounds_cpu.py) ----------
# Every channel's operands have one sign: non-negative staged inputs, positive weights, dz and y with a positive
# offset; ReLU masks about half on. Then |S| is about sum |t| and no tile's share cancels.

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def fwd_data(N, H, W, Cin, Cout, ks, stride, affine, bias, dtype, seed, residual=False):
    """operands of a forward conv whose output statistics are gathered: x >= 0, input BatchNorm + ReLU (about half
    of the staged inputs zero) when `affine`, positive weights and bias; `residual`: a = relu(bn(x) + x2)"""
    g = _gen(seed)
    K = Cin * ks * ks
    d = dict(x=q(torch.rand(N, Cin, H, W, generator=g), dtype).float(),
             w=q((torch.rand(Cout, Cin, ks, ks, generator=g) + 0.2) / math.sqrt(K), dtype).float())
    if affine:
        d['sc'] = torch.rand(Cin, generator=g) + 0.5
        d['sh'] = -d['sc'] * (0.4 + 0.2 * torch.rand(Cin, generator=g))
    if bias:
        d['bias'] = torch.rand(Cout, generator=g) * 0.5 + 0.1
    if residual:
        d['x2'] = q(torch.rand(N, Cin, H, W, generator=g) * 0.25, dtype).float()
    return d


def fwd_reference(d, ks, stride, dtype):
    """(y, e): f64 forward output over the operands the kernel stages, and the per-output error bound"""
    x = d['x'].double()
    if 'sc' in d:
        v = x * d['sc'].double().view(1, -1, 1, 1) + d['sh'].double().view(1, -1, 1, 1)
        a, da = stage(v, dtype, relu=True, addend=d.get('x2'))
    else:
        a, da = x, torch.zeros_like(x)
    b = d['bias'].double() if 'bias' in d else None
    return conv_fwd(a, da, d['w'].double(), b, stride, ks // 2)


def fwd_terms(y, e):
    """[(label, t, e_t)] of the forward batch sums"""
    t2, e2 = square(y, e)
    return [('sum y', y, e), ('sum y^2', t2, e2)]


def bs_data(N, H, W, Cin, Cout, ks, stride, mode, dtype, seed):
    """operands of an input-gradient launch with backward statistics (forward-conv view: x [N,Cin,H,W] -> y
    [N,Cout,Ho,Wo]): dY > 0, positive weights, the raw BatchNorm input y > 0, the old gradient (accumulated into) >= 0;
    mode bn_relu: mask = bs_y*scale+shift > 0, sum_mask: mask = bs_mask > 0, unmasked: none"""
    g = _gen(seed)
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    K = Cin * ks * ks
    d = dict(dy=q(torch.rand(N, Cout, Ho, Wo, generator=g) + 0.5, dtype).float(),
             w=q((torch.rand(Cout, Cin, ks, ks, generator=g) + 0.2) / math.sqrt(K), dtype).float(),
             yraw=q(torch.rand(N, Cin, H, W, generator=g) + 0.25, dtype).float(),
             prev=q(torch.rand(N, Cin, H, W, generator=g) * 0.5, dtype).float(), mode=mode)
    if mode == 'bn_relu':
        d['sc'] = torch.rand(Cin, generator=g) + 0.5
        d['sh'] = -d['sc'] * (0.7 + 0.1 * torch.rand(Cin, generator=g))   # (a threshold off the bf16 grid of y)
    elif mode == 'sum_mask':
        d['m'] = q(torch.randn(N, Cin, H, W, generator=g), dtype).float()
    return d


def bs_reference(d, ks, stride):
    """[(label, t, e_t)] of the backward-statistics rows: (sum dz, sum dz*y), dz = (dgrad + old) * mask"""
    w, dy = d['w'].double(), d['dy'].double()
    yr, prev = d['yraw'].double(), d['prev'].double()
    v, m, K = conv_dgrad(dy, w, yr.shape[2:], stride, ks // 2)
    v = v + prev
    ev = contraction(v, m + prev.abs(), K, 1)
    if d['mode'] == 'bn_relu':
        z = yr * d['sc'].double().view(1, -1, 1, 1) + d['sh'].double().view(1, -1, 1, 1)   # (fmaf: sign exact)
        keep = (z > 0).double()
        edge = (z.abs() <= 2 * U * (yr.abs() * d['sc'].double().view(1, -1, 1, 1) + d['sh'].double().abs().view(1, -1, 1, 1))).double()
    elif d['mode'] == 'sum_mask':
        keep = (d['m'].double() > 0).double()
        edge = (d['m'] == 0).double()
    else:
        keep, edge = torch.ones_like(v), torch.zeros_like(v)
    dz, edz = mask_terms(v, ev, keep, edge)
    t2, e2 = product(dz, edz, yr)
    return [('sum dz', dz, edz), ('sum dz*y', t2, e2)]


def fused_data(N, H, W, Cin, Cout, dtype, seed):
    """operands of the fused 3x3 backward (hrnet_conv3x3_bwd_fused): dz >= 0 carrying its ReLU mask, the raw conv output
    y > 0, BatchNorm-backward coefficients A, B, C > 0 (g = A*dz + B*y + C > 0), positive weights, the conv input x >= 0
    behind BatchNorm + ReLU (the output mask [a > 0] about half on), residual addend >= 0, next BatchNorm input > 0"""
    g = _gen(seed)
    dz = torch.rand(N, Cout, H, W, generator=g) * (torch.rand(N, Cout, H, W, generator=g) > 0.5).float()
    d = dict(dz=q(dz, dtype).float(), y=q(torch.rand(N, Cout, H, W, generator=g) + 0.25, dtype).float(),
             coef=torch.stack([torch.rand(Cout, generator=g) + 0.5, torch.rand(Cout, generator=g) * 0.15 + 0.05,
                               torch.rand(Cout, generator=g) * 0.15 + 0.05]),
             x=q(torch.rand(N, Cin, H, W, generator=g), dtype).float(),
             sc=torch.rand(Cin, generator=g) + 0.5,
             w=q((torch.rand(Cout, Cin, 3, 3, generator=g) + 0.2) / math.sqrt(Cout * 9), dtype).float(),
             addend=q(torch.rand(N, Cin, H, W, generator=g) * 0.5, dtype).float(),
             bs_y=q(torch.rand(N, Cin, H, W, generator=g) + 0.25, dtype).float())
    d['sh'] = -d['sc'] * (0.4 + 0.2 * torch.rand(Cin, generator=g))
    return d


def fused_reference(d, dtype):
    """[(label, t, e_t)] of the fused backward's rows: (sum dx, sum dx*bs_y), dx = (conv^T(g) + addend) * [a > 0] with
    g = fmaf(A, dz, fmaf(B, y, C)) staged in the dtype and a = relu(fmaf(x, scale, shift)) staged in the dtype"""
    A, Bc, Cc = (d['coef'][k].double().view(1, -1, 1, 1) for k in range(3))
    dz, y = d['dz'].double(), d['y'].double()
    v = A * dz + Bc * y + Cc
    g, dg = stage(v, dtype, slack=3 * U * ((A * dz).abs() + (Bc * y).abs() + Cc.abs()))
    w, add = d['w'].double(), d['addend'].double()
    dx, m, K = conv_dgrad(g, w, d['x'].shape[2:], 1, 1)
    e = contraction(dx, m + add, K, 1) + torch.nn.grad.conv2d_input(dx.shape, w.abs(), dg, padding=1)
    dx = dx + add
    a, da = stage(d['x'].double() * d['sc'].double().view(1, -1, 1, 1) + d['sh'].double().view(1, -1, 1, 1), dtype,
                  relu=True)
    keep = (a > 0).double()
    edge = ((da > 0) & (a <= da)).double()
    t1, e1 = mask_terms(dx, e, keep, edge)
    t2, e2 = product(t1, e1, d['bs_y'].double())
    return [('sum dx', t1, e1), ('sum dx*y', t2, e2)]
