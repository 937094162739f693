"""Float64 references, per-element bounds, input generators and case lists for the 2-D backbone contraction kernels
(conv_body.h in its six modes, conv_ring.hip, gemm_pw.hip, wgrad.hip, bwd_fused.hip, bwd_pw.hip). Nothing here imports
the project: tests/test_contraction_refs_cpu.py pins these functions without a GPU, tests/test_contraction_kernels_gpu.py
holds the kernels to them.

Every case is generated twice.

(a) Integer lattice. All operands are small integers, the input scale is +-1, shift / bias / cC are integers, cA is in
    {+-1, +-2}, cB in {-1, 0, 1}. Every product and partial sum is an integer below 2^24, so f32 accumulation is exact
    in any order (float atomics included) and the device must EQUAL the float64 reference. Where the output is stored
    in bf16 the largest sum |a||w| (+ |bias| + |addend| + |prior|) over the output elements is at most 256: every
    result is a bf16 value, and one lost or doubled product changes the stored bits. That is reached by density, not
    by a small K: values from {-1, 0, 1} with P(nonzero) = min(1, sqrt(150 / K)) per operand, where the operand is what
    the MFMA sees (relu(x + shift), g = cA dz + cB y + cC), not the tensor in memory. f32 outputs take dense values in
    [-2, 2]. `lattice_conditions` asserts all of it per case, and the decisive zeros: pre-activations of exactly 0 in
    front of a prologue ReLU, mask operands +0 and -0, a == 0 under mask_out, zeros in dz.

(b) Real-valued. Normal draws rounded through the device dtype, weights scaled by 1 / sqrt(K). With u = 2^-24,
    v = 2^-8 and K the products of one output (pad channels included), per element:
      contraction            (K + 3) u S, S the same contraction over absolute values (+ |bias| + |prior| + |addend|)
      bf16 store             + v (|ref| + contraction bound)
      f32 prologue           + 2 u ((|x scale| + |shift|) conv |w|)   (3 u with the residual term of conv2d_sum)
      f32 g = cA dz + cB y + cC   + 2 u ((|cA dz| + |cB y| + |cC|) conv |w|)
      rows of the fused backward   the sum over the pixels of the f32 element's bound (x |bs_y|) + (P + 3) u sum |dx (bs_y)|;
                                   bwd_pw_kernel<64, 256> sums the STORED tile, so there the stored element's bound
    In bf16 the transformed operand is known to the bit instead: the scale is a signed power of two, the shift a
    multiple of 2^-12 below 4, |x| is 0 or at least 2^-12 and at most 2, so x scale + shift (+ x2) is exact in f32 fused
    or not and its bf16 rounding is determinate (`exact_in_f32`); the bf16 real-valued runs of the fused backward
    kernels take coef = None and leave the coefficient path to the lattice.

What the kernels do with a prior value (read from the code, bounded as read): conv_body.h adds the old output in f32
to accumulator + bias before the single rounding of the store (accumulate = 1, also through the LDS ring);
bwd_fused.hip and bwd_pw.hip add the addend in f32 to the accumulator before the mask and the single rounding, in place
or not. So the prior's term is |prior| inside S - one rounding, not two.

Out of scope, because coefficients built on the device involve invstd, which is not known to the bit:
hrnet_conv2d_bnref, the in_sums prologue (of hrnet_conv2d_sum as well) and the HrBnBwdRef form of the fused backward
launches. The statistics themselves (rows of sum y / sum y^2) stay with tests/test_bn_sums_gpu.py."""
import collections
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
V = 2.0 ** -8
BF16_EXACT = 256.0          # integers up to here are bf16 values
F32_EXACT = 2.0 ** 24
DTYPES = ('f32', 'bf16')


# ---- number formats -------------------------------------------------------------------------------------------
def q(t, dtype):
    """float64 tensor rounded (to nearest even) through the device dtype, kept in float64"""
    t = t.float()
    return (t.bfloat16().float() if dtype == 'bf16' else t).double()


def bf16_truncate(t):
    """float64 tensor (f32-representable) -> bf16 by truncation, the wrong store the sensitivity tests apply"""
    bits = t.float().contiguous().view(torch.int32)
    return (bits & -65536).view(torch.float32).double()


def exact_in_f32(t):
    return bool((t.float().double() == t).all())


def is_integer(t):
    return bool((t == t.round()).all())


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def density(K):
    return min(1.0, math.sqrt(150.0 / K))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _sparse(rng, shape, p, vals=(-1.0, 1.0)):
    return _t(rng.choice(vals, shape) * (rng.random(shape) < p))


def _dense(rng, shape):
    return _t(rng.integers(-2, 3, shape))


def bc(v):
    return v.view(1, -1, 1, 1)


def _pad_c(t, c, dim=1, value=0.0):
    """zero-pad (or `value`-pad) dimension `dim` of t to c entries"""
    if t.shape[dim] == c:
        return t
    shape = list(t.shape)
    shape[dim] = c - t.shape[dim]
    return torch.cat([t, torch.full(shape, value, dtype=t.dtype)], dim)


# ---- float64 references ---------------------------------------------------------------------------------------
def out_hw(H, W, ks, stride):
    p = ks // 2
    return (H + 2 * p - ks) // stride + 1, (W + 2 * p - ks) // stride + 1


def conv(a, w, stride=1, bias=None):
    return F.conv2d(a, w, bias, stride=stride, padding=w.shape[-1] // 2)


def dgrad(dy, w, stride, hw):
    """input gradient of y = conv(x, w, stride) for an input of extent hw"""
    ks = w.shape[-1]
    p = ks // 2
    oh = hw[0] - ((dy.shape[2] - 1) * stride - 2 * p + ks)
    ow = hw[1] - ((dy.shape[3] - 1) * stride - 2 * p + ks)
    return F.conv_transpose2d(dy, w, None, stride=stride, padding=p, output_padding=(oh, ow))


def dgrad_zero_stuffed(dy, w, hw):
    """the stride-2 input gradient as the kernels' zero-stuffed form states it: dY spread over a (2Ho-1) x (2Wo-1)
    grid, a stride-1 conv with the flipped, transposed kernel, cropped to hw"""
    n, c, ho, wo = dy.shape
    assert ho == (hw[0] + 1) // 2 and wo == (hw[1] + 1) // 2
    z = torch.zeros(n, c, hw[0], hw[1], dtype=dy.dtype)
    z[:, :, ::2, ::2] = dy
    return F.conv2d(z, w.flip(2, 3).transpose(0, 1), None, stride=1, padding=w.shape[-1] // 2)


def wgrad(a, dy, ks, stride):
    """weight gradient [Cout][Cin][ks][ks] of y = conv(a, w, stride)"""
    shape = (dy.shape[1], a.shape[1], ks, ks)
    return torch.nn.grad.conv2d_weight(a, shape, dy, stride=stride, padding=ks // 2)


def prologue(x, sc, sh, relu, x2=None):
    t = x if sc is None else x * bc(sc) + bc(sh)
    if x2 is not None:
        t = t + x2
    return F.relu(t) if relu else t


def prologue_abs(x, sc, sh, x2=None):
    """sum of the magnitudes the f32 prologue rounds"""
    t = (x * bc(sc)).abs() + bc(sh).abs()
    return t if x2 is None else t + x2.abs()


def contraction_bound(K, S):
    return (K + 3) * U * S


def stored_bound(ref, cb, dtype):
    """contraction bound cb -> bound of the stored element"""
    return cb + V * (ref.abs() + cb) if dtype == 'bf16' else cb


# ---- forward convolution --------------------------------------------------------------------------------------
ConvCase = collections.namedtuple('ConvCase', 'N H W cin cout ks stride form cin_real cout_real')
FORMS = {
    # affine, relu, bias, statistics rows, accumulate -> hrnet_conv_mode
    'fwd': dict(affine=True, relu=True, bias=False, stats=True, acc=False, mode=2),
    'fwd_raw': dict(affine=False, relu=False, bias=False, stats=True, acc=False, mode=2),
    'fwdb': dict(affine=True, relu=True, bias=True, stats=True, acc=False, mode=4),
    'fwdb_ns': dict(affine=False, relu=False, bias=True, stats=False, acc=False, mode=4),
    'gen': dict(affine=True, relu=True, bias=False, stats=False, acc=False, mode=0),
    'gen_acc': dict(affine=True, relu=False, bias=False, stats=False, acc=True, mode=0),
    'dg': dict(affine=False, relu=False, bias=False, stats=False, acc=False, mode=3),
}


def cc(N, H, W, cin, cout, ks, stride, form, cin_real=None, cout_real=None):
    return ConvCase(N, H, W, cin, cout, ks, stride, form, cin_real or cin, cout_real or cout)


def _lattice_input(rng, shape, p, dense, sc, sh, relu, x2=None):
    """x such that the staged operand a = relu?(sc x + sh (+ x2)) has the wanted density; returns (x, a).
    relu: pre-activations are 1 with probability p, else one of {-2, -1, 0} - the exact zeros in front of the ReLU"""
    if dense:
        t = _dense(rng, shape)
    elif relu:
        # (at most 7 in 8 positive, so that a small K, where p = 1, still has its zeros)
        t = torch.where(_t(rng.random(shape)) < min(p, 0.875),torch.ones(shape, dtype=torch.float64), _t(rng.integers(-2, 1, shape)))
    else:
        t = _sparse(rng, shape, p)
    if sc is None:
        return t, (F.relu(t) if relu else t)
    x = (t - bc(sh) - (0 if x2 is None else x2)) * bc(sc)        # sc = +-1
    return x, (F.relu(t) if relu else t)


def _affine(rng, c, c_real, dtype, lattice):
    """per-channel scale / shift of an input prologue, pad channels scale 1 shift 0"""
    if lattice:
        sc, sh = _t(rng.choice([-1.0, 1.0], c_real)), _t(rng.integers(-2, 3, c_real))
    elif dtype == 'bf16':
        sc = _t(rng.choice([-2.0, -1.0, 1.0, 2.0], c_real))
        sh = _t(rng.integers(-4 * 4096 + 1, 4 * 4096, c_real) / 4096.0)
    else:
        sc = q(_t(rng.uniform(0.5, 1.5, c_real) * rng.choice([-1.0, 1.0], c_real)), 'f32')
        sh = q(_t(rng.normal(0.0, 0.5, c_real)), 'f32')
    return _pad_c(sc, c, 0, 1.0), _pad_c(sh, c, 0, 0.0)


def _real_input(rng, shape, dtype, clamp=None):
    """normal draws through the device dtype; bf16 prologue inputs: |x| <= clamp, and 0 or at least 2^-12"""
    x = _t(rng.normal(0.0, 1.0, shape))
    if clamp is not None:
        x = x.clamp(-clamp, clamp)
    x = q(x, dtype)
    if clamp is not None and dtype == 'bf16':
        x = torch.where(x.abs() < 2.0 ** -12, torch.zeros_like(x), x)
    return x


@functools.lru_cache(maxsize=4)
def conv_data(case, dtype, lattice):
    """operands (NCHW float64, tensor channel counts: pad channels are zero), reference and bound of one forward case.
    keys: x w sc sh bias prior a ref S bound K t (pre-activation, lattice)"""
    c = case
    f = FORMS[c.form]
    rng = np.random.default_rng(seed_of('conv', c, dtype, lattice))
    K = c.ks * c.ks * c.cin
    Ho, Wo = out_hw(c.H, c.W, c.ks, c.stride)
    dense = lattice and dtype == 'f32'
    p = density(K)
    xs, ws = (c.N, c.cin_real, c.H, c.W), (c.cout_real, c.cin_real, c.ks, c.ks)
    sc = sh = None
    if f['affine']:
        sc, sh = _affine(rng, c.cin, c.cin_real, dtype, lattice)
    e_a = None
    if lattice:
        x, a = _lattice_input(rng, xs, p, dense, None if sc is None else sc[:c.cin_real],
                              None if sh is None else sh[:c.cin_real], f['relu'])
        w = _dense(rng, ws) if dense else _sparse(rng, ws, p)
        bias = _t(rng.integers(-3, 4, c.cout_real)) if f['bias'] else None
        prior = (_dense(rng, (c.N, c.cout_real, Ho, Wo)) if dense else _sparse(rng, (c.N, c.cout_real, Ho, Wo), 0.5)) if f['acc'] else None
    else:
        x = _real_input(rng, xs, dtype, clamp=2.0 if f['affine'] else None)
        w = q(_t(rng.normal(0.0, 1.0, ws)) / math.sqrt(K), dtype)
        bias = q(_t(rng.normal(0.0, 1.0, c.cout_real)), 'f32') if f['bias'] else None
        prior = q(_t(rng.normal(0.0, 1.0, (c.N, c.cout_real, Ho, Wo))), dtype) if f['acc'] else None
        a = prologue(x, None if sc is None else sc[:c.cin_real], None if sh is None else sh[:c.cin_real], f['relu'])
        if dtype == 'bf16':
            a = q(a, 'bf16')           # determinate: the pre-activation is exact in f32 (exactness_conditions)
        elif f['affine']:
            e_a = 2 * U * prologue_abs(x, sc[:c.cin_real], sh[:c.cin_real])
    x, a, w = _pad_c(x, c.cin), _pad_c(a, c.cin), _pad_c(_pad_c(w, c.cin), c.cout, 0)
    bias = None if bias is None else _pad_c(bias, c.cout, 0)
    prior = None if prior is None else _pad_c(prior, c.cout)
    ref = conv(a, w, c.stride, bias)
    S = conv(a.abs(), w.abs(), c.stride, None if bias is None else bias.abs())
    if prior is not None:
        ref, S = ref + prior, S + prior.abs()
    bound = None
    if not lattice:
        cb = contraction_bound(K, S)
        if e_a is not None:
            cb = cb + conv(_pad_c(e_a, c.cin), w.abs(), c.stride)
        bound = stored_bound(ref, cb, dtype)
    return dict(x=x, w=w, sc=sc, sh=sh, bias=bias, prior=prior, a=a, ref=ref, S=S, bound=bound, K=K)


def lattice_conditions(d, out_dtype, zeros_of=()):
    """the conditions of (a) for one generated case: integers, exactness of every sum, the decisive zeros"""
    for k, v in d.items():
        if torch.is_tensor(v) and k not in ('bound',):
            assert is_integer(v), k
    cap = BF16_EXACT if out_dtype == 'bf16' else F32_EXACT - 1
    for k in ('S', 'S_dx'):
        if d.get(k) is not None:
            assert float(d[k].max()) <= cap, (k, float(d[k].max()), cap)
    for k in ('S_gw', 'S_rows'):
        if d.get(k) is not None:
            assert float(d[k].max()) < F32_EXACT, (k, float(d[k].max()))
    for k in zeros_of:
        assert bool((d[k] == 0).any()), 'no exact zero in ' + k


def exactness_conditions(x, sc, sh, x2=None):
    """bf16 real-valued prologue: scale a signed power of two, shift a multiple of 2^-12 below 4, |x| 0 or >= 2^-12, and
    the pre-activation exact in f32 - so the kernel's fmaf (or a multiply and an add) rounds nothing"""
    assert bool(((sc.abs().log2() % 1) == 0).all())
    assert bool((sh * 4096 == (sh * 4096).round()).all()) and float(sh.abs().max()) < 4
    for t in (x,) if x2 is None else (x, x2):
        nz = t[t != 0]
        assert nz.numel() == 0 or float(nz.abs().min()) >= 2.0 ** -12
    pre = x * bc(sc) + bc(sh)
    assert exact_in_f32(x * bc(sc)) and exact_in_f32(pre)
    if x2 is not None:
        assert exact_in_f32(pre + x2)


# tile ids of conv_body.h (choose_tile) -> (tile h, tile w, output-channel block); CONV_TILE[case] is the id a case is
# meant for (None: the one-pixel and one-line maps, any tile), which the GPU test asserts through hrnet_conv_tile_walk
TILES = {0: (16, 16, 32), 1: (8, 16, 64), 2: (8, 8, 64), 3: (8, 8, 32), 4: (8, 16, 128), 6: (16, 16, 32), 7: (8, 16, 64)}
ALL_FORMS = ('fwd', 'fwd_raw', 'fwdb', 'fwdb_ns', 'gen', 'gen_acc', 'dg')
_BY_TILE = (
    # map extents of one pixel and one line, every mode
    (None, [cc(1, 1, 1, 32, 32, 3, 1, f) for f in ALL_FORMS] + [cc(1, 1, 17, 32, 32, 3, 1, f) for f in ALL_FORMS] +
     [cc(1, 17, 1, 40, 48, 3, 1, f) for f in ALL_FORMS]),
    # id 0: 16x16 / BN32
    (0, [cc(1, 16, 16, 32, 32, 3, 1, 'fwd'), cc(1, 17, 19, 40, 32, 3, 1, 'fwdb'), cc(1, 17, 19, 48, 16, 3, 1, 'gen_acc'),
         cc(1, 16, 16, 72, 32, 1, 1, 'dg'), cc(1, 17, 19, 8, 32, 3, 1, 'fwd', cin_real=3),
         cc(1, 16, 16, 128, 32, 1, 1, 'fwd'), cc(1, 16, 16, 480, 32, 1, 1, 'fwdb', cout_real=21)]),
    # id 3: 8x8 / BN32, km = 2 for 3x3; stride 2 with Cout 32
    (3, [cc(2, 8, 8, 96, 32, 3, 1, 'fwd'), cc(1, 9, 7, 40, 32, 3, 1, 'gen'), cc(1, 9, 7, 72, 32, 3, 1, 'fwdb', cout_real=21),
         cc(2, 16, 16, 32, 32, 3, 2, 'fwd_raw'), cc(1, 13, 21, 48, 32, 3, 2, 'fwdb'), cc(1, 9, 7, 64, 32, 1, 1, 'gen_acc')]),
    # id 1: 8x16 / BN64
    (1, [cc(1, 16, 16, 64, 64, 3, 1, 'fwd'), cc(1, 17, 33, 40, 64, 3, 1, 'gen'), cc(1, 17, 33, 96, 80, 3, 1, 'fwdb_ns'),
         cc(1, 16, 16, 64, 48, 1, 1, 'fwd'), cc(1, 16, 16, 72, 144, 3, 1, 'dg'), cc(1, 16, 16, 256, 64, 1, 1, 'fwd'),
         cc(1, 16, 16, 96, 64, 1, 1, 'dg')]),
    # the width rule: Wo of 17..24 with Cout > 32 goes to the 8x8 tiles (demoted to BN32 below 512 workgroups)
    (3, [cc(1, 16, 20, 48, 64, 3, 1, 'fwd'), cc(1, 17, 24, 32, 80, 3, 1, 'gen_acc'), cc(2, 8, 8, 256, 128, 1, 1, 'fwd')]),
    # id 4: 8x16 / BN128 (1x1, Cout >= 128); Cin on both sides of the km switch (2 kstep: 64 bf16, 32 f32)
    (4, [cc(1, 16, 16, 64, 128, 1, 1, 'fwd'), cc(1, 16, 17, 96, 144, 1, 1, 'fwdb'), cc(1, 16, 16, 32, 256, 1, 1, 'gen'),
         cc(1, 16, 16, 40, 128, 1, 1, 'dg'), cc(1, 16, 16, 96, 128, 1, 1, 'dg')]),
    # id 2: 8x8 / BN64, only with >= 512 workgroups
    (2, [cc(8, 64, 64, 32, 256, 3, 2, 'fwd'), cc(128, 8, 8, 32, 256, 3, 1, 'gen')]),
    # several tiles per workgroup (tpw 2), and a last workgroup that walks fewer tiles
    (0, [cc(130, 32, 32, 32, 32, 3, 1, 'fwd'), cc(130, 32, 32, 32, 32, 1, 1, 'fwdb'), cc(130, 32, 32, 32, 32, 1, 1, 'gen_acc'),
         cc(130, 32, 32, 32, 32, 3, 1, 'dg'), cc(513, 16, 16, 32, 32, 1, 1, 'fwd')]),
)
CONV_CASES = tuple(c for _, group in _BY_TILE for c in group)
CONV_TILE = {c: t for t, group in _BY_TILE for c in group}
# Cin at the 16-byte minimum: 8 for bf16, 4 for f32
MIN_CIN_CASES = {'bf16': cc(1, 9, 7, 8, 32, 3, 1, 'fwd'), 'f32': cc(1, 9, 7, 4, 32, 3, 1, 'fwd')}

# the LDS ring (bf16): (case, ring id, hrnet_conv_ring_enable value)
RING_FWD_CASES = (
    (cc(2, 16, 16, 32, 32, 3, 1, 'gen'), 1, 1), (cc(1, 17, 19, 32, 16, 3, 1, 'dg'), 1, 1),
    (cc(2, 16, 16, 64, 64, 3, 1, 'gen'), 2, 1), (cc(1, 17, 33, 64, 48, 3, 1, 'dg'), 2, 1),
    (cc(3, 16, 16, 128, 128, 3, 1, 'gen'), 3, 1), (cc(1, 20, 37, 96, 64, 3, 1, 'gen'), 3, 2),
    (cc(5, 8, 8, 256, 256, 3, 1, 'gen'), 4, 1), (cc(2, 8, 8, 96, 80, 3, 1, 'dg'), 4, 1),
)
# gemm_pw (bf16): pixel counts around the block of G_BM pixels; (Cin = Cout, with bias, pixels as a multiple of G_BM + r)
GEMM_CHANNELS = (256, 480)
GEMM_PIXELS = ((0, 1), (1, -1), (1, 1), (3, 5))


def gemm_case(ch, bias, pixels):
    return cc(1, 1, pixels, ch, ch, 1, 1, 'fwdb_ns' if bias else 'dg')


# ---- conv with the residual sum in its prologue ---------------------------------------------------------------------
SumCase = collections.namedtuple('SumCase', 'N H W cin cout ks')
SUM_CASES = (SumCase(1, 1, 1, 32, 32, 3), SumCase(1, 17, 19, 40, 32, 3), SumCase(2, 8, 8, 96, 48, 3),
             SumCase(1, 16, 16, 64, 64, 3), SumCase(1, 16, 17, 96, 128, 1), SumCase(1, 9, 7, 64, 32, 1),
             SumCase(130, 32, 32, 32, 32, 1), SumCase(1, 16, 16, 128, 32, 1), SumCase(1, 16, 16, 256, 64, 1),
             SumCase(2, 8, 8, 256, 32, 1))
RING_SUM_CASES = ((SumCase(2, 16, 16, 32, 32, 3), 1), (SumCase(1, 17, 19, 32, 32, 3), 1), (SumCase(1, 17, 33, 64, 64, 3), 2))


@functools.lru_cache(maxsize=4)
def sum_data(case, dtype, lattice):
    """hrnet_conv2d_sum: a = relu(sc x + sh + x2), y = conv(a). keys: x x2 w sc sh a ref S bound e_side K"""
    c = case
    rng = np.random.default_rng(seed_of('sum', c, dtype, lattice))
    K = c.ks * c.ks * c.cin
    dense = lattice and dtype == 'f32'
    p = density(K)
    xs, ws = (c.N, c.cin, c.H, c.W), (c.cout, c.cin, c.ks, c.ks)
    sc, sh = _affine(rng, c.cin, c.cin, dtype, lattice)
    e_side = None
    if lattice:
        x2 = _dense(rng, xs) if dense else _sparse(rng, xs, 0.5)
        x, a = _lattice_input(rng, xs, p, dense, sc, sh, True, x2)
        w = _dense(rng, ws) if dense else _sparse(rng, ws, p)
    else:
        x = _real_input(rng, xs, dtype, clamp=2.0)
        x2 = _real_input(rng, xs, dtype, clamp=4.0)
        w = q(_t(rng.normal(0.0, 1.0, ws)) / math.sqrt(K), dtype)
        a = prologue(x, sc, sh, True, x2)
        if dtype == 'bf16':
            a = q(a, 'bf16')
        else:
            e_side = 3 * U * prologue_abs(x, sc, sh, x2)
    ref = conv(a, w)
    S = conv(a.abs(), w.abs())
    bound = None
    if not lattice:
        cb = contraction_bound(K, S)
        if e_side is not None:
            cb = cb + conv(e_side, w.abs())
        bound = stored_bound(ref, cb, dtype)
    return dict(x=x, x2=x2, w=w, sc=sc, sh=sh, a=a, ref=ref, S=S, bound=bound, e_side=e_side, K=K,
                t=x * bc(sc) + bc(sh) + x2)


# ---- input gradients ------------------------------------------------------------------------------------------------
# forward-conv view: x [N, cin, H, W] -> y [N, cout, Ho, Wo]; the launch reads dy and the mode-1 packed weights and
# writes dx. form: 'dg' plain (stride 2: the four-parity S2D form), 'zs' stride 2 zero-stuffed through CONV_GENERIC
# (in_relu on dy selects that body), 'bs_*' hrnet_conv2d_bwdstats with its mask source, '+m' = bs_store_masked
DgradCase = collections.namedtuple('DgradCase', 'N H W cin cout ks stride form acc')
DGRAD_CASES = (
    DgradCase(1, 1, 1, 32, 32, 3, 1, 'dg', 0), DgradCase(1, 17, 19, 32, 40, 3, 1, 'dg', 1),
    DgradCase(1, 16, 16, 64, 72, 3, 1, 'dg', 0), DgradCase(2, 8, 8, 48, 96, 3, 1, 'dg', 1),
    DgradCase(1, 16, 17, 144, 64, 1, 1, 'dg', 1), DgradCase(1, 9, 7, 32, 64, 1, 1, 'dg', 0),
    DgradCase(2, 8, 8, 256, 128, 1, 1, 'dg', 1),
    # 3x3 stride 2, odd and even out_hw; S2D tile 6 (fewer than 64 input channels of the forward) and 7
    DgradCase(1, 16, 16, 32, 32, 3, 2, 'dg', 0), DgradCase(2, 17, 19, 48, 64, 3, 2, 'dg', 1),
    DgradCase(1, 32, 34, 64, 40, 3, 2, 'dg', 1), DgradCase(1, 17, 33, 80, 128, 3, 2, 'dg', 0),
    DgradCase(1, 16, 16, 32, 32, 3, 2, 'zs', 0), DgradCase(1, 17, 19, 48, 64, 3, 2, 'zs', 1),
    DgradCase(1, 20, 18, 64, 40, 3, 2, 'zs', 0),
    # backward statistics (CONV_BS): the dx it stores
    DgradCase(1, 17, 19, 32, 40, 3, 1, 'bs_bn_relu', 1), DgradCase(1, 17, 19, 32, 40, 3, 1, 'bs_sum_mask+m', 1),
    DgradCase(1, 16, 16, 64, 64, 3, 1, 'bs_unmasked', 0), DgradCase(2, 8, 8, 48, 96, 3, 1, 'bs_bn_relu+m', 0),
    DgradCase(1, 16, 16, 64, 256, 1, 1, 'bs_bn_relu', 1), DgradCase(1, 16, 17, 144, 64, 1, 1, 'bs_sum_mask', 1), DgradCase(1, 16, 16, 256, 64, 1, 1, 'bs_bn_relu+m', 1),
    DgradCase(2, 17, 19, 32, 64, 3, 2, 'bs_bn_relu+m', 1), DgradCase(1, 32, 34, 64, 40, 3, 2, 'bs_sum_mask', 0),
    DgradCase(1, 16, 16, 32, 32, 3, 2, 'bs_unmasked', 1), DgradCase(130, 32, 32, 32, 32, 1, 1, 'bs_sum_mask+m', 1),
    DgradCase(130, 32, 32, 32, 32, 3, 1, 'dg', 1),
)
# the LDS ring's input gradient (bf16; channel counts of the launch: dy has cout channels): (case, ring id, enable)
RING_DGRAD_CASES = (
    (DgradCase(3, 16, 16, 128, 128, 3, 1, 'dg', 1), 3, 1), (DgradCase(2, 16, 16, 64, 96, 3, 1, 'dg', 0), 3, 1),
    (DgradCase(5, 8, 8, 256, 256, 3, 1, 'dg', 1), 4, 1), (DgradCase(1, 20, 37, 64, 96, 3, 1, 'bs_sum_mask+m', 1), 3, 2),
    (DgradCase(3, 16, 16, 128, 128, 3, 1, 'bs_bn_relu', 1), 3, 1), (DgradCase(5, 8, 8, 128, 256, 3, 1, 'bs_bn_relu+m', 0), 4, 1),
    (DgradCase(2, 16, 16, 128, 128, 3, 1, 'bs_unmasked', 1), 3, 1),
)


@functools.lru_cache(maxsize=4)
def dgrad_data(case, dtype, lattice):
    """keys: dy w prior ref S bound K, and for the backward-statistics forms bs_y bs_mask bs_sc bs_sh m (mask operand)
    v (the unmasked gradient)"""
    c = case
    rng = np.random.default_rng(seed_of('dgrad', c, dtype, lattice))
    K = c.ks * c.ks * c.cout
    Ho, Wo = out_hw(c.H, c.W, c.ks, c.stride)
    dense = lattice and dtype == 'f32'
    p = density(K)
    ys, ws, xs = (c.N, c.cout, Ho, Wo), (c.cout, c.cin, c.ks, c.ks), (c.N, c.cin, c.H, c.W)
    if lattice:
        dy = _dense(rng, ys) if dense else _sparse(rng, ys, min(1.0, 2 * p) if c.form == 'zs' else p)
        w = _dense(rng, ws) if dense else _sparse(rng, ws, p)
        prior = (_dense(rng, xs) if dense else _sparse(rng, xs, 0.5)) if c.acc else None
    else:
        dy = q(_t(rng.normal(0.0, 1.0, ys)), dtype)
        w = q(_t(rng.normal(0.0, 1.0, ws)) / math.sqrt(c.ks * c.ks * c.cin), dtype)
        prior = q(_t(rng.normal(0.0, 1.0, xs)), dtype) if c.acc else None
    g = F.relu(dy) if c.form == 'zs' else dy            # (in_relu on the raw gradient: what selects CONV_GENERIC)
    v = dgrad(g, w, c.stride, (c.H, c.W))
    S = dgrad(g.abs(), w.abs(), c.stride, (c.H, c.W))
    if prior is not None:
        v, S = v + prior, S + prior.abs()
    d = dict(dy=dy, w=w, prior=prior, v=v, S=S, K=K)
    ref = v
    if c.form.startswith('bs_'):
        kind = c.form[3:].split('+')[0]
        d['bs_y'] = _dense(rng, xs) if lattice else q(_t(rng.normal(0.0, 1.0, xs)), dtype)
        if kind == 'bn_relu':
            if lattice:
                d['bs_sc'], d['bs_sh'] = _t(rng.choice([-1.0, 1.0], c.cin)), _t(rng.integers(-2, 3, c.cin))
            else:
                d['bs_sc'] = q(_t(rng.uniform(0.5, 1.5, c.cin) * rng.choice([-1.0, 1.0], c.cin)), 'f32')
                d['bs_sh'] = q(_t(rng.normal(0.0, 0.5, c.cin)), 'f32')
            d['m'] = d['bs_y'] * bc(d['bs_sc']) + bc(d['bs_sh'])
        elif kind == 'sum_mask':
            # (+0 and -0 among the mask operands: neither is > 0)
            m = _t(rng.choice([-1.0, -0.0, 0.0, 1.0], xs)) if lattice else q(_t(rng.normal(0.0, 1.0, xs)), dtype)
            d['bs_mask'] = d['m'] = m
        if c.form.endswith('+m') and 'm' in d:
            ref = v * (d['m'] > 0)
    d['ref'] = ref
    d['bound'] = None if lattice else stored_bound(v, contraction_bound(K, S), dtype)
    return d


# ---- weight gradients -----------------------------------------------------------------------------------------------
# x [N, cin, H, W] (cin_real real channels), dy [N, cout, Ho, Wo] (cout_real real); wg = the choose_wg id meant
WgradCase = collections.namedtuple('WgradCase', 'N H W cin cout ks stride affine cin_real cout_real wg')


def wc(N, H, W, cin, cout, ks, stride, affine, wg, cin_real=None, cout_real=None):
    return WgradCase(N, H, W, cin, cout, ks, stride, affine, cin_real or cin, cout_real or cout, wg)


WGRAD_CASES = (
    wc(1, 1, 1, 32, 32, 3, 1, True, 1), wc(1, 1, 17, 32, 32, 3, 1, False, 1), wc(1, 17, 1, 40, 64, 3, 1, True, 3),
    wc(1, 1, 17, 64, 48, 1, 1, True, 10),
    wc(2, 16, 16, 32, 32, 3, 1, True, 0), wc(1, 16, 33, 40, 32, 3, 1, False, 0),
    wc(2, 8, 8, 48, 32, 3, 1, True, 1), wc(2, 16, 16, 32, 32, 3, 2, False, 1), wc(2, 9, 7, 8, 32, 3, 1, True, 1, cin_real=3),
    wc(1, 16, 16, 72, 64, 3, 1, True, 2), wc(1, 16, 33, 96, 80, 3, 1, False, 2),
    wc(3, 8, 8, 96, 64, 3, 1, False, 3), wc(1, 13, 21, 48, 144, 3, 2, True, 3), wc(1, 16, 20, 32, 64, 3, 1, True, 3),
    wc(2, 9, 7, 64, 48, 1, 1, True, 10), wc(3, 8, 8, 96, 32, 1, 1, False, 10, cout_real=21),
    wc(1, 9, 7, 256, 256, 1, 1, True, 11), wc(1, 16, 17, 480, 256, 1, 1, False, 11),
    wc(521, 8, 8, 32, 32, 3, 1, True, 1),          # 521 tiles, a prime: no even split
)
WGRAD_UNEVEN = WGRAD_CASES[-1]
WGRAD_STEM = wc(2, 9, 7, 32, 64, 1, 1, False, 10, cin_real=27)      # the im2col'ed 3x3 stem: k = (r 3 + s) 3 + ci
# choose_wg id -> (tile h, tile w, output-channel block)
WG_TILES = {0: (16, 16, 32), 1: (8, 8, 32), 2: (16, 16, 64), 3: (8, 8, 64), 10: (8, 16, 64), 11: (8, 16, 128)}


@functools.lru_cache(maxsize=4)
def wgrad_data(case, dtype, lattice):
    """keys: x dy sc sh a prior (what the gradient buffer holds, real extents) ref (real extents) S_gw bound P"""
    c = case
    rng = np.random.default_rng(seed_of('wgrad', c, dtype, lattice))
    Ho, Wo = out_hw(c.H, c.W, c.ks, c.stride)
    P = c.N * Ho * Wo
    xs, ys = (c.N, c.cin_real, c.H, c.W), (c.N, c.cout_real, Ho, Wo)
    sc = sh = e_a = None
    if c.affine:
        sc, sh = _affine(rng, c.cin, c.cin_real, dtype, lattice)
    if lattice:
        x, a = _lattice_input(rng, xs, 1.0, True, None if sc is None else sc[:c.cin_real],
                              None if sh is None else sh[:c.cin_real], c.affine)
        dy = _dense(rng, ys)
    else:
        x = _real_input(rng, xs, dtype, clamp=2.0 if c.affine else None)
        dy = q(_t(rng.normal(0.0, 1.0, ys)), dtype)
        a = prologue(x, None if sc is None else sc[:c.cin_real], None if sh is None else sh[:c.cin_real], c.affine)
        if dtype == 'bf16':
            a = q(a, 'bf16')
        elif c.affine:
            e_a = 2 * U * prologue_abs(x, sc[:c.cin_real], sh[:c.cin_real])
    gshape = (c.cout_real, c.cin_real, c.ks, c.ks)
    prior = _t(rng.integers(-3, 4, gshape)) if lattice else q(_t(rng.normal(0.0, 1.0, gshape)), 'f32')
    ref = wgrad(a, dy, c.ks, c.stride)
    S = wgrad(a.abs(), dy.abs(), c.ks, c.stride)
    bound = None
    if not lattice:
        # P products per element, summed within a tile, across tiles, across splits: any order is within gamma_P
        bound = contraction_bound(P, S)
        if e_a is not None:
            bound = bound + wgrad(e_a, dy.abs(), c.ks, c.stride)
    return dict(x=_pad_c(x, c.cin), dy=_pad_c(dy, c.cout), sc=sc, sh=sh, a=_pad_c(a, c.cin), prior=prior, ref=ref,
                S_gw=S + prior.abs(), bound=bound, P=P)


def kflat_to_oihw(g, cin_real, ks):
    """[Cout][k = (r ks + s) cin_real + ci] of the im2col'ed stem -> [Cout][cin_real][ks][ks]"""
    return g.reshape(g.shape[0], ks, ks, cin_real).permute(0, 3, 1, 2).contiguous()


# ---- fused backward: 3x3 (bwd_fused.hip) and 1x1 (bwd_pw.hip) ------------------------------------------------------------
# a = relu(sc x + sh) or x; g = cA dz + cB y + cC (rounded to the compute dtype) or dz; gw = wgrad(a, g);
# v = dgrad(g, w) (+ addend); dx = v [a > 0] when mask_out; rows = (sum dx, sum dx bs_y)
FusedCase = collections.namedtuple('FusedCase', 'N H W cin cout ks affine addend mask coef rows')
COMBOS = ((True, False, True, True, True), (False, True, True, True, True), (True, True, True, True, True),
           (False, False, False, False, False))
FUSED_CASES = (
    [FusedCase(2, 16, 16, 32, 32, 3, *k) for k in COMBOS] +
    [FusedCase(1, 17, 19, 32, 32, 3, *COMBOS[2]), FusedCase(1, 1, 1, 32, 32, 3, *COMBOS[2]),
     FusedCase(1, 20, 12, 48, 48, 3, *COMBOS[2]), FusedCase(2, 16, 16, 64, 64, 3, *COMBOS[2]),
     FusedCase(1, 17, 19, 64, 32, 3, *COMBOS[0]), FusedCase(1, 16, 16, 40, 64, 3, *COMBOS[1]),
     FusedCase(1, 20, 12, 96, 96, 3, *COMBOS[2]), FusedCase(2, 16, 16, 128, 128, 3, *COMBOS[1]),
     FusedCase(1, 9, 17, 128, 64, 3, *COMBOS[0]), FusedCase(1, 16, 16, 8, 32, 3, *COMBOS[2]),
     FusedCase(130, 16, 16, 32, 32, 3, *COMBOS[2])])         # more tiles than splits: several tiles per walk
PW_CASES = (
    [FusedCase(2, 16, 16, 64, 256, 1, *COMBOS[0]), FusedCase(2, 16, 16, 256, 64, 1, *COMBOS[1]),
     FusedCase(2, 16, 16, 64, 64, 1, *COMBOS[2]), FusedCase(1, 9, 7, 64, 256, 1, *COMBOS[0]),
     FusedCase(3, 11, 13, 256, 64, 1, *COMBOS[1]), FusedCase(1, 8, 8, 64, 256, 1, *COMBOS[3]),
     FusedCase(1, 1, 1, 64, 64, 1, *COMBOS[2]), FusedCase(1, 8, 8, 64, 64, 1, *COMBOS[3]),
     FusedCase(1, 9, 7, 64, 64, 1, *COMBOS[0]), FusedCase(1, 9, 7, 64, 64, 1, *COMBOS[1]),
     FusedCase(1, 8, 8, 256, 64, 1, False, False, False, True, True),
     FusedCase(5, 64, 64, 64, 64, 1, *COMBOS[2]), FusedCase(5, 64, 64, 256, 64, 1, *COMBOS[1]),
     FusedCase(5, 64, 64, 64, 256, 1, *COMBOS[0])])           # 320 tiles on 160 workgroups


def fused_formula(a, g, w, addend, mask, bsy):
    """(dx, gw, rows) of the fused backward from the staged operands"""
    ks = w.shape[-1]
    v = dgrad(g, w, 1, a.shape[2:])
    if addend is not None:
        v = v + addend
    if mask:
        v = v * (a > 0)
    rows = torch.stack([v.sum((0, 2, 3)), (v * bsy).sum((0, 2, 3)) if bsy is not None else torch.zeros(a.shape[1], dtype=v.dtype)])
    return v, wgrad(a, g, ks, 1), rows


def _lattice_coef(rng, shape, p, dense):
    """(cA, cB, cC, dz, y, g): g = cA dz + cB y + cC with the density asked for. Channels with |cA| = 2 take cB = 0, an
    even cC and even g so that dz is an integer; the others exercise cB and odd cC"""
    n, co, h, w_ = shape
    cA = _t(rng.choice([-2.0, -1.0, 1.0, 2.0], co))
    two = cA.abs() == 2
    cB = torch.where(two, torch.zeros(co, dtype=torch.float64), _t(rng.choice([-1.0, 0.0, 1.0], co)))
    cC = torch.where(two, _t(rng.choice([-2.0, 0.0, 2.0], co)), _t(rng.integers(-1, 2, co)))
    y = _sparse(rng, shape, 0.5)
    g1 = _dense(rng, shape) if dense else _sparse(rng, shape, p)
    g2 = 2 * (_dense(rng, shape).clamp(-1, 1) if dense else _sparse(rng, shape, p / 2))
    g = torch.where(bc(two), g2, g1)
    dz = (g - bc(cB) * y - bc(cC)) / bc(cA)
    return cA, cB, cC, dz, y, g


@functools.lru_cache(maxsize=4)
def fused_data(case, dtype, lattice):
    """keys: x sc sh a dz y coef ([3][cout] or None) g w addend bsy dx gw rows prior (of the atomic gradient)
    S_dx S_gw S_rows b_dx b_gw b_rows"""
    c = case
    rng = np.random.default_rng(seed_of('fused', c, dtype, lattice))
    K = c.ks * c.ks * c.cout
    P = c.N * c.H * c.W
    dense = lattice and dtype == 'f32'
    p = min(density(K), 0.875)        # (a small K, where the density is 1, still has zeros in dz)
    xs, ys, ws = (c.N, c.cin, c.H, c.W), (c.N, c.cout, c.H, c.W), (c.cout, c.cin, c.ks, c.ks)
    sc = sh = e_a = e_g = coef = y = None
    if c.affine:
        sc, sh = _affine(rng, c.cin, c.cin, dtype, lattice)
    use_coef = c.coef and (lattice or dtype == 'f32')      # bf16 in reals: coef = None, the lattice holds that path
    if lattice:
        x, a = _lattice_input(rng, xs, 0.5, dense, sc, sh, c.affine)
        if use_coef:
            cA, cB, cC, dz, y, g = _lattice_coef(rng, ys, p, dense)
            coef = torch.stack([cA, cB, cC])
        else:
            dz = g = _dense(rng, ys) if dense else _sparse(rng, ys, p)
        w = _dense(rng, ws) if dense else _sparse(rng, ws, p)
        addend = (_dense(rng, xs).clamp(-1, 1) if dense else _sparse(rng, xs, 0.5)) if c.addend else None
        bsy = _sparse(rng, xs, 0.5) if c.rows else None
    else:
        x = _real_input(rng, xs, dtype, clamp=2.0 if c.affine else None)
        a = prologue(x, sc, sh, c.affine)
        if dtype == 'bf16':
            a = q(a, 'bf16')
        elif c.affine:
            e_a = 2 * U * prologue_abs(x, sc, sh)
        dz = q(_t(rng.normal(0.0, 1.0, ys)), dtype) * _t(rng.random(ys) < 0.6)      # zeros where a ReLU was off
        g = dz
        if use_coef:
            y = q(_t(rng.normal(0.0, 1.0, ys)), dtype)
            coef = q(torch.stack([_t(rng.uniform(0.5, 1.5, c.cout)), _t(rng.normal(0, 0.2, c.cout)), _t(rng.normal(0, 0.1, c.cout))]), 'f32')
            g = bc(coef[0]) * dz + bc(coef[1]) * y + bc(coef[2])
            e_g = 2 * U * ((bc(coef[0]) * dz).abs() + (bc(coef[1]) * y).abs() + bc(coef[2]).abs())
        w = q(_t(rng.normal(0.0, 1.0, ws)) / math.sqrt(c.ks * c.ks * c.cin), dtype)
        addend = q(_t(rng.normal(0.0, 1.0, xs)), dtype) if c.addend else None
        bsy = q(_t(rng.normal(0.0, 1.0, xs)), dtype) if c.rows else None
    dx, gw, rows = fused_formula(a, g, w, addend, c.mask, bsy)
    S_dx = dgrad(g.abs(), w.abs(), 1, (c.H, c.W)) + (0 if addend is None else addend.abs())
    S_gw = wgrad(a.abs(), g.abs(), c.ks, 1)
    gprior = _t(rng.integers(-3, 4, ws)) if lattice else q(_t(rng.normal(0.0, 1.0, ws)), 'f32')
    d = dict(x=x, sc=sc, sh=sh, a=a, dz=dz, y=y, coef=coef, g=g, w=w, addend=addend, bsy=bsy, dx=dx, gw=gw, rows=rows,
             prior=gprior, S_dx=S_dx, S_gw=S_gw + gprior.abs(), K=K, P=P)
    live = (a > 0) if c.mask else torch.ones_like(a, dtype=torch.bool)
    if c.rows:
        d['S_rows'] = torch.stack([(S_dx * live).sum((0, 2, 3)), (S_dx * live * bsy.abs()).sum((0, 2, 3))])
    if not lattice:
        cb = contraction_bound(K, S_dx)
        if e_g is not None:
            cb = cb + dgrad(e_g, w.abs(), 1, (c.H, c.W))
        cb = cb * live
        d['b_dx'] = stored_bound(dx, cb, dtype)
        d['b_gw'] = contraction_bound(P, S_gw)
        if e_a is not None:
            d['b_gw'] = d['b_gw'] + wgrad(e_a, g.abs(), c.ks, 1)
        if e_g is not None:
            d['b_gw'] = d['b_gw'] + wgrad(a.abs(), e_g, c.ks, 1)
        if c.rows:
            # the sums take the f32 value before the store's rounding: its error, plus a chain of P (+ 1 product) additions
            d['b_rows'] = torch.stack([cb.sum((0, 2, 3)) + (P + 3) * U * dx.abs().sum((0, 2, 3)),
                                       (cb * bsy.abs()).sum((0, 2, 3)) + (P + 3) * U * (dx * bsy).abs().sum((0, 2, 3))])
            # bwd_pw_kernel<64, 256> (the 256-channel input side) sums the tile it has just stored, read back from LDS in
            # the compute dtype: every term carries the store's rounding as well
            sb = d['b_dx']
            d['b_rows_stored'] = torch.stack([sb.sum((0, 2, 3)) + (P + 3) * U * dx.abs().sum((0, 2, 3)),
                                              (sb * bsy.abs()).sum((0, 2, 3)) + (P + 3) * U * (dx * bsy).abs().sum((0, 2, 3))])
    return d


# ---- mutations for the sensitivity tests (applied to a reference output) ----------------------------------------------
def lose_one_product(ref, a, w, stride=1):
    """ref of conv(a, w) with ONE product a[n, ci, iy, ix] * w[co, ci, r, s] missing: the largest one of some element.
    Returns (mutated, index of the element)"""
    ks = w.shape[-1]
    pad = ks // 2
    n, co = 0, 0
    best, at = 0.0, None
    for oy in range(ref.shape[2]):
        for ox in range(ref.shape[3]):
            for r in range(ks):
                for s in range(ks):
                    iy, ix = oy * stride + r - pad, ox * stride + s - pad
                    if 0 <= iy < a.shape[2] and 0 <= ix < a.shape[3]:
                        prod = (a[n, :, iy, ix] * w[co, :, r, s]).abs()
                        if float(prod.max()) > best:
                            best, at = float(prod.max()), (oy, ox, r, s, int(prod.argmax()), iy, ix)
    oy, ox, r, s, ci, iy, ix = at
    out = ref.clone()
    out[n, co, oy, ox] -= a[n, ci, iy, ix] * w[co, ci, r, s]
    return out, (n, co, oy, ox)
