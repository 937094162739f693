"""Float64 references of the resampling, layout and reduction glue kernels of csrc/eltwise.hip, the bounds they are
compared under and the inputs of tests/test_glue_kernels_gpu.py. Nothing here imports project code:
tests/test_glue_refs_cpu.py pins every reference to an independent statement of the same operation and checks the
lattice inputs on a machine without a GPU.

Bounds (none of them comes from what a kernel gives):

    sums (column sum, slab sum, linear combination)   |got - ref64| <= n * 2^-24 * sum |terms|   per output, n terms:
        every one of the n - 1 additions of ANY float32 summation order (and the rounding of a term or of the result)
        rounds a partial sum that is at most sum |terms|
    bilinear kernels, f32     max |got - ref64| <= max(2 * dev32, 2^-22 * max |ref64|), dev32 = the largest deviation of
        the same reference evaluated in float32 on the CPU from its float64 value, for that case
    bilinear kernels, bf16    the same + 2^-9 * max |ref64| for the rounding to storage
    and never looser than tests/test_kernels_gpu.py and tests/test_head_mix_gpu.py allow (the `cap` arguments).

Lattice inputs: integers small enough that every product and every partial sum of every summation order is a float32;
there the kernels must give the bits of the float64 reference.

The window emulation (bilin_src32 / bilin_window32 / window_report) restates, in float32, the arithmetic by which the
transposes decide which destination pixels a source pixel receives from; the kernels hold the x weights of one window
in MAXW registers per pass."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                       # unit roundoff of float32
MAXW = 20                            # x-window weights per pass (CATB_MAXW)
F32_VEC, BF16_VEC = 4, 8             # channels per 16-byte vector


def vec_of(dtype):
    return F32_VEC if dtype == torch.float32 else BF16_VEC


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def is_f32(a):
    """every element of the float64 array is a float32 value"""
    a = np.asarray(a, dtype=np.float64)
    return bool((a.astype(np.float32).astype(np.float64) == a).all())


# ---- the float32 window arithmetic of the transposes ---------------------------------------------------------------

def bilin_src32(d, in_size, out_size, align):
    """source taps (i0, i1) and the weight l1 of i1 for destinations d: float32 steps for align_corners = 0, an exact
    integer quotient with a float32 remainder / (out - 1) for align_corners = 1 (bilin_src of csrc/common.h)"""
    if align and out_size > 1:               # an exact integer quotient and remainder, l1 = rem / (out - 1)
        num = np.asarray(d, dtype=np.int64) * (in_size - 1)
        i0 = num // (out_size - 1)
        l1 = (num - i0 * (out_size - 1)).astype(np.float32) / np.float32(out_size - 1)
        return i0, i0 + (i0 < in_size - 1), l1
    d = np.asarray(d, dtype=np.float32)
    if align:
        src = np.zeros_like(d)
    else:
        scale = np.float32(in_size) / np.float32(out_size)
        src = np.maximum((d + np.float32(0.5)) * scale - np.float32(0.5), np.float32(0))
    assert src.dtype == np.float32
    i0 = np.minimum(src.astype(np.int32), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    return i0, i1, src - i0.astype(np.float32)


def weights32(in_size, out_size, align):
    """[out][in] float32: the weight with which destination d reads source s, as the transposes re-evaluate it"""
    d = np.arange(out_size)
    i0, i1, l1 = bilin_src32(d, in_size, out_size, align)
    m = np.zeros((out_size, in_size), np.float32)
    m[d, i0] += np.float32(1) - l1
    m[d, i1] += l1
    return m


def bilin_window32(s, in_size, out_size, align):
    """[d0, d1): the destinations that the transposes visit for source s"""
    s = np.asarray(s)
    sf = s.astype(np.float32)
    if align:
        inv = np.float32(out_size - 1) / np.float32(in_size - 1) if in_size > 1 else np.float32(0)
        lo, hi = (sf - np.float32(1)) * inv, (sf + np.float32(1)) * inv
    else:
        f = np.float32(out_size) / np.float32(in_size)
        lo = (sf - np.float32(0.5)) * f - np.float32(0.5)
        hi = (sf + np.float32(1.5)) * f - np.float32(0.5)
    d0 = np.floor(lo).astype(np.int64) - 1
    d1 = np.ceil(hi).astype(np.int64) + 2
    d0 = np.where((d0 < 0) | (s == 0), 0, d0)
    d1 = np.where((d1 > out_size) | (s == in_size - 1), out_size, d1)
    return d0, d1


def window_report(in_size, out_size, align):
    """(missed, beyond): the (s, d, weight) with non-zero weight outside the window of s, and those MAXW or more
    columns from its start"""
    m = weights32(in_size, out_size, align)
    d0, d1 = bilin_window32(np.arange(in_size), in_size, out_size, align)
    missed, beyond = [], []
    for s in range(in_size):
        for d in np.flatnonzero(m[:, s]):
            if d < d0[s] or d >= d1[s]:
                missed.append((s, int(d), float(m[d, s])))
            elif d - d0[s] >= MAXW:
                beyond.append((s, int(d), float(m[d, s])))
    return missed, beyond


def gate_admits(in_size, out_size):
    """the host gate of the streamed upsample transpose, for one axis pair (ws -> W)"""
    return in_size <= out_size and in_size <= 256 and 2 * ((out_size + in_size - 1) // in_size) + 4 <= MAXW


# (ws, W) with align_corners = 1 that the gate admits and whose window carries weight beyond its first MAXW columns;
# tests/test_glue_refs_cpu.py derives this list from window_report over every in <= 39, out <= 129
BEYOND_ALIGN_SHAPES = [(3, 22), (3, 23), (3, 24), (4, 30), (4, 31), (4, 32), (5, 39), (5, 40), (6, 48)]
NEIGHBOUR_ALIGN_SHAPES = [(3, 21), (4, 29), (8, 64)]
PLAIN_SHAPES = [(3, 24), (4, 31), (9, 24)]


# ---- bilinear upsample + concat and the transposes -------------------------------------------------------------------

def interp_matrix(in_size, out_size, align, dtype=torch.float64):
    """[out][in]: bilinear interpolation along one axis as torch states it (upsample_bilinear2d), in `dtype`"""
    d = torch.arange(out_size, dtype=dtype)
    if align:
        src = d * (torch.tensor(in_size - 1, dtype=dtype) / torch.tensor(max(out_size - 1, 1), dtype=dtype))
    else:
        src = ((d + 0.5) * (torch.tensor(in_size, dtype=dtype) / torch.tensor(out_size, dtype=dtype)) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(in_size - 1)
    i1 = (i0 + 1).clamp_max(in_size - 1)
    l1 = src - i0.to(dtype)
    m = torch.zeros(out_size, in_size, dtype=dtype)
    rows = torch.arange(out_size)
    m[rows, i0] += 1 - l1
    m[rows, i1] += l1
    return m


def upsample(x, H, W, align):
    """NCHW -> NCHW at H x W, in x.dtype; a map already at H x W is copied"""
    if tuple(x.shape[2:]) == (H, W):
        return x.clone()
    my, mx = interp_matrix(x.shape[2], H, align, x.dtype), interp_matrix(x.shape[3], W, align, x.dtype)
    return torch.einsum('Yy,ncyx,Xx->ncYX', my, x, mx)


def bilinear_cat(xs, H, W, align):
    return torch.cat([upsample(x, H, W, align) for x in xs], 1)


def upsample_t(g, hs, ws, align):
    """transpose of the upsampling hs x ws -> g.shape[2:], applied to g (NCHW): autograd of F.interpolate in g.dtype"""
    if tuple(g.shape[2:]) == (hs, ws):
        return g.clone()
    x = torch.zeros(g.shape[0], g.shape[1], hs, ws, dtype=g.dtype, requires_grad=True)
    F.interpolate(x, size=tuple(g.shape[2:]), mode='bilinear', align_corners=bool(align)).backward(g)
    return x.grad


def bilinear_cat_t(gcat, branches, align):
    """gcat NCHW over the concatenated channels; branches [(c, h, w)] -> the gradient of every branch"""
    out, off = [], 0
    for c, h, w in branches:
        out.append(upsample_t(gcat[:, off:off + c].contiguous(), h, w, align))
        off += c
    return out


# ---- im2col, layouts, sums -----------------------------------------------------------------------------------------

def im2col_stem(img, kpad):
    """img [N][C][H][W] -> cols [N][Ho][Wo][kpad] of the 3x3 / stride 2 / pad 1 stem, column tap * C + c, zero beyond"""
    img = np.asarray(img)
    n, c, h, w = img.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    pad = np.zeros((n, c, 2 * ho + 1, 2 * wo + 1), img.dtype)
    pad[:, :, 1:h + 1, 1:w + 1] = img
    cols = np.zeros((n, ho, wo, kpad), img.dtype)
    for tap in range(9):
        r, s = divmod(tap, 3)
        cols[..., tap * c:(tap + 1) * c] = pad[:, :, r:r + 2 * ho:2, s:s + 2 * wo:2].transpose(0, 2, 3, 1)
    return cols


def nchw_to_nhwc(x, cp):
    x = np.asarray(x)
    n, c, h, w = x.shape
    out = np.zeros((n, h, w, cp), x.dtype)
    out[..., :c] = x.transpose(0, 2, 3, 1)
    return out


def nhwc_to_nchw(x, c):
    return np.ascontiguousarray(np.asarray(x)[..., :c].transpose(0, 3, 1, 2))


def column_sum(dy, c):
    """dy [pixels][Cp] -> (sum, sum |.|) over the pixels of the first c columns, float64"""
    dy = np.asarray(dy, dtype=np.float64)
    return dy[:, :c].sum(0), np.abs(dy[:, :c]).sum(0)


def slab_sum(slabs, cout_real, cin_real, ks, kflat):
    """slabs [ns][Cout][taps][Cin] (kflat 0) or [ns][Cout][Cin] holding column tap * cin_real + ci (kflat 1)
    -> (sum, sum |.|) in OIHW order [cout_real][cin_real][ks][ks], float64"""
    s = np.asarray(slabs, dtype=np.float64)
    taps = ks * ks
    if kflat:
        real = s[:, :cout_real, :taps * cin_real].reshape(s.shape[0], cout_real, taps, cin_real)
    else:
        real = s[:, :cout_real, :, :cin_real]
    real = real.transpose(0, 1, 3, 2).reshape(s.shape[0], cout_real, cin_real, ks, ks)
    return real.sum(0), np.abs(real).sum(0)


def lincomb(srcs, coefs):
    """(sum_j coef_j * src_j, sum_j |coef_j * src_j|), float64"""
    terms = [np.float64(c) * np.asarray(s, dtype=np.float64) for s, c in zip(srcs, coefs)]
    return sum(terms), sum(np.abs(t) for t in terms)


# ---- bounds -----------------------------------------------------------------------------------------------------------

def sum_bound(n_terms, abs_sum):
    return n_terms * U * np.asarray(abs_sum, dtype=np.float64)


def check_sum(name, got, ref64, abs_sum, n_terms):
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    bound = sum_bound(n_terms, abs_sum)
    err = np.abs(got - ref64)
    k = int(np.argmax(err - bound)) if err.size else 0
    print('{:66s} abs err {:.3e} bound {:.3e}'.format(name, float(err.flat[k]), float(bound.flat[k])))
    assert np.isfinite(got).all() and (err <= bound).all(), (name, float(err.flat[k]), float(bound.flat[k]))


def bilinear_bound(ref64, ref32, bf16, cap_rel):
    """(allowed absolute error, dev32, the float32 part of the bound); cap_rel * max |ref64| is what the older test of
    the same kernel allows"""
    r64 = np.asarray(ref64, dtype=np.float64)
    m = float(np.abs(r64).max())
    dev32 = float(np.abs(np.asarray(ref32, dtype=np.float64) - r64).max())
    b32 = max(2 * dev32, 2.0 ** -22 * m)
    bound = b32 + (2.0 ** -9 * m if bf16 else 0.0)
    return min(bound, cap_rel * m), dev32, b32


def rounding_allowance(ref64, b32):
    """per element: what a float32 result within b32 of ref64 can be off by after a correct rounding to bf16. A value
    v in [2^k, 2^(k+1)) rounds to 8 significant bits with an error of at most 2^(k-8) <= 2^-8 |v|"""
    return b32 + 2.0 ** -8 * (np.abs(np.asarray(ref64, dtype=np.float64)) + b32)


def check_bilinear(name, got, ref64, ref32, bf16, cap_rel):
    """-> (name, err, bound, within the bound, within a correct rounding): printed here, asserted by assert_all once
    all cases of a test have been printed. The last verdict is the bound itself for f32; for bf16 it holds every
    element to rounding_allowance, which a correctly rounding kernel meets wherever max |ref64| lies in its binade"""
    got, r64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    bound, dev32, b32 = bilinear_bound(r64, ref32, bf16, cap_rel)
    finite = bool(np.isfinite(got).all())
    err = float(np.abs(got - r64).max()) if finite else float('inf')
    ok = finite and err <= bound
    rounded = ok if not bf16 else finite and bool((np.abs(got - r64) <= rounding_allowance(r64, b32)).all())
    print('{:66s} abs err {:.3e} bound {:.3e} (dev32 {:.2e}, max |ref| {:.3f}){}'.format(
        name, err, bound, dev32, float(np.abs(r64).max()), '' if ok else '  BEYOND' + ('' if rounded else ' ROUNDING')))
    return name, err, bound, ok, rounded


def assert_all(results):
    """first what no correct kernel can miss, then the bound as stated"""
    bad = [(n, e, b) for n, e, b, _, rounded in results if not rounded]
    assert not bad, '{} of {} cases beyond a correct rounding: {}'.format(len(bad), len(results), bad[:12])
    bad = [(n, e, b) for n, e, b, ok, _ in results if not ok]
    assert not bad, '{} of {} cases beyond their bound: {}'.format(len(bad), len(results), bad[:12])


# ---- inputs -----------------------------------------------------------------------------------------------------------

def rng(*key):
    return np.random.RandomState(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def real(shape, *key):
    return rng(*key).standard_normal(shape).astype(np.float32)


def ints(shape, bound, *key):
    return rng(*key).randint(-bound, bound + 1, size=shape).astype(np.float32)


def as_stored(a, dtype):
    """the float32 array rounded to what the device tensor of `dtype` holds"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()


# ---- bf16 inputs whose largest result is a power of two -----------------------------------------------------------------
# The bf16 bound adds 2^-9 * max |ref| for the rounding to storage. A result v in [2^k, 2^(k+1)) rounds with an error of
# up to 2^(k-8), so that term covers a correct rounding exactly when no result lies strictly inside the binade of
# max |ref|, that is when max |ref| is a power of two P and the results that reach it are exact. The bf16 cases plant
# that: the corner destination (0, 0) reads (forward) or feeds (transpose) the corner source alone, with weight 1, in
# both align_corners modes, so a value P put there arrives unchanged. Everything else of the input stays random.

def pow2_at_least(x):
    return 2.0 ** math.ceil(math.log2(float(x)))


def corner_footprint(in_size, out_size, align):
    """number of leading destinations that read source 0"""
    return int(torch.nonzero(interp_matrix(in_size, out_size, align)[:, 0]).max()) + 1


def plant_forward(xs):
    """NCHW inputs of the concat: element (0, 0, 0, 0) of every branch becomes P >= every |input|; interpolation is a
    convex combination, so max |cat| = P, reached at the corner pixels"""
    xs = [np.array(x, dtype=np.float32) for x in xs]
    P = pow2_at_least(max(float(np.abs(x).max()) for x in xs))
    for x in xs:
        x[0, 0, 0, 0] = P
    return xs


def plant_upsample_t(G, sizes, align):
    """G NCHW: in plane (0, 0) the destinations that feed the corner source of any output size become zero, then the
    corner destination becomes P >= every |result| of every size: each output holds P at (0, 0, 0, 0) exactly"""
    G = np.array(G, dtype=np.float32)
    H, W = G.shape[2:]
    fy = max(corner_footprint(hs, H, align) for hs, _ in sizes)
    fx = max(corner_footprint(ws, W, align) for _, ws in sizes)
    G[0, 0, :fy, :fx] = 0
    g64 = torch.from_numpy(G).double()
    G[0, 0, 0, 0] = pow2_at_least(max(float(upsample_t(g64, hs, ws, align).abs().max()) for hs, ws in sizes))
    return G


def plant_cat_t(gcat, branches, inits, align):
    """the same for every branch of the concat transpose, in the first channel plane of its slice; the destinations
    inits (accumulate = 1) hold 0 at their corner, and P covers the results with and without them"""
    gcat, inits = np.array(gcat, dtype=np.float32), [np.array(i, dtype=np.float32) for i in inits]
    H, W = gcat.shape[2:]
    off = 0
    for k, (c, h, w) in enumerate(branches):
        gcat[0, off, :corner_footprint(h, H, align), :corner_footprint(w, W, align)] = 0
        inits[k][0, 0, 0, 0] = 0
        off += c
    grads = bilinear_cat_t(torch.from_numpy(gcat).double(), branches, align)
    off = 0
    for k, (c, h, w) in enumerate(branches):
        g = grads[k].numpy()
        gcat[0, off, 0, 0] = pow2_at_least(max(np.abs(g).max(), np.abs(g + inits[k]).max()))
        off += c
    return gcat, inits


# bilinear concat: (N, H, W, [(channel vectors, h, w)]); channels = vectors * (4 for f32, 8 for bf16), so the branch
# offsets are no multiples of 32
CAT_CASES = [
    (1, 5, 7, [(1, 5, 7)]),                                        # a lone identity branch
    (3, 13, 24, [(1, 13, 24), (2, 5, 9)]),                         # 5 -> 13 and 9 -> 24, non-square, N = 3
    (1, 16, 32, [(1, 16, 32), (1, 1, 1), (3, 8, 16)]),             # a 1 x 1 branch
    (1, 32, 40, [(1, 32, 40), (1, 2, 2), (1, 16, 20), (2, 4, 5)]),   # factor 16 and 2 -> 40: several window passes
    (3, 32, 32, [(1, 2, 2), (1, 32, 32)]),                         # factor 16 first, the identity second
]
LATTICE_FACTORS = (2, 4, 8, 16)
LATTICE_BOUND = 64


def lattice_cat_case(f):
    """align = 0, integer factor f: (N, H, W, branches [(c, h, w)], xs, gcat, inits), all integers of |x| <= 64.
    Every weight is a multiple of 1 / (2 f), so every product of two weights and an input is a multiple of
    1 / (4 f^2) below 2^6: with f <= 16 every partial sum of a footprint (weights summing to f^2) stays below
    2^24 / (4 f^2) and is exact in float32"""
    n, hs, ws, c = 2, 3, 2, 4
    H, W = hs * f, ws * f
    branches = [(c, H, W), (c, hs, ws)]
    xs = [ints((n, cc, h, w), LATTICE_BOUND, f, k) for k, (cc, h, w) in enumerate(branches)]
    gcat = ints((n, 2 * c, H, W), LATTICE_BOUND, f, 7)
    inits = [ints((n, cc, h, w), LATTICE_BOUND, f, 10 + k) for k, (cc, h, w) in enumerate(branches)]
    return n, H, W, branches, xs, gcat, inits


# layout conversions
LAYOUT_HW = [(1, 1), (1, 31), (4, 8), (3, 11), (5, 13)]              # H * W of 1, 31, 32, 33, 65
LAYOUT_CH = [(8, 5), (40, 33), (96, 96), (32, 1)]                    # (Cp, C)
LAYOUT_N = (1, 3)


def bf16_specials():
    """float32 values whose rounding to bf16 is decided by the rule: exact ties both ways (to the even neighbour below
    and above), just off a tie, the largest finite float32 (rounds to inf), +-inf, float32 and bf16 denormals, a NaN"""
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # ties: 1.00390625 -> 1.0, 1.01171875 -> 1.015625
            0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,      # one ulp off the ties
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F800000, 0xFF800000,
            0x00000001, 0x00008000, 0x00018000, 0x00018001, 0x80008001, 0x007FFFFF, 0x00800000,
            0x00000000, 0x80000000, 0x7FC00000]
    return np.array(bits, dtype=np.uint32).view(np.float32)


def with_specials(a):
    """the float32 array with bf16_specials() planted from its first element on (as many as fit)"""
    a = np.array(a, dtype=np.float32)
    sp = bf16_specials()
    k = min(a.size, sp.size)
    a.reshape(-1)[:k] = sp[:k]
    return a


def bf16_bits(a):
    """int16 bits of torch's round-to-nearest-even conversion of the float32 array"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy()


def same_bf16(got_bits, x):
    """got_bits (int16) are the bf16 bits of the float32 array x under round-to-nearest-even; a NaN has to stay a NaN"""
    want = bf16_bits(x)
    nan = np.isnan(np.asarray(x, dtype=np.float32))
    got_bits = np.asarray(got_bits).reshape(want.shape)
    got_nan = (got_bits.astype(np.int32) & 0x7FFF) > 0x7F80
    return bool((got_bits[~nan] == want[~nan]).all() and got_nan[nan].all())


# stem im2col: (C, Kpad); the first is the pixel kernel, the others the generic one
IM2COL_CK = [(3, 32), (3, 64), (1, 16), (4, 40)]
IM2COL_HW = [(1, 1), (1, 2), (2, 5), (5, 8), (8, 33), (33, 1), (33, 33)]
IM2COL_N = (1, 3)

# bias gradient
BIAS_PIXELS = (1, 63, 64, 130, 4097)
BIAS_CP = {torch.float32: (32, 48, 1024), torch.bfloat16: (32, 24, 2048)}
BIAS_REFUSED_CP = {torch.float32: 257 * 4, torch.bfloat16: 257 * 8}
BIAS_INT = 8


def bias_case(pixels, cp, lattice, dtype):
    """(dy [pixels][Cp] as stored, old [Cp])"""
    if lattice:
        return ints((pixels, cp), BIAS_INT, pixels, cp), ints((cp,), BIAS_INT, pixels, cp, 1)
    return as_stored(real((pixels, cp), pixels, cp, 2), dtype), real((cp,), pixels, cp, 3)


# weight-gradient slab sum: (Cout, Cin, ks, Cout_real, Cin_real, kflat)
WRED_NSPLIT = (1, 3, 4, 5, 15, 16, 17, 112, 113, 127, 128, 129, 241)
WRED_FORMS = [(16, 16, 1, 5, 4, 0), (16, 16, 3, 5, 4, 0),        # vector form
              (16, 32, 3, 5, 3, 1), (16, 8, 3, 5, 3, 0)]         # scalar form, both slab layouts
WRED_INT = 8


def wred_case(nsplit, form, lattice):
    """(slabs with NaN in every pad position, old gradient OIHW)"""
    cout, cin, ks, co, ci, kflat = form
    taps = ks * ks
    gen = (lambda shape, *k: ints(shape, WRED_INT, *k)) if lattice else real
    val = gen((nsplit, co, taps, ci), nsplit, cin, ks, kflat)
    if kflat:
        slabs = np.full((nsplit, cout, cin), np.nan, np.float32)
        slabs[:, :co, :taps * ci] = val.reshape(nsplit, co, taps * ci)
    else:
        slabs = np.full((nsplit, cout, taps, cin), np.nan, np.float32)
        slabs[:, :co, :, :ci] = val
    return slabs, gen((co, ci, ks, ks), nsplit, cin, ks, kflat, 1)


# linear combination
GRID_CAP = 256 * 16 * 256                                         # elements of one pass of a capped element-wise grid
LINCOMB_N = (1, 255, 257, GRID_CAP + 1)
LINCOMB_INT, LINCOMB_COEF_INT = 64, 4


def lincomb_case(n, k, lattice):
    if lattice:
        return [ints((n,), LINCOMB_INT, n, k, j) for j in range(k)], ints((k,), LINCOMB_COEF_INT, n, k, 99)
    return [real((n,), n, k, j) for j in range(k)], real((k,), n, k, 99)


# fill: byte counts; the last two pass the grid cap of 16-byte stores and the low 32 bits of the length
FILL_BYTES = (0, 1, 15, 16, 17, 4096 + 7, 256 * 16 * 256 * 16 + 16 * 3 + 5, 2 ** 32 + 48 + 5)

