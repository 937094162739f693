"""Float64 references of the fuse-sum and BatchNorm-backward passes of csrc/eltwise.hip (sum_terms, grad_term,
bn_bwd_reduce, pool_reduce, bn_bwd_finalize), the bounds they are compared under and the inputs of
tests/test_fuse_kernels_gpu.py. Nothing here imports project code; tests/test_fuse_refs_cpu.py pins every reference to
an independent statement of the same operation (torch float64 interpolate / batch_norm / autograd) and checks the
properties the inputs claim. All tensors are NHWC numpy arrays.

Bounds (none of them comes from what a kernel gives), u = 2^-24:

    lattice cases       inputs are multiples of 1/16 in [-4, 4], scales and coefficients in +-{0.5, 1, 1.5, 2}: every
        fmaf, product and partial sum of any order is an exact float32, so the device must give the bits of the float64
        reference (rounded to nearest even where the output is stored as bf16). `lattice_exact` is the property.
    element-wise outputs (sum_terms out, grad_term dst / dst2, stored dz)
        |got - ref64| <= (n + 1) * u * sum |terms| per element; n counts the additions the element passes through (terms
        of the sum, the f * f pooled pixels, the old value of an accumulating store; the two addends of grad_term's
        coefficients), the terms taken after their affine: an affine is one fmaf, one rounding of at most u |term|, and
        every addition of any order rounds a partial result of at most sum |terms|.
        bf16 outputs: a correct rounding of an f32 value inside that bound (glue_refs.rounding_allowance).
        An element whose float64 inner-ReLU pre-activation lies within 4 u (|scale y| + |shift|) of 0 may fall either
        way and is left out (`near`); at most SKIP_CAP of a case's elements.
    sums_mode terms     scale / shift from batch sums: float64 restatement of hr_bn_from_sums; the device forms it in
        f32 with sqrtf and a division, so each is allowed 4 * e_ref + 2 u relative, e_ref = the largest relative
        deviation over the channels of the same restatement run in float32 on the CPU. The sums have
        var >= mean^2 / 4 (no cancellation in e_ref) or a variance that both precisions clamp to exactly 0.
    partial rows        per channel 2 * D * u * sum |t| (tests/bn_bounds.py), the host adding the rows in float64. D is
        the longest chain of f32 additions a term passes through: bn_bwd_reduce_block gives a thread
        ceil(npix / (blocks * rows)) pixels of f * f additions each and adds `rows` threads in LDS; pool_reduce_block
        is the same with f * f = 4 at level 1 and four more additions per level above. The data are of one sign per
        channel with magnitudes in [1, 1.25]: one pixel's share of a sum is far above the bound (`share_ok`).
    bn_bwd_finalize     works in double from the rows it is given: 2 u relative (the f32 rounding of the float64
        formula; with accumulate the rounding of the term and of the sum: 2 u (|old| + |term|))."""
import math

import numpy as np

import glue_refs as G

U = G.U
SKIP_CAP = 1e-3
COPIES = 8                           # HR_BN_COPIES
SUM_MAXC = 384
EW_GRID_CAP = 4096                   # blocks of a capped element-wise grid, 256 threads each
ROWS_KERNEL_VECTORS = 4 * 4096 * 256   # grad_term takes grad_term_rows_kernel from this many 16-byte vectors on
VEC = {'f32': 4, 'bf16': 8}


def np_dtype_round(a, dt):
    """float32 values rounded to the storage type of `dt` ('f32' | 'bf16'), as float32"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if dt == 'f32' else torch.from_numpy(a).to(torch.bfloat16).float().numpy()


# ---- resampling ------------------------------------------------------------------------------------------------------

def up(x, sh):
    """nearest up-sampling by 2^sh of an NHWC array"""
    f = 1 << sh
    return x if f == 1 else x.repeat(f, axis=1).repeat(f, axis=2)


def pool(x, sh):
    """sum over the 2^sh x 2^sh blocks of an NHWC array"""
    f = 1 << sh
    N, H, W, C = x.shape
    return x.reshape(N, H // f, f, W // f, f, C).sum(axis=(2, 4))


# ---- references ------------------------------------------------------------------------------------------------------

def sum_terms(terms, relu_out):
    """terms: dicts src (NHWC, at the output size >> sh), sh, scale, shift ([C] or None), relu
    -> (ref64, sum |terms| after their affine, n additions)"""
    ref, tot = 0.0, 0.0
    for t in terms:
        v = up(np.asarray(t['src'], dtype=np.float64), t['sh'])
        if t.get('scale') is not None:
            v = v * np.asarray(t['scale'], dtype=np.float64) + np.asarray(t['shift'], dtype=np.float64)
            a = np.abs(up(np.asarray(t['src'], dtype=np.float64), t['sh']) * t['scale']) + np.abs(t['shift'])
        else:
            a = np.abs(v)
        if t.get('relu'):
            v = np.maximum(v, 0.0)
        ref, tot = ref + v, tot + a
    if relu_out:
        ref = np.maximum(ref, 0.0)
    return ref, tot, len(terms)


def bn_from_sums(sums, inv_count, eps, gamma, beta, dt=np.float64):
    """hr_bn_from_sums restated in precision dt: sums [COPIES][2][C] -> (scale, shift, mean, clamped variance)"""
    s = np.asarray(sums).astype(dt)
    s1, s2 = np.zeros(s.shape[2], dt), np.zeros(s.shape[2], dt)
    for k in range(COPIES):
        s1, s2 = s1 + s[k, 0], s2 + s[k, 1]
    m = s1 * dt(inv_count)
    v = s2 * dt(inv_count) - m * m
    v = np.where(v < 0, dt(0), v)
    scale = np.asarray(gamma).astype(dt) / np.sqrt(v + dt(eps))
    shift = np.asarray(beta).astype(dt) - m * scale
    assert scale.dtype == dt and shift.dtype == dt
    return scale, shift, m, v


def sums_allowance(sums, inv_count, eps, gamma, beta):
    """-> (scale64, shift64, allowed |d scale| [C], allowed |d shift| [C], e_ref of scale, e_ref of shift)"""
    sc, sf, _, _ = bn_from_sums(sums, inv_count, eps, gamma, beta)
    sc32, sf32, _, _ = bn_from_sums(sums, inv_count, eps, gamma, beta, np.float32)
    e_sc = float(np.max(np.abs(sc32.astype(np.float64) - sc) / np.abs(sc)))
    e_sf = float(np.max(np.abs(sf32.astype(np.float64) - sf) / np.abs(sf)))
    return sc, sf, (4 * e_sc + 2 * U) * np.abs(sc), (4 * e_sf + 2 * U) * np.abs(sf), e_sc, e_sf


def dz(g, mask, y, scale, shift, sh, inner_relu):
    """the pooled, masked gradient of compute_dz: g, mask at (H << sh, W << sh), y at (H, W)
    -> (dz64, sum |terms|, near: elements whose inner-ReLU decision lies within rounding of 0, or None)"""
    g = np.asarray(g, dtype=np.float64)
    if mask is not None:
        g = np.where(np.asarray(mask, dtype=np.float64) > 0, g, 0.0)
    d, a, near = pool(g, sh), pool(np.abs(g), sh), None
    if inner_relu:
        y = np.asarray(y, dtype=np.float64)
        if scale is not None:
            z = y * np.asarray(scale, dtype=np.float64) + np.asarray(shift, dtype=np.float64)
            near = np.abs(z) <= 4 * U * (np.abs(y * scale) + np.abs(shift))
            near &= z != 0                           # (an exact 0 is decided: > 0 fails)
        else:
            z = y
        d, a = np.where(z > 0, d, 0.0), np.where(z > 0, a, 0.0)
    return d, a, near


def grad_term(d, a, y, coef, old):
    """dst = A * dz + B * y + Cc (+ old) of grad_term_block: d, a from dz(); coef [3][C] or None; old or None
    -> (ref64, sum |terms|)"""
    if coef is not None:
        c = np.asarray(coef, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        d, a = c[0] * d + c[1] * y + c[2], np.abs(c[0]) * a + np.abs(c[1] * y) + np.abs(c[2])
    if old is not None:
        d, a = d + np.asarray(old, dtype=np.float64), a + np.abs(old)
    return d, a


def grad_adds(sh, coef, acc):
    return (1 << sh) ** 2 + (2 if coef else 0) + (1 if acc else 0)


def row_sums(d, y):
    """(sum dz, sum dz * y) per channel and the sums of the absolute values: [2][C] each"""
    d, y = np.asarray(d, dtype=np.float64), np.asarray(y, dtype=np.float64)
    C = d.shape[-1]
    t = np.stack([d.reshape(-1, C), (d * y).reshape(-1, C)])
    return t.sum(axis=1), np.abs(t).sum(axis=1)


def finalize(rows, count, gamma, mean, invstd):
    """bn_bwd_finalize_block in float64: rows [blocks][2][C] -> (dgamma, dbeta, coef [3][C])"""
    s = np.asarray(rows, dtype=np.float64).sum(axis=0)
    g, mu, r = (np.asarray(v, dtype=np.float64) for v in (gamma, mean, invstd))
    dg = r * (s[1] - mu * s[0])
    db = s[0]
    A = g * r
    B = -g * r * r * dg / count
    Cc = -g * r * db / count + g * r * r * mu * dg / count
    return dg, db, np.stack([A, B, Cc])


# ---- launch geometry and the chain length D ---------------------------------------------------------------------------

def ew_blocks(vectors):
    return int(min(max((vectors + 255) // 256, 1), EW_GRID_CAP))


def reduce_blocks(npix):
    return int(min(max(npix // 64, 1), 2048))


def reduce_geometry(npix, C, vec):
    """(blocks, rows) of bn_bwd_reduce_block"""
    return reduce_blocks(npix), 256 // (C // vec)


def reduce_D(npix, C, vec, sh):
    blocks, rows = reduce_geometry(npix, C, vec)
    return -(-npix // (blocks * rows)) * (1 << sh) ** 2 + rows


def pool_geometry(n1, C, vec, nlev):
    """(blocks, rows) of pool_reduce_block over n1 level-1 blocks"""
    group = {1: 1, 2: 4, 3: 16}[nlev]
    return reduce_blocks(n1), 256 // (C // vec) // group * group


def pool_D(n1, C, vec, nlev, level):
    blocks, rows = pool_geometry(n1, C, vec, nlev)
    return -(-n1 // (blocks * rows)) * 4 + 4 * (level - 1) + rows


def longest_walk(npix, blocks, rows):
    """direct count: the most pixels one thread of the (blocks x rows) walk of the reduction kernels visits"""
    return max(len(range(b * rows + r, npix, blocks * rows)) for b in range(blocks) for r in range(rows))


def rows_bound(D, abs_sums):
    return 2.0 * D * U * np.asarray(abs_sums, dtype=np.float64)


def share_ok(D, abs_sums, smallest_share):
    """the bound is at most half of the smallest single pixel's share of each sum"""
    return bool((rows_bound(D, abs_sums) <= 0.5 * np.asarray(smallest_share)).all())


# ---- checks ----------------------------------------------------------------------------------------------------------

RATIOS = {}                          # test name -> worst error / bound seen (printed by report())


def _note(key, ratio):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(ratio))


def report(key):
    print('{}: worst error / bound {:.3f}'.format(key, RATIOS.get(key, 0.0)))


def check_elem(key, name, got, ref64, abs_sum, n, bf16, skip=None, extra=0.0):
    """per element |got - ref64| <= (n + 1) u sum |terms| (+ extra: the sums_mode allowance), bf16: a correct
    rounding of such a value"""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    b32 = (n + 1) * U * np.asarray(abs_sum, dtype=np.float64) + extra
    allow = G.rounding_allowance(ref64, b32) if bf16 else b32
    err = np.abs(got - ref64)
    if skip is not None:
        assert skip.mean() <= SKIP_CAP, (name, float(skip.mean()))
        err = np.where(skip, 0.0, err)
    assert np.isfinite(got).all(), name
    ratio = float(np.max(np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), np.where(err > 0, np.inf, 0.0))))
    k = int(np.argmax(err - allow))
    print('{:72s} abs err {:.3e} bound {:.3e} ratio {:.3f}'.format(name, float(err.flat[k]), float(allow.flat[k]), ratio))
    _note(key, ratio)
    assert ratio <= 1.0, (name, float(err.flat[k]), float(allow.flat[k]))


def check_rows(key, name, rows, ref, abs_sums, D):
    """rows [blocks][2][C] added in float64 against ref [2][C] under 2 D u sum |t|"""
    got = np.asarray(rows, dtype=np.float64).sum(axis=0)
    bound = rows_bound(D, abs_sums)
    err = np.abs(got - ref)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    k = int(np.argmax(err - bound))
    print('{:72s} abs err {:.3e} bound {:.3e} ratio {:.3f} (D {})'.format(name, float(err.flat[k]), float(bound.flat[k]),
                                                                         ratio, D))
    _note(key, ratio)
    assert np.isfinite(got).all() and ratio <= 1.0, (name, float(err.flat[k]), float(bound.flat[k]))


def check_rel(key, name, got, ref64, scale_abs, rel):
    """|got - ref64| <= rel * scale_abs per element"""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    bound = rel * np.asarray(scale_abs, dtype=np.float64)
    err = np.abs(got - ref64)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print('{:72s} worst err / bound {:.3f}'.format(name, ratio))
    _note(key, ratio)
    assert np.isfinite(got).all() and ratio <= 1.0, (name, ratio)


def stored_bits(ref64, dt):
    """the float64 lattice result as the device stores it: exact in float32, rounded to nearest even into bf16"""
    r32 = np.asarray(ref64, dtype=np.float64).astype(np.float32)
    assert (r32.astype(np.float64) == ref64).all()
    return np_dtype_round(r32, dt)


# ---- inputs ----------------------------------------------------------------------------------------------------------

LATTICE_STEP = 16.0
LATTICE_MAX = 4.0
SCALES = (0.5, 1.0, 1.5, 2.0)
DENORMAL = 2.0 ** -130               # a positive denormal of float32 and of bf16
MASK_VALUES = (0.0, -0.0, -1.0, -0.25, 1.0, 0.5, DENORMAL)


def lattice(shape, *key):
    return G.ints(shape, int(LATTICE_MAX * LATTICE_STEP), *key) / np.float32(LATTICE_STEP)


def lattice_scale(C, *key, signed=False):
    r = G.rng(*key)
    s = np.asarray(SCALES, np.float32)[r.randint(0, len(SCALES), size=C)]
    return s * (r.choice(np.asarray([-1.0, 1.0], np.float32), size=C) if signed else np.float32(1))


def lattice_coef(C, *key):
    return np.stack([lattice_scale(C, *key, 1, signed=True), lattice_scale(C, *key, 2, signed=True),
                     lattice((C,), *key, 3)])


def mask_tensor(shape, *key):
    """+0.0, -0.0, negative and positive values and a positive denormal, each a seventh of the elements"""
    v = np.asarray(MASK_VALUES, np.float32)
    assert v[6] > 0 and np.signbit(v[1]) and not np.signbit(v[0])
    return v[G.rng(*key).randint(0, len(v), size=shape)]


def relu_lattice(shape, *key):
    """(y, scale, shift) on the lattice with scale * y + shift == 0 on an eighth of the elements, chosen at random"""
    C = shape[-1]
    y, scale = lattice(shape, *key, 1), lattice_scale(C, *key, 2)
    y0 = G.ints((C,), 16, *key, 3) / np.float32(8)       # multiples of 1/8 up to 2: scale * y0 is on the lattice
    shift = -scale * y0
    hit = G.rng(*key, 4).randint(0, 8, size=shape) == 0
    y = np.where(hit, np.broadcast_to(y0, shape), y).astype(np.float32)
    return y, scale, shift.astype(np.float32)


FINEST = 2.0 ** -9                   # (1/2 of a scale) * (1/16 of dz) * (1/16 of y): the finest step of any product


def on_lattice(*arrays):
    """every array holds multiples of 1/16 of at most 4 in magnitude: 7 bits, values of bf16 as well"""
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        if not ((a * LATTICE_STEP == np.round(a * LATTICE_STEP)).all() and (np.abs(a) <= LATTICE_MAX).all()):
            return False
    return True


def on_scales(*arrays):
    return all(bool(np.isin(np.abs(np.asarray(a, dtype=np.float64)), SCALES).all()) for a in arrays)


def lattice_exact(abs_sum, step=FINEST):
    """every term of a result is a multiple of `step` (FINEST for products with a scale, 2^-8 for dz * y), so every
    partial sum of any order is one too and is at most sum |terms| in magnitude: below 2^24 steps it is a float32"""
    return float(np.max(abs_sum)) / step < 2.0 ** 24


def real(shape, dt, *key):
    return np_dtype_round(G.real(shape, *key), dt)


def one_sign(shape, dt, *key):
    """magnitudes in [1, 1.25], one sign per channel"""
    r = G.rng(*key)
    sign = r.choice(np.asarray([-1.0, 1.0], np.float32), size=shape[-1])
    v = np_dtype_round((1.0 + 0.25 * r.random_sample(shape)).astype(np.float32) * sign, dt)
    assert (np.abs(v) >= 1).all() and (np.abs(v) <= 1.25).all()
    return v


SPLIT = 1.125 + 2.0 ** -9            # between two bf16 values of [1, 1.25], 2^-9 from either


def relu_split(y, *key):
    """(y, scale, shift [C]) that put scale * y + shift on both sides of 0 for one-sign y of magnitude [1, 1.25]: the
    pre-activation is 0 at |y| = SPLIT, and a y within 2^-10 of that is moved to magnitude 1, so that no decision lies
    within rounding of 0 (these cases sum what they decide)"""
    C = y.shape[-1]
    sign = np.sign(y.reshape(-1, C)[0])
    y = np.where(np.abs(np.abs(y) - SPLIT) < 2.0 ** -10, sign, y).astype(np.float32)
    scale = (0.5 + G.rng(*key).random_sample(C)).astype(np.float32)
    shift = (-scale.astype(np.float64) * sign * SPLIT).astype(np.float32)
    return y, scale, shift


def sums_case(C, *key):
    """batch sums [COPIES][2][C] of 64 pixels, gamma, beta, inv_count, eps (not the default 1e-5): mean in [-2, -0.5],
    var in [mean^2 / 4 + 0.05, mean^2 / 4 + 1], gamma and beta positive (no cancellation in the shift); every eighth
    channel is a constant -0.5 whose sums leave var = -2^-25 in both precisions: the clamp acts"""
    r = G.rng(*key)
    n = 64.0
    mean = -(0.5 + 1.5 * r.random_sample(C))
    var = mean * mean / 4 + 0.05 + 0.95 * r.random_sample(C)
    w = r.random_sample((COPIES, C)) + 0.5
    w /= w.sum(axis=0)
    sums = np.zeros((COPIES, 2, C), np.float64)
    sums[:, 0], sums[:, 1] = w * mean * n, w * (var + mean * mean) * n
    clamp = np.arange(C) % 8 == 3
    sums[:, :, clamp] = 0.0
    sums[0, 0, clamp], sums[0, 1, clamp] = -32.0, 16.0 * (1 - 2.0 ** -23)
    gamma = (0.5 + r.random_sample(C)).astype(np.float32)
    beta = (0.25 + r.random_sample(C)).astype(np.float32)
    return sums.astype(np.float32), gamma, beta, 1.0 / n, 1e-3, clamp


def finalize_case(blocks, C, *key):
    """synthetic partial rows [blocks][2][C], gamma, mean, invstd, count, old dgamma / dbeta"""
    r = G.rng(blocks, C, *key)
    rows = r.standard_normal((blocks, 2, C)).astype(np.float32)
    gamma = (0.5 + r.random_sample(C)).astype(np.float32)
    mean = r.standard_normal(C).astype(np.float32)
    invstd = (0.5 + r.random_sample(C)).astype(np.float32)
    old = r.standard_normal((2, C)).astype(np.float32)
    return rows, gamma, mean, invstd, float(37 * blocks), old


FIN_BLOCKS = (1, 31, 32, 33, 63, 64, 65, 2048)      # the ends of the two-way unrolled 32-lane loop of partial_sums
FIN_C = (1, 32, 33, 48, 480)

# (N, H, W, channel vectors) -------------------------------------------------------------------------------------------
ONE_VECTOR = (1, 8, 8, 1)
W48 = (2, 8, 24, 12)
ODD = (3, 5, 7, 8)                   # C = 32 in f32; the same vectors in bf16
BIG = (2, 128, 128, 40)              # 1.31 M vectors: more than one turn of the 4096 x 256 grid
GRAD_SHAPE = (2, 4, 6, 12)
REDUCE_SHAPES = [((1, 1, 1, 1), (0, 1, 3)), ((1, 8, 16, 1), (0, 1, 3)), ((3, 5, 7, 12), (0, 1, 3)),
                 ((2, 8, 8, 256), (0,))]            # (shape, shifts): cv = 256 is rows = 1, a thread walks 64 pixels
POOL_CASES = [((1, 8, 8, 8), (1, 2, 3)), ((2, 16, 24, 8), (1, 2, 3)), ((2, 16, 24, 12), (1, 2, 3)),
              ((2, 16, 24, 16), (3,))]              # (full-resolution shape, nlev values)
# (low-resolution shape, shift); the last one is one block in the reduce, the finalize and the apply pass
E2E_CASES = [((3, 5, 7, 12), 0), ((2, 8, 24, 12), 0), ((2, 8, 24, 12), 3), ((1, 2, 2, 1), 1)]


BOUNDARY_PERIOD = 4099               # pixels; a prime, so no grid or row stride of the kernels is a multiple of it


def rows_boundary_pixels(cv):
    """the smallest pixel count that grad_term hands to grad_term_rows_kernel"""
    return -(-ROWS_KERNEL_VECTORS // cv)


def reduce_inputs(shape, sh, dt, lattice_case, with_mask, inner_relu, *key):
    """-> dict g, mask (at the high resolution), y, scale, shift of one bn_bwd_reduce / grad_term case"""
    N, H, W, cv = shape
    C = cv * VEC[dt]
    hi, lo = (N, H << sh, W << sh, C), (N, H, W, C)
    if lattice_case:
        y, scale, shift = relu_lattice(lo, *key, 1)
        g = lattice(hi, *key, 2)
    else:
        y, g = one_sign(lo, dt, *key, 1), one_sign(hi, dt, *key, 2)
        y, scale, shift = relu_split(y, *key, 3)
    mask = mask_tensor(hi, *key, 4) if with_mask else None
    return dict(g=g, mask=mask, y=y, scale=scale if inner_relu else None, shift=shift if inner_relu else None)


def grad_configs():
    """(sh, shape, with mask, inner_relu, with scale, with coef, accumulate)"""
    out = []
    k = 0
    for sh in (0, 1, 2, 3, 4):
        shape = (1, 2, 2, 12) if sh == 4 else GRAD_SHAPE
        for inner_relu, with_scale in ((0, False), (1, True), (1, False)):
            for with_coef in (True, False):
                out.append((sh, shape, k % 3 != 2, inner_relu, with_scale, with_coef, k % 2 == 1))
                out.append((sh, shape, k % 3 != 1, inner_relu, with_scale, with_coef, k % 2 == 0))
                k += 1
    return out


def grad_inputs(shape, sh, dt, lattice, with_mask, inner_relu, with_scale, *key):
    inp = reduce_inputs(shape, sh, dt, lattice, with_mask, True, *key)
    if not lattice:                                      # (values of both signs: nothing here is summed per channel)
        inp['g'], inp['y'] = real(inp['g'].shape, dt, *key, 7), real(inp['y'].shape, dt, *key, 8)
        inp['scale'], inp['shift'] = G.real(inp['scale'].shape, *key, 9), G.real(inp['shift'].shape, *key, 10)
    if not (inner_relu and with_scale):
        inp['scale'] = inp['shift'] = None
    return inp


def reduce_configs():
    """(shape, shift, with mask, inner_relu)"""
    return [(shape, sh, m, r) for shape, shifts in REDUCE_SHAPES for sh in shifts for m in (False, True)
            for r in (0, 1)]


def lattice_terms(shape, dt, specs, *key):
    """specs: (sh, affine, relu) per term -> terms on the lattice; an affine term's pre-activation is exactly 0 on an
    eighth of its elements"""
    N, H, W, cv = shape
    Cc = cv * VEC[dt]
    terms = []
    for k, (sh, affine, relu) in enumerate(specs):
        lo = (N, H >> sh, W >> sh, Cc)
        if affine:
            y, scale, shift = relu_lattice(lo, *key, k)
            terms.append(dict(src=y, sh=sh, scale=scale, shift=shift, relu=relu))
        else:
            terms.append(dict(src=lattice(lo, *key, k), sh=sh, scale=None, shift=None, relu=relu))
    return terms


def w48_specs():
    """four terms with shifts (0, 1, 2, 3), the identity (no affine) term in each slot in turn - sum_terms takes the
    shifts in any order -, per-term ReLU and relu_out both ways, and one set with no scale at all"""
    out = []
    for ident in range(4):
        shifts = [0, 1, 2, 3]
        shifts = shifts[ident:] + shifts[:ident]         # (the slot of the identity term carries shift 0 .. 3 in turn)
        for relu_out in (0, 1):
            out.append(([(shifts[k], k != ident, (k + relu_out) % 2 == 0) for k in range(4)], relu_out))
    out.append(([(0, False, False), (1, False, True), (2, False, False), (3, False, True)], 1))
    return out


def sum_lattice_cases():
    """(shape, specs, relu_out) of the lattice cases of sum_terms"""
    cases = [(ONE_VECTOR, [(0, True, True)], 1), (ONE_VECTOR, [(0, False, False), (3, True, False)], 0)]
    cases += [(W48, specs, ro) for specs, ro in w48_specs()]
    cases += [(ODD, [(0, True, True)], 0), (ODD, [(0, True, False), (0, False, False)], 1)]
    return cases


def pool_inputs(shape, nlev, dt, lattice_case, with_mask, *key):
    N, H, W, cv = shape
    Cc = cv * VEC[dt]
    top = reduce_inputs((N, H, W, cv), 0, dt, lattice_case, with_mask, False, *key)
    ys = []
    for l in range(1, nlev + 1):
        low = (N, H >> l, W >> l, Cc)
        ys.append(lattice(low, *key, 20 + l) if lattice_case else one_sign(low, dt, *key, 20 + l))
    return dict(g=top['g'], mask=top['mask'], ys=ys)
