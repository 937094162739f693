"""The resampling, layout and reduction glue kernels of csrc/eltwise.hip over the shapes at which they can go wrong:
1 to 4 concat branches with offsets that are no multiples of 32, 1 x 1 and identity branches, non-integer ratios and
windows of more than one pass, the streamed upsample transpose at every align_corners shape whose x window passes 20
columns, at widths where lanes exit and at row bands that end short, layout tiles of 31 / 32 / 33 / 65 pixels and
1 / 5 / 33 / 96 channels with unrounded inputs (round-to-nearest-even into bf16: ties, inf, denormals, NaN), both stem
im2col kernels at odd sizes, the column sum at one row per block and several turns of its loop, the slab sum at the
ends of both unrolled loops with NaN in every pad position, the zero fill past the grid cap and past 2^32 bytes, the
linear combination at k = 1..8.

Each kernel is called through the C ABI and compared with the float64 reference of tests/glue_refs.py under the bounds
stated there; tests/test_glue_refs_cpu.py pins the references, the lattice inputs and the case list of the window
test on the CPU. Integer-lattice inputs compare bit for bit. Every output lies inside a larger buffer of sentinels, 64
elements on each side (16-byte aligned), which must come back bit-unchanged with the payload fully written; every
kernel runs twice and must give the same bits. Every real-valued case prints its measured error next to its bound.
Each test runs in a spawned child (tests/spawned.py).

The bf16 cases of the bilinear kernels use inputs whose largest result is a power of two (glue_refs.plant_*): the
storage term 2^-9 * max |ref| of their bound is half an ulp of the binade BELOW max |ref|, so it covers a correct
rounding only when no result lies strictly inside the top binade; on plain random inputs the float64 reference
itself, rounded to bf16, misses it (tests/test_glue_refs_cpu.py). Every bf16 case is also held, element by element,
to a correct rounding of a float32 result that meets the f32 bound (glue_refs.rounding_allowance), asserted first.

The wide align_corners cases (200 -> 300 and 256 -> 512 columns) are what made bilin_src form its align_corners
coordinate as an exact integer quotient and remainder: as the float product d * ((in - 1) / (out - 1)) it left 1.5e-5
in a weight at a coordinate near 255 (3.040e-05 and 4.653e-05 against 8.510e-06 and 1.025e-05, equal to torch's
float32 kernel to three digits)."""
import ctypes

import numpy as np
import pytest
import torch

import glue_refs as R
from spawned import spawned

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PAD = 64
# bit patterns of quiet NaNs with a payload that no kernel produces
SENTINEL = {torch.float32: (torch.int32, 0x7FC5C3E1), torch.bfloat16: (torch.int16, 0x7FC5)}
DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
DTYPE_IDS = ['f32', 'bf16']


def _C():
    from hipnet import _capi as C
    return C


def _pp(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _ip(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _dev(a, dtype=torch.float32):
    """numpy float32 (already a value of `dtype`) -> device tensor of dtype"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV).contiguous()


def _nhwc(x_nchw, dtype, cp=None):
    x = np.asarray(x_nchw, dtype=np.float32)
    return _dev(R.nchw_to_nhwc(x, cp or x.shape[1]), dtype)


class Guarded(object):
    """n elements of dtype inside PAD sentinels on each side; `init` fills the payload (an in/out argument)"""

    def __init__(self, n, dtype=torch.float32, init=None):
        self.n, self.dtype = int(n), dtype
        self.idt, self.s = SENTINEL[dtype]
        self.raw = torch.full((self.n + 2 * PAD,), self.s, dtype=self.idt, device=DEV)
        self.t = self.raw.view(dtype)[PAD:PAD + self.n]
        assert self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).reshape(-1).to(dtype))

    def ptr(self):
        return self.t.data_ptr()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.raw == self.s).all())

    def get(self, what):
        """(float32 values, integer bits) of the payload, after checking that it was written completely (no sentinel
        left) and the guards not at all"""
        torch.cuda.synchronize()
        raw = self.raw.cpu()
        assert bool((raw[:PAD] == self.s).all()) and bool((raw[PAD + self.n:] == self.s).all()), \
            what + ': write outside the output'
        pay = raw[PAD:PAD + self.n]
        assert not bool((pay == self.s).any()), what + ': an output element was not written'
        return pay.view(self.dtype).float().numpy().copy(), pay.numpy().copy()


def _twice(what, run):
    """run() -> list of (values, bits), on fresh outputs each time: bit-identical both times; -> the values"""
    a, b = run(), run()
    for (_, x), (_, y) in zip(a, b):
        assert R.same_bits(x, y), what + ': two runs differ'
    return [v for v, _ in a]


def _nchw(flat, n, h, w, c):
    return np.ascontiguousarray(flat.reshape(n, h, w, c).transpose(0, 3, 1, 2))


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# ---- bilinear upsample + concat and its transpose ---------------------------------------------------------------------

def _cat_forward(C, dtype, xs, N, H, W, br, align, name):
    """xs: NCHW float32 arrays (values of dtype); br [(c, h, w)] -> NCHW float32 of the concat"""
    xd = [_nhwc(x, dtype) for x in xs]
    cs, hs, ws = [c for c, _, _ in br], [h for _, h, _ in br], [w for _, _, w in br]

    def run():
        out = Guarded(N * H * W * sum(cs), dtype)
        C.call('hrnet_bilinear_cat', C.dtype_id(dtype), out.ptr(), _pp([t.data_ptr() for t in xd]), _ip(hs), _ip(ws),
               _ip(cs), len(br), N, H, W, align, C.stream_ptr())
        return [out.get(name)]
    return _nchw(_twice(name, run)[0], N, H, W, sum(cs))


def _cat_backward(C, dtype, gcat, N, H, W, br, align, inits, name):
    """gcat NCHW float32; inits: None (accumulate = 0, onto sentinel NaN) or the NCHW destinations of accumulate = 1"""
    gd = _nhwc(gcat, dtype)
    cs, hs, ws = [c for c, _, _ in br], [h for _, h, _ in br], [w for _, _, w in br]

    def run():
        outs = [Guarded(N * h * w * c, dtype, None if inits is None else R.nchw_to_nhwc(inits[k], c))
                for k, (c, h, w) in enumerate(br)]
        C.call('hrnet_bilinear_cat_bwd', C.dtype_id(dtype), gd.data_ptr(), _pp([o.ptr() for o in outs]), _ip(hs),
               _ip(ws), _ip(cs), len(br), N, H, W, align, 0 if inits is None else 1, C.stream_ptr())
        return [o.get(name) for o in outs]
    return [_nchw(v, N, h, w, c) for v, (c, h, w) in zip(_twice(name, run), br)]


@spawned
def test_bilinear_concat_and_transposes_on_the_integer_lattice_are_bit_equal():
    """f32, align_corners = 0, factors 2 / 4 / 8 / 16, integer inputs: every product and partial sum is exact, so the
    concat, its transpose (accumulate 0 and 1) and the upsample transpose (both forms) give the reference's bits"""
    C = _C()
    f32 = torch.float32
    for f in R.LATTICE_FACTORS:
        N, H, W, br, xs, gcat, inits = R.lattice_cat_case(f)
        name = 'lattice factor {}'.format(f)
        got = _cat_forward(C, f32, xs, N, H, W, br, 0, name + ' fwd')
        want = R.bilinear_cat([_t64(x) for x in xs], H, W, 0).numpy()
        assert R.same_bits(got, want.astype(np.float32)), name + ' fwd'
        grads = [g.numpy() for g in R.bilinear_cat_t(_t64(gcat), br, 0)]
        for acc in (0, 1):
            got = _cat_backward(C, f32, gcat, N, H, W, br, 0, inits if acc else None, name + ' bwd')
            for k, g in enumerate(got):
                want = grads[k] + (inits[k] if acc else 0.0)
                assert R.same_bits(g, want.astype(np.float32)), '{} bwd branch {} accumulate {}'.format(name, k, acc)
        # the transpose over all channels, to the low-resolution size alone
        (c, hs, ws) = br[1]
        want = R.upsample_t(_t64(gcat), hs, ws, 0).numpy().astype(np.float32)
        gd = _nhwc(gcat, f32)
        for streamed in (1, 0):
            out = Guarded(N * hs * ws * 2 * c, f32)
            args = (C.dtype_id(f32), gd.data_ptr(), _pp([out.ptr()]), _ip([hs]), _ip([ws]), 1, N, H, W, 2 * c, 0,
                    streamed, C.stream_ptr())
            if f == 16:                                          # 2 * 16 + 4 > 20: beyond the gate
                with pytest.raises(RuntimeError):
                    C.call('hrnet_upsample_bilinear_t', *args)
                assert out.untouched()
                continue
            C.call('hrnet_upsample_bilinear_t', *args)
            got = _nchw(out.get(name)[0], N, hs, ws, 2 * c)
            assert R.same_bits(got, want), '{} upsample_t streamed {}'.format(name, streamed)
        print(name + ': forward, transpose and upsample transpose bit-equal')


@pytest.mark.parametrize('dt', DTYPE_IDS)
@spawned
def test_bilinear_concat_forward_and_backward_over_branch_shapes(dt):
    C = _C()
    dtype = DT[dt]
    vec, bf16 = R.vec_of(dtype), dtype == torch.bfloat16
    results = []
    for ci, (N, H, W, brv) in enumerate(R.CAT_CASES):
        br = [(v * vec, h, w) for v, h, w in brv]
        ctot = sum(c for c, _, _ in br)
        xs = [R.as_stored(R.real((N, c, h, w), ci, k), dtype) for k, (c, h, w) in enumerate(br)]
        gcat = R.as_stored(R.real((N, ctot, H, W), ci, 8), dtype)
        inits = [R.as_stored(R.real((N, c, h, w), ci, 20 + k), dtype) for k, (c, h, w) in enumerate(br)]
        if bf16:                                         # max |cat| a power of two (glue_refs.plant_forward)
            xs = R.plant_forward(xs)
        gcat0, inits0 = gcat, inits
        for align in (0, 1):
            name = 'cat {} case {} ({} branches, {}x{}) align {}'.format(dt, ci, len(br), H, W, align)
            if bf16:
                gcat, inits = R.plant_cat_t(gcat0, br, inits0, align)
            got = _cat_forward(C, dtype, xs, N, H, W, br, align, name)
            ref64 = R.bilinear_cat([_t64(x) for x in xs], H, W, align)
            ref32 = R.bilinear_cat([_t32(x) for x in xs], H, W, align)
            results.append(R.check_bilinear(name + ' fwd', got, ref64, ref32, bf16, 3e-2 if bf16 else 1e-4))
            off = 0
            for k, (c, h, w) in enumerate(br):           # an identity branch is a copy
                if (h, w) == (H, W):
                    assert R.same_bits(got[:, off:off + c], xs[k]), name + ': identity branch'
                off += c
            g64, g32 = R.bilinear_cat_t(_t64(gcat), br, align), R.bilinear_cat_t(_t32(gcat), br, align)
            for acc in (0, 1):
                got = _cat_backward(C, dtype, gcat, N, H, W, br, align, inits if acc else None, name)
                for k in range(len(br)):
                    r64 = g64[k] + (_t64(inits[k]) if acc else 0.0)
                    r32 = g32[k] + (_t32(inits[k]) if acc else 0.0)
                    results.append(R.check_bilinear('{} bwd branch {} accumulate {}'.format(name, k, acc), got[k], r64,
                                                    r32, bf16, 6e-2 if bf16 else 2e-4))
    R.assert_all(results)


# ---- the upsample transpose over all channels ---------------------------------------------------------------------

def _upsample_t(C, dtype, G, sizes, align, streamed, name):
    """G NCHW float32 (values of dtype) -> the NCHW float32 result of every output size"""
    N, Cc, H, W = G.shape
    gd = _nhwc(G, dtype)

    def run():
        outs = [Guarded(N * hs * ws * Cc, dtype) for hs, ws in sizes]
        C.call('hrnet_upsample_bilinear_t', C.dtype_id(dtype), gd.data_ptr(), _pp([o.ptr() for o in outs]),
               _ip([h for h, _ in sizes]), _ip([w for _, w in sizes]), len(sizes), N, H, W, Cc, align, streamed,
               C.stream_ptr())
        return [o.get(name) for o in outs]
    return [_nchw(v, N, hs, ws, Cc) for v, (hs, ws) in zip(_twice(name, run), sizes)]


def _upsample_t_cases(C, dt, cases):
    """cases: (N, H, W, channel vectors, [(hs, ws)], align); both forms of the call"""
    dtype = DT[dt]
    vec, bf16 = R.vec_of(dtype), dtype == torch.bfloat16
    results = []
    for N, H, W, cv, sizes, align in cases:
        G = R.as_stored(R.real((N, cv * vec, H, W), H, W, sizes[0][0], sizes[0][1], align), dtype)
        if bf16:                                         # max |result| a power of two (glue_refs.plant_upsample_t)
            G = R.plant_upsample_t(G, sizes, align)
        refs = [(R.upsample_t(_t64(G), hs, ws, align), R.upsample_t(_t32(G), hs, ws, align)) for hs, ws in sizes]
        for streamed in (1, 0):
            name = 'upsample_t {} {}x{} -> {} align {} streamed {}'.format(dt, H, W, sizes, align, streamed)
            got = _upsample_t(C, dtype, G, sizes, align, streamed, name)
            for k, (r64, r32) in enumerate(refs):
                results.append(R.check_bilinear('{} out {}'.format(name, k), got[k], r64, r32, bf16,
                                                2.0 ** -8 if bf16 else 2e-6))
    R.assert_all(results)


@pytest.mark.parametrize('dt', DTYPE_IDS)
@spawned
def test_upsample_transpose_where_the_align_corners_window_passes_twenty_columns(dt):
    """the nine (ws -> W) shapes of glue_refs.BEYOND_ALIGN_SHAPES, on the x axis and on the y axis: a kernel that holds
    20 x weights and walks them once drops the last destinations of the middle columns"""
    cases = []
    for a, b in R.BEYOND_ALIGN_SHAPES:
        cases.append((1, 4, b, 1, [(2, a)], 1))          # on x
        cases.append((1, b, 4, 1, [(a, 2)], 1))          # on y
    cases.append((3, 32, 24, 2, [(4, 3)], 1))            # both at once, N = 3, two channel vectors
    _upsample_t_cases(_C(), dt, cases)


@pytest.mark.parametrize('dt', DTYPE_IDS)
@spawned
def test_upsample_transpose_over_ratios_widths_and_row_bands(dt):
    cases = []
    for align, shapes in ((1, R.NEIGHBOUR_ALIGN_SHAPES), (0, R.PLAIN_SHAPES)):
        for a, b in shapes:
            cases.append((1, 4, b, 1, [(2, a)], align))
            cases.append((1, b, 4, 1, [(a, 2)], align))
    # one channel vector per workgroup, lanes of w >= ws exit; two chunks of channels
    cases += [(1, 3, 258, 2, [(2, 129)], 0), (1, 3, 400, 2, [(2, 200)], 0), (1, 3, 256, 2, [(2, 256)], 0)]
    # hs = 7 from H = 40: three row bands of 3, 3 and 1 rows; the rows between them feed both
    cases += [(3, 40, 6, 1, [(7, 3)], 0), (3, 40, 6, 1, [(7, 3)], 1)]
    # three outputs in one call; a set the tile form declines (9 does not divide 24) and one it takes
    cases += [(1, 24, 24, 1, [(12, 12), (9, 9), (5, 7)], 0), (1, 24, 24, 1, [(12, 12), (9, 9), (5, 7)], 1),
              (2, 16, 16, 1, [(8, 8), (4, 4), (2, 2)], 0)]
    _upsample_t_cases(_C(), dt, cases)


@pytest.mark.parametrize('dt', DTYPE_IDS)
@spawned
def test_upsample_transpose_of_wide_maps_with_align_corners(dt):
    """ws of 200 and 256 at ratios that are no powers of two: one channel vector per workgroup, lanes of w >= ws exit,
    and source coordinates near 255, where a float32 product for the coordinate would leave 1.5e-5 in a weight"""
    _upsample_t_cases(_C(), dt, [(1, 3, 300, 2, [(2, 200)], 1), (1, 3, 512, 2, [(2, 256)], 1)])


@spawned
def test_upsample_transpose_refuses_what_it_cannot_serve_and_writes_nothing():
    C = _C()
    for dtype in (torch.float32, torch.bfloat16):
        vec = R.vec_of(dtype)
        # (H, W, sizes): beyond the gate; more than 256 columns; an output larger than the input; a refused output
        # behind a served one
        for H, W, sizes in ((4, 40, [(2, 4)]), (2, 300, [(2, 300)]), (2, 514, [(1, 257)]), (4, 8, [(5, 4)]),
                            (4, 40, [(2, 20), (2, 4)])):
            for streamed in (1, 0):
                gd = _dev(R.real((1, H, W, vec), H, W), dtype)
                outs = [Guarded(hs * ws * vec, dtype) for hs, ws in sizes]
                with pytest.raises(RuntimeError):
                    C.call('hrnet_upsample_bilinear_t', C.dtype_id(dtype), gd.data_ptr(), _pp([o.ptr() for o in outs]),
                           _ip([h for h, _ in sizes]), _ip([w for _, w in sizes]), len(sizes), 1, H, W, vec, 1,
                           streamed, C.stream_ptr())
                assert all(o.untouched() for o in outs), (H, W, sizes, streamed)


# ---- layout conversions ----------------------------------------------------------------------------------------------

@spawned
def test_layout_conversions_are_exact_and_round_to_nearest_even():
    C = _C()
    for dtype in (torch.float32, torch.bfloat16):
        bf16 = dtype == torch.bfloat16
        for N in R.LAYOUT_N:
            for H, W in R.LAYOUT_HW:
                for Cp, Cc in R.LAYOUT_CH:
                    name = 'layout {} N {} {}x{} Cp {} C {}'.format(dtype, N, H, W, Cp, Cc)
                    # NHWC (dtype) -> NCHW f32: NaN in the pad channels, which nothing may read into the result
                    x = R.as_stored(R.real((N, Cc, H, W), N, H, W, Cp), dtype)
                    src = np.full((N, H, W, Cp), np.nan, np.float32)
                    src[..., :Cc] = x.transpose(0, 2, 3, 1)
                    sd = _dev(src, dtype)

                    def run():
                        out = Guarded(N * Cc * H * W)
                        C.call('hrnet_nhwc_to_nchw', C.dtype_id(dtype), sd.data_ptr(), out.ptr(), N, H, W, Cp, Cc,
                               C.stream_ptr())
                        return [out.get(name)]
                    got = _twice(name, run)[0]
                    assert R.same_bits(got.reshape(N, Cc, H, W), R.nhwc_to_nchw(src, Cc)), name + ' to NCHW'
                    # NCHW f32 (unrounded, with the rounding cases planted) -> NHWC (dtype) onto 7.0
                    y = R.with_specials(R.real((N, Cc, H, W), N, H, W, Cp, 1))
                    yd = torch.from_numpy(y).to(DEV)

                    def run2():
                        out = Guarded(N * H * W * Cp, dtype, np.full(N * H * W * Cp, 7.0, np.float32))
                        C.call('hrnet_nchw_to_nhwc', C.dtype_id(dtype), yd.data_ptr(), out.ptr(), N, H, W, Cp, Cc,
                               C.stream_ptr())
                        torch.cuda.synchronize()
                        raw = out.raw.cpu()
                        assert bool((raw[:PAD] == out.s).all()) and bool((raw[PAD + out.n:] == out.s).all()), name
                        bits = raw[PAD:PAD + out.n].numpy().copy()
                        return [(bits, bits)]
                    bits = _twice(name, run2)[0].reshape(N, H, W, Cp)
                    want = R.nchw_to_nhwc(y, Cp)
                    assert not bits[..., Cc:].any(), name + ': pad channels must be zero'
                    if bf16:
                        assert R.same_bf16(bits[..., :Cc], want[..., :Cc]), name + ' to NHWC bf16'
                    else:
                        assert R.same_bits(bits[..., :Cc].view(np.float32), want[..., :Cc]), name + ' to NHWC'
    print('layout conversions: {} shapes, both directions, both types, exact'.format(
        len(R.LAYOUT_N) * len(R.LAYOUT_HW) * len(R.LAYOUT_CH)))


# ---- stem im2col --------------------------------------------------------------------------------------------------------

@spawned
def test_im2col_stem_both_kernels_at_odd_sizes():
    C = _C()
    for dtype in (torch.float32, torch.bfloat16):
        bf16 = dtype == torch.bfloat16
        for N in R.IM2COL_N:
            for H, W in R.IM2COL_HW:
                Ho, Wo = (H + 1) // 2, (W + 1) // 2
                cols3 = {}
                for Cc, Kpad in R.IM2COL_CK:
                    name = 'im2col {} N {} C {} {}x{} Kpad {}'.format(dtype, N, Cc, H, W, Kpad)
                    img = R.with_specials(R.real((N, Cc, H, W), N, Cc, H, W))
                    imgd = torch.from_numpy(img).to(DEV)

                    def run():
                        out = Guarded(N * Ho * Wo * Kpad, dtype)
                        C.call('hrnet_im2col_stem', C.dtype_id(dtype), imgd.data_ptr(), out.ptr(), N, Cc, H, W, Ho, Wo,
                               Kpad, C.stream_ptr())
                        return [out.get(name)]
                    a, b = run(), run()
                    assert R.same_bits(a[0][1], b[0][1]), name + ': two runs differ'
                    bits = a[0][1].reshape(N, Ho, Wo, Kpad)
                    want = R.im2col_stem(img, Kpad)
                    if bf16:
                        assert R.same_bf16(bits, want), name
                    else:
                        assert R.same_bits(bits.view(np.float32), want), name
                    assert not bits[..., 9 * Cc:].any(), name + ': columns beyond 9 C must be zero'
                    if Cc == 3:
                        cols3[Kpad] = bits
                # the pixel kernel and the generic one: the same 27 columns (a NaN is a NaN in both)
                p, q = cols3[32][..., :27], cols3[64][..., :27]
                nan = np.isnan(R.im2col_stem(R.with_specials(R.real((N, 3, H, W), N, 3, H, W)), 27))
                assert (p[~nan] == q[~nan]).all(), (dtype, N, H, W)
    print('im2col: {} shapes x {} kernels, both types, exact'.format(len(R.IM2COL_N) * len(R.IM2COL_HW),
                                                                     len(R.IM2COL_CK)))


# ---- column sum -----------------------------------------------------------------------------------------------------------

@spawned
def test_bias_grad_over_widths_pixel_counts_and_accumulate():
    C = _C()
    for dtype in (torch.float32, torch.bfloat16):
        for Cp in R.BIAS_CP[dtype]:
            for pixels in R.BIAS_PIXELS:
                blocks = C.call('hrnet_reduce_blocks', 1, 1, pixels, Cp)
                for lattice in (True, False):
                    dy, old = R.bias_case(pixels, Cp, lattice, dtype)
                    dyd = _dev(dy, dtype)
                    for Cc in (Cp, Cp - 3):
                        s, a = R.column_sum(dy, Cc)
                        for acc in (0, 1):
                            name = 'bias_grad {} Cp {} C {} pixels {} accumulate {} {}'.format(
                                dtype, Cp, Cc, pixels, acc, 'lattice' if lattice else 'real')

                            def run():
                                db, scratch = Guarded(Cc, init=old[:Cc] if acc else None), Guarded(blocks * Cp)
                                C.call('hrnet_bias_grad', C.dtype_id(dtype), dyd.data_ptr(), db.ptr(), scratch.ptr(),
                                       pixels, Cp, Cc, acc, C.stream_ptr())
                                return [db.get(name), scratch.get(name)]
                            got = _twice(name, run)[0]
                            want = s + (old[:Cc].astype(np.float64) if acc else 0.0)
                            if lattice:
                                assert R.same_bits(got, want.astype(np.float32)), name
                            else:
                                R.check_sum(name, got, want, a + (np.abs(old[:Cc]) if acc else 0.0), pixels + acc)
        # 257 vectors of channels: more than one workgroup holds
        Cp = R.BIAS_REFUSED_CP[dtype]
        dyd, db, scratch = _dev(R.real((2, Cp), Cp), dtype), Guarded(Cp), Guarded(Cp)
        with pytest.raises(RuntimeError):
            C.call('hrnet_bias_grad', C.dtype_id(dtype), dyd.data_ptr(), db.ptr(), scratch.ptr(), 2, Cp, Cp, 0,
                   C.stream_ptr())
        assert db.untouched() and scratch.untouched()


# ---- slab sum ---------------------------------------------------------------------------------------------------------------

@spawned
def test_wgrad_reduce_on_synthetic_slabs_at_the_ends_of_its_loops():
    C = _C()
    for form in R.WRED_FORMS:
        Cout, Cin, ks, co, ci, kflat = form
        for ns in R.WRED_NSPLIT:
            for lattice in (True, False):
                slabs, old = R.wred_case(ns, form, lattice)
                sd = torch.from_numpy(slabs).to(DEV)
                s, a = R.slab_sum(slabs, co, ci, ks, kflat)
                for acc in (0, 1):
                    name = 'wgrad_reduce Cout {} Cin {} ks {} real {}x{} kflat {} nsplit {} accumulate {} {}'.format(
                        Cout, Cin, ks, co, ci, kflat, ns, acc, 'lattice' if lattice else 'real')

                    def run():
                        g = Guarded(s.size, init=old if acc else None)
                        C.call('hrnet_wgrad_reduce', sd.data_ptr(), g.ptr(), ns, Cout, Cin, ks, co, ci, kflat, acc,
                               C.stream_ptr())
                        return [g.get(name)]
                    got = _twice(name, run)[0].reshape(s.shape)
                    want = s + (old.astype(np.float64) if acc else 0.0)
                    if lattice:
                        assert R.same_bits(got, want.astype(np.float32)), name
                    else:
                        R.check_sum(name, got, want, a + (np.abs(old) if acc else 0.0), ns + acc)


# ---- zero fill --------------------------------------------------------------------------------------------------------------

@spawned
def test_fill_zero_tails_the_grid_cap_and_the_high_length_word():
    C = _C()
    G = 256
    for nbytes in R.FILL_BYTES:
        for rep in (0, 1):
            buf = torch.full((G + nbytes + G,), 0xFF, dtype=torch.uint8, device=DEV)
            p = buf.data_ptr() + G
            assert p % 16 == 0
            C.call('hrnet_fill_zero', p, nbytes, C.stream_ptr())
            torch.cuda.synchronize()
            nz = int(torch.count_nonzero(buf[G:G + nbytes])) if nbytes else 0
            assert nz == 0, ('fill_zero', nbytes, nz)
            assert bool((buf[:G] == 0xFF).all()) and bool((buf[G + nbytes:] == 0xFF).all()), ('fill_zero', nbytes)
            del buf
        print('fill_zero {} bytes: all zero, the bytes around them untouched'.format(nbytes))
    buf = torch.full((G + 64 + G,), 0xFF, dtype=torch.uint8, device=DEV)
    for off in (1, 4, 8):
        with pytest.raises(RuntimeError):
            C.call('hrnet_fill_zero', buf.data_ptr() + G + off, 32, C.stream_ptr())
    with pytest.raises(RuntimeError):
        C.call('hrnet_fill_zero', None, 32, C.stream_ptr())
    torch.cuda.synchronize()
    assert bool((buf == 0xFF).all())


# ---- linear combination -----------------------------------------------------------------------------------------------------

def _lincomb(C, out, n, srcs, coefs):
    C.call('hrnet_lincomb_f32', out.ptr(), n, len(coefs), _pp([None if t is None else t.data_ptr() for t in srcs]),
           (ctypes.c_float * len(coefs))(*[float(c) for c in coefs]), C.stream_ptr())


@spawned
def test_lincomb_f32_over_term_counts_lengths_nan_and_refusals():
    C = _C()
    for n in R.LINCOMB_N:
        for k in (range(1, 9) if n <= 257 else (1, 8)):
            for lattice in (True, False):
                srcs, coefs = R.lincomb_case(n, k, lattice)
                sd = [torch.from_numpy(s).to(DEV) for s in srcs]
                name = 'lincomb n {} k {} {}'.format(n, k, 'lattice' if lattice else 'real')

                def run():
                    out = Guarded(n)
                    _lincomb(C, out, n, sd, coefs)
                    return [out.get(name)]
                got = _twice(name, run)[0]
                s, a = R.lincomb(srcs, coefs)
                if lattice:
                    assert R.same_bits(got, s.astype(np.float32)), name
                else:
                    R.check_sum(name, got, s, a, k)
    # 0 * NaN is NaN, as in torch
    x = np.array([1.0, np.nan, 3.0, np.inf], np.float32)
    y = np.array([2.0, 5.0, np.nan, 7.0], np.float32)
    want = (torch.from_numpy(x) * 0.0 + torch.from_numpy(y) * 1.5).numpy()
    out = Guarded(4)
    _lincomb(C, out, 4, [torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)], [0.0, 1.5])
    got = out.get('lincomb nan')[0]
    assert np.isnan(want).tolist() == [False, True, True, True] and np.isnan(got).tolist() == np.isnan(want).tolist()
    assert got[0] == want[0] == 3.0
    # refused: no term, nine terms, no element, a null source
    t = [torch.zeros(8, device=DEV) for _ in range(9)]
    out = Guarded(8)
    for n, srcs, coefs in ((8, [], []), (8, t, [1.0] * 9), (0, t[:2], [1.0, 1.0]), (8, [t[0], None, t[2]], [1.0] * 3)):
        with pytest.raises(RuntimeError):
            C.call('hrnet_lincomb_f32', out.ptr(), n, len(coefs),
                   _pp([None if s is None else s.data_ptr() for s in srcs] or [None]),
                   (ctypes.c_float * max(len(coefs), 1))(*coefs), C.stream_ptr())
    assert out.untouched()
