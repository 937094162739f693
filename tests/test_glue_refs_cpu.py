"""tests/glue_refs.py on the CPU: its float64 references against independent statements of the same operations
(torch.nn.functional.unfold, F.interpolate, an explicit transpose matrix and a finite difference, plain loops), the
lattice inputs of tests/test_glue_kernels_gpu.py (every result and every partial sum of any order is a float32, so the
bit-equality asked of the kernels rests on the reference alone), and the float32 window arithmetic of the bilinear
transposes: which (ws, W, align) shapes carry weight more than 20 columns from the start of a window."""
import numpy as np
import torch
import torch.nn.functional as F

import glue_refs as R

F64 = torch.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


# ---- references ------------------------------------------------------------------------------------------------------

def test_forward_reference_is_interpolate_and_concat():
    for align in (False, True):
        for n, H, W, br in R.CAT_CASES:
            xs = [_t(R.real((n, 4 * c, h, w), H, W, k)) for k, (c, h, w) in enumerate(br)]
            want = torch.cat([F.interpolate(x, size=(H, W), mode='bilinear', align_corners=align) for x in xs], 1)
            got = R.bilinear_cat(xs, H, W, align)
            assert got.shape == want.shape
            assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())
    # every row of the matrix sums to one; one source pixel gives a constant map
    for i, o, align in ((1, 7, 0), (1, 7, 1), (5, 13, 0), (9, 24, 1), (2, 40, 1)):
        m = R.interp_matrix(i, o, align)
        assert float((m.sum(1) - 1).abs().max()) <= 1e-15 and float(m.min()) >= 0


def test_transpose_reference_is_the_explicit_matrix_transpose_and_a_finite_difference():
    for align in (0, 1):
        for (hs, ws), (H, W) in (((3, 4), (7, 9)), ((1, 1), (4, 5)), ((2, 2), (32, 40)), ((5, 9), (13, 24))):
            g = _t(R.real((2, 3, H, W), hs, ws, H, W))
            my, mx = R.interp_matrix(hs, H, align), R.interp_matrix(ws, W, align)
            want = torch.einsum('Yy,ncYX,Xx->ncyx', my, g, mx)
            got = R.upsample_t(g, hs, ws, align)
            assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())
    # the transpose is the gradient of <g, up(x)>: central differences of that linear function are exact up to rounding
    hs, ws, H, W, align = 3, 2, 7, 5, 1
    g = _t(R.real((1, 1, H, W), 5))
    got = R.upsample_t(g, hs, ws, align)
    for y in range(hs):
        for x in range(ws):
            e = torch.zeros(1, 1, hs, ws, dtype=F64)
            e[0, 0, y, x] = 0.5
            fd = float(((R.upsample(e, H, W, align) - R.upsample(-e, H, W, align)) * g).sum())
            assert abs(fd - float(got[0, 0, y, x])) <= 1e-14 * float(g.abs().sum())
    # the concat form slices the channels of its branches
    gcat = _t(R.real((2, 12, 6, 8), 6))
    outs = R.bilinear_cat_t(gcat, [(4, 6, 8), (8, 3, 4)], 0)
    assert torch.equal(outs[0], gcat[:, :4]) and torch.equal(outs[1], R.upsample_t(gcat[:, 4:].contiguous(), 3, 4, 0))


def test_im2col_reference_is_unfold():
    for c, kpad in R.IM2COL_CK:
        for h, w in R.IM2COL_HW:
            img = R.real((2, c, h, w), c, h, w)
            got = R.im2col_stem(img, kpad)
            un = F.unfold(torch.from_numpy(img), 3, padding=1, stride=2)              # [N][c * 9 + tap][Ho * Wo]
            ho, wo = (h + 1) // 2, (w + 1) // 2
            un = un.reshape(2, c, 9, ho, wo).permute(0, 3, 4, 2, 1).reshape(2, ho, wo, 9 * c).numpy()
            assert got.shape == (2, ho, wo, kpad)
            assert R.same_bits(got[..., :9 * c], un) and not got[..., 9 * c:].any()


def test_layout_and_sum_references_against_plain_loops():
    x = R.real((2, 3, 2, 5), 1)
    nhwc = R.nchw_to_nhwc(x, 8)
    for n in range(2):
        for c in range(8):
            for h in range(2):
                for w in range(5):
                    assert nhwc[n, h, w, c] == (x[n, c, h, w] if c < 3 else 0.0)
    assert R.same_bits(R.nhwc_to_nchw(nhwc, 3), x)
    dy = R.real((7, 8), 2)
    s, a = R.column_sum(dy, 5)
    assert s.shape == (5,) and all(abs(s[c] - sum(float(v) for v in dy[:, c])) <= 1e-14 for c in range(5))
    assert all(abs(a[c] - sum(abs(float(v)) for v in dy[:, c])) <= 1e-14 for c in range(5))
    # slab sum: both slab layouts hold the same values and give the same OIHW gradient
    form0, form1 = (16, 8, 3, 5, 3, 0), (16, 32, 3, 5, 3, 1)
    val = R.real((4, 5, 9, 3), 3)
    s0 = np.full((4, 16, 9, 8), np.nan, np.float32)
    s0[:, :5, :, :3] = val
    s1 = np.full((4, 16, 32), np.nan, np.float32)
    s1[:, :5, :27] = val.reshape(4, 5, 27)
    g0, a0 = R.slab_sum(s0, 5, 3, 3, 0)
    g1, a1 = R.slab_sum(s1, 5, 3, 3, 1)
    assert g0.shape == (5, 3, 3, 3) and np.array_equal(g0, g1) and np.array_equal(a0, a1) and np.isfinite(g0).all()
    for co, ci, r, q in ((0, 0, 0, 0), (4, 2, 2, 1), (2, 1, 0, 2)):
        assert abs(g0[co, ci, r, q] - sum(float(val[k, co, r * 3 + q, ci]) for k in range(4))) <= 1e-14
    # the generated cases keep NaN in every pad position and none in the summed region
    for form in R.WRED_FORMS:
        slabs, old = R.wred_case(5, form, False)
        g, _ = R.slab_sum(slabs, form[3], form[4], form[2], form[5])
        assert np.isfinite(g).all() and old.shape == g.shape
        assert np.isnan(slabs).sum() == slabs.size - 5 * form[3] * form[4] * form[2] ** 2
    srcs, coefs = R.lincomb_case(9, 3, False)
    s, a = R.lincomb(srcs, coefs)
    assert abs(s[4] - sum(float(coefs[j]) * float(srcs[j][4]) for j in range(3))) <= 1e-15
    assert abs(a[4] - sum(abs(float(coefs[j]) * float(srcs[j][4])) for j in range(3))) <= 1e-15


def test_bf16_rounding_cases_are_what_they_claim():
    sp = R.bf16_specials()
    b = R.bf16_bits(sp).astype(np.int32) & 0xFFFF
    bits = sp.view(np.uint32)
    k = {int(v): int(o) for v, o in zip(bits, b)}
    assert k[0x3F808000] == 0x3F80 and k[0x3F818000] == 0x3F82         # ties go to the even neighbour: down, up
    assert k[0xBF808000] == 0xBF80 and k[0xBF818000] == 0xBF82
    assert k[0x3F808001] == 0x3F81 and k[0x3F817FFF] == 0x3F81
    assert k[0x7F7FFFFF] == 0x7F80 and k[0xFF7FFFFF] == 0xFF80         # the largest finite float32 rounds to inf
    assert k[0x7F7F7FFF] == 0x7F7F and k[0x7F800000] == 0x7F80
    assert k[0x00000001] == 0 and k[0x00008000] == 0 and k[0x00018000] == 2 and k[0x007FFFFF] == 0x0080
    assert (k[0x7FC00000] & 0x7FFF) > 0x7F80
    assert R.same_bf16(R.bf16_bits(sp), sp)
    wrong = R.bf16_bits(sp).copy()
    wrong[1] -= 1                                                      # truncation of the second tie
    assert not R.same_bf16(wrong, sp)
    x = R.with_specials(R.real((3, 5, 4, 2), 4))
    assert R.same_bits(x.reshape(-1)[:sp.size].view(np.uint32), bits)


# ---- lattice inputs --------------------------------------------------------------------------------------------------

def test_lattice_inputs_give_float32_results_in_every_order():
    """integers: a sum whose sum of |terms|, counted in the common unit of its terms, stays at or below 2^24 has only
    float32 partial sums, whatever the order"""
    for f in R.LATTICE_FACTORS:
        n, H, W, br, xs, gcat, inits = R.lattice_cat_case(f)
        unit = 1.0 / (4 * f * f)
        for a in xs + [gcat] + inits:
            assert np.abs(a).max() <= R.LATTICE_BOUND and (a == np.round(a)).all()
        cat = R.bilinear_cat([_t(x) for x in xs], H, W, 0).numpy()
        assert R.is_f32(cat) and (cat / unit == np.round(cat / unit)).all()
        for m in (R.interp_matrix(br[1][1], H, 0), R.interp_matrix(br[1][2], W, 0)):
            assert ((m * 2 * f) == (m * 2 * f).round()).all()                      # weights: multiples of 1 / (2 f)
        grads = R.bilinear_cat_t(_t(gcat), br, 0)
        mass = R.bilinear_cat_t(_t(np.abs(gcat)), br, 0)                           # weights >= 0: the sum of |terms|
        for g, a, init in zip(grads, mass, inits):
            g, a = g.numpy(), a.numpy() + np.abs(init)
            assert R.is_f32(g) and R.is_f32(g + init) and (g / unit == np.round(g / unit)).all()
            assert a.max() / unit <= 2.0 ** 24
    for dtype in (torch.float32, torch.bfloat16):
        for cp in R.BIAS_CP[dtype]:
            for pixels in R.BIAS_PIXELS:
                dy, old = R.bias_case(pixels, cp, True, dtype)
                assert R.same_bits(R.as_stored(dy, dtype), dy) and (dy == np.round(dy)).all()
                s, a = R.column_sum(dy, cp)
                assert R.is_f32(s) and R.is_f32(s + old) and (a + np.abs(old)).max() <= 2.0 ** 24
    for form in R.WRED_FORMS:
        for ns in R.WRED_NSPLIT:
            slabs, old = R.wred_case(ns, form, True)
            s, a = R.slab_sum(slabs, form[3], form[4], form[2], form[5])
            assert (s == np.round(s)).all() and R.is_f32(s + old) and (a + np.abs(old)).max() <= 2.0 ** 24
    for n in R.LINCOMB_N:
        for k in range(1, 9):
            srcs, coefs = R.lincomb_case(min(n, 4099), k, True)
            s, a = R.lincomb(srcs, coefs)
            assert (s == np.round(s)).all() and a.max() <= 2.0 ** 24


# ---- the window arithmetic -------------------------------------------------------------------------------------------

def test_emulated_weights_are_the_reference_weights():
    for i, o in ((3, 24), (4, 32), (5, 13), (9, 24), (2, 40), (1, 6), (7, 7)):
        for align in (0, 1):
            m32, m64 = R.weights32(i, o, align), R.interp_matrix(i, o, align).numpy()
            assert np.abs(m32 - m64).max() <= 8 * i * R.U, (i, o, align)


def test_window_never_misses_and_which_shapes_pass_twenty_columns():
    """over every in <= 39 and out <= 129 in both modes: no destination with a non-zero weight lies outside the window
    of its source (the concat transpose, which walks the window in passes of 20, sees every one), and the shapes that
    the gate of the streamed transpose admits with weight 20 or more columns from the start of a window are the nine
    align_corners shapes below - a kernel that holds 20 weights and walks them once drops those"""
    beyond = {0: [], 1: []}
    for align in (0, 1):
        for i in range(1, 40):
            for o in range(i, 130):
                missed, far = R.window_report(i, o, align)
                assert not missed, (i, o, align, missed[:3])
                if far and R.gate_admits(i, o):
                    beyond[align].append((i, o))
    assert beyond[0] == []
    assert beyond[1] == R.BEYOND_ALIGN_SHAPES
    # the case of the issue: W = 24 from ws = 3, column 1 sees [0, 24) and its last three weights fall off the end
    d0, d1 = R.bilin_window32(np.array([1]), 3, 24, 1)
    assert (int(d0[0]), int(d1[0])) == (0, 24)
    _, far = R.window_report(3, 24, 1)
    assert [(s, d) for s, d, _ in far] == [(1, 20), (1, 21), (1, 22)]
    assert [round(w, 2) for _, _, w in far] == [0.26, 0.17, 0.09]
    # what the other upsample-transpose cases of the GPU file rely on
    for i, o in R.NEIGHBOUR_ALIGN_SHAPES:
        assert R.gate_admits(i, o) and not R.window_report(i, o, 1)[1]
    for i, o in R.PLAIN_SHAPES:
        assert R.gate_admits(i, o) and not R.window_report(i, o, 0)[1]
    assert not R.gate_admits(4, 40) and not R.gate_admits(257, 257) and not R.gate_admits(5, 4)
    # the concat transpose's multi-pass cases: factor 16 and 2 -> 40 reach past one pass in both modes
    for i, o in ((2, 32), (2, 40)):
        for align in (0, 1):
            d0, d1 = R.bilin_window32(np.arange(i), i, o, align)
            assert (d1 - d0).max() > R.MAXW


def _pow2(x):
    m, _ = np.frexp(float(x))
    return m == 0.5


def test_bf16_inputs_put_the_largest_result_on_a_power_of_two():
    """the bf16 bound adds 2^-9 * max |ref| for the rounding to storage; a value just above a power of two rounds with
    an error of up to 2^-8 of itself, so on random inputs the float64 reference itself, rounded to bf16 as torch
    rounds, lies beyond that bound. With the planted inputs of the GPU tests max |ref| is a power of two, reached by
    exact results, and the correctly rounded reference meets the bound as stated: what is asked of the kernels there
    is a correct rounding of a float32 result that meets the f32 bound"""
    bf = torch.bfloat16

    def ideal_ok(r64, r32, cap):
        ideal = r64.float().to(bf).double().numpy()
        return R.check_bilinear('ideal', ideal, r64, r32, True, cap)[3]
    G0 = R.as_stored(R.real((1, 8, 22, 4), 22, 4, 3, 2, 1), bf)                   # 22 x 4 -> 3 x 2, align_corners = 1
    r64 = R.upsample_t(torch.from_numpy(G0).double(), 3, 2, 1)
    assert not _pow2(r64.abs().max()) and not ideal_ok(r64, R.upsample_t(torch.from_numpy(G0), 3, 2, 1), 2.0 ** -8)
    for sizes, shape, align in (([(3, 2)], (1, 8, 22, 4), 1), ([(2, 3)], (1, 8, 4, 24), 1), ([(7, 3)], (3, 8, 40, 6), 0),
                                ([(12, 12), (9, 9), (5, 7)], (1, 8, 24, 24), 1), ([(2, 200)], (1, 16, 3, 300), 1)):
        G = R.plant_upsample_t(R.as_stored(R.real(shape, *shape), bf), sizes, align)
        assert R.same_bits(R.as_stored(G, bf), G)
        for hs, ws in sizes:
            r64, r32 = R.upsample_t(torch.from_numpy(G).double(), hs, ws, align), R.upsample_t(torch.from_numpy(G), hs, ws, align)
            assert _pow2(r64.abs().max()) and float(r64[0, 0, 0, 0]) == float(r64.abs().max())
            assert ideal_ok(r64, r32, 2.0 ** -8)
    for ci, (n, H, W, brv) in enumerate(R.CAT_CASES):
        br = [(8 * v, h, w) for v, h, w in brv]
        xs = R.plant_forward([R.as_stored(R.real((n, c, h, w), ci, k), bf) for k, (c, h, w) in enumerate(br)])
        gcat0 = R.as_stored(R.real((n, sum(c for c, _, _ in br), H, W), ci, 8), bf)
        inits0 = [R.as_stored(R.real((n, c, h, w), ci, 20 + k), bf) for k, (c, h, w) in enumerate(br)]
        for align in (0, 1):
            cat = R.bilinear_cat([_t(x) for x in xs], H, W, align)
            assert _pow2(cat.abs().max())
            assert ideal_ok(cat, R.bilinear_cat([torch.from_numpy(x) for x in xs], H, W, align), 3e-2)
            gcat, inits = R.plant_cat_t(gcat0, br, inits0, align)
            assert R.same_bits(R.as_stored(gcat, bf), gcat)
            g64 = R.bilinear_cat_t(_t(gcat), br, align)
            g32 = R.bilinear_cat_t(torch.from_numpy(gcat), br, align)
            for k in range(len(br)):
                for r64, r32 in ((g64[k], g32[k]), (g64[k] + _t(inits[k]), g32[k] + torch.from_numpy(inits[k]))):
                    assert _pow2(r64.abs().max()) and ideal_ok(r64, r32, 6e-2)
