"""tests/contraction_refs.py pinned without a GPU: its float64 references against independent formulations (unfold and
an int64 matmul, a scatter over taps, autograd), the lattice and exactness conditions of every case in its lists, and
the sensitivity of the two checks (equality on the lattice, the per-element bound in reals) to the mistakes a
contraction kernel makes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import contraction_refs as R


def _ints(rng, shape, lo=-3, hi=4):
    return torch.from_numpy(rng.integers(lo, hi, shape))


def _conv_unfold(a, w, stride):
    """int64: im2col and one matmul per image"""
    ks = w.shape[-1]
    n, c, h, w_ = a.shape
    ho, wo = R.out_hw(h, w_, ks, stride)
    cols = F.unfold(a.double(), ks, padding=ks // 2, stride=stride).round().long()      # [n, c ks ks, L]
    out = torch.matmul(w.reshape(w.shape[0], -1).long(), cols)
    return out.reshape(n, w.shape[0], ho, wo)


def _dgrad_scatter(dy, w, stride, hw):
    """int64: every tap's product scattered to the input position it came from"""
    n, co, ho, wo = dy.shape
    ks = w.shape[-1]
    pad = ks // 2
    buf = torch.zeros(n, w.shape[1], hw[0] + 2 * ks, hw[1] + 2 * ks, dtype=torch.long)
    for r in range(ks):
        for s in range(ks):
            t = torch.einsum('nohw,oi->nihw', dy, w[:, :, r, s])
            buf[:, :, r:r + stride * ho:stride, s:s + stride * wo:stride] += t          # iy + pad = stride oy + r
    return buf[:, :, pad:pad + hw[0], pad:pad + hw[1]]


def _wgrad_unfold(a, dy, ks, stride):
    cols = F.unfold(a.double(), ks, padding=ks // 2, stride=stride).round().long()      # [n, ci ks ks, L]
    g = torch.einsum('nkl,nol->ok', cols, dy.reshape(dy.shape[0], dy.shape[1], -1))
    return g.reshape(dy.shape[1], a.shape[1], ks, ks)


@pytest.mark.parametrize('shape', [(2, 5, 7, 6, 3, 1), (1, 6, 5, 4, 3, 2), (2, 7, 4, 5, 1, 1), (1, 1, 9, 3, 3, 1), (1, 8, 8, 3, 3, 2)])
def test_references_equal_independent_integer_formulations(shape):
    n, h, w_, ci, ks, stride = shape
    co = 5
    rng = np.random.default_rng(11 + h + ks + stride)
    a, w = _ints(rng, (n, ci, h, w_)), _ints(rng, (co, ci, ks, ks))
    ho, wo = R.out_hw(h, w_, ks, stride)
    dy = _ints(rng, (n, co, ho, wo))
    assert torch.equal(R.conv(a.double(), w.double(), stride).long(), _conv_unfold(a, w, stride))
    want = _dgrad_scatter(dy, w, stride, (h, w_))
    assert torch.equal(R.dgrad(dy.double(), w.double(), stride, (h, w_)).long(), want)
    if stride == 2:
        # the zero-stuffed form, through the int64 im2col with the flipped, transposed kernel
        assert torch.equal(R.dgrad_zero_stuffed(dy.double(), w.double(), (h, w_)).long(), want)
        z = torch.zeros(n, co, h, w_, dtype=torch.long)
        z[:, :, ::2, ::2] = dy
        assert torch.equal(_conv_unfold(z, w.flip(2, 3).transpose(0, 1).contiguous(), 1), want)
    assert torch.equal(R.wgrad(a.double(), dy.double(), ks, stride).long(), _wgrad_unfold(a, dy, ks, stride))


@pytest.mark.parametrize('ks', [3, 1])
@pytest.mark.parametrize('combo', R.COMBOS)
def test_fused_backward_formula_equals_autograd(ks, combo):
    """the formula of tests/test_bwd_fused_gpu.py's reference, written out: autograd of conv(a, w) under g, the addend,
    the mask [a > 0], the two row sums"""
    affine, use_add, mask, use_coef, use_rows = combo
    case = R.FusedCase(2, 6, 5, 8, 16, ks, affine, use_add, mask, use_coef, use_rows)
    for dtype in R.DTYPES:
        d = R.fused_data(case, dtype, True)
        a = d['a'].clone().requires_grad_(True)
        w = d['w'].clone().requires_grad_(True)
        F.conv2d(a, w, None, padding=ks // 2).backward(d['g'])
        v = a.grad.clone()
        if use_add:
            v = v + d['addend']
        if mask:
            v = v * (d['a'] > 0)
        assert torch.equal(v, d['dx']) and torch.equal(w.grad, d['gw'])
        assert torch.equal(v.sum((0, 2, 3)), d['rows'][0])
        if use_rows:
            assert torch.equal((v * d['bsy']).sum((0, 2, 3)), d['rows'][1])
        if use_coef:
            cA, cB, cC = d['coef']
            assert torch.equal(d['g'], R.bc(cA) * d['dz'] + R.bc(cB) * d['y'] + R.bc(cC))
            assert set(cA.abs().tolist()) <= {1.0, 2.0} and set(cB.tolist()) <= {-1.0, 0.0, 1.0} and R.is_integer(cC)


def test_kflat_layout_of_the_stem_gradient():
    g = torch.arange(2 * 27, dtype=torch.float64).reshape(2, 27)
    o = R.kflat_to_oihw(g, 3, 3)
    for co, ci, r, s in ((0, 0, 0, 0), (1, 2, 1, 0), (1, 1, 2, 2)):
        assert o[co, ci, r, s] == g[co, (r * 3 + s) * 3 + ci]


def test_rounding_helpers():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 3 * 2.0 ** -8, 255.0, 257.0], dtype=torch.float64)
    assert R.q(t, 'bf16').tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, -1.0 - 2.0 ** -6, 255.0, 256.0]      # ties to even
    assert R.bf16_truncate(t).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -7, -1.0 - 2.0 ** -7, 255.0, 256.0]
    assert R.exact_in_f32(torch.tensor([1.0 + 2.0 ** -23], dtype=torch.float64))
    assert not R.exact_in_f32(torch.tensor([1.0 + 2.0 ** -24], dtype=torch.float64))


# ---- the conditions of every case ---------------------------------------------------------------------------------
def _conv_cases(dtype):
    cases = list(R.CONV_CASES) + [R.MIN_CIN_CASES[dtype]]
    if dtype == 'bf16':
        cases += [c for c, _, _ in R.RING_FWD_CASES]
        cases += [R.gemm_case(ch, b, 128 * m + r) for ch in R.GEMM_CHANNELS for b in (0, 1) for m, r in R.GEMM_PIXELS]
    return cases


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_forward_cases_meet_the_lattice_and_exactness_conditions(dtype):
    worst = 0.0
    for case in _conv_cases(dtype):
        f = R.FORMS[case.form]
        d = R.conv_data(case, dtype, True)
        R.lattice_conditions(d, dtype)
        worst = max(worst, float(d['S'].max()))
        assert torch.equal(d['ref'], d['ref'].round())
        assert float(d['x'][:, case.cin_real:].abs().sum()) == 0 and float(d['w'][case.cout_real:].abs().sum()) == 0
        if f['relu']:
            pre = d['x'] * R.bc(d['sc']) + R.bc(d['sh'])
            assert bool((pre[:, :case.cin_real] == 0).any()), case      # exact zeros in front of the ReLU
            assert set(d['sc'].tolist()) <= {-1.0, 1.0} and R.is_integer(d['sh'])
        if dtype == 'bf16':
            assert torch.equal(R.q(d['ref'], 'bf16'), d['ref'])          # every result is a bf16 value
        if dtype == 'bf16' and f['affine'] and case.N <= 8:
            r = R.conv_data(case, dtype, False)
            R.exactness_conditions(r['x'][:, :case.cin_real], r['sc'][:case.cin_real], r['sh'][:case.cin_real])
    print('{}: largest sum |a||w| + |bias| + |prior| over the forward cases {}'.format(dtype, worst))


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_residual_sum_cases_meet_the_conditions(dtype):
    for case in list(R.SUM_CASES) + [c for c, _ in R.RING_SUM_CASES]:
        d = R.sum_data(case, dtype, True)
        R.lattice_conditions(d, dtype, zeros_of=('t',))
        assert torch.equal(F.relu(d['t']), d['a'])
        if dtype == 'bf16' and case.N <= 8:
            r = R.sum_data(case, dtype, False)
            R.exactness_conditions(r['x'], r['sc'], r['sh'], r['x2'])
            assert torch.equal(R.q(F.relu(r['t']), 'bf16'), r['a'])


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_input_gradient_cases_meet_the_conditions(dtype):
    cases = list(R.DGRAD_CASES) + ([c for c, _, _ in R.RING_DGRAD_CASES] if dtype == 'bf16' else [])
    for case in cases:
        d = R.dgrad_data(case, dtype, True)
        R.lattice_conditions(d, dtype, zeros_of=('m',) if 'm' in d else ())
        if 'bs_mask' in d:
            m = d['bs_mask']
            neg0 = (m == 0) & torch.signbit(m)
            assert bool(neg0.any()) and bool(((m == 0) & ~torch.signbit(m)).any())     # -0 and +0: neither is > 0
        if case.form.endswith('+m') and 'm' in d:
            assert bool(((d['m'] == 0) & (d['v'] != 0)).any()), case    # a decision at 0 that shows in the stored value


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_weight_gradient_cases_meet_the_conditions(dtype):
    for case in R.WGRAD_CASES:
        d = R.wgrad_data(case, dtype, True)
        R.lattice_conditions(d, 'f32')
        assert d['ref'].shape == (case.cout_real, case.cin_real, case.ks, case.ks)
        if case.affine:
            pre = d['x'] * R.bc(d['sc']) + R.bc(d['sh'])
            assert bool((pre[:, :case.cin_real] == 0).any())
            if dtype == 'bf16' and case.N <= 8:
                r = R.wgrad_data(case, dtype, False)
                R.exactness_conditions(r['x'][:, :case.cin_real], r['sc'][:case.cin_real], r['sh'][:case.cin_real])


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_fused_backward_cases_meet_the_conditions(dtype):
    for case in list(R.FUSED_CASES) + (list(R.PW_CASES) if dtype == 'bf16' else []):
        if dtype == 'f32' and case.cout > 32:
            continue                                   # (the f32 instantiation serves Cout <= 32)
        d = R.fused_data(case, dtype, True)
        R.lattice_conditions(d, dtype, zeros_of=('a', 'dz'))
        assert float(d['rows'].abs().max()) < R.F32_EXACT
        if case.mask:
            assert bool(((d['a'] == 0) & (R.dgrad(d['g'], d['w'], 1, (case.H, case.W)) != 0)).any()), case
        if dtype == 'bf16':
            assert torch.equal(R.q(d['dx'], 'bf16'), d['dx']) and torch.equal(R.q(d['g'], 'bf16'), d['g'])
            if case.affine and case.N <= 8:
                r = R.fused_data(case, dtype, False)
                R.exactness_conditions(r['x'], r['sc'], r['sh'])
                assert r['coef'] is None                # the bf16 real-valued runs leave the coefficients to the lattice


# ---- sensitivity: what each check sees -------------------------------------------------------------------------------
def _ratio(mut, ref, bound):
    err = (mut - ref).abs()
    return float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())


SENS_CONV = (R.cc(1, 9, 7, 256, 32, 3, 1, 'fwd'), R.cc(1, 9, 7, 64, 32, 1, 1, 'fwdb'), R.cc(1, 9, 7, 40, 32, 3, 2, 'gen_acc'))


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('case', SENS_CONV)
def test_one_lost_product_breaks_both_checks_forward(dtype, case):
    """K = 2304 here: one product of sum |a||w| ~ 150 is 0.7 % of an element, under 3e-2 of the largest output, and it
    still changes the lattice bits and exceeds the bound by far more than 2"""
    lat = R.conv_data(case, dtype, True)
    mut, at = R.lose_one_product(lat['ref'] - (0 if lat['prior'] is None else lat['prior']), lat['a'], lat['w'], case.stride)
    assert mut[at] != (lat['ref'] - (0 if lat['prior'] is None else lat['prior']))[at]
    real = R.conv_data(case, dtype, False)
    base = real['ref'] - (0 if real['prior'] is None else real['prior']) - (0 if real['bias'] is None else R.bc(real['bias']))
    mut, at = R.lose_one_product(base, real['a'], real['w'], case.stride)
    r = float((mut[at] - base[at]).abs() / real['bound'][at])
    print(case, dtype, 'one lost product / bound', r)
    assert r >= 2.0


@pytest.mark.parametrize('case', SENS_CONV)
def test_truncated_store_exceeds_the_bound_but_never_twice(case):
    """Truncation instead of round-to-nearest-even on the bf16 store. In reals the error of an element is below one
    bf16 ulp, at most 2 v |ref|, against a bound of v |ref| + (1 + v) x the contraction bound: it exceeds the bound on
    some elements (the share is printed; it falls as K grows and the contraction term with it) - the GPU test, which
    asserts ratio <= 1 everywhere, fails - but never by a factor of 2, so that factor is not asserted here. On the lattice every result is a bf16 value by construction, so a wrong rounding of the STORE is
    invisible there; the lattice sees a wrong rounding only where it loses a product. Truncation is the real-valued
    check's to catch."""
    real = R.conv_data(case, 'bf16', False)
    mut = R.bf16_truncate(real['ref'])
    err = (mut - real['ref']).abs()
    over = float((err > real['bound']).double().mean())
    worst = _ratio(mut, real['ref'], real['bound'])
    print(case, 'truncated store: share of elements over the bound {:.2f}, worst ratio {:.2f}'.format(over, worst))
    assert over > 0 and 1.0 < worst <= 2.0
    # the correctly rounded store stays inside
    assert _ratio(R.q(real['ref'], 'bf16'), real['ref'], real['bound']) <= 1.0
    lat = R.conv_data(case, 'bf16', True)
    assert torch.equal(R.bf16_truncate(lat['ref']), lat['ref'])


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_pad_channel_and_sum_checks(dtype):
    """a pad channel set to 1: reference and bound are exactly 0 there, so any value fails both checks; and the
    residual-sum conv: a lost product, and a wrong `side`"""
    case = R.cc(1, 9, 7, 72, 32, 3, 1, 'fwdb', cout_real=21)
    for lattice in (True, False):
        d = R.conv_data(case, dtype, lattice)
        assert float(d['ref'][:, 21:].abs().max()) == 0 and float(d['S'][:, 21:].abs().max()) == 0
        if not lattice:
            assert float(d['bound'][:, 21:].max()) == 0
    sc = R.SumCase(1, 9, 7, 96, 32, 3)
    lat, real = R.sum_data(sc, dtype, True), R.sum_data(sc, dtype, False)
    mut, at = R.lose_one_product(lat['ref'], lat['a'], lat['w'])
    assert mut[at] != lat['ref'][at]
    mut, at = R.lose_one_product(real['ref'], real['a'], real['w'])
    assert float((mut[at] - real['ref'][at]).abs() / real['bound'][at]) >= 2.0


DG_SENS = (R.DgradCase(1, 9, 7, 32, 256, 3, 1, 'dg', 1), R.DgradCase(1, 9, 7, 32, 64, 3, 2, 'dg', 0),
           R.DgradCase(1, 9, 7, 32, 64, 3, 2, 'zs', 0), R.DgradCase(1, 9, 7, 32, 64, 3, 1, 'bs_bn_relu+m', 1),
           R.DgradCase(1, 9, 7, 32, 64, 1, 1, 'bs_sum_mask+m', 1))


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('case', DG_SENS)
def test_input_gradient_checks_see_a_lost_product_and_a_flipped_mask(dtype, case):
    for lattice in (True, False):
        d = R.dgrad_data(case, dtype, lattice)
        g = F.relu(d['dy']) if case.form == 'zs' else d['dy']
        # one product lost: dy[n, co, oy, ox] * w[co, ci, r, s] taken out of the element it belongs to
        prod = (g[0, :, 0, 0].view(-1, 1) * d['w'][:, :, 1 if case.ks == 3 else 0, 1 if case.ks == 3 else 0]).abs()
        co, ci = divmod(int(prod.argmax()), prod.shape[1])
        delta = float(prod[co, ci])
        assert delta > 0
        if lattice:
            assert delta >= 1                              # the stored integer moves
        elif 'm' not in d or not case.form.endswith('+m') or bool(d['m'][0, ci, 0, 0] > 0):
            assert delta / float(d['bound'][0, ci, 0, 0]) >= 2.0
        if case.form.endswith('+m'):
            # one mask decision at 0 flipped: the element stores v instead of 0
            if lattice:
                at = ((d['m'] == 0) & (d['v'] != 0)).nonzero()[0]
            else:
                at = ((d['m'] <= 0) & (d['v'] != 0)).nonzero()[0]
            at = tuple(int(i) for i in at)
            assert d['ref'][at] == 0 and d['v'][at] != 0
            if not lattice:
                assert float(d['v'][at].abs() / d['bound'][at].clamp_min(1e-300)) >= 2.0


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('case', [R.wc(2, 16, 16, 32, 32, 3, 1, True, 0), R.wc(2, 9, 7, 64, 48, 1, 1, False, 10),
                                  R.wc(3, 8, 8, 96, 32, 1, 1, False, 10, cout_real=21)])
def test_weight_gradient_checks_see_one_lost_pixel(dtype, case):
    for lattice in (True, False):
        d = R.wgrad_data(case, dtype, lattice)
        dy = d['dy'][:, :case.cout_real].clone()
        a = d['a'][:, :case.cin_real]
        oy, ox = dy.shape[2] // 2, dy.shape[3] // 2
        dy[0, :, oy, ox] = 0
        mut = R.wgrad(a, dy, case.ks, case.stride)
        assert not torch.equal(mut, d['ref'])
        if not lattice:
            r = _ratio(mut, d['ref'], d['bound'])
            print(case, dtype, 'one lost pixel / bound', r)
            assert r >= 2.0


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('case', [R.FusedCase(1, 9, 7, 32, 32, 3, True, True, True, True, True),
                                  R.FusedCase(1, 9, 7, 64, 64, 1, True, True, True, True, True)])
def test_fused_backward_checks_see_each_mutation(dtype, case):
    for lattice in (True, False):
        d = R.fused_data(case, dtype, lattice)
        v = R.dgrad(d['g'], d['w'], 1, (case.H, case.W)) + d['addend']
        # a mask decision at a == 0 flipped
        at = tuple(int(i) for i in ((d['a'] == 0) & (v != 0)).nonzero()[0])
        assert d['dx'][at] == 0 and v[at] != 0
        # one pixel lost from the weight gradient
        g = d['g'].clone()
        g[0, :, 4, 3] = 0
        mut_gw = R.wgrad(d['a'], g, case.ks, 1)
        assert not torch.equal(mut_gw, d['gw'])
        # one product lost from a live element of dx; the rows move with it
        live = (d['a'][0] > 0).nonzero()
        ci, iy, ix = (int(i) for i in live[len(live) // 2])
        c = case.ks // 2
        prod = (d['g'][0, :, iy, ix] * d['w'][:, ci, c, c]).abs()
        delta = float(prod.max())
        assert delta > 0
        if lattice:
            assert delta >= 1 and float(d['S_rows'].max()) < R.F32_EXACT
        else:
            assert float(v[at].abs() / d['b_dx'][at].clamp_min(1e-300)) >= 2.0
            assert _ratio(mut_gw, d['gw'], d['b_gw']) >= 2.0
            assert delta / float(d['b_dx'][0, ci, iy, ix]) >= 2.0
            assert delta / float(d['b_rows'][0, ci]) >= 2.0
