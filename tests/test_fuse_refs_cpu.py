"""tests/fuse_refs.py on the CPU: every reference against an independent statement of the same operation (torch
float64 interpolate, avg_pool, batch_norm and autograd), the exactness the lattice inputs claim, the share of elements
the real-valued cases leave out, the one-pixel share against the bound of every reduction case, the batch sums'
variance, and the chain lengths D against a direct count."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fuse_refs as R
import glue_refs as G

DTS = ['f32', 'bf16']


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _nchw(a):
    return _t(a).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def test_up_and_pool_are_nearest_interpolation_and_its_transpose():
    x = G.real((2, 3, 5, 4), 1).astype(np.float64)
    for sh in (0, 1, 2, 3):
        f = 1 << sh
        want = F.interpolate(_nchw(x), scale_factor=f, mode='nearest') if sh else _nchw(x)
        assert np.array_equal(R.up(x, sh), _nhwc(want))
        g = G.real((2, 3 * f, 5 * f, 4), 2, sh).astype(np.float64)
        want = F.avg_pool2d(_nchw(g), f) * (f * f)
        assert np.abs(R.pool(g, sh) - _nhwc(want)).max() <= 1e-12
        assert abs((R.up(x, sh) * g).sum() - (x * R.pool(g, sh)).sum()) <= 1e-9


def test_sum_terms_reference_is_torch_float64():
    N, H, W, C = 2, 8, 16, 8
    terms = []
    for k, (sh, affine, relu) in enumerate([(0, False, False), (1, True, True), (3, True, False), (2, False, True)]):
        t = dict(src=G.real((N, H >> sh, W >> sh, C), 3, k), sh=sh, scale=None, shift=None, relu=relu)
        if affine:
            t.update(scale=G.real((C,), 3, k, 1), shift=G.real((C,), 3, k, 2))
        terms.append(t)
    for relu_out in (0, 1):
        want = 0
        for t in terms:
            v = _nchw(t['src'])
            if t['scale'] is not None:
                v = v * _t(t['scale']).view(1, -1, 1, 1) + _t(t['shift']).view(1, -1, 1, 1)
            if t['relu']:
                v = torch.relu(v)
            want = want + (F.interpolate(v, size=(H, W), mode='nearest') if t['sh'] else v)
        if relu_out:
            want = torch.relu(want)
        ref, tot, n = R.sum_terms(terms, relu_out)
        assert np.abs(ref - _nhwc(want)).max() <= 1e-13 and n == 4
        assert (tot >= np.abs(ref) - 1e-12).all()


def test_bn_from_sums_reference_is_torch_batch_norm():
    C, n = 6, 64
    x = G.real((n, C), 4).astype(np.float64) * 0.7 - 1.3
    sums = np.zeros((R.COPIES, 2, C))
    for k in range(R.COPIES):
        part = x[k * 8:(k + 1) * 8]
        sums[k, 0], sums[k, 1] = part.sum(axis=0), (part * part).sum(axis=0)
    gamma, beta = G.real((C,), 5).astype(np.float64), G.real((C,), 6).astype(np.float64)
    scale, shift, mean, var = R.bn_from_sums(sums, 1.0 / n, 1e-3, gamma, beta)
    want = F.batch_norm(_t(x), None, None, _t(gamma), _t(beta), True, 0.0, 1e-3).numpy()
    assert np.abs(x * scale + shift - want).max() <= 1e-12
    assert np.abs(mean - x.mean(axis=0)).max() <= 1e-13 and np.abs(var - x.var(axis=0)).max() <= 1e-12
    s32 = R.bn_from_sums(sums, 1.0 / n, 1e-3, gamma, beta, np.float32)
    assert all(v.dtype == np.float32 for v in s32)


@pytest.mark.parametrize('sh', [0, 1, 3])
@pytest.mark.parametrize('inner_relu,with_scale', [(0, False), (1, True), (1, False)])
def test_dz_reference_is_float64_autograd(sh, inner_relu, with_scale):
    inp = R.grad_inputs((2, 4, 6, 2), sh, 'f32', False, True, inner_relu, with_scale, 7, sh)
    d, a, near = R.dz(inp['g'], inp['mask'], inp['y'], inp['scale'], inp['shift'], sh, inner_relu)
    z = _nchw(inp['y'])
    if inp['scale'] is not None:
        z = z * _t(inp['scale']).view(1, -1, 1, 1) + _t(inp['shift']).view(1, -1, 1, 1)
    z.requires_grad_(True)
    o = torch.relu(z) if inner_relu else z
    o = F.interpolate(o, scale_factor=1 << sh, mode='nearest') if sh else o
    (o * _nchw(inp['g']) * (_nchw(inp['mask']) > 0)).sum().backward()
    assert np.abs(d - _nhwc(z.grad)).max() <= 1e-12
    assert (a >= np.abs(d) - 1e-12).all()


@pytest.mark.parametrize('sh', [0, 2])
def test_rows_finalize_and_apply_are_float64_autograd_of_batch_norm(sh):
    """row_sums -> finalize -> grad_term is the BatchNorm backward of relu(ident + up(bn(y)))"""
    N, H, W, C, eps = 2, 3, 5, 4, 1e-5
    y = G.real((N, H, W, C), 8, sh).astype(np.float64)
    gamma, beta = G.real((C,), 9).astype(np.float64), G.real((C,), 10).astype(np.float64)
    hi = (N, H << sh, W << sh, C)
    ident, gout = G.real(hi, 11, sh).astype(np.float64), G.real(hi, 12, sh).astype(np.float64)
    yt, gt, bt = _nchw(y).requires_grad_(True), _t(gamma).requires_grad_(True), _t(beta).requires_grad_(True)
    z = F.batch_norm(yt, None, None, gt, bt, True, 0.0, eps)
    z = F.interpolate(z, scale_factor=1 << sh, mode='nearest') if sh else z
    out = torch.relu(_nchw(ident) + z)
    out.backward(_nchw(gout))
    mean, invstd = y.mean(axis=(0, 1, 2)), 1.0 / np.sqrt(y.var(axis=(0, 1, 2)) + eps)
    d, a, _ = R.dz(gout, _nhwc(out), None, None, None, sh, 0)
    s, _ = R.row_sums(d, y)
    rows = np.stack([s * 0.25, s * 0.75])                # two partial rows
    dg, db, coef = R.finalize(rows, N * H * W, gamma, mean, invstd)
    dy, _ = R.grad_term(d, a, y, coef, None)
    assert np.abs(dg - gt.grad.numpy()).max() <= 1e-11 and np.abs(db - bt.grad.numpy()).max() <= 1e-11
    assert np.abs(dy - _nhwc(yt.grad)).max() <= 1e-11
    old = G.real(dy.shape, 13).astype(np.float64)
    assert np.array_equal(R.grad_term(d, a, y, coef, old)[0], dy + old)


@pytest.mark.parametrize('dt', DTS)
def test_lattice_inputs_are_exact_and_hit_zero_and_every_mask_value(dt):
    shape = (2, 4, 6, 12 * R.VEC[dt])
    y, scale, shift = R.relu_lattice(shape, 14)
    coef = R.lattice_coef(shape[-1], 15)
    assert R.on_lattice(y, shift, coef[2], R.lattice(shape, 16)) and R.on_scales(scale, coef[0], coef[1])
    assert G.same_bits(R.np_dtype_round(y, dt), y) and G.same_bits(R.np_dtype_round(R.lattice(shape, 16), dt),
                                                                   R.lattice(shape, 16))
    z = y.astype(np.float64) * scale + shift
    assert 0.10 <= (z == 0).mean() <= 0.16              # an eighth by construction, plus chance
    assert (z > 0).any() and (z < 0).any()
    m = R.mask_tensor(shape, 17)
    stored = R.np_dtype_round(m, dt)
    assert G.same_bits(stored, m)                        # bf16 holds every mask value, the denormal included
    for v in R.MASK_VALUES:
        hit = (m == np.float32(v)) & (np.signbit(m) == np.signbit(np.float32(v)))
        assert 0.08 <= hit.mean() <= 0.21, v
    assert (m[m > 0] >= np.float32(R.DENORMAL)).all() and (m == np.float32(R.DENORMAL)).any()
    assert 0 < np.float32(R.DENORMAL) < np.finfo(np.float32).tiny


@pytest.mark.parametrize('dt', DTS)
def test_lattice_results_are_float32_in_any_order(dt):
    """every lattice case of the GPU tests meets lattice_exact; on one of them the float32 sums in two shuffled orders
    give the float64 result"""
    for ci, (sh, shape, with_mask, inner_relu, with_scale, with_coef, accumulate) in enumerate(R.grad_configs()):
        inp = R.grad_inputs(shape, sh, dt, True, with_mask, inner_relu, with_scale, 31, ci, 1)
        assert R.on_lattice(inp['g'], inp['y']) and (inp['scale'] is None or R.on_scales(inp['scale']))
        coef = R.lattice_coef(shape[3] * R.VEC[dt], 32, ci) if with_coef else None
        acc = R.lattice(inp['y'].shape, 33, ci) if accumulate else None
        d, a, near = R.dz(inp['g'], inp['mask'], inp['y'], inp['scale'], inp['shift'], sh, inner_relu)
        assert near is None or not near.any()            # on the lattice a pre-activation is 0 or far from it
        ref, tot = R.grad_term(d, a, inp['y'], coef, acc)
        assert R.lattice_exact(tot) and G.is_f32(ref)
    for ci, (shape, sh, with_mask, inner_relu) in enumerate(R.reduce_configs()):
        if shape[3] == 256 and sh > 0:
            continue
        inp = R.reduce_inputs(shape, sh, dt, True, with_mask, inner_relu, 61, ci)
        d, a, _ = R.dz(inp['g'], inp['mask'], inp['y'], inp['scale'], inp['shift'], sh, inner_relu)
        s, sa = R.row_sums(d, inp['y'])
        assert R.lattice_exact(a) and R.lattice_exact(sa, 2.0 ** -8) and G.is_f32(s)
    for ci, (shape, specs, relu_out) in enumerate(R.sum_lattice_cases()):
        terms = R.lattice_terms(shape, dt, specs, 11, ci)
        for t in terms:
            assert R.on_lattice(t['src']) and (t['scale'] is None or (R.on_scales(t['scale']) and R.on_lattice(t['shift'])))
            assert G.same_bits(R.np_dtype_round(t['src'], dt), t['src'])
        ref, tot, n = R.sum_terms(terms, relu_out)
        assert R.lattice_exact(tot) and G.is_f32(ref) and n == len(specs)
        for t in terms:                                  # an affine pre-activation is exactly 0 on about an eighth
            if t['scale'] is not None and t['src'].size >= 256:
                assert ((t['src'].astype(np.float64) * t['scale'] + t['shift']) == 0).mean() >= 0.08
    for ci, (shape, levels) in enumerate(R.POOL_CASES):
        for nlev in levels:
            inp = R.pool_inputs(shape, nlev, dt, True, True, 71, ci, nlev)
            assert R.on_lattice(inp['g'], *inp['ys'])
            for l in range(1, nlev + 1):
                d, a, _ = R.dz(inp['g'], inp['mask'], None, None, None, l, 0)
                s, sa = R.row_sums(R.stored_bits(d, dt), inp['ys'][l - 1])
                assert R.lattice_exact(a) and R.lattice_exact(sa, 2.0 ** -8) and G.is_f32(s)
    inp = R.reduce_inputs((3, 5, 7, 12), 3, dt, True, True, 1, 61, 99)
    d, _, _ = R.dz(inp['g'], inp['mask'], inp['y'], inp['scale'], inp['shift'], 3, 1)
    t = np.stack([d, d * inp['y']]).reshape(2, -1, d.shape[-1]).astype(np.float32)
    want, _ = R.row_sums(d, inp['y'])
    for seed in (1, 2):
        order = np.random.RandomState(seed).permutation(t.shape[1])
        acc = np.zeros((2, d.shape[-1]), np.float32)
        for p in order:
            acc = acc + t[:, p]
        assert acc.dtype == np.float32 and np.array_equal(acc.astype(np.float64), want)
    for cv in (12, 2):                                   # the rows-boundary cases: element-wise only
        npix = R.rows_boundary_pixels(cv)
        assert (npix - 1) * cv < R.ROWS_KERNEL_VECTORS <= npix * cv
        rows = 256 // cv                                 # no stride of either kernel is a multiple of the period
        assert all(k % R.BOUNDARY_PERIOD for k in (rows, R.EW_GRID_CAP * rows, R.EW_GRID_CAP * 256, cv, 256))
        tile = R.reduce_inputs((1, 1, R.BOUNDARY_PERIOD, cv), 0, dt, True, True, True, 45, cv)
        coef = R.lattice_coef(cv * R.VEC[dt], 46)
        acc = R.lattice(tile['y'].shape, 47)
        assert R.on_lattice(tile['g'], tile['y'], tile['shift'], acc, coef[2], R.lattice(tile['y'].shape, 48))
        d, a, near = R.dz(tile['g'], tile['mask'], tile['y'], tile['scale'], tile['shift'], 0, 1)
        assert not near.any() and R.lattice_exact(R.grad_term(d, a, tile['y'], coef, acc)[1])


@pytest.mark.parametrize('dt', DTS)
def test_real_valued_cases_leave_out_at_most_a_thousandth(dt):
    worst = 0.0
    for ci, (sh, shape, with_mask, inner_relu, with_scale, with_coef, accumulate) in enumerate(R.grad_configs()):
        inp = R.grad_inputs(shape, sh, dt, False, with_mask, inner_relu, with_scale, 31, ci, 0)
        _, _, near = R.dz(inp['g'], inp['mask'], inp['y'], inp['scale'], inp['shift'], sh, inner_relu)
        if near is not None:
            worst = max(worst, float(near.mean()))
    inp = R.grad_inputs(R.BIG, 1, dt, False, True, 1, True, 41)
    _, _, near = R.dz(inp['g'], inp['mask'], inp['y'], inp['scale'], inp['shift'], 1, 1)
    worst = max(worst, float(near.mean()))
    assert worst <= R.SKIP_CAP, worst
    # the reduction cases sum what they decide: none of their decisions may lie near 0 at all
    for ci, (shape, sh, with_mask, inner_relu) in enumerate(R.reduce_configs()):
        inp = R.reduce_inputs(shape, sh, dt, False, with_mask, inner_relu, 61, ci)
        _, _, near = R.dz(inp['g'], inp['mask'], inp['y'], inp['scale'], inp['shift'], sh, inner_relu)
        assert near is None or not near.any(), (shape, sh)
        if inner_relu and inp['y'].size >= 1000:
            z = inp['y'].astype(np.float64) * inp['scale'] + inp['shift']
            assert 0.2 <= (z > 0).mean() <= 0.8          # the ReLU splits the one-sign data


@pytest.mark.parametrize('dt', DTS)
def test_one_pixel_share_is_at_least_twice_the_bound(dt):
    vec = R.VEC[dt]
    for ci, (shape, sh, with_mask, inner_relu) in enumerate(R.reduce_configs()):
        N, H, W, cv = shape
        inp = R.reduce_inputs(shape, sh, dt, False, with_mask, inner_relu, 61, ci)
        d, a, _ = R.dz(inp['g'], inp['mask'], inp['y'], inp['scale'], inp['shift'], sh, inner_relu)
        _, sa = R.row_sums(d, inp['y'])
        share = np.abs(inp['g']).min()
        assert share >= 1 and np.abs(inp['y']).min() >= 1
        D = R.reduce_D(N * H * W, cv * vec, vec, sh)
        assert R.share_ok(D, sa, [[share], [share * np.abs(inp['y']).min()]]), (shape, sh, D)
    for shape, levels in R.POOL_CASES:
        N, H, W, cv = shape
        n1 = N * (H >> 1) * (W >> 1)
        for nlev in levels:
            for l in range(1, nlev + 1):                 # the largest sums the inputs can give: 1.25 per pixel and y
                sa = np.array([[N * H * W * 1.25], [N * H * W * 1.25 * 1.25]])
                assert R.share_ok(R.pool_D(n1, cv * vec, vec, nlev, l), sa, [[1.0], [1.0]]), (shape, nlev, l)
    # a dropped pixel fails: the error it leaves is at least twice the bound
    g = R.one_sign((3, 5, 7, 12 * vec), dt, 18)
    y = R.one_sign((3, 5, 7, 12 * vec), dt, 19)
    s, sa = R.row_sums(g, y)
    dropped = g.astype(np.float64).copy()
    dropped[1, 2, 3] = 0
    err = np.abs(R.row_sums(dropped, y)[0] - s)
    assert (err >= 2 * R.rows_bound(R.reduce_D(105, 12 * vec, vec, 0), sa)).all()


def test_batch_sums_have_no_cancellation_and_a_clamped_channel():
    for C in (48, 96, 16, R.SUM_MAXC):
        for key in range(4):
            sums, gamma, beta, inv, eps, clamp = R.sums_case(C, 17, C, key)
            assert eps != 1e-5 and clamp.any() and not clamp.all()
            for dt in (np.float64, np.float32):
                s = sums.astype(dt)
                m = s[:, 0].sum(axis=0, dtype=dt) * dt(inv)
                v = s[:, 1].sum(axis=0, dtype=dt) * dt(inv) - m * m
                assert (v[clamp] < 0).all(), dt          # slightly negative in both precisions: the clamp acts
                assert (v[~clamp] >= m[~clamp] ** 2 / 4).all(), dt
                assert (R.bn_from_sums(sums, inv, eps, gamma, beta, dt)[3][clamp] == 0).all()
            sc, sf, dsc, dsf, e_sc, e_sf = R.sums_allowance(sums, inv, eps, gamma, beta)
            # about seven roundings ahead of the variance, amplified by (E x^2 + mean^2) / var <= 9, not more
            assert e_sc <= 64 * R.U and e_sf <= 64 * R.U
            assert (sc > 0).all() and (sf > 0).all()
            assert np.array_equal(sc[clamp], gamma[clamp].astype(np.float64) / np.sqrt(eps))


def test_chain_lengths_match_a_direct_count():
    for npix, C, vec, sh in ((105, 48, 4, 3), (128, 8, 8, 1), (768, 96, 8, 0), (128, 1024, 4, 0)):
        blocks, rows = R.reduce_geometry(npix, C, vec)
        assert R.reduce_D(npix, C, vec, sh) == R.longest_walk(npix, blocks, rows) * (1 << sh) ** 2 + rows
    for n1, C, vec, nlev in ((192, 48, 4, 3), (16, 32, 4, 2)):
        blocks, rows = R.pool_geometry(n1, C, vec, nlev)
        steps = max(len(range(b * rows, n1, blocks * rows)) for b in range(blocks))
        for l in range(1, nlev + 1):
            assert R.pool_D(n1, C, vec, nlev, l) == steps * 4 + 4 * (l - 1) + rows
    assert R.reduce_geometry(128, 4, 4) == (2, 256)      # the second workgroup has no pixel
    assert R.reduce_geometry(105, 48, 4) == (1, 21) and R.pool_geometry(192, 48, 4, 2) == (3, 20)
    assert R.pool_geometry(192, 48, 4, 3)[1] == 16 and R.pool_geometry(192, 64, 4, 3)[1] == 16
    assert R.ew_blocks(2 * 128 * 128 * 40) == R.EW_GRID_CAP < 2 * 128 * 128 * 40 // 256


def test_finalize_cases_cover_the_loop_ends():
    assert set(R.FIN_BLOCKS) >= {1, 31, 32, 33, 63, 64, 65} and max(R.FIN_BLOCKS) == 2048
    rows, gamma, mean, invstd, count, old = R.finalize_case(33, 48, 0)
    dg, db, coef = R.finalize(rows, count, gamma, mean, invstd)
    s = rows.astype(np.float64).sum(axis=0)
    assert np.allclose(db, s[0]) and np.allclose(dg, invstd * (s[1] - mean * s[0]), rtol=1e-12)
    assert coef.shape == (3, 48) and np.isfinite(coef).all()
