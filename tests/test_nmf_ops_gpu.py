"""The NMF kernels (csrc/nmf.hip through hipnet.nmf) against tests/hamburger_ref.py in float64 on the same float32 inputs:
product, Gram matrix, both updates, the reconstruction and nmf2d with six steps, over shapes (G, D, N, R) that are
multiples of nothing, single rows and columns, R = 512 (a row of T spans eight tiles) and R > D, each in both orientations
of the feature matrix; the halves of a dual tensor (leading dimension, channel offset, batch stride) in NCHW and NHWC, a
pointer that is 4-byte but not 16-byte aligned, a dead pixel, an all-zero map, equal bits on two calls and the refusals.

Every result is held to err <= bound(e_ref) = 4 * e_ref + 2 * 2^-24 with err = max|dev - ref64| / max|ref64| and e_ref the
same measure of the float32 CPU restatement of that one op (of the whole iteration for nmf2d). Each test prints its
figures before it asserts."""
import numpy as np
import pytest
import torch

import hamburger_ref as R

pytestmark = pytest.mark.gpu
# the last shape is beyond the issue's list: 130 matrices make the coefficient update a launch of 260 tiles of 64 x 64, the
# threshold (256) above which the engine takes its 64 x 64 tile; every smaller launch here takes the 32 x 32 one
SHAPES = [(3, 24, 35, 8), (1, 40, 33, 48), (2, 1, 5, 3), (2, 7, 1, 1), (1, 16, 20, 512), (2, 64, 64, 16), (130, 33, 70, 5)]
STEPS = 6
_CACHE = {}


def _data(shape):
    """float32 CPU inputs of one shape, drawn once: X (G, D, N) non-negative with a few exact zeros, normalised bases
    (G, D, R), positive coefficients (G, N, R) whose rows sum to 1"""
    if shape not in _CACHE:
        G, D, N, Rr = shape
        g = torch.Generator().manual_seed(1000 * G + 100 * D + 10 * N + Rr)
        X = torch.relu(torch.randn(G, D, N, generator=g) + 0.3)
        bases = R.normalise(torch.rand(G, D, Rr, generator=g))
        coef = torch.softmax(torch.randn(G, N, Rr, generator=g), dim=-1)
        _CACHE[shape] = dict(X=X, bases=bases, coef=coef)
    return _CACHE[shape]


def _ref(shape, name, fn):
    """fn(X, bases, coef) in float64 and float32 on the CPU, once per (shape, op): (ref64, ref32) as float64 arrays"""
    key = (shape, name)
    if key not in _CACHE:
        d = _data(shape)
        with torch.no_grad():
            _CACHE[key] = tuple(fn(*(d[k].to(t) for k in ('X', 'bases', 'coef'))).double().numpy()
                                for t in (torch.float64, torch.float32))
    return _CACHE[key]


def _dev_x(X, orient):
    """X (G, D, N) on the device with X[d, n] at d * ld + n (orient 0) or n * ld + d (orient 1)"""
    return X.cuda() if orient == 0 else X.transpose(1, 2).contiguous().cuda().transpose(1, 2)


def _hold(label, dev, refs):
    ref64, ref32 = refs
    err, e_ref = R.rel(dev.double().cpu().numpy(), ref64), R.rel(ref32, ref64)
    print('{}: err {:.3g}, e_ref {:.3g}, bound {:.3g}'.format(label, err, e_ref, R.bound(e_ref)))
    assert err <= R.bound(e_ref), label


OPS = {
    'product': lambda X, b, c: R.product(X, b),
    'gram_bases': lambda X, b, c: R.gram(b),
    'gram_coef': lambda X, b, c: R.gram(c),
    'update_coef': lambda X, b, c: R.update_coef(c, b, X),
    'update_bases': lambda X, b, c: R.update_bases(b, c, X),
    'reconstruct': lambda X, b, c: torch.bmm(b, c.transpose(1, 2)),
    'nmf': lambda X, b, c: R.factorise(X, b, STEPS),
}


@pytest.mark.parametrize('orient', [0, 1])
@pytest.mark.parametrize('shape', SHAPES)
def test_single_kernels(shape, orient):
    """measured on the MI355X over the seven shapes, the same in both orientations: err <= 2.7e-7 (product), 3.1e-7 (Gram),
    3.9e-7 (updates), 5.2e-7 (reconstruction; (1, 16, 20, 512): e_ref 3.3e-7, bound 1.4e-6) with e_ref 0 .. 3.3e-7 and
    bounds 1.2e-7 .. 1.4e-6. At (2, 1, 5, 3) product and Gram of the bases are exact (err 0 within a bound of 1.2e-7)"""
    from hipnet import nmf
    d = _data(shape)
    x, b, c = _dev_x(d['X'], orient), d['bases'].cuda(), d['coef'].cuda()
    tag = '{} orient {} '.format(shape, orient)
    _hold(tag + 'product', nmf.product(x, b), _ref(shape, 'product', OPS['product']))
    gb, gc = nmf.gram(b), nmf.gram(c)
    _hold(tag + 'gram_bases', gb, _ref(shape, 'gram_bases', OPS['gram_bases']))
    _hold(tag + 'gram_coef', gc, _ref(shape, 'gram_coef', OPS['gram_coef']))
    # the update kernel on the float32 Gram matrix of the DEVICE: the reference forms its own from the same bases
    _hold(tag + 'update_coef', nmf.update_coef(c, b, x, gb), _ref(shape, 'update_coef', OPS['update_coef']))
    _hold(tag + 'update_bases', nmf.update_bases(b, c, x, gc), _ref(shape, 'update_bases', OPS['update_bases']))
    out = torch.full_like(x, -7.0)
    assert nmf.reconstruct(b, c, out) is out and out.stride() == x.stride()
    _hold(tag + 'reconstruct', out, _ref(shape, 'reconstruct', OPS['reconstruct']))
    torch.cuda.synchronize()


@pytest.mark.parametrize('orient', [0, 1])
@pytest.mark.parametrize('shape', SHAPES)
def test_six_steps(shape, orient):
    """the whole iteration on given bases, six steps: measured err 4.7e-8 .. 7.1e-7 with e_ref 4.7e-8 .. 6.0e-7; closest to
    its bound at (1, 16, 20, 512): err 4.4e-7, e_ref 1.9e-7, bound 8.6e-7. Two runs give equal bits"""
    from hipnet import nmf
    d = _data(shape)
    x, b = _dev_x(d['X'], orient), d['bases'].cuda()
    out = nmf.factorise(x, b, STEPS, torch.empty_like(x))
    again = nmf.factorise(x, b, STEPS, torch.empty_like(x))
    _hold('{} orient {} nmf'.format(shape, orient), out, _ref(shape, 'nmf', OPS['nmf']))
    assert torch.equal(out, again) and bool(torch.isfinite(out).all())
    assert torch.equal(b.cpu(), d['bases']) and torch.equal(x.cpu(), d['X'])          # the inputs keep their bits


def test_split_gram_and_its_scratch():
    """K = 600 rows take three parts through the scratch (measured err 2.2e-7, e_ref 7.0e-7, bound 2.9e-6); scratch smaller
    than the query's answer is refused, not run; equal bits on two calls"""
    from hipnet import nmf
    g = torch.Generator().manual_seed(7)
    a = torch.rand(2, 600, 8, generator=g)
    need = nmf.gram_scratch(2, 600, 8)
    assert need == 2 * 3 * 64
    dev = nmf.gram(a.cuda())
    _hold('split gram', dev, tuple(R.gram(a.to(t)).double().numpy() for t in (torch.float64, torch.float32)))
    out = torch.zeros(2, 8, 8, device='cuda')
    with pytest.raises(RuntimeError, match='scratch'):
        nmf.gram(a.cuda(), out, torch.empty(need - 1, device='cuda'))
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                                  # refused before any launch
    assert torch.equal(nmf.gram(a.cuda(), out, torch.empty(need + 5, device='cuda')), dev)


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('spatial', [True, False])
def test_halves_of_a_dual_tensor(layout, spatial):
    """nmf2d on channels 5 .. 28 of a 31-channel 5x7 map with S = 1 and S = 2, B = 2, read in place and written into the
    same channels of another tensor: a leading dimension larger than the row, a channel offset that breaks 16-byte
    alignment, a batch stride larger than the matrix. The neighbours of the target keep their bits. measured, the same in
    both layouts: err 2.3e-7 .. 5.9e-7 with e_ref 2.3e-7 .. 6.3e-7, bounds 1.0e-6 .. 2.7e-6"""
    from hipnet import nmf
    B, Ct, H, W, c0, ch, Rr = 2, 31, 5, 7, 5, 24, 6
    g = torch.Generator().manual_seed(21 + spatial)
    full = torch.relu(torch.randn(B, Ct, H, W, generator=g) + 0.3)
    wide = full.cuda() if layout == 'nchw' else full.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)
    for S in (1, 2):
        D = ch // S if spatial else H * W
        bases = R.normalise(torch.rand(B * S, D, Rr, generator=g))
        target = torch.full_like(wide, -3.0)
        got = nmf.nmf2d(wide[:, c0:c0 + ch], bases.cuda(), STEPS, spatial, S, out=target[:, c0:c0 + ch])
        assert got.data_ptr() == target[:, c0:c0 + ch].data_ptr()
        refs = tuple(R.nmf2d(full[:, c0:c0 + ch].to(t), bases.to(t), STEPS, spatial, S).double().numpy()
                     for t in (torch.float64, torch.float32))
        _hold('{} spatial {} S {}'.format(layout, spatial, S), target[:, c0:c0 + ch], refs)
        assert bool((target[:, :c0] == -3.0).all()) and bool((target[:, c0 + ch:] == -3.0).all())
        fresh = nmf.nmf2d(wide[:, c0:c0 + ch], bases.cuda(), STEPS, spatial, S)         # a new NCHW tensor
        assert fresh.is_contiguous() and torch.equal(fresh, target[:, c0:c0 + ch])


def _misaligned(t):
    """the same values at a device address that is a multiple of 4 but not of 16"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device='cuda')
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize('orient', [0, 1])
def test_misaligned_pointers(orient):
    """every operand 4 bytes past a 16-byte boundary, sizes that are multiples of 4 (the vector path would be taken were
    the pointers aligned): the element-wise loads give the aligned call's bits (update_coef: err 2.9e-7, bound 1.3e-6)"""
    from hipnet import nmf
    shape = (2, 64, 64, 16)
    d = _data(shape)
    x, b, c = _dev_x(d['X'], orient), d['bases'].cuda(), d['coef'].cuda()
    xm = _misaligned(x if orient == 0 else x.transpose(1, 2))
    xm = xm if orient == 0 else xm.transpose(1, 2)
    bm, cm = _misaligned(b), _misaligned(c)
    gb = nmf.gram(b)
    assert torch.equal(nmf.gram(bm), gb)
    gbm = _misaligned(gb)
    assert torch.equal(nmf.product(xm, bm), nmf.product(x, b))
    want = nmf.update_coef(c, b, x, gb)
    assert torch.equal(nmf.update_coef(cm, bm, xm, gbm, out=_misaligned(torch.zeros_like(c))), want)
    _hold('misaligned update_coef', want, _ref(shape, 'update_coef', OPS['update_coef']))
    gc = nmf.gram(c)
    assert torch.equal(nmf.update_bases(bm, cm, xm, _misaligned(gc)), nmf.update_bases(b, c, x, gc))
    out, outm = torch.empty_like(x), torch.empty_like(xm)
    assert outm.stride() == xm.stride()
    assert torch.equal(nmf.reconstruct(bm, cm, outm), nmf.reconstruct(b, c, out))
    assert torch.equal(nmf.factorise(xm, bm, STEPS, outm), nmf.factorise(x, b, STEPS, out))


@pytest.mark.parametrize('orient', [0, 1])
def test_dead_pixel_and_all_zero_map(orient):
    """an all-zero column of X (a dead pixel after the ReLU) leaves its coefficient row exactly 0 and everything finite; an
    all-zero X gives an all-zero, finite result (six steps with the dead pixels: err 3.1e-7, e_ref 3.2e-7, bound 1.4e-6)"""
    from hipnet import nmf
    shape = (3, 24, 35, 8)
    d = _data(shape)
    X = d['X'].clone()
    X[:, :, 11] = 0.0
    X[1, :, 0] = 0.0
    x, b, c = _dev_x(X, orient), d['bases'].cuda(), d['coef'].cuda()
    coef = nmf.update_coef(c, b, x, nmf.gram(b))
    assert float(coef[:, 11].abs().max()) == 0.0 and float(coef[1, 0].abs().max()) == 0.0
    assert float(coef[0, 0].min()) > 0 and bool(torch.isfinite(coef).all())
    out = nmf.factorise(x, b, STEPS, torch.full_like(x, 9.0))
    assert bool(torch.isfinite(out).all()) and float(out[:, :, 11].abs().max()) == 0.0 and float(out[1, :, 0].abs().max()) == 0.0
    refs = tuple(R.factorise(X.to(t), d['bases'].to(t), STEPS).double().numpy() for t in (torch.float64, torch.float32))
    _hold('dead pixel', out, refs)
    zero = nmf.factorise(torch.zeros_like(x), b, STEPS, torch.full_like(x, 9.0))
    assert bool(torch.isfinite(zero).all()) and float(zero.abs().max()) == 0.0


def test_refusals_on_the_device():
    from hipnet import nmf
    x = torch.rand(2, 8, 6, device='cuda')
    b, c = torch.rand(2, 8, 3, device='cuda'), torch.rand(2, 6, 3, device='cuda')
    with pytest.raises(ValueError, match='one of the last two must be 1'):
        nmf.product(torch.rand(2, 8, 12, device='cuda')[:, :, ::2], b)
    with pytest.raises(ValueError, match='bases'):
        nmf.product(x, c)
    with pytest.raises(ValueError, match='float32'):
        nmf.gram(b.double())
    with pytest.raises(ValueError, match='out of place'):
        nmf.update_coef(c, b, x, nmf.gram(b), out=c)
    with pytest.raises(ValueError, match='S = 3'):
        nmf.nmf2d(torch.rand(1, 8, 2, 3, device='cuda'), b[:1], 1, True, 3)
    with pytest.raises(ValueError, match='steps'):
        nmf.nmf2d(torch.rand(2, 8, 2, 3, device='cuda'), b, -1, True, 1)
    with pytest.raises(NotImplementedError, match='backward is not built'):
        nmf.gram(b.clone().requires_grad_(True))
    with torch.no_grad():
        assert tuple(nmf.gram(b.clone().requires_grad_(True)).shape) == (2, 3, 3)
    assert np.isfinite(float(nmf.softmax_rows(c).sum()))
