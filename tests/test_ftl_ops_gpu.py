"""hrnet_ftl_gather / hrnet_ftl_scatter / hrnet_conv2d_3x3g (csrc/ftl.hip) on the device against float64 CPU references,
within bound(e_ref) = 4 e_ref + 2 * 2^-24 where e_ref is the error of a float32 CPU evaluation of the same thing
(tests/ftl_ref.py). The shapes are the smallest at which the geometry can go wrong: triplets that cross rows (3 x 4), odd
maps (5 x 3, 9 x 9), every parity class of a transposed layer with and without output_padding, channel counts that are no
multiple of the 16-channel pass (20) or of the 16-channel output tile (21), more than one tile per axis (the *_tiles cases
run as strips of 128 consecutive pixels, the others as 8 x 16 tiles), and one shape per tile variant of the dispatch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ftl_ref as R

pytestmark = pytest.mark.gpu

CANARY = 12345.0


def _dev(t):
    return t.to('cuda')


def _nhwc(x, ld, off):
    """NCHW CPU tensor -> NHWC device map of ld channels with x at [off, off + C) and NaN elsewhere (never to be read)"""
    N, C, H, W = x.shape
    m = torch.full((N, H, W, ld), float('nan'), dtype=torch.float32)
    m[..., off:off + C] = x.permute(0, 2, 3, 1)
    return _dev(m.contiguous())


# ---- the transforms -----------------------------------------------------------------------------------------------------
def _transform_ref(x, coef, dtype):
    """x (N, C, P) per-channel pixel rows, coef (N, 12) -> x A + c on triplets, in dtype"""
    N, C, P = x.shape
    t = x.to(dtype).reshape(N, C, P // 3, 3)
    A, c = coef[:, :9].to(dtype).reshape(N, 1, 3, 3), coef[:, 9:].to(dtype).reshape(N, 1, 1, 3)
    return (t @ A + c).reshape(N, C, P)


TRANSFORMS = [  # V, C, (h, w), camera set, B
    (2, 20, (3, 4), 'unit', 2), (3, 48, (4, 3), 'mhp', 1), (4, 20, (6, 6), 'mhp', 2), (4, 48, (3, 4), 'unit', 1),
    (3, 20, (6, 6), 'unit', 3), (2, 48, (4, 3), 'mhp', 2)]


@pytest.mark.parametrize('V,C,hw,kind,B', TRANSFORMS)
def test_gather_and_scatter(V, C, hw, kind, B):
    from hipnet import ftl
    h, w = hw
    rng = np.random.RandomState(7 + V + C + h)
    ext, K = R.cameras(kind, B, V, rng)
    coef_g, coef_s = ftl.affines(_dev(torch.tensor(ext)), torch.tensor(K))
    assert coef_g.is_cuda and coef_g.dtype == torch.float32 and tuple(coef_s.shape) == (B, V, 12)
    x = torch.tensor(rng.standard_normal((B * V, C, h, w)), dtype=torch.float32)
    # gather: out of a slice of a wider input, into slices (wider than C) of a canary-filled map
    ldx, x_off, slice_, y_off = C + 12, 8, C + 4, 4
    ldy = y_off + V * slice_ + 4
    out = torch.full((B, h, w, ldy), CANARY, dtype=torch.float32, device='cuda')
    got = ftl.gather(_nhwc(x, ldx, x_off), coef_g, V, c=C, x_off=x_off, out=out, y_off=y_off, slice=slice_)
    assert got is out
    torch.cuda.synchronize()
    got = out.cpu()
    cg = coef_g.cpu().reshape(B * V, 12)
    ref = _transform_ref(x.reshape(B * V, C, h * w), cg, torch.float64)
    e_ref = R.rel(_transform_ref(x.reshape(B * V, C, h * w), cg, torch.float32), ref)
    written = torch.zeros(ldy, dtype=torch.bool)
    for v in range(V):
        lo = y_off + v * slice_
        written[lo:lo + C] = True
        mine = got[..., lo:lo + C].permute(0, 3, 1, 2).reshape(B, C, h * w)
        want = ref.reshape(B, V, C, h * w)[:, v]
        err = R.rel(mine, want, denom=float(ref.abs().max()))
        print('gather V {} C {} {}x{} {} view {}: err {:.2e} e_ref {:.2e}'.format(V, C, h, w, kind, v, err, e_ref))
        assert err <= R.bound(e_ref)
    assert bool((got[..., ~written] == CANARY).all())
    # the default layout: slices of C, a new map
    plain = ftl.gather(_nhwc(x, C, 0), coef_g, V).cpu()
    assert tuple(plain.shape) == (B, h, w, V * C)
    assert torch.equal(plain.reshape(B, h, w, V, C), torch.stack([got[..., y_off + v * slice_:y_off + v * slice_ + C]
                                                                  for v in range(V)], 3))

    # scatter: one fused map per frame to every view, slot b V + v
    f = torch.tensor(rng.standard_normal((B, C, h, w)), dtype=torch.float32)
    ldf, f_off, ldo, o_off = C + 8, 4, C + 16, 8
    out = torch.full((B * V, h, w, ldo), CANARY, dtype=torch.float32, device='cuda')
    ftl.scatter(_nhwc(f, ldf, f_off), coef_s, V, c=C, f_off=f_off, out=out, y_off=o_off)
    torch.cuda.synchronize()
    got = out.cpu()
    cs = coef_s.cpu().reshape(B * V, 12)
    fr = f.reshape(B, 1, C, h * w).expand(B, V, C, h * w).reshape(B * V, C, h * w)
    ref = _transform_ref(fr, cs, torch.float64)
    e_ref = R.rel(_transform_ref(fr, cs, torch.float32), ref)
    mine = got[..., o_off:o_off + C].permute(0, 3, 1, 2).reshape(B * V, C, h * w)
    err = R.rel(mine, ref)
    print('scatter V {} C {} {}x{} {}: err {:.2e} e_ref {:.2e}'.format(V, C, h, w, kind, err, e_ref))
    assert err <= R.bound(e_ref)
    assert bool((got[..., :o_off] == CANARY).all()) and bool((got[..., o_off + C:] == CANARY).all())
    assert torch.equal(ftl.scatter(_nhwc(f, C, 0), coef_s, V).cpu(), got[..., o_off:o_off + C])


def test_transform_refusals():
    from hipnet import ftl
    z = lambda *s: torch.zeros(*s, device='cuda')
    coef = z(1, 3, 12)
    with pytest.raises(ValueError, match='triplets'):
        ftl.gather(z(3, 4, 4, 20), coef, 3)
    with pytest.raises(ValueError, match='triplets'):
        ftl.scatter(z(1, 2, 2, 20), coef, 3)
    with pytest.raises(ValueError, match='multiples of 4'):
        ftl.gather(z(3, 3, 4, 18), coef, 3)
    with pytest.raises(ValueError, match='multiples of 4'):
        ftl.gather(z(3, 3, 4, 24), coef, 3, c=20, x_off=2)
    with pytest.raises(ValueError, match='do not lie'):
        ftl.gather(z(3, 3, 4, 20), coef, 3, out=z(1, 3, 4, 56))
    with pytest.raises(ValueError, match='coef'):
        ftl.gather(z(4, 3, 4, 20), coef, 2)
    with pytest.raises(ValueError, match='maps for V'):
        ftl.gather(z(4, 3, 4, 20), coef, 3)
    with pytest.raises(NotImplementedError, match='inference only'):
        ftl.gather(z(3, 3, 4, 20).requires_grad_(), coef, 3)
    # the C entry's own checks, through the raw launchers
    with pytest.raises(RuntimeError, match='triplets'):
        ftl.gather_raw(z(3, 4, 4, 20), coef, z(1, 4, 4, 60), 1, 3, 20, 0, 0, 20)
    with pytest.raises(RuntimeError, match='outside ld'):
        ftl.scatter_raw(z(1, 3, 4, 20), coef, z(3, 3, 4, 20), 1, 3, 20, 0, 4)


# ---- the convolution ----------------------------------------------------------------------------------------------------
# name -> (N, H, W, Cin, Cout, kind, bias, relu, into a slice); kind 's2' = Conv2d(3, 2, 2), 's1' = Conv2d(3, 1, 1),
# 't0' / 't1' = ConvTranspose2d(3, 2, 2, output_padding 0 / 1)
CONVS = {
    's2_4x8': (2, 4, 8, 20, 21, 's2', True, True, False), 's2_5x3': (1, 5, 3, 96, 48, 's2', False, False, True),
    's2_9x9': (2, 9, 9, 20, 48, 's2', True, False, True), 's2_tiles': (1, 40, 36, 20, 21, 's2', True, True, False),
    't0_3x4': (2, 3, 4, 96, 21, 't0', True, True, True), 't0_6x6': (1, 6, 6, 20, 48, 't0', False, True, False),
    't1_3x4': (1, 3, 4, 20, 21, 't1', True, False, False), 't1_9x9': (2, 9, 9, 96, 48, 't1', True, True, True),
    't1_tiles': (1, 18, 20, 20, 21, 't1', False, True, False), 's1_5x7': (3, 5, 7, 20, 21, 's1', True, True, True),
    's1_tiles': (1, 20, 40, 96, 48, 's1', True, False, False),
    # one shape per tile variant of the dispatch: 64 output channels per workgroup (512 pixel-tile x channel blocks), 32
    'wide64': (8, 64, 64, 4, 128, 's1', True, True, False), 'wide32': (4, 64, 64, 8, 48, 's1', False, False, False),
}
GEOMETRY = {'s2': (2, 2, 1), 's1': (1, 1, 1), 't0': (1, 0, 2), 't1': (1, 0, 2)}


def _conv_inputs(name):
    N, H, W, cin, cout, kind, bias, relu, sliced = CONVS[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    x = torch.tensor(rng.standard_normal((N, cin, H, W)), dtype=torch.float32)
    shape = (cin, cout, 3, 3) if kind[0] == 't' else (cout, cin, 3, 3)
    w = torch.tensor(rng.standard_normal(shape) * (2.0 / (9 * cin)) ** 0.5, dtype=torch.float32)
    b = torch.tensor(rng.standard_normal(cout) * 0.5, dtype=torch.float32) if bias else None
    return x, w, b


def _conv_ref(name, x, w, b, dtype):
    kind, relu = CONVS[name][5], CONVS[name][7]
    x, w, b = x.to(dtype), w.to(dtype), None if b is None else b.to(dtype)
    if kind == 's2':
        y = F.conv2d(x, w, b, stride=2, padding=2)
    elif kind == 's1':
        y = F.conv2d(x, w, b, padding=1)
    else:
        y = F.conv_transpose2d(x, w, b, stride=2, padding=2, output_padding=int(kind[1]))
    return F.relu(y) if relu else y


_REFS = {}


def _reference(name):
    """(inputs, float64 reference, e_ref), computed once per case"""
    if name not in _REFS:
        x, w, b = _conv_inputs(name)
        y64 = _conv_ref(name, x, w, b, torch.float64)
        _REFS[name] = ((x, w, b), y64, R.rel(_conv_ref(name, x, w, b, torch.float32), y64))
    return _REFS[name]


def _conv_device(name, x, w, b):
    from hipnet import conv_kxk, ftl, nhwc
    _, H, W, cin, cout, kind, bias, relu, sliced = CONVS[name]
    N = x.shape[0]
    stride, pad_lo, z = GEOMETRY[kind]
    if kind[0] == 't':
        packed = nhwc.conv_transpose_pack(_dev(w))
        Ho, Wo = (ftl.out_size(n, 1, 0, 2, int(kind[1])) for n in (H, W))
    else:
        packed = conv_kxk.pack(_dev(w))
        Ho, Wo = ftl.out_size(H, stride, pad_lo), ftl.out_size(W, stride, pad_lo)
    ldx, x_off = (cin + 8, 4) if sliced else (cin, 0)
    xd = _nhwc(x, ldx, x_off)
    bd = None if b is None else _dev(b)
    if sliced:
        ldy, y_off = cout + 7, 3
        out = torch.full((N, Ho, Wo, ldy), CANARY, dtype=torch.float32, device='cuda')
        got = ftl.conv3x3g(xd, packed, cout, stride, pad_lo, z, bias=bd, relu=relu, cin=cin, x_off=x_off, out=out, y_off=y_off)
        assert got is out
        torch.cuda.synchronize()
        got = got.cpu()
        assert bool((got[..., :y_off] == CANARY).all()) and bool((got[..., y_off + cout:] == CANARY).all())
        return got[..., y_off:y_off + cout].permute(0, 3, 1, 2)
    got = ftl.conv3x3g(xd, packed, cout, stride, pad_lo, z, out_hw=(Ho, Wo), bias=bd, relu=relu)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (N, Ho, Wo, cout)
    return got.cpu().permute(0, 3, 1, 2)


@pytest.mark.parametrize('name', sorted(CONVS))
def test_conv3x3g(name):
    (x, w, b), y64, e_ref = _reference(name)
    got = _conv_device(name, x, w, b)
    assert tuple(got.shape) == tuple(y64.shape)
    err = R.rel(got, y64)
    print('conv3x3g {}: {} -> {}, err {:.2e}, e_ref {:.2e}, bound {:.2e}'.format(name, tuple(x.shape), tuple(y64.shape), err,
                                                                                   e_ref, R.bound(e_ref)))
    assert err <= R.bound(e_ref)


@pytest.mark.parametrize('name', ['s2_9x9', 't1_9x9', 's1_5x7', 's2_tiles', 't1_tiles'])
def test_conv3x3g_equal_bits_across_batch_sizes(name):
    """the sum of an output does not depend on the launch geometry: one image alone and the same image among three"""
    (x, w, b), _, _ = _reference(name)
    one = _conv_device(name, x[:1], w, b)
    three = _conv_device(name, torch.cat([x[:1] * 2, x[:1], x[:1] * 0.5]), w, b)
    assert torch.equal(one[0], three[1]) and not torch.equal(one[0], three[0])
    assert torch.equal(_conv_device(name, x[:1], w, b), one)              # and two runs give equal bits


def test_conv3x3g_refusals():
    from hipnet import ftl
    z = lambda *s: torch.zeros(*s, device='cuda')
    x, packed = z(1, 4, 8, 8), z(16 * 9 * 8)
    assert tuple(ftl.conv3x3g(x, packed, 16, 2, 2).shape) == (1, 3, 5, 16)
    for hw in ((4, 5), (1, 5), (3, 6), (3, 3)):                               # 4 x 8 at stride 2, pad_lo 2: 2 .. 3 x 4 .. 5
        with pytest.raises(ValueError, match='give'):
            ftl.conv3x3g(x, packed, 16, 2, 2, out_hw=hw)
    assert tuple(ftl.conv3x3g(x, packed, 16, 2, 2, out_hw=(2, 4)).shape) == (1, 2, 4, 16)
    with pytest.raises(ValueError, match='give'):
        ftl.conv3x3g(x, packed, 16, 1, 0, 2, out_hw=(8, 13))                 # transposed 4 x 8: 5 .. 7 x 13 .. 15
    with pytest.raises(ValueError, match='z = 2'):
        ftl.conv3x3g(x, packed, 16, 2, 0, 2)
    with pytest.raises(ValueError, match='pad_lo = 3'):
        ftl.conv3x3g(x, packed, 16, 1, 3)
    with pytest.raises(ValueError, match='multiples of 4'):
        ftl.conv3x3g(z(1, 4, 8, 12), packed, 16, 2, 2, cin=8, x_off=2)
    with pytest.raises(ValueError, match='do not lie'):
        ftl.conv3x3g(x, packed, 16, 2, 2, out=z(1, 3, 5, 20), y_off=8)
    with pytest.raises(ValueError, match='packed weights'):
        ftl.conv3x3g(x, packed, 17, 2, 2)
    with pytest.raises(ValueError, match='bias'):
        ftl.conv3x3g(x, packed, 16, 2, 2, bias=z(15))
    with pytest.raises(NotImplementedError, match='inference only'):
        ftl.conv3x3g(x.clone().requires_grad_(), packed, 16, 2, 2)
    # the C entry's own checks, through the raw launcher
    with pytest.raises(RuntimeError, match='Ho x Wo'):
        ftl.conv(x, packed, None, z(1, 4, 5, 16), 8, 0, 16, 0, 2, 2, 1, False)
    with pytest.raises(RuntimeError, match='multiples of 4'):
        ftl.conv(z(1, 4, 8, 12), packed, None, z(1, 3, 5, 16), 8, 2, 16, 0, 2, 2, 1, False)
