"""hrnet_ftl_gather_bwd / hrnet_ftl_scatter_bwd / hrnet_conv2d_3x3g_wgrad (csrc/ftl_train.hip) and the two data-gradient
identities of hipnet.ftl_train on the device against float64 CPU autograd, within bound(e_ref) = 4 e_ref + 2 * 2^-24 where
e_ref is the error of a float32 CPU evaluation of the same thing (tests/ftl_ref.py). Inputs are float16-valued. The shapes
are the smallest at which the geometry can go wrong: triplets that cross rows, odd maps, channel counts that are no
multiple of the 16-channel blocks (20, 21, 55 real of 56), more than one 8 x 16 pixel tile and so more than one split."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ftl_ref as R
from test_ftl_ops_gpu import TRANSFORMS

pytestmark = pytest.mark.gpu

CANARY = 12345.0


def _dev(t):
    return t.to('cuda')


def _f16(rng, shape, scale=1.0):
    return torch.tensor((rng.standard_normal(shape) * scale).astype(np.float16).astype(np.float32))


def _nhwc(x, ld, off, fill=float('nan')):
    """NCHW CPU tensor -> NHWC device map of ld channels with x at [off, off + C) and `fill` elsewhere"""
    N, C, H, W = x.shape
    m = torch.full((N, H, W, ld), fill, dtype=torch.float32)
    m[..., off:off + C] = x.permute(0, 2, 3, 1)
    return _dev(m.contiguous())


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- the transforms' backward -------------------------------------------------------------------------------------------
def _transform_grad(x, coef, g, dtype):
    """the gradient of sum(g * (x A + c)) in x, by autograd in dtype: x, g (N, C, P), coef (N, 12)"""
    N, C, P = x.shape
    xt = x.to(dtype).clone().requires_grad_()
    A, c = coef[:, :9].to(dtype).reshape(N, 1, 3, 3), coef[:, 9:].to(dtype).reshape(N, 1, 1, 3)
    y = (xt.reshape(N, C, P // 3, 3) @ A + c).reshape(N, C, P)
    (y * g.to(dtype)).sum().backward()
    return xt.grad


@pytest.mark.parametrize('V,C,hw,kind,B', TRANSFORMS)
def test_gather_and_scatter_backward(V, C, hw, kind, B):
    from hipnet import ftl, ftl_train
    h, w = hw
    rng = np.random.RandomState(11 + V + C + h)
    ext, K = R.cameras(kind, B, V, rng)
    coef_g, coef_s = ftl.affines(_dev(torch.tensor(ext)), torch.tensor(K))
    x = _f16(rng, (B * V, C, h * w))
    # gather: the gradient of the concatenated map is a slice of a wider NaN-filled map, view v at d_off + v slice
    g = _f16(rng, (B, V, C, h, w))
    slice_, d_off, x_off = C + 4, 8, 4
    ldd, ldx = d_off + V * slice_ + 4, C + 12
    dcat = torch.full((B, h, w, ldd), float('nan'), dtype=torch.float32)
    for v in range(V):
        dcat[..., d_off + v * slice_:d_off + v * slice_ + C] = g[:, v].permute(0, 2, 3, 1)
    out = torch.full((B * V, h, w, ldx), CANARY, dtype=torch.float32, device='cuda')
    got = ftl_train.gather_bwd(_dev(dcat), coef_g, V, C, d_off=d_off, slice=slice_, out=out, x_off=x_off)
    assert got is out
    torch.cuda.synchronize()
    got = out.cpu()
    cg = coef_g.cpu().reshape(B * V, 12)
    gf = g.reshape(B * V, C, h * w)
    ref = _transform_grad(x, cg, gf, torch.float64)
    e_ref = R.rel(_transform_grad(x, cg, gf, torch.float32), ref)
    mine = got[..., x_off:x_off + C].permute(0, 3, 1, 2).reshape(B * V, C, h * w)
    err = R.rel(mine, ref)
    print('gather_bwd V {} C {} {}x{} {}: err {:.2e} e_ref {:.2e}'.format(V, C, h, w, kind, err, e_ref))
    assert err <= R.bound(e_ref)
    assert bool((got[..., :x_off] == CANARY).all()) and bool((got[..., x_off + C:] == CANARY).all())
    # the default layout: slices of C, a new map
    plain = ftl_train.gather_bwd(_dev(g.permute(0, 3, 4, 1, 2).reshape(B, h, w, V * C).contiguous()), coef_g, V, C).cpu()
    assert tuple(plain.shape) == (B * V, h, w, C) and _same_bits(plain, got[..., x_off:x_off + C].contiguous())

    # scatter: df[b] = sum_v dy[b V + v] A^T, the views in slot order b V + v
    gy = _f16(rng, (B * V, C, h, w))
    ldy, y_off, ldf, f_off = C + 16, 8, C + 8, 4
    out = torch.full((B, h, w, ldf), CANARY, dtype=torch.float32, device='cuda')
    ftl_train.scatter_bwd(_nhwc(gy, ldy, y_off), coef_s, V, c=C, y_off=y_off, out=out, f_off=f_off)
    torch.cuda.synchronize()
    got = out.cpu()
    cs = coef_s.cpu().reshape(B * V, 12)
    per_view = lambda dt: _transform_grad(x, cs, gy.reshape(B * V, C, h * w), dt).reshape(B, V, C, h * w).sum(1)
    ref = per_view(torch.float64)
    e_ref = R.rel(per_view(torch.float32), ref)
    mine = got[..., f_off:f_off + C].permute(0, 3, 1, 2).reshape(B, C, h * w)
    err = R.rel(mine, ref)
    print('scatter_bwd V {} C {} {}x{} {}: err {:.2e} e_ref {:.2e}'.format(V, C, h, w, kind, err, e_ref))
    assert err <= R.bound(e_ref)
    assert bool((got[..., :f_off] == CANARY).all()) and bool((got[..., f_off + C:] == CANARY).all())
    assert _same_bits(ftl_train.scatter_bwd(_nhwc(gy, C, 0), coef_s, V).cpu(), got[..., f_off:f_off + C].contiguous())


def test_transform_backward_refusals():
    from hipnet import ftl_train
    z = lambda *s: torch.zeros(*s, device='cuda')
    coef = z(1, 3, 12)
    out = torch.full((3, 3, 4, 20), CANARY, device='cuda')
    with pytest.raises(ValueError, match='triplets'):
        ftl_train.gather_bwd(z(1, 4, 4, 60), coef, 3, 20)
    with pytest.raises(ValueError, match='multiples of 4'):
        ftl_train.gather_bwd(z(1, 3, 4, 64), coef, 3, 20, d_off=2, out=out)
    with pytest.raises(ValueError, match='do not lie'):
        ftl_train.gather_bwd(z(1, 3, 4, 56), coef, 3, 20, out=out)
    with pytest.raises(ValueError, match='maps for V'):
        ftl_train.scatter_bwd(z(4, 3, 4, 20), coef, 3)
    with pytest.raises(ValueError, match='coef'):
        ftl_train.scatter_bwd(z(6, 3, 4, 20), coef, 3)
    # the C entry's own checks, through the raw launchers
    with pytest.raises(RuntimeError, match='triplets'):
        ftl_train.gather_bwd_raw(z(1, 4, 4, 60), coef, out, 1, 3, 20, 0, 20, 0)
    with pytest.raises(RuntimeError, match='outside ld'):
        ftl_train.gather_bwd_raw(z(1, 3, 4, 56), coef, out, 1, 3, 20, 0, 20, 0)
    with pytest.raises(RuntimeError, match='outside ld'):
        ftl_train.scatter_bwd_raw(z(3, 3, 4, 20), coef, out, 1, 3, 20, 0, 4)
    with pytest.raises(RuntimeError, match='multiples of 4'):
        ftl_train.scatter_bwd_raw(z(3, 3, 4, 24), coef, out, 1, 3, 20, 2, 0)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())


# ---- the weight gradient ------------------------------------------------------------------------------------------------
# (H, W) -> (Ho, Wo), stride, pad_lo
MAPS = {'s2_4x8': ((4, 8), (3, 5), 2, 2), 's2_5x3': ((5, 3), (4, 3), 2, 2), 's2_16x16': ((16, 16), (9, 9), 2, 2),
        's2_tiles': ((17, 33), (10, 18), 2, 2), 's1_p0': ((5, 9), (3, 7), 1, 0), 's1_p1': ((5, 9), (5, 9), 1, 1),
        's1_p2': ((5, 9), (7, 11), 1, 2)}
CHANNELS = [(20, 20, 21), (48, 48, 16), (56, 55, 32)]     # (Cin slice, Cin_real, Cout)
SENTINEL = -777.0


def _wgrad_ref(x, gy, stride, pad_lo, dtype):
    """dW (Cout, Cin, 3, 3) of sum(gy * conv(x, W)) by autograd: pad_lo in front, whatever Ho needs behind"""
    N, ci, H, W = x.shape
    Ho, Wo = gy.shape[2:]
    ph, pw = (Ho - 1) * stride + 3 - H - pad_lo, (Wo - 1) * stride + 3 - W - pad_lo
    xp = F.pad(x.to(dtype), (pad_lo, max(pw, 0), pad_lo, max(ph, 0)))
    wt = torch.zeros((gy.shape[1], ci, 3, 3), dtype=dtype, requires_grad=True)
    y = F.conv2d(xp, wt, stride=stride)[:, :, :Ho, :Wo]
    (y * gy.to(dtype)).sum().backward()
    return wt.grad


_WREFS = {}


def _wgrad_case(name, chan, N):
    key = (name, chan, N)
    if key not in _WREFS:
        (H, W), (Ho, Wo), stride, pad_lo = MAPS[name]
        cin, real, cout = chan
        rng = np.random.RandomState(sum(map(ord, name)) + cin + cout + N)
        x = _f16(rng, (N, cin, H, W))
        x[:, real:] = 0.5            # the pad channels of the slice are read (finite), and have no gradient
        gy = _f16(rng, (N, cout, Ho, Wo))
        ref = _wgrad_ref(x, gy, stride, pad_lo, torch.float64)
        e_ref = R.rel(_wgrad_ref(x, gy, stride, pad_lo, torch.float32)[:, :real], ref[:, :real])
        _WREFS[key] = (x, gy, ref[:, :real], e_ref)
    return _WREFS[key]


def _run_wgrad(x, gy, real, stride, pad_lo, stream=None):
    """(dW on the CPU, checked for its sentinels); sources at non-zero offsets of NaN-filled maps; dw, the scratch and
    its tail between sentinels"""
    from hipnet import ftl_train
    N, cin, H, W = x.shape
    cout, Ho, Wo = gy.shape[1:]
    xd, gd = _nhwc(x, cin + 12, 8), _nhwc(gy, cout + 7, 3)
    nbytes, nsplit, per = ftl_train.wgrad_plan(N, Ho, Wo, cin, cout)
    tiles = N * -(-Ho // 8) * -(-Wo // 16)
    assert nbytes % 4 == 0 and 1 <= nsplit <= tiles and (nsplit - 1) * per < tiles <= nsplit * per
    n, tail = nbytes // 4, 64
    sbuf = torch.full((8 + n + tail,), SENTINEL, dtype=torch.float32, device='cuda')
    wbuf = torch.full((8 + cout * real * 9 + 8,), SENTINEL, dtype=torch.float32, device='cuda')
    dw = wbuf[8:8 + cout * real * 9].view(cout, real, 3, 3)
    torch.cuda.synchronize()                                   # the fills above, before another stream may run
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        got = ftl_train.conv3x3g_wgrad(xd, gd, cout, stride, pad_lo, cin=cin, cin_real=real, x_off=8, y_off=3,
                                       scratch=sbuf[8:8 + n + tail], dw=dw)
    torch.cuda.synchronize()
    assert got is dw
    s, wb = sbuf.cpu(), wbuf.cpu()
    assert bool((s[:8] == SENTINEL).all()) and bool((s[8 + n:] == SENTINEL).all())
    assert bool((wb[:8] == SENTINEL).all()) and bool((wb[-8:] == SENTINEL).all())
    return dw.cpu().clone(), nsplit


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('chan', CHANNELS, ids=lambda c: 'c{}_{}_{}'.format(*c))
@pytest.mark.parametrize('name', sorted(MAPS))
def test_conv3x3g_wgrad(name, chan, N):
    x, gy, ref, e_ref = _wgrad_case(name, chan, N)
    _, _, stride, pad_lo = MAPS[name]
    got, nsplit = _run_wgrad(x, gy, chan[1], stride, pad_lo)
    err = R.rel(got, ref)
    print('conv3x3g_wgrad {} {} N {}: {} splits, err {:.2e}, e_ref {:.2e}, bound {:.2e}'.format(
        name, chan, N, nsplit, err, e_ref, R.bound(e_ref)))
    assert torch.isfinite(got).all() and err <= R.bound(e_ref)
    if name == 's2_tiles':
        assert nsplit > 1


@pytest.mark.parametrize('name,stride,N', [('s2_tiles', 2, 3), ('s1_p1', 1, 40)])
def test_conv3x3g_wgrad_several_tiles_per_split(name, stride, N):
    """256 x 256 channels are 256 blocks of dW, so the plan asks for 4 splits: 12 (40) pixel tiles give 3 (10) tiles per
    split and the workgroup's loop over tiles, with its re-staged LDS window, runs more than once"""
    from hipnet import ftl_train
    (H, W), (Ho, Wo), _, pad_lo = MAPS[name]
    chan = (256, 256, 256)
    assert ftl_train.wgrad_plan(N, Ho, Wo, 256, 256)[1:] == (4, -(-N * -(-Ho // 8) * -(-Wo // 16) // 4))
    x, gy, ref, e_ref = _wgrad_case(name, chan, N)
    got, nsplit = _run_wgrad(x, gy, 256, stride, pad_lo)
    err = R.rel(got, ref)
    print('conv3x3g_wgrad {} 256 x 256 N {}: {} splits, err {:.2e}, e_ref {:.2e}'.format(name, N, nsplit, err, e_ref))
    assert err <= R.bound(e_ref)


@pytest.mark.parametrize('name,chan,N', [('s2_tiles', (56, 55, 32), 3), ('s2_5x3', (20, 20, 21), 1),
                                         ('s1_p1', (48, 48, 16), 3)])
def test_conv3x3g_wgrad_equal_bits(name, chan, N):
    x, gy, _, _ = _wgrad_case(name, chan, N)
    _, _, stride, pad_lo = MAPS[name]
    one, _ = _run_wgrad(x, gy, chan[1], stride, pad_lo)
    two, _ = _run_wgrad(x, gy, chan[1], stride, pad_lo)
    other, _ = _run_wgrad(x, gy, chan[1], stride, pad_lo, stream=torch.cuda.Stream())
    assert _same_bits(one, two) and _same_bits(one, other)


@pytest.mark.parametrize('chan', CHANNELS, ids=lambda c: 'c{}_{}_{}'.format(*c))
def test_conv3x3g_wgrad_against_kxk_wgrad(chan):
    """stride 1, pad_lo 1 is the 3x3 of hrnet_conv2d_kxk_wgrad: the same MFMA chain per split, so equal bits are expected;
    the bound of the reference holds either way"""
    from hipnet import conv_kxk_train
    x, gy, ref, e_ref = _wgrad_case('s1_p1', chan, 3)
    got, _ = _run_wgrad(x, gy, chan[1], 1, 1)
    cin, real, cout = chan
    kxk, _ = conv_kxk_train.conv_kxk_wgrad(_nhwc(x, cin + 12, 8), _nhwc(gy, cout + 7, 3), cout, 3, cin=cin, cin_real=real,
                                           x_off=8, y_off=3, want_bias=False)
    torch.cuda.synchronize()
    kxk = kxk.cpu()
    err = R.rel(got, kxk.double())
    print('conv3x3g_wgrad vs kxk_wgrad {}: equal bits {}, difference {:.2e}, e_ref {:.2e}'.format(chan, _same_bits(got, kxk),
                                                                                                  err, e_ref))
    assert _same_bits(got, kxk) or (err <= R.bound(e_ref) and R.rel(kxk, ref) <= R.bound(e_ref))


# ---- ConvTranspose2d(3, 2, 2, op): the weight gradient with the roles swapped, and both data-gradient identities ----------
TCASES = [(op, hw, chan) for op in (0, 1) for hw in ((3, 4), (9, 9)) for chan in ((20, 21), (48, 16))]


def _tconv_grads(x, w, gy, op, dtype):
    xt, wt = x.to(dtype).clone().requires_grad_(), w.to(dtype).clone().requires_grad_()
    y = F.conv_transpose2d(xt, wt, stride=2, padding=2, output_padding=op)
    (y * gy.to(dtype)).sum().backward()
    return xt.grad, wt.grad


@pytest.mark.parametrize('op,hw,chan', TCASES)
def test_conv_transpose_gradients(op, hw, chan):
    from hipnet import ftl, ftl_train
    (h, w), (ci, co), N = hw, chan, 2
    ho, wo = 2 * h - 3 + op, 2 * w - 3 + op
    rng = np.random.RandomState(3 + op + h + ci)
    x, wt = _f16(rng, (N, ci, h, w)), _f16(rng, (ci, co, 3, 3), (2.0 / (9 * ci)) ** 0.5)
    gy = _f16(rng, (N, co, ho, wo))
    cop = (co + 3) // 4 * 4
    gyp = F.pad(gy, (0, 0, 0, 0, 0, cop - co))                  # zero pad channels up to a multiple of 4
    dx64, dw64 = _tconv_grads(x, wt, gy, op, torch.float64)
    dx32, dw32 = _tconv_grads(x, wt, gy, op, torch.float32)
    # the weight gradient: x := the output gradient (the large map), dy := the layer's input, stride 2, pad_lo 2
    got = ftl_train.conv3x3g_wgrad(_nhwc(gyp, cop + 8, 4), _nhwc(x, ci + 5, 2), ci, 2, 2, cin=cop, cin_real=co, x_off=4,
                                   y_off=2)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (ci, co, 3, 3)
    err, e_ref = R.rel(got.cpu(), dw64), R.rel(dw32, dw64)
    print('tconv wgrad op {} {}x{} {}: err {:.2e} e_ref {:.2e}'.format(op, h, w, chan, err, e_ref))
    assert err <= R.bound(e_ref)
    # the data gradient: the forward kernel at stride 2, pad_lo 2 on conv_pack of the weight as it stands
    packed = ftl_train.pack_dgrad_transpose(_dev(wt), cop)
    out = torch.full((N, h, w, ci + 7), CANARY, dtype=torch.float32, device='cuda')
    ftl.conv3x3g(_nhwc(gyp, cop + 8, 4), packed, ci, 2, 2, 1, cin=cop, x_off=4, out=out, y_off=3)
    torch.cuda.synchronize()
    o = out.cpu()
    err, e_ref = R.rel(o[..., 3:3 + ci].permute(0, 3, 1, 2), dx64), R.rel(dx32, dx64)
    print('tconv dgrad op {} {}x{} {}: err {:.2e} e_ref {:.2e}'.format(op, h, w, chan, err, e_ref))
    assert err <= R.bound(e_ref)
    assert bool((o[..., :3] == CANARY).all()) and bool((o[..., 3 + ci:] == CANARY).all())


def _conv_s2_dgrad(x, w, gy, dtype):
    xt = x.to(dtype).clone().requires_grad_()
    (F.conv2d(xt, w.to(dtype), stride=2, padding=2) * gy.to(dtype)).sum().backward()
    return xt.grad


@pytest.mark.parametrize('hw', [(4, 8), (5, 3), (16, 16), (17, 33)])
@pytest.mark.parametrize('chan', [(20, 21), (48, 16)])
def test_conv_stride2_data_gradient(hw, chan):
    """dgrad of Conv2d(3, 2, 2) = the forward kernel on the zero-stuffed gradient (stride 1, pad_lo 0, z 2, Ho = H_in) with
    nhwc.conv_transpose_pack of the weight; even and odd H_in both lie in the size range of their gradient"""
    from hipnet import ftl, ftl_train
    (h, w), (ci, co), N = hw, chan, 2
    ho, wo = R.enc_size(h), R.enc_size(w)
    rng = np.random.RandomState(5 + h + w + ci)
    x, wt, gy = _f16(rng, (N, ci, h, w)), _f16(rng, (co, ci, 3, 3), (2.0 / (9 * ci)) ** 0.5), _f16(rng, (N, co, ho, wo))
    cop = (co + 3) // 4 * 4
    gyp = F.pad(gy, (0, 0, 0, 0, 0, cop - co))
    ref = _conv_s2_dgrad(x, wt, gy, torch.float64)
    e_ref = R.rel(_conv_s2_dgrad(x, wt, gy, torch.float32), ref)
    packed = ftl_train.pack_dgrad(_dev(wt), cop)
    got = ftl.conv3x3g(_nhwc(gyp, cop + 8, 4), packed, ci, 1, 0, 2, out_hw=(h, w), cin=cop, x_off=4)
    torch.cuda.synchronize()
    err = R.rel(got.cpu().permute(0, 3, 1, 2), ref)
    print('conv s2 dgrad {}x{} {}: err {:.2e} e_ref {:.2e}'.format(h, w, chan, err, e_ref))
    assert tuple(got.shape) == (N, h, w, ci) and err <= R.bound(e_ref)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_conv3x3g_wgrad_refusals():
    from hipnet import ftl_train
    z = lambda *s: torch.zeros(*s, device='cuda')
    x, dy = z(1, 4, 8, 8), z(1, 3, 5, 16)
    dw = torch.full((16, 8, 3, 3), CANARY, device='cuda')
    scratch = torch.full((ftl_train.wgrad_plan(1, 3, 5, 8, 16)[0] // 4,), CANARY, device='cuda')
    assert tuple(ftl_train.conv3x3g_wgrad(x, dy, 16, 2, 2).shape) == (16, 8, 3, 3)
    for hw in ((4, 5), (1, 5), (3, 6), (3, 3)):                               # 4 x 8 at stride 2, pad_lo 2: 2 .. 3 x 4 .. 5
        with pytest.raises(ValueError, match='give'):
            ftl_train.conv3x3g_wgrad(x, z(1, hw[0], hw[1], 16), 16, 2, 2, dw=dw, scratch=scratch)
    with pytest.raises(ValueError, match='pad_lo = 3'):
        ftl_train.conv3x3g_wgrad(x, dy, 16, 1, 3, dw=dw)
    with pytest.raises(ValueError, match='multiples of 4'):
        ftl_train.conv3x3g_wgrad(z(1, 4, 8, 12), dy, 16, 2, 2, cin=8, x_off=2, dw=dw)
    with pytest.raises(ValueError, match='scratch of'):
        ftl_train.conv3x3g_wgrad(x, dy, 16, 2, 2, dw=dw, scratch=scratch[:-1])
    with pytest.raises(ValueError, match='real input'):
        ftl_train.conv3x3g_wgrad(x, dy, 16, 2, 2, cin_real=9)
    with pytest.raises(ValueError, match='dw'):
        ftl_train.conv3x3g_wgrad(x, dy, 16, 2, 2, dw=z(16, 8, 9))
    # the C entry's own checks, through the raw launcher: HR_E_BADARG before the first launch, nothing written
    with pytest.raises(RuntimeError, match='Ho x Wo'):
        ftl_train.wgrad(x, z(1, 4, 5, 16), scratch, dw, 8, 8, 0, 16, 0, 2, 2)
    with pytest.raises(RuntimeError, match='multiples of 4'):
        ftl_train.wgrad(z(1, 4, 8, 12), dy, scratch, dw, 8, 8, 2, 16, 0, 2, 2)
    with pytest.raises(RuntimeError, match='scratch of'):
        ftl_train.wgrad(x, dy, scratch[:-1], dw, 8, 8, 0, 16, 0, 2, 2)
    with pytest.raises(RuntimeError, match='outside ldy'):
        ftl_train.wgrad(x, dy, scratch, dw, 8, 8, 0, 16, 4, 2, 2)
    torch.cuda.synchronize()
    assert bool((dw == CANARY).all()) and bool((scratch == CANARY).all())
