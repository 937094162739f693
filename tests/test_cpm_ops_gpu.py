"""hrnet_conv2d_kxk, hrnet_maxpool2d_3x3s2 and hrnet_avgpool2d_9s8 (csrc/conv_kxk.hip, hipnet.conv_kxk) on the GPU against
F.conv2d / F.max_pool2d / F.avg_pool2d in float64 on the CPU, computed here.

err = max|dev - ref64| / max|ref64| must stay within cpm_ref.bound(e_ref) = 4 * e_ref + 2 * 2^-24, e_ref being the same
measure of torch's float32 op on the CPU (the convention of tests/swin_ref.py). Map sizes sit on the borders of the
kernel's pixel tile (Th, Tw), read from hrnet_conv_kxk_tile: 1x2, 5x9 (smaller than an 11x11 halo), (Th+1) x (Tw+1) and
(2 Th - 1) x (Tw + 3). The wide layers (32 -> 512, 128 -> 128, 128 -> 22) stay on the small maps so that the float64
reference of the whole file takes seconds."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cpm_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -12345.678


def _K():
    from hipnet import conv_kxk
    return conv_kxk


@functools.lru_cache(maxsize=None)
def _sizes():
    th, tw = _K().tile()[:2]
    return ((1, 2), (5, 9), (th + 1, tw + 1), (2 * th - 1, tw + 3))


def _draw(seed, n, h, w, ci, co, ks):
    rng = np.random.RandomState(seed)
    x = torch.tensor(rng.standard_normal((n, ci, h, w)))
    wgt = torch.tensor(rng.standard_normal((co, ci, ks, ks)) * np.sqrt(2.0 / (ci * ks * ks)))
    b = torch.tensor(rng.standard_normal(co) * 0.1)
    return x, wgt, b


def _device_map(x, ld, off, fill):
    """CPU NCHW f64 -> device NHWC f32 (B, H, W, ld) with x's channels at [off, off + C) and `fill` elsewhere"""
    n, c, h, w = x.shape
    t = torch.full((n, h, w, ld), float(fill), dtype=torch.float32)
    t[..., off:off + c] = x.permute(0, 2, 3, 1).float()
    return t.to(DEV)


def _check_conv(label, n, h, w, ci, co, ks, seed, cip=None, ldx=None, x_off=0, ldy=None, y_off=0):
    """every (bias, ReLU) variant of one layer shape against float64; returns the largest err / bound"""
    K = _K()
    cip = (ci + 3) // 4 * 4 if cip is None else cip
    ldx = cip if ldx is None else ldx
    x, wgt, b = _draw(seed, n, h, w, ci, co, ks)
    xd = _device_map(x, ldx, x_off, 3.0)            # foreign channels hold 3: reading one would show
    if cip > ci:
        xd[..., x_off + ci:x_off + cip] = 0.0       # the slice's own pad channels are zero, as the model keeps them
    packed = K.pack(wgt.float().to(DEV), cip)
    ref64 = F.conv2d(x, wgt, None, padding=ks // 2)
    ref32 = F.conv2d(x.float(), wgt.float(), None, padding=ks // 2).double()
    worst = 0.0
    for bias, relu in ((False, False), (True, True), (True, False), (False, True)):
        r64 = ref64 + b.view(1, -1, 1, 1) if bias else ref64
        r32 = (ref32.float() + b.float().view(1, -1, 1, 1)).double() if bias else ref32
        if relu:
            r64, r32 = r64.clamp_min(0), r32.clamp_min(0)
        bd = b.float().to(DEV) if bias else None
        if ldy is None:
            y = K.conv_kxk(xd, packed, co, ks, bias=bd, relu=relu, cin=cip, x_off=x_off)
            y2 = K.conv_kxk(xd, packed, co, ks, bias=bd, relu=relu, cin=cip, x_off=x_off)
            got = y
        else:
            y = torch.full((n, h, w, ldy), SENTINEL, dtype=torch.float32, device=DEV)
            y2 = y.clone()
            K.conv_kxk(xd, packed, co, ks, bias=bd, relu=relu, cin=cip, x_off=x_off, out=y, y_off=y_off)
            K.conv_kxk(xd, packed, co, ks, bias=bd, relu=relu, cin=cip, x_off=x_off, out=y2, y_off=y_off)
            outside = torch.cat([y[..., :y_off], y[..., y_off + co:]], -1)
            assert torch.equal(outside, torch.full_like(outside, SENTINEL)), label + ': wrote outside its slice'
            got = y[..., y_off:y_off + co]
        torch.cuda.synchronize()
        assert torch.equal(y, y2), label + ': two launches differ'
        got = got.double().cpu().permute(0, 3, 1, 2).numpy()
        assert np.isfinite(got).all(), label
        denom = max(float(r64.abs().max()), 1e-30)
        err, e_ref = R.rel(got, r64.numpy(), denom), R.rel(r32.numpy(), r64.numpy(), denom)
        print('{} bias {} relu {}: err {:.3g} e_ref {:.3g} bound {:.3g}'.format(label, bias, relu, err, e_ref, R.bound(e_ref)))
        assert err <= R.bound(e_ref), (label, bias, relu, err, R.bound(e_ref))
        worst = max(worst, err / R.bound(e_ref))
    return worst


@pytest.mark.parametrize('si', range(4))
@pytest.mark.parametrize('ks', (1, 5, 9, 11))
def test_image_and_concat_layers(ks, si):
    """3 (in 4) -> 128, the image layers' 4-channel path, and 55 (in 56) -> 128, Mconv1's concatenated input read at
    channel offset 8 of a 72-wide map whose other channels hold 3; N alternates between 1 and 3.
    MI355X: err / bound at most 0.37 over the 16 cases' 192 launches (55/56 -> 128, ks 5, 1x2: err 2.0e-07, bound 5.4e-07)."""
    h, w = _sizes()[si]
    n = 3 if (si + ks // 4) % 2 == 0 else 1
    seed = 100 * ks + si
    _check_conv('3/4->128 ks{} {}x{} N{}'.format(ks, h, w, n), n, h, w, 3, 128, ks, seed)
    _check_conv('3/4->128@4/12 ks{} {}x{} N{}'.format(ks, h, w, 4 - n), 4 - n, h, w, 3, 128, ks, seed + 1, ldx=12, x_off=4)
    _check_conv('55/56->128 ks{} {}x{} N{}'.format(ks, h, w, n), n, h, w, 55, 128, ks, seed + 2, ldx=72, x_off=8)


@pytest.mark.parametrize('n', (1, 3))
@pytest.mark.parametrize('si', (0, 1))
def test_wide_layers_on_small_maps(si, n):
    """32 -> 512 at ks 9 (conv5_stage1), 128 -> 128 at ks 11 (Mconv2/3: sums of 15 488 terms) and 512 -> 512 at ks 1 on the
    1x2 and 5x9 maps. MI355X, 128 -> 128 ks 11: err 1.0e-07 .. 2.5e-07 against bounds of 3.9e-07 .. 2.4e-06 (e_ref 6.7e-08 ..
    5.7e-07), at most 0.27 of the bound: the per-kernel-row partial sums keep the long sum inside the plain bound, so no
    case needs the emulated-order bound. 32 -> 512: at most 0.39 of the bound."""
    h, w = _sizes()[si]
    _check_conv('32->512 ks9 {}x{} N{}'.format(h, w, n), n, h, w, 32, 512, 9, 7 + si)
    _check_conv('128->128 ks11 {}x{} N{}'.format(h, w, n), n, h, w, 128, 128, 11, 9 + si)
    _check_conv('512->512 ks1 {}x{} N{}'.format(h, w, n), n, h, w, 512, 512, 1, 11 + si)


@pytest.mark.parametrize('si', (0, 1, 2))
@pytest.mark.parametrize('ks', (1, 11))
def test_heat_map_layer_writes_only_its_slice(ks, si):
    """128 -> 22 written at channel 32 of a 56-wide map filled with a sentinel (Mconv5 into the concatenated map), and
    at channel 5 of a 31-wide one (no 16-byte stores possible): every channel outside the slice keeps the sentinel's
    bits. The layout stores the real channels only, so there are no pad channels inside the slice."""
    h, w = _sizes()[si]
    n = 1 + 2 * (si % 2)
    _check_conv('128->22@32/56 ks{} {}x{}'.format(ks, h, w), n, h, w, 128, 22, ks, 40 + si, ldy=56, y_off=32)
    _check_conv('128->22@5/31 ks{} {}x{}'.format(ks, h, w), n, h, w, 128, 22, ks, 50 + si, ldy=31, y_off=5)


def test_tile_constants():
    """the exported constants are the documented ones, and an unknown index gives 0"""
    K = _K()
    th, tw, kc, maxks = K.tile()
    assert (th, tw) == (8, 16) and kc == 16 and maxks == 11
    from hipnet import _capi as C
    assert C.call('hrnet_conv_kxk_tile', 4) == 0 and C.call('hrnet_conv_kxk_tile', -1) == 0


def test_bad_arguments_are_refused_and_write_nothing():
    from hipnet import _capi as C
    K = _K()
    x = torch.randn(1, 4, 4, 8, device=DEV)
    w = torch.randn(16 * 9 * 8, device=DEV)
    y = torch.full((1, 4, 4, 16), SENTINEL, device=DEV)
    s = C.stream_ptr()
    E = C.VALUES['HR_E_BADARG']
    lib = C.lib()

    def call(dtype=C.HR_F32, xp=None, wp=None, yp=None, N=1, H=4, W=4, cin=8, ldx=8, x_off=0, cout=16, ldy=16, y_off=0, ks=3,
             relu=0):
        return lib.hrnet_conv2d_kxk(dtype, x.data_ptr() if xp is None else xp, w.data_ptr() if wp is None else wp, None,
                                    y.data_ptr() if yp is None else yp, N, H, W, cin, ldx, x_off, cout, ldy, y_off, ks, relu, s)

    bad = dict(bf16=dict(dtype=C.HR_BF16), even_ks=dict(ks=2), ks0=dict(ks=0), ks13=dict(ks=13), neg_ks=dict(ks=-3),
               cin_align=dict(cin=6), ldx_align=dict(ldx=10), x_off_align=dict(x_off=2), x_off_out=dict(x_off=4),
               x_off_neg=dict(x_off=-4), y_off_out=dict(y_off=4), y_off_neg=dict(y_off=-1), cout0=dict(cout=0), n0=dict(N=0),
               h0=dict(H=0), cin0=dict(cin=0), x_unaligned=dict(xp=x.data_ptr() + 4), w_unaligned=dict(wp=w.data_ptr() + 4),
               relu2=dict(relu=2))
    for name, kw in bad.items():
        assert call(**kw) == E, name
        assert lib.hrnet_last_error_string()
    assert lib.hrnet_conv2d_kxk(C.HR_F32, None, w.data_ptr(), None, y.data_ptr(), 1, 4, 4, 8, 8, 0, 16, 16, 0, 3, 0, s) == E
    assert lib.hrnet_conv2d_kxk(C.HR_F32, x.data_ptr(), None, None, y.data_ptr(), 1, 4, 4, 8, 8, 0, 16, 16, 0, 3, 0, s) == E
    assert lib.hrnet_conv2d_kxk(C.HR_F32, x.data_ptr(), w.data_ptr(), None, None, 1, 4, 4, 8, 8, 0, 16, 16, 0, 3, 0, s) == E
    pool_bad = [lib.hrnet_maxpool2d_3x3s2(None, y.data_ptr(), 1, 4, 4, 8, 8, 0, 16, 0, s),
                lib.hrnet_maxpool2d_3x3s2(x.data_ptr(), y.data_ptr(), 1, 4, 4, 8, 8, 4, 16, 0, s),
                lib.hrnet_maxpool2d_3x3s2(x.data_ptr(), y.data_ptr(), 1, 4, 4, 8, 8, 0, 16, 12, s),
                lib.hrnet_maxpool2d_3x3s2(x.data_ptr(), y.data_ptr(), 1, 0, 4, 8, 8, 0, 16, 0, s),
                lib.hrnet_avgpool2d_9s8(x.data_ptr(), y.data_ptr(), 1, 6, 8, 16, 0, s),      # torch refuses H < 7 as well
                lib.hrnet_avgpool2d_9s8(x.data_ptr(), y.data_ptr(), 1, 1, 1, 16, 0, s),
                lib.hrnet_avgpool2d_9s8(x.data_ptr(), y.data_ptr(), 1, 2, 3, 16, 0, s),
                lib.hrnet_avgpool2d_9s8(x.data_ptr(), y.data_ptr(), 1, 8, 8, 16, 16, s),
                lib.hrnet_avgpool2d_9s8(None, y.data_ptr(), 1, 8, 8, 16, 0, s)]
    assert pool_bad == [E] * len(pool_bad), pool_bad
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full_like(y, SENTINEL))
    assert call() == 0                                   # and the good call of the same table goes through
    torch.cuda.synchronize()
    assert not torch.equal(y, torch.full_like(y, SENTINEL))
    # the checked host layer refuses before any device call
    with pytest.raises(ValueError):
        K.conv_kxk(x.cpu(), w, 16, 3)
    with pytest.raises(ValueError):
        K.conv_kxk(x, w, 16, 4)
    with pytest.raises(ValueError):
        K.conv_kxk(x, w, 16, 3, cin=6)
    with pytest.raises(ValueError):
        K.conv_kxk(x, w[:-1], 16, 3)
    with pytest.raises(ValueError):
        K.conv_kxk(x, w, 16, 3, out=torch.empty(1, 4, 4, 20, device=DEV), y_off=8)
    with pytest.raises(NotImplementedError, match='inference only'):
        K.conv_kxk(x.clone().requires_grad_(True), w, 16, 3)
    with pytest.raises(NotImplementedError, match='inference only'):
        K.maxpool3x3s2(x.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        K.avgpool9s8(torch.zeros(1, 1, 2, 3, device=DEV))
    with pytest.raises(ValueError):
        K.maxpool3x3s2(x.cpu())


@pytest.mark.parametrize('h,w', ((1, 1), (2, 3), (7, 9), (16, 16)))
def test_max_pool(h, w):
    """MaxPool2d(3, 2, 1) on 5 channels at offset 3 of a 12-wide map into offset 2 of a 9-wide one; exact (a maximum
    rounds nothing). The all-negative map fails a zero-padded implementation."""
    K = _K()
    rng = np.random.RandomState(h * 31 + w)
    for n, negative in ((1, False), (3, True)):
        x = torch.tensor(rng.standard_normal((n, 5, h, w)))
        if negative:
            x = -x.abs() - 0.5
        ref = F.max_pool2d(x, 3, 2, 1)
        xd = _device_map(x, 12, 3, 1e9)
        y = torch.full((n, ref.shape[2], ref.shape[3], 9), SENTINEL, dtype=torch.float32, device=DEV)
        K.maxpool3x3s2(xd, c=5, x_off=3, out=y, y_off=2)
        torch.cuda.synchronize()
        assert torch.equal(y[..., 2:7].cpu().permute(0, 3, 1, 2), ref.float())
        outside = torch.cat([y[..., :2], y[..., 7:]], -1)
        assert torch.equal(outside, torch.full_like(outside, SENTINEL))
        fresh = K.maxpool3x3s2(xd[..., 3:8].contiguous())
        assert torch.equal(fresh, y[..., 2:7])


@pytest.mark.parametrize('h,w', ((7, 9), (8, 16), (16, 16), (40, 72)))
def test_avg_pool_of_the_centre_map(h, w):
    """AvgPool2d(9, 8, 1), count_include_pad, into channel 54 of a 56-wide map. 1x1 and 2x3 maps are refused, as torch
    refuses them (test_bad_arguments): the smallest map with an output is 7x7."""
    K = _K()
    rng = np.random.RandomState(h + w)
    for n in (1, 3):
        x = torch.tensor(rng.uniform(0, 1, (n, 1, h, w)))
        ref64 = F.avg_pool2d(x, 9, 8, 1)
        ref32 = F.avg_pool2d(x.float(), 9, 8, 1).double()
        y = torch.full((n, ref64.shape[2], ref64.shape[3], 56), SENTINEL, dtype=torch.float32, device=DEV)
        K.avgpool9s8(x.float().to(DEV), out=y, y_off=54)
        torch.cuda.synchronize()
        got = y[..., 54].double().cpu().numpy()
        err, e_ref = R.rel(got, ref64[:, 0].numpy()), R.rel(ref32.numpy(), ref64.numpy())
        print('avgpool {}x{} N{}: err {:.3g} e_ref {:.3g} bound {:.3g}'.format(h, w, n, err, e_ref, R.bound(e_ref)))
        assert err <= R.bound(e_ref)
        outside = torch.cat([y[..., :54], y[..., 55:]], -1)
        assert torch.equal(outside, torch.full_like(outside, SENTINEL))
