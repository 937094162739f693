"""hrnet_conv2d_kxk_wgrad, hrnet_conv2d_kxk_dgrad and hrnet_maxpool2d_3x3s2_bwd (csrc/conv_kxk_train.hip,
hipnet.conv_kxk_train) on the GPU against float64 F.conv2d / F.max_pool2d autograd on the CPU, computed here.

err = max|dev - ref64| / max|ref64| per tensor must stay within cpm_ref.bound(e_ref) = 4 * e_ref + 2 * 2^-24, e_ref being
the same measure of torch's float32 CPU autograd, taken in the same test. Inputs are float16-valued. Maps 1x2, 5x9, 8x16
(one pixel tile exactly), 9x17 (four tiles, three of them one row or column) and 17x33 (nine tiles, so several splits of
the weight gradient); N 1 and 3; ks 1, 5, 9, 11; (Cin, Cout) = (4 with 3 real, 16), (20, 22), (56 with 55 real, 32) and,
on the 5x9 map, (128, 128). Every source is a slice at a non-zero offset of a wider map whose foreign channels hold 3;
every destination sits between sentinels that must keep their bits: the Conv2d-layout gradient's neighbours, the bias
gradient's, the scratch tail and the channels around the data gradient's slice."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cpm_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -12345.678
GUARD = 64
MAPS = ((1, 2), (5, 9), (8, 16), (9, 17), (17, 33))
CHANNELS = ((3, 4, 16), (20, 20, 22), (55, 56, 32))          # (real Cin, the slice read, Cout)


def _T():
    from hipnet import conv_kxk_train
    return conv_kxk_train


def _f16(a):
    return torch.tensor(np.asarray(a, dtype=np.float16).astype(np.float64))


def _device_map(x, ld, off, fill, pad_to=None):
    """CPU NCHW f64 -> device NHWC f32 (B, H, W, ld): x's channels at [off, off + C), zeros up to off + pad_to (the slice's
    own pad channels), `fill` elsewhere"""
    n, c, h, w = x.shape
    t = torch.full((n, h, w, ld), float(fill), dtype=torch.float32)
    t[..., off:off + (pad_to or c)] = 0.0
    t[..., off:off + c] = x.permute(0, 2, 3, 1).float()
    return t.to(DEV)


def _guarded(numel):
    buf = torch.full((GUARD + numel + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + numel]


def _intact(buf, numel):
    g = torch.full((GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    return torch.equal(buf[:GUARD], g) and torch.equal(buf[GUARD + numel:], g)


def _oracle(x, wgt, dy, dtype):
    xx, ww = x.detach().clone().to(dtype).requires_grad_(True), wgt.detach().clone().to(dtype).requires_grad_(True)
    bb = torch.zeros(wgt.shape[0], dtype=dtype, requires_grad=True)
    F.conv2d(xx, ww, bb, padding=wgt.shape[2] // 2).backward(dy.to(dtype))
    return xx.grad.double(), ww.grad.double(), bb.grad.double()


def _within(label, got, r64, r32):
    denom = max(float(r64.abs().max()), 1e-30)
    err, e_ref = R.rel(got, r64.numpy(), denom), R.rel(r32.numpy(), r64.numpy(), denom)
    print('{}: err {:.3g} e_ref {:.3g} bound {:.3g}'.format(label, err, e_ref, R.bound(e_ref)))
    assert np.isfinite(np.asarray(got)).all(), label
    assert err <= R.bound(e_ref), (label, err, e_ref, R.bound(e_ref))


def _check_layer(label, n, h, w, ci, cip, co, ks, seed):
    T = _T()
    rng = np.random.RandomState(seed)
    x = _f16(rng.standard_normal((n, ci, h, w)))
    wgt = _f16(rng.standard_normal((co, ci, ks, ks)) * np.sqrt(2.0 / (ci * ks * ks)))
    dy = _f16(rng.standard_normal((n, co, h, w)))
    dx64, dw64, db64 = _oracle(x, wgt, dy, torch.float64)
    dx32, dw32, db32 = _oracle(x, wgt, dy, torch.float32)
    cop = (co + 3) // 4 * 4
    x_off, y_off = 8, 4
    xd = _device_map(x, x_off + cip + 4, x_off, 3.0, cip)
    dyd = _device_map(dy, y_off + cop + 8, y_off, 3.0, cop)

    # ---- weight and bias gradient: the Conv2d layout between sentinels, the scratch with a sentinel tail
    nbytes, nsplit, per = T.wgrad_plan(n, h, w, cip, co, ks)
    tiles = n * ((h + 7) // 8) * ((w + 15) // 16)
    assert nbytes % 4 == 0 and 1 <= nsplit <= tiles and (nsplit - 1) * per < tiles <= nsplit * per
    runs = []
    for rep in range(2):
        wbuf, dw = _guarded(co * ci * ks * ks)
        bbuf, db = _guarded(co)
        sbuf, scratch = _guarded(nbytes // 4)
        T.conv_kxk_wgrad(xd, dyd, co, ks, cin=cip, cin_real=ci, x_off=x_off, y_off=y_off, scratch=scratch,
                         dw=dw.view(co, ci, ks, ks), db=db)
        torch.cuda.synchronize()
        assert _intact(wbuf, dw.numel()) and _intact(bbuf, co) and _intact(sbuf, nbytes // 4), label + ': wrote outside'
        runs.append((dw.clone(), db.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), label + ': two runs differ'
    if n == 3:      # another stream, fresh allocations (the scratch and the results included): the same bits
        stream = torch.cuda.Stream(device=DEV)
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            xd2, dyd2 = xd.clone(), dyd.clone()
            dw2, db2 = T.conv_kxk_wgrad(xd2, dyd2, co, ks, cin=cip, cin_real=ci, x_off=x_off, y_off=y_off)
        stream.synchronize()
        assert tuple(dw2.shape) == (co, ci, ks, ks)
        assert torch.equal(dw2.reshape(-1), runs[0][0]) and torch.equal(db2, runs[0][1]), label + ': stream / allocation'
    _within(label + ' dW', runs[0][0].view(co, ci, ks, ks).double().cpu().numpy(), dw64, dw32)
    _within(label + ' db', runs[0][1].double().cpu().numpy(), db64, db32)
    dw_only, none = T.conv_kxk_wgrad(xd, dyd, co, ks, cin=cip, cin_real=ci, x_off=x_off, y_off=y_off, want_bias=False)
    assert none is None and torch.equal(dw_only.reshape(-1), runs[0][0])

    # ---- data gradient: plain, masked, and masked + accumulated onto a non-zero destination; real channels only
    packed_t = T.pack_dgrad(wgt.float().to(DEV), cop)
    mask = torch.tensor(rng.randint(-1, 2, (n, ci, h, w)).astype(np.float64))     # -1, 0, 1: zero does not pass
    md = _device_map(mask, 4 + ci + 3, 4, 1.0)
    dest = _f16(rng.standard_normal((n, ci, h, w)))
    for d_off, ld in ((4, 4 + ci + 5), (3, 3 + ci + 2)):       # 16-byte stores possible / not
        for masked, accumulate in ((False, False), (True, False), (True, True), (False, True)):
            out = _device_map(dest, ld, d_off, SENTINEL)
            out2 = out.clone()
            for o in (out, out2):
                T.conv_kxk_dgrad(dyd, packed_t, ci, ks, cout=cop, y_off=y_off, out=o, x_off=d_off,
                                 mask=md if masked else None, m_off=4, accumulate=accumulate)
            torch.cuda.synchronize()
            assert torch.equal(out, out2), label + ': two dgrad runs differ'
            outside = torch.cat([out[..., :d_off], out[..., d_off + ci:]], -1)
            assert torch.equal(outside, torch.full_like(outside, SENTINEL)), label + ': dgrad wrote outside its slice'
            r64, r32 = dx64, dx32.float()
            if masked:
                r64, r32 = r64 * (mask > 0), r32 * (mask > 0).float()
            if accumulate:
                r64, r32 = r64 + dest, r32 + dest.float()
            got = out[..., d_off:d_off + ci].double().cpu().permute(0, 3, 1, 2).numpy()
            _within('{} dx@{} mask {} acc {}'.format(label, d_off, masked, accumulate), got, r64, r32.double())
    if ci % 4 == 0:
        fresh = T.conv_kxk_dgrad(dyd, packed_t, ci, ks, cout=cop, y_off=y_off)
        plain = _device_map(dest, 4 + ci + 5, 4, SENTINEL)
        T.conv_kxk_dgrad(dyd, packed_t, ci, ks, cout=cop, y_off=y_off, out=plain, x_off=4)
        assert torch.equal(fresh, plain[..., 4:4 + ci])


@pytest.mark.parametrize('mi', range(len(MAPS)))
@pytest.mark.parametrize('ks', (1, 5, 9, 11))
def test_wgrad_and_dgrad(ks, mi):
    h, w = MAPS[mi]
    for n in (1, 3):
        for j, (ci, cip, co) in enumerate(CHANNELS):
            _check_layer('{}/{}->{} ks{} {}x{} N{}'.format(ci, cip, co, ks, h, w, n), n, h, w, ci, cip, co, ks,
                         1000 * ks + 100 * mi + 10 * n + j)


@pytest.mark.parametrize('n', (1, 3))
@pytest.mark.parametrize('ks', (1, 5, 9, 11))
def test_wide_layer_on_the_5x9_map(ks, n):
    """128 -> 128: 64 channel blocks, at ks 11 the 31 accumulators per wave of Mconv2 / Mconv3"""
    _check_layer('128->128 ks{} 5x9 N{}'.format(ks, n), n, 5, 9, 128, 128, 128, ks, 7000 + 10 * ks + n)


def test_wgrad_plan_of_the_network_layers():
    """the split rule of csrc/conv_kxk_split.h at the shapes DESIGN.md quotes"""
    T = _T()
    assert T.wgrad_plan(1, 32, 32, 128, 128, 11) == (8 * (64 * 121 * 256 + 128) * 4, 8, 1)
    assert T.wgrad_plan(16, 32, 32, 128, 128, 11) == (16 * (64 * 121 * 256 + 128) * 4, 16, 8)
    assert T.wgrad_plan(16, 256, 256, 4, 128, 9)[1:] == (128, 64)
    assert T.wgrad_plan(3, 17, 33, 56, 32, 5)[1:] == (27, 1)


@pytest.mark.parametrize('c', (1, 5))
@pytest.mark.parametrize('h,w', ((1, 1), (2, 3), (7, 9), (16, 16)))
def test_max_pool_backward(h, w, c):
    """small integers: exact ties everywhere, all-equal windows (the constant map) and ties across the padding edge. The
    gradient is integer-valued, so the comparison with torch's float64 autograd (first maximum in scan order) is exact"""
    T = _T()
    rng = np.random.RandomState(97 * h + 7 * w + c)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for n, kind in ((1, 'ties'), (3, 'ties'), (2, 'constant'), (2, 'negative')):
        if kind == 'constant':
            x = torch.full((n, c, h, w), 2.0, dtype=torch.float64)
        else:
            x = torch.tensor(rng.randint(-1, 3, (n, c, h, w)).astype(np.float64))
            if kind == 'negative':
                x = x - 5.0
        dy = torch.tensor(rng.randint(-8, 9, (n, c, ho, wo)).astype(np.float64))
        xx = x.clone().requires_grad_(True)
        F.max_pool2d(xx, 3, 2, 1).backward(dy)
        ref = xx.grad
        xd = _device_map(x, 3 + c + 4, 3, 1e9)
        dyd = _device_map(dy, 2 + c + 1, 2, 1e9)
        for relu_mask in (False, True):
            out = torch.full((n, h, w, 1 + c + 2), SENTINEL, dtype=torch.float32, device=DEV)
            T.maxpool3x3s2_bwd(xd, dyd, c=c, x_off=3, dy_off=2, out=out, dx_off=1, relu_mask=relu_mask)
            torch.cuda.synchronize()
            want = ref * (x > 0) if relu_mask else ref
            assert torch.equal(out[..., 1:1 + c].cpu().permute(0, 3, 1, 2).double(), want), (kind, n, relu_mask)
            outside = torch.cat([out[..., :1], out[..., 1 + c:]], -1)
            assert torch.equal(outside, torch.full_like(outside, SENTINEL))
        fresh = T.maxpool3x3s2_bwd(xd[..., 3:3 + c].contiguous(), dyd[..., 2:2 + c].contiguous())
        assert torch.equal(fresh.cpu().permute(0, 3, 1, 2).double(), ref)


def test_bad_arguments_are_refused_and_write_nothing():
    from hipnet import _capi as C
    T = _T()
    lib, s, E, F32 = C.lib(), C.stream_ptr(), C.VALUES['HR_E_BADARG'], C.HR_F32
    x = torch.randn(1, 4, 4, 8, device=DEV)
    dy = torch.randn(1, 4, 4, 16, device=DEV)
    wt = torch.randn(16 * 9 * 16, device=DEV)
    nbytes = T.wgrad_plan(1, 4, 4, 8, 16, 3)[0]
    outs = {k: torch.full((n,), SENTINEL, device=DEV) for k, n in
            (('dw', 16 * 8 * 9), ('db', 16), ('scratch', nbytes // 4), ('dx', 4 * 4 * 8), ('px', 4 * 4 * 8))}

    def wg(dtype=F32, xp=x.data_ptr(), dyp=dy.data_ptr(), sp=outs['scratch'].data_ptr(), sb=nbytes, dwp=outs['dw'].data_ptr(),
           N=1, H=4, W=4, cin=8, real=8, ldx=8, x_off=0, cout=16, ldy=16, y_off=0, ks=3):
        return lib.hrnet_conv2d_kxk_wgrad(dtype, xp, dyp, sp, sb, dwp, outs['db'].data_ptr(), N, H, W, cin, real, ldx, x_off, cout,
                                          ldy, y_off, ks, s)

    def dg(dtype=F32, dyp=dy.data_ptr(), wp=wt.data_ptr(), dxp=outs['dx'].data_ptr(), mp=None, N=1, H=4, W=4, cout=16, ldy=16,
           y_off=0, cin=8, ldx=8, x_off=0, ldm=0, m_off=0, ks=3, acc=0):
        return lib.hrnet_conv2d_kxk_dgrad(dtype, dyp, wp, dxp, mp, N, H, W, cout, ldy, y_off, cin, ldx, x_off, ldm, m_off, ks,
                                          acc, s)

    def pb(xp=x.data_ptr(), dyp=dy.data_ptr(), dxp=outs['px'].data_ptr(), N=1, H=4, W=4, c=8, ldx=8, x_off=0, lddy=16, dy_off=0,
           lddx=8, dx_off=0, relu=0):
        return lib.hrnet_maxpool2d_3x3s2_bwd(xp, dyp, dxp, N, H, W, c, ldx, x_off, lddy, dy_off, lddx, dx_off, relu, s)

    bad_wg = dict(bf16=dict(dtype=C.HR_BF16), even_ks=dict(ks=2), ks0=dict(ks=0), ks13=dict(ks=13), cin_align=dict(cin=6, real=6),
                  ldx_align=dict(ldx=10), x_off_align=dict(x_off=2), x_off_out=dict(x_off=4), x_off_neg=dict(x_off=-4),
                  y_off_out=dict(y_off=4), y_off_neg=dict(y_off=-1), cout0=dict(cout=0), n0=dict(N=0), h0=dict(H=0),
                  real0=dict(real=0), real9=dict(real=9), x_unaligned=dict(xp=x.data_ptr() + 4), null_x=dict(xp=None),
                  null_dy=dict(dyp=None), null_scratch=dict(sp=None), null_dw=dict(dwp=None), short=dict(sb=nbytes - 1),
                  dy_unaligned=dict(dyp=dy.data_ptr() + 2))
    for name, kw in bad_wg.items():
        assert wg(**kw) == E, 'wgrad ' + name
        assert lib.hrnet_last_error_string()
    bad_dg = dict(bf16=dict(dtype=C.HR_BF16), even_ks=dict(ks=4), ks13=dict(ks=13), cout_align=dict(cout=14), ldy_align=dict(ldy=18),
                  y_off_align=dict(y_off=2), y_off_out=dict(y_off=4), x_off_out=dict(x_off=1), x_off_neg=dict(x_off=-1),
                  mask_out=dict(mp=x.data_ptr(), ldm=8, m_off=1), cin0=dict(cin=0), w0=dict(W=0), acc2=dict(acc=2),
                  null_dy=dict(dyp=None), null_w=dict(wp=None), null_dx=dict(dxp=None), alias=dict(dxp=dy.data_ptr()),
                  dy_unaligned=dict(dyp=dy.data_ptr() + 4), w_unaligned=dict(wp=wt.data_ptr() + 4))
    for name, kw in bad_dg.items():
        assert dg(**kw) == E, 'dgrad ' + name
    bad_pb = dict(null_x=dict(xp=None), null_dy=dict(dyp=None), null_dx=dict(dxp=None), h0=dict(H=0), c0=dict(c=0),
                  x_out=dict(x_off=1), dy_out=dict(dy_off=9), dx_out=dict(dx_off=1), dx_neg=dict(dx_off=-1), relu2=dict(relu=2),
                  alias_x=dict(dxp=x.data_ptr()), alias_dy=dict(dxp=dy.data_ptr()))
    for name, kw in bad_pb.items():
        assert pb(**kw) == E, 'pool ' + name
    import ctypes
    b, ns = ctypes.c_int64(0), ctypes.c_int(0)
    assert lib.hrnet_conv2d_kxk_wgrad_scratch(F32, 1, 4, 4, 8, 16, 2, ctypes.byref(b), ctypes.byref(ns), None) == E
    assert lib.hrnet_conv2d_kxk_wgrad_scratch(F32, 1, 4, 4, 8, 16, 3, None, ctypes.byref(ns), None) == E
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert torch.equal(t, torch.full_like(t, SENTINEL)), k
    assert wg() == 0 and dg() == 0 and pb() == 0      # and the good calls of the same tables go through
    torch.cuda.synchronize()
    for k in ('dw', 'db', 'dx', 'px'):
        assert not (outs[k] == SENTINEL).any(), k
    # the checked host layer refuses before any device call
    for call in (lambda: T.conv_kxk_wgrad(x.cpu(), dy, 16, 3), lambda: T.conv_kxk_wgrad(x, dy, 16, 4),
                 lambda: T.conv_kxk_wgrad(x, dy, 16, 3, cin=6), lambda: T.conv_kxk_wgrad(x, dy, 16, 3, cin_real=9),
                 lambda: T.conv_kxk_wgrad(x, dy, 16, 3, y_off=4), lambda: T.conv_kxk_wgrad(x, dy[:, :2], 16, 3),
                 lambda: T.conv_kxk_wgrad(x, dy, 16, 3, scratch=outs['scratch'][:-1]),
                 lambda: T.conv_kxk_wgrad(x, dy, 16, 3, dw=torch.empty(16, 8, 3, 2, device=DEV)),
                 lambda: T.conv_kxk_dgrad(dy, wt[:-1], 8, 3), lambda: T.conv_kxk_dgrad(dy, wt, 8, 3, cout=14),
                 lambda: T.conv_kxk_dgrad(dy, wt, 8, 3, x_off=4), lambda: T.conv_kxk_dgrad(dy, wt, 8, 3, out=dy),
                 lambda: T.conv_kxk_dgrad(dy, wt, 8, 3, mask=x[:, :2]), lambda: T.conv_kxk_dgrad(dy.double(), wt, 8, 3),
                 lambda: T.maxpool3x3s2_bwd(x, dy), lambda: T.maxpool3x3s2_bwd(x, dy[:, :2, :2], c=17),
                 lambda: T.maxpool3x3s2_bwd(x, dy[:, :2, :2].contiguous(), c=8, dx_off=2),
                 lambda: T.pack_dgrad(torch.zeros(16, 8, 3, 3)), lambda: T.pack_dgrad(torch.zeros(16, 8, 3, 3, device=DEV), ci_lo=8)):
        with pytest.raises(ValueError):
            call()
