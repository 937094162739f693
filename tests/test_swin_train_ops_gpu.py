"""The training kernels of csrc/swin.hip and the decoder's training step through hipnet.swin_train on the GPU: gradients
against torch.autograd.grad of the float64 restatement of tests/swin_ref.py (and tests/swin_train_ref.py) on the CPU.

err = max|dev - ref64| / max|ref64| must stay within swin_ref.bound(e_ref) = 4 * e_ref + 2 * 2^-24, e_ref being the same
measure of the restatement differentiated in float32 on the CPU. Where the float64 gradient is exactly zero the rule has no
denominator and the device must give exact zeros. The inverse gathers are exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import swin_ref as R
import swin_train_ref as TR

pytestmark = pytest.mark.gpu


def _check(label, dev, r64, r32, bad, denom=None):
    dev = dev.detach().double().cpu().numpy()
    r64, r32 = r64.detach().numpy(), r32.detach().double().numpy()
    assert dev.shape == r64.shape and np.isfinite(dev).all(), label
    if denom is None and not np.abs(r64).max() > 0:
        if np.abs(dev).max() != 0:
            bad.append((label, 'exact zeros expected', float(np.abs(dev).max())))
        return
    err, e_ref = R.rel(dev, r64, denom), R.rel(r32, r64, denom)
    print('{}: err {:.3g} e_ref {:.3g} bound {:.3g}'.format(label, err, e_ref, R.bound(e_ref)))
    if not err <= R.bound(e_ref):
        bad.append((label, err, e_ref, R.bound(e_ref)))


def _attn_inputs(B, H, W, heads, hd, ws, seed):
    """float32-valued float64 tensors: qkv (B, H W, 3 C), a non-zero qkv bias and bias table, and dout (B, H W, C)"""
    g = torch.Generator().manual_seed(seed)
    C = heads * hd
    f = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).double()
    return f(B, H * W, 3 * C), 0.5 * f(3 * C) + 0.25, 0.5 * f((2 * ws - 1) ** 2, heads), f(B, H * W, C)


def _attn_ref(qkv, bias, table, dout, H, W, heads, ws, shift, scale, dtype):
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (qkv, bias, table)]
    out = R.attention_from_qkv(leaves[0], leaves[1], leaves[2], H, W, heads, ws, shift, scale)
    return torch.autograd.grad(out, leaves, dout.to(dtype))


def _attn_device(qkv, bias, table, dout, H, W, heads, ws, shift, scale):
    from hipnet import swin_train as ST
    leaves = [t.float().cuda().requires_grad_(True) for t in (qkv, bias, table)]
    out = ST.window_attention(leaves[0], leaves[1], leaves[2], H, W, heads, ws, shift, scale)
    grads = torch.autograd.grad(out, leaves, dout.float().cuda())
    torch.cuda.synchronize()
    return grads


# (H, W), ws, shifts, (heads, hd) pairs
ATTENTION_CASES = [
    ((4, 4), 7, (0, 3), ((3, 16), (3, 32))),              # one padded window
    ((7, 7), 7, (0, 3), ((3, 16), (3, 32))),              # no padding: all of dqkv_bias exactly 0
    ((8, 8), 7, (0, 3), ((3, 16), (1, 1))),               # 2x2 windows
    ((11, 7), 3, (0, 1), ((3, 16),)),                     # ws = 3
    ((1, 1), 7, (0, 3), ((3, 16),)),                      # a single token
    ((9, 6), 7, (0, 3), ((2, 48), (1, 128))),             # 2 and 4 staged chunks
]


@pytest.mark.parametrize('HW,ws,shifts,shapes', ATTENTION_CASES)
def test_window_attention_backward_against_the_restatement(HW, ws, shifts, shapes):
    """every (shift, heads x hd, B in (1, 3)) of the row; each run twice, the bits must be equal. dqkv, the k / v thirds of
    dqkv_bias and dtable are each under the rule; the q third of dqkv_bias is exactly zero, and with no padded token
    (7 x 7) all of it is.
    MI355X, err / e_ref / bound of the closest case per output over the 112 checked triples: dqkv 1.69e-07 / 5.34e-08 /
    3.33e-07 (8x8, shift 3, heads 1, hd 1, B 1: 0.51 of the bound), dbias k, v 1.0e-07 / 2.0e-08 / 1.99e-07 (8x8, shift 0,
    hd 1, B 3: two values, 0.50), dtable 3.02e-07 / 1.51e-07 / 7.24e-07 (4x4, shift 0, hd 32, B 3: 0.42). With the partial
    sums of dbias and dtable kept in float32 the hd 1 case gave 2.05e-07 against its bound of 1.99e-07: they are float64
    from the first addition on."""
    H, W = HW
    bad = []
    for heads, hd in shapes:
        C = heads * hd
        for shift in shifts:
            for B in (1, 3):
                qkv, bias, table, dout = _attn_inputs(B, H, W, heads, hd, ws, seed=1000 * H + 10 * W + shift + B)
                scale = hd ** -0.5
                args = (qkv, bias, table, dout, H, W, heads, ws, shift, scale)
                r64, r32 = _attn_ref(*args, dtype=torch.float64), _attn_ref(*args, dtype=torch.float32)
                a, b = _attn_device(*args), _attn_device(*args)
                assert all(torch.equal(s, t) for s, t in zip(a, b)), 'two runs differ'
                label = '{}x{} ws {} shift {} heads {} hd {} B {}'.format(H, W, ws, shift, heads, hd, B)
                _check(label + ' dqkv', a[0], r64[0], r32[0], bad)
                assert float(r64[1][:C].abs().max()) == 0                   # the restatement's own q third
                if float(a[1][:C].abs().max()) != 0:
                    bad.append((label, 'q third of dqkv_bias is not exactly zero'))
                if H % ws == 0 and W % ws == 0:
                    assert float(r64[1].abs().max()) == 0
                _check(label + ' dbias k, v', a[1][C:], r64[1][C:], r32[1][C:], bad)
                _check(label + ' dtable', a[2], r64[2], r32[2], bad)
    assert not bad, bad


@pytest.mark.parametrize('shift', [0, 3])
def test_window_attention_backward_stays_in_its_window(shift):
    """8 x 8 tokens, ws 7, B = 2: a dout that is zero outside the first window of image 1 leaves the dqkv rows of every other
    window, and of image 0, exactly zero; inside the window it is the full run's value only where dout was kept whole
    (checked against the restatement under the rule)."""
    H = W = 8
    heads, hd, ws = 3, 16, 7
    qkv, bias, table, dout = _attn_inputs(2, H, W, heads, hd, ws, seed=91 + shift)
    pi, pj = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    Hp = Wp = 14
    inside = (((pi - shift) % Hp) // ws == 0) & (((pj - shift) % Wp) // ws == 0)
    keep = torch.zeros(2, H * W, dtype=torch.bool)
    keep[1] = inside.reshape(-1)
    assert 0 < int(keep.sum()) < H * W
    dout = dout * keep[:, :, None]
    args = (qkv, bias, table, dout, H, W, heads, ws, shift, 0.25)
    dev = _attn_device(*args)
    assert float(dev[0][~keep.cuda()].abs().max()) == 0
    assert float(dev[0][keep.cuda()].abs().min()) > 0
    bad = []
    _check('one window', dev[0], _attn_ref(*args, dtype=torch.float64)[0], _attn_ref(*args, dtype=torch.float32)[0], bad)
    assert not bad, bad


def test_window_attention_backward_computes_only_what_is_asked():
    from hipnet import swin_train as ST
    H = W = 4
    qkv, bias, table, dout = _attn_inputs(1, H, W, 3, 16, 7, seed=5)
    q = qkv.float().cuda().requires_grad_(True)
    out = ST.window_attention(q, bias.float().cuda(), table.float().cuda(), H, W, 3, 7, 0, 0.25)
    gq, = torch.autograd.grad(out, [q], dout.float().cuda())
    full = _attn_device(qkv, bias, table, dout, H, W, 3, 7, 0, 0.25)
    assert torch.equal(gq, full[0])
    with torch.no_grad():
        assert not ST.window_attention(q, bias.float().cuda(), table.float().cuda(), H, W, 3, 7, 0, 0.25).requires_grad


@pytest.mark.parametrize('H,W', [(8, 8), (5, 3), (1, 1)])
def test_merge_scatter_is_the_gathers_inverse(H, W):
    from hipnet import swin_train as ST
    g = torch.Generator().manual_seed(H * 10 + W)
    B, C = 2, 48
    x = torch.randn(B, H * W, C, generator=g, dtype=torch.float32)
    dy = torch.randn(B, ((H + 1) // 2) * ((W + 1) // 2), 4 * C, generator=g, dtype=torch.float32)
    xr = x.clone().requires_grad_(True)
    want, = torch.autograd.grad(R.merge_gather(xr, H, W), [xr], dy)
    xd = x.cuda().requires_grad_(True)
    y = ST.merge_gather(xd, H, W)
    assert torch.equal(y.detach().cpu(), R.merge_gather(x, H, W))
    got, = torch.autograd.grad(y, [xd], dy.cuda())
    assert torch.equal(got.cpu(), want)                                    # exact: every element is written once
    if H % 2 or W % 2:
        # a gradient that lives only at the zero padding reaches nothing
        pad = (R.merge_gather(torch.ones_like(x), H, W) == 0).float()
        assert float(pad.sum()) > 0
        got, = torch.autograd.grad(ST.merge_gather(xd, H, W), [xd], (dy * pad).cuda())
        assert float(got.abs().max()) == 0


@pytest.mark.parametrize('Cin,H,W,p', [(3, 41, 25, 4), (480, 16, 16, 2)])
def test_patch_rows_backward_is_the_gathers_inverse(Cin, H, W, p):
    from hipnet import swin_train as ST
    g = torch.Generator().manual_seed(Cin + p)
    B = 2
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float32)
    xr = x.clone().requires_grad_(True)
    rows, Hp, Wp = R.embed_rows(xr, p)
    drows = torch.randn(rows.shape, generator=g, dtype=torch.float32)
    want, = torch.autograd.grad(rows, [xr], drows)
    xd = x.cuda().requires_grad_(True)
    got_rows, Hd, Wd = ST.patch_rows(xd, p)
    assert (Hd, Wd) == (Hp, Wp) and torch.equal(got_rows.detach().cpu(), rows.detach())
    got, = torch.autograd.grad(got_rows, [xd], drows.cuda())
    assert torch.equal(got.cpu(), want)
    if H % p or W % p:
        pad = (R.embed_rows(torch.ones_like(x), p)[0] == 0).float()
        assert float(pad.sum()) > 0
        got, = torch.autograd.grad(ST.patch_rows(xd, p)[0], [xd], (drows * pad).cuda())
        assert float(got.abs().max()) == 0


@pytest.mark.parametrize('size,cin', [(1, 96), (4, 96), (1, 768), (4, 768)])
def test_decoder_training_step_against_torch(size, cin):
    """ConvTranspose2d(cin, cin / 2, 3, 2, 1, 1) + bias, Conv2d 1x1 + bias, BatchNorm2d on batch statistics with negative
    gammas, ReLU, B = 2, and its backward for a random upstream gradient, against torch.nn.functional in float64: the output,
    the input gradient and every parameter gradient are under the rule; so are the updated running statistics, and
    num_batches_tracked is 1. Both convolution biases sit under the BatchNorm (the transposed convolution's through the
    linear 1x1): their gradients are zero analytically and rounding noise of the order of 1e-17 in float64, so the rule's own
    denominator is noise; they are held with max|dbeta| as the denominator.
    MI355X, err / e_ref / bound: the closest is dgamma of 1x1 768 -> 384 at 9.38e-07 / 5.27e-07 / 2.23e-06 (0.42); the input
    gradient of 4x4 768 -> 384 is 4.23e-07 / 4.34e-07 / 1.86e-06 on hrnet_swin_deconv_dgrad (2.92e-06, beyond the bound, on
    the single float32 chain of the stride-2 form of hrnet_conv2d); the 1x1 bias gradient is 0 against 3e-16."""
    from hipnet import swin_train as ST
    g = torch.Generator().manual_seed(size * 1000 + cin + 1)
    B, cout = 2, cin // 2
    f = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).double()
    x = f(B, cin, size, size)
    P = [f(cin, cout, 3, 3) / (cin * 2.25) ** 0.5, 0.1 * f(cout) + 0.05, f(cout, cout, 1, 1) / cout ** 0.5,
         0.1 * f(cout) + 0.05,
         (torch.rand(cout, generator=g).double() + 0.5) * torch.where(torch.arange(cout) % 3 == 0, -1.0, 1.0).double(),
         0.2 * f(cout)]
    mean0, var0 = (0.3 * f(cout)).float().double(), (torch.rand(cout, generator=g) * 1.5 + 0.5).double()
    dy = f(B, cout, 2 * size, 2 * size)

    def ref(dt):
        leaves = [t.to(dt).clone().requires_grad_(True) for t in [x] + P]
        xx, wT, bT, w1, b1, gamma, beta = leaves
        rm, rv = mean0.to(dt).clone(), var0.to(dt).clone()
        y = F.conv_transpose2d(xx, wT, bT, stride=2, padding=1, output_padding=1)
        y = torch.relu(F.batch_norm(F.conv2d(y, w1, b1), rm, rv, gamma, beta, True, 0.1, 1e-5))
        return [y] + list(torch.autograd.grad(y, leaves, dy.to(dt))) + [rm, rv]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert float((r64[0] == 0).double().mean()) > 0.2                   # the ReLU does cut
    up = torch.nn.ConvTranspose2d(cin, cout, 3, stride=2, padding=1, output_padding=1)
    conv, bn = torch.nn.Conv2d(cout, cout, 1), torch.nn.BatchNorm2d(cout, momentum=0.1)
    with torch.no_grad():
        for dst, src in zip((up.weight, up.bias, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean,
                             bn.running_var), P + [mean0, var0]):
            dst.copy_(src.float())
    up, conv, bn = up.cuda(), conv.cuda(), bn.cuda()
    xd = x.float().cuda().permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    y = ST.decoder_step(xd, up, conv, bn)
    assert tuple(y.shape) == (B, 2 * size, 2 * size, cout)
    leaves = [xd, up.weight, up.bias, conv.weight, conv.bias, bn.weight, bn.bias]
    grads = torch.autograd.grad(y, leaves, dy.float().cuda().permute(0, 2, 3, 1).contiguous())
    torch.cuda.synchronize()
    assert int(bn.num_batches_tracked) == 1
    bad = []
    tag = 'decoder step {}x{} {} -> {} '.format(size, size, cin, cout)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    _check(tag + 'y', nchw(y), r64[0], r32[0], bad)
    _check(tag + 'dx', nchw(grads[0]), r64[1], r32[1], bad)
    dbeta = float(r64[7].abs().max())
    for k, name in enumerate(('dW up', 'db up', 'dW 1x1', 'db 1x1', 'dgamma', 'dbeta'), start=1):
        _check(tag + name, grads[k], r64[k + 1], r32[k + 1], bad, denom=dbeta if name.startswith('db ') else None)
    _check(tag + 'running_mean', bn.running_mean, r64[8], r32[8], bad)
    _check(tag + 'running_var', bn.running_var, r64[9], r32[9], bad)
    assert not bad, bad
