"""The f32 / bf16 NHWC layer ops of the heads on the GPU (hipnet.nhwc, and hipnet.burger_train.conv_bn_relu_train on its
BatchNorm helpers) against F.conv2d, F.batch_norm(training=True) and relu in float64 on the same float32 inputs, each
under the project's rule err = max|dev - ref64| / max|ref64| <= bound(e_ref) = 4 * e_ref + 2 * 2^-24, e_ref being the same
measure of the float32 computation on the CPU. 40 real input channels in a 48-channel map, 24 real output channels in 32,
on a (2, 5, 7) map: pad channels on both sides, an odd map, more than one 16-channel group. Each test prints its figures
before it asserts. MI355X: e_ref at most 3.3e-7; the closest to its bound is dgamma of the 3x3 ConvBNReLU, err 3.36e-7 under
7.52e-7; the layout, packing and no-graph comparisons are equal bits."""
import pytest
import torch
import torch.nn.functional as F

import hamburger_ref as R

pytestmark = pytest.mark.gpu
B, H, W, CI, CIP, CO, COP = 2, 5, 7, 40, 48, 24, 32
_CACHE = {}


def _api():
    from hipnet import burger_train as BT
    from hipnet import nhwc
    import types
    return types.SimpleNamespace(
        conv1x1_train=nhwc.conv1x1_train, conv_bn_relu_train=BT.conv_bn_relu_train, conv_nhwc=nhwc.conv_nhwc,
        to_nhwc=nhwc.to_nhwc, to_nchw=nhwc.to_nchw, pack=nhwc.pack, pack_taps=nhwc.pack_taps)


def _hold(label, dev, ref64, ref32):
    dev, ref64, ref32 = (t.detach().double().cpu().numpy() for t in (dev, ref64, ref32))
    err, e_ref = R.rel(dev, ref64), R.rel(ref32, ref64)
    print('{}: err {:.3g}, e_ref {:.3g}, bound {:.3g}'.format(label, err, e_ref, R.bound(e_ref)))
    assert e_ref <= 1e-4 and err <= R.bound(e_ref), label


def _nhwc(t, cp):
    """NCHW CPU tensor -> NHWC on the device with zero pad channels up to cp"""
    out = torch.zeros(t.shape[0], t.shape[2], t.shape[3], cp, device='cuda')
    out[..., :t.shape[1]] = t.permute(0, 2, 3, 1).cuda()
    return out


def _nchw(t, c):
    return t[..., :c].permute(0, 3, 1, 2)


def _data(ks, seed):
    """the inputs as drawn (float32, CPU): x, weight, bias, gamma, beta, gy"""
    key = ('data', ks)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(seed)
        _CACHE[key] = dict(x=torch.randn(B, CI, H, W, generator=g),
                           w=torch.randn(CO, CI, ks, ks, generator=g) / (CI * ks * ks) ** 0.5,
                           b=torch.randn(CO, generator=g) * 0.5, gamma=torch.rand(CO, generator=g) + 0.5,
                           beta=torch.randn(CO, generator=g) * 0.2, gy=torch.randn(B, CO, H, W, generator=g))
    return _CACHE[key]


# ---- Conv2d 1x1 (+ bias) (+ ReLU) ----------------------------------------------------------------------------------------
def _conv1x1_refs(bias, relu):
    key = ('conv1x1', bias, relu)
    if key not in _CACHE:
        d, refs = _data(1, 11), {}
        for dt in (torch.float64, torch.float32):
            x, w, b = (d[k].to(dt).clone().requires_grad_(True) for k in ('x', 'w', 'b'))
            y = F.conv2d(x, w, b if bias else None)
            y = torch.relu(y) if relu else y
            grads = torch.autograd.grad(y, [x, w] + ([b] if bias else []), d['gy'].to(dt))
            refs[dt] = [y.detach()] + list(grads)
        _CACHE[key] = refs
    return _CACHE[key]


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('bias', [False, True])
def test_conv1x1_train(bias, relu):
    A = _api()
    d, refs = _data(1, 11), _conv1x1_refs(bias, relu)
    conv = torch.nn.Conv2d(CI, CO, 1, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(d['w'])
        if bias:
            conv.bias.copy_(d['b'])
    conv = conv.cuda()
    params = [conv.weight] + ([conv.bias] if bias else [])
    x, gy = _nhwc(d['x'], CIP).requires_grad_(True), _nhwc(d['gy'], COP)
    y = A.conv1x1_train(x, conv, relu_out=relu)
    grads = torch.autograd.grad(y, [x] + params, gy)
    torch.cuda.synchronize()
    tag = ' bias {} relu {}'.format(bias, relu)
    assert tuple(y.shape) == (B, H, W, COP) and not bool(y[..., CO:].any()) and not bool(grads[0][..., CI:].any())
    dev = [_nchw(y, CO), _nchw(grads[0], CI)] + list(grads[1:])
    for name, got, r64, r32 in zip(('y', 'dx', 'dw', 'db'), dev, refs[torch.float64], refs[torch.float32]):
        _hold(name + tag, got, r64, r32)
    # the parameters' gradients do not depend on whether the input wants one; no graph, the same forward
    y2 = A.conv1x1_train(x.detach(), conv, relu_out=relu)
    only = torch.autograd.grad(y2, params, gy)
    assert torch.equal(y2, y) and all(torch.equal(a, b) for a, b in zip(only, grads[1:]))
    with torch.no_grad():
        plain = A.conv1x1_train(x, conv, relu_out=relu)
    assert not plain.requires_grad and torch.equal(plain, y)


# ---- Conv2d, BatchNorm2d on batch statistics, ReLU: the gradients --------------------------------------------------------
def _conv_bn_refs(ks):
    key = ('conv_bn', ks)
    if key not in _CACHE:
        d, refs = _data(ks, 13 + ks), {}
        for dt in (torch.float64, torch.float32):
            x, w, gamma, beta = (d[k].to(dt).clone().requires_grad_(True) for k in ('x', 'w', 'gamma', 'beta'))
            y = torch.relu(F.batch_norm(F.conv2d(x, w, padding=ks // 2), None, None, gamma, beta, True, 0.0, 1e-5))
            refs[dt] = list(torch.autograd.grad(y, [x, w, gamma, beta], d['gy'].to(dt)))
        _CACHE[key] = refs
    return _CACHE[key]


@pytest.mark.parametrize('ks', [1, 3])
def test_conv_bn_relu_train_gradients(ks):
    A = _api()
    d, refs = _data(ks, 13 + ks), _conv_bn_refs(ks)
    conv, bn = torch.nn.Conv2d(CI, CO, ks, padding=ks // 2, bias=False), torch.nn.BatchNorm2d(CO)
    with torch.no_grad():
        conv.weight.copy_(d['w'])
        bn.weight.copy_(d['gamma'])
        bn.bias.copy_(d['beta'])
    conv, bn = conv.cuda(), bn.cuda()
    params = [conv.weight, bn.weight, bn.bias]
    x, gy = _nhwc(d['x'], CIP).requires_grad_(True), _nhwc(d['gy'], COP)
    y = A.conv_bn_relu_train(x, conv, bn, ks)
    grads = torch.autograd.grad(y, [x] + params, gy)
    y2 = A.conv_bn_relu_train(x.detach(), conv, bn, ks)                  # no input gradient is formed
    only = torch.autograd.grad(y2, params, gy)
    torch.cuda.synchronize()
    assert not bool(grads[0][..., CI:].any()) and torch.equal(y2, y) and int(bn.num_batches_tracked) == 0
    names = ('dx', 'dw', 'dgamma', 'dbeta')
    for name, got, r64, r32 in zip(names, [_nchw(grads[0], CI)] + list(grads[1:]), refs[torch.float64], refs[torch.float32]):
        _hold('{} ks {}'.format(name, ks), got, r64, r32)
    for name, got, r64, r32 in zip(names[1:], only, refs[torch.float64][1:], refs[torch.float32][1:]):
        _hold('{} ks {}, x without a gradient'.format(name, ks), got, r64, r32)


# ---- layout --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('shape,cp', [((2, 3, 5, 7), 16), ((1, 21, 4, 4), 32)])
def test_layout_round_trip_and_backward(shape, cp, dtype):
    A = _api()
    g = torch.Generator().manual_seed(shape[1] + cp)
    c = shape[1]
    x = torch.randn(shape, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(shape[0], shape[2], shape[3], cp, generator=g).cuda().to(dtype)     # pad channels not zero
    y = A.to_nhwc(x, cp, dtype)
    assert y.dtype == dtype and tuple(y.shape) == (shape[0], shape[2], shape[3], cp)
    assert torch.equal(y[..., :c], x.detach().to(dtype).permute(0, 2, 3, 1)) and not bool(y[..., c:].any())
    dx, = torch.autograd.grad(y, x, gy)
    assert dx.dtype == torch.float32 and torch.equal(dx, A.to_nchw(gy, c))              # the backward of each is the other
    assert torch.equal(dx, gy[..., :c].permute(0, 3, 1, 2).float())
    yl = y.detach().requires_grad_(True)
    z = A.to_nchw(yl, c)
    assert z.dtype == torch.float32 and torch.equal(z, x.detach().to(dtype).float())    # the round trip is exact
    gz = torch.randn(shape, generator=g).cuda()
    dy, = torch.autograd.grad(z, yl, gz)
    assert dy.dtype == dtype and torch.equal(dy, A.to_nhwc(gz, cp, dtype)) and not bool(dy[..., c:].any())
    assert torch.equal(dy[..., :c], gz.to(dtype).permute(0, 2, 3, 1))


# ---- the nine taps of a 3x3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1])
def test_pack_taps_equals_nine_packs(mode):
    A = _api()
    w = _data(3, 16)['w'].cuda()
    with torch.cuda.device(w.device):
        taps = A.pack_taps(w, CO, CI, COP, CIP, mode)
        singles = []
        for t in range(9):
            src = 8 - t if mode else t
            singles.append(A.pack(w[:, :, src // 3, src % 3].contiguous(), CO, CI, 1, COP, CIP, mode))
    torch.cuda.synchronize()
    assert tuple(taps.shape) == ((9, COP, CIP) if mode == 0 else (9, CIP, COP)) and taps.is_contiguous()
    assert torch.equal(taps.reshape(9, -1), torch.stack(singles))
    want = torch.zeros(9, COP, CIP)
    want[:, :CO, :CI] = _data(3, 16)['w'].reshape(CO, CI, 9).permute(2, 0, 1)
    if mode:
        want = want.flip(0).transpose(1, 2)
    assert torch.equal(taps.cpu(), want)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    A = _api()
    x = torch.zeros(B, H, W, CIP, device='cuda')
    conv, bn = torch.nn.Conv2d(CI, CO, 1).cuda(), torch.nn.BatchNorm2d(CO).cuda()
    nobias = torch.nn.Conv2d(CI, CO, 1, bias=False).cuda()
    for call in (lambda: A.conv1x1_train(x.cpu(), conv), lambda: A.conv_bn_relu_train(x.cpu(), nobias, bn, 1),
                 lambda: A.to_nhwc(torch.zeros(2, 3, 5, 7), 16), lambda: A.to_nchw(x.cpu(), 21),
                 lambda: A.conv_nhwc(x.cpu(), torch.zeros(COP * CIP, device='cuda'), COP, 1)):
        with pytest.raises(ValueError, match='HIP-device'):
            call()
    for call in (lambda: A.conv1x1_train(x.double(), conv), lambda: A.conv_bn_relu_train(x.double(), nobias, bn, 1),
                 lambda: A.to_nhwc(torch.zeros(2, 3, 5, 7, device='cuda').double(), 16),
                 lambda: A.conv_nhwc(x.double(), torch.zeros(COP * CIP, device='cuda'), COP, 1)):
        with pytest.raises(ValueError, match='float32 only'):
            call()
    narrow = torch.zeros(B, H, W, 24, device='cuda')
    for call in (lambda: A.conv1x1_train(narrow, conv), lambda: A.conv_bn_relu_train(narrow, nobias, bn, 1),
                 lambda: A.to_nhwc(torch.zeros(2, 3, 5, 7, device='cuda'), 24)):
        with pytest.raises(ValueError, match='multiple of 16'):
            call()
    with pytest.raises(NotImplementedError, match='backward is not built'):
        A.conv_nhwc(x.clone().requires_grad_(True), torch.zeros(COP * CIP, device='cuda'), COP, 1)
