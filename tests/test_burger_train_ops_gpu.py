"""The training ops of pose_hrnet_hamburger on the GPU (csrc/burger_train.hip through hipnet.burger_train, the one-step ham
gradient through hipnet.nmf_train) against float64 on the same float32 inputs, each under the project's rule
err = max|dev - ref64| / max|ref64| <= bound(e_ref) = 4 * e_ref + 2 * 2^-24, e_ref being the same measure of the float32
computation on the CPU. Each test prints its figures before it asserts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hamburger_ref as R
import hamburger_train_ref as T

pytestmark = pytest.mark.gpu
ROWS = [1, 3, 257, 4099]          # one row, a tail after the vector width, more than one workgroup, a prime
_CACHE = {}


def _hold(label, dev, ref64, ref32):
    dev = dev.detach().double().cpu().numpy() if isinstance(dev, torch.Tensor) else np.asarray(dev, dtype=np.float64)
    ref64, ref32 = (np.asarray(r.detach().double().numpy() if isinstance(r, torch.Tensor) else r) for r in (ref64, ref32))
    err, e_ref = R.rel(dev, ref64), R.rel(ref32, ref64)
    print('{}: err {:.3g}, e_ref {:.3g}, bound {:.3g}'.format(label, err, e_ref, R.bound(e_ref)))
    assert e_ref <= 1e-4 and err <= R.bound(e_ref), label


# ---- burger_mix ----------------------------------------------------------------------------------------------------------
def _mix_data(rows, C, coef_ham):
    key = ('mix', rows, C, coef_ham)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(17 * rows + C)
        u, s, gy = (torch.randn(rows, C, generator=g) for _ in range(3))
        ch, cs = torch.tensor([coef_ham]), torch.tensor([0.8125])
        refs = {}
        for dt in (torch.float64, torch.float32):
            a, b, h, c = (t.to(dt).clone().requires_grad_(True) for t in (u, s, ch, cs))       # the cached inputs stay as drawn
            out = torch.relu(h * a + c * b)
            refs[dt] = [out.detach()] + list(torch.autograd.grad(out, [a, b, h, c], gy.to(dt)))
        _CACHE[key] = (u, s, gy, ch, cs, refs[torch.float64], refs[torch.float32])
    return _CACHE[key]


def _offset(t):
    """the same values at a pointer that is 4-byte but not 16-byte aligned"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
    flat[1:] = t.reshape(-1).cuda()
    v = flat[1:].reshape(t.shape)
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize('C', [16, 48])
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('coef_ham', [0.0, 1.375])
def test_burger_mix_and_backward(rows, C, coef_ham):
    from hipnet import burger_train as BT
    u, s, gy, ch, cs, r64, r32 = _mix_data(rows, C, coef_ham)
    for place in (lambda t: t.cuda(), _offset):                     # the 16-byte path, then the element-wise one
        du_, su_, ch_, cs_ = (place(t).requires_grad_(True) for t in (u, s, ch, cs))
        out = BT.burger_mix(du_, su_, ch_, cs_)
        grads = torch.autograd.grad(out, [du_, su_, ch_, cs_], place(gy))
        torch.cuda.synchronize()
        for name, dev, a, b in zip(('out', 'du', 'ds', 'dcoef_ham', 'dcoef_shortcut'), [out] + list(grads), r64, r32):
            if name == 'du' and coef_ham == 0.0:
                assert not bool(grads[0].any())                    # the reference's start: exactly zero
                continue
            _hold('{} rows {} C {}'.format(name, rows, C), dev, a, b)


def test_burger_mix_aliases_and_equal_bits():
    from hipnet import burger_train as BT
    rows, C = 4099, 48
    u, s, gy, ch, cs, r64, r32 = _mix_data(rows, C, 1.375)
    U, S_, G, H, Cs = (t.cuda() for t in (u, s, gy, ch, cs))
    out = BT.burger_mix(U, S_, H, Cs)
    assert not out.requires_grad
    first = BT.mix_backward(G, out, U, S_, H, Cs)
    again = BT.mix_backward(G, out, U, S_, H, Cs)
    assert all(torch.equal(a, b) for a, b in zip(first, again))      # dcoef included: the sums have one order
    only = BT.mix_backward(G, out, U, S_, H, Cs, want_du=False, want_dcoef=False)
    assert only[0] is None and only[2] is None and torch.equal(only[1], first[1])
    g_alias = G.clone()
    du, _, dcoef = BT.mix_backward(g_alias, out, U, S_, H, Cs, du=g_alias)         # du written over g
    assert du.data_ptr() == g_alias.data_ptr() and torch.equal(du, first[0]) and torch.equal(dcoef, first[2])
    u_alias = U.clone()
    BT._mix_forward(u_alias, S_, H, Cs, out=u_alias)                                # out written over u
    assert torch.equal(u_alias, out)
    _hold('dcoef', first[2], torch.stack([r64[3], r64[4]]).reshape(2), torch.stack([r32[3], r32[4]]).reshape(2))


# ---- dropout2d -----------------------------------------------------------------------------------------------------------
def test_dropout2d():
    from hipnet import burger_train as BT
    B, P, C = 2, 35, 48
    g = torch.Generator().manual_seed(5)
    x, gy = torch.randn(B, 5, 7, C, generator=g), torch.randn(B, 5, 7, C, generator=g)
    keep = ((torch.rand(B, C, generator=g) >= 0.3).float() / 0.9)
    keep[1] = 0.0                                                   # a whole sample dropped
    want, dwant = x * keep.reshape(B, 1, 1, C), gy * keep.reshape(B, 1, 1, C)
    for place in (lambda t: t.cuda(), _offset):
        xd = place(x).requires_grad_(True)
        y = BT.dropout2d(xd, place(keep))
        dx, = torch.autograd.grad(y, xd, place(gy))
        assert torch.equal(y.cpu(), want) and torch.equal(dx.cpu(), dwant)           # one exact product per element
    assert not bool(y[1].any()) and P == 35
    xa = x.cuda()
    BT.C.call('hrnet_dropout2d', xa.data_ptr(), keep.cuda().data_ptr(), xa.data_ptr(), B, P, C, BT.C.stream_ptr())
    assert torch.equal(xa.cpu(), want)                              # y written over x


# ---- the hams ------------------------------------------------------------------------------------------------------------
def _ham_data(S, Rr, steps):
    key = ('ham', S, Rr, steps)
    if key not in _CACHE:
        B, H, W, C = 2, 5, 7, 48
        g = torch.Generator().manual_seed(100 * S + Rr + steps)
        low = torch.relu(torch.randn(B, C, H, W, generator=g) + 0.3)
        specs = [(True, 0, 24, S), (False, 24, 24, S)]
        bases = [R.normalise(torch.rand(B * S, 24 // S, Rr, generator=g)), R.normalise(torch.rand(B * S, H * W, Rr, generator=g))]
        gy = torch.randn(B, C, H, W, generator=g)
        refs = {}
        for dt in (torch.float64, torch.float32):
            x = low.to(dt).clone().requires_grad_(True)
            out = torch.cat([T.nmf2d_train(x[:, c0:c0 + ch], b.to(dt), steps, sp, S)
                             for (sp, c0, ch, _), b in zip(specs, bases)], dim=1)
            refs[dt] = (out.detach(), torch.autograd.grad(out, x, gy.to(dt))[0])
        _CACHE[key] = (low, specs, bases, gy, refs[torch.float64], refs[torch.float32])
    return _CACHE[key]


@pytest.mark.parametrize('steps', [0, 6])
@pytest.mark.parametrize('Rr', [8, 40])
@pytest.mark.parametrize('S', [1, 2])
def test_hams_train(S, Rr, steps):
    """a spatial ham on channels 0-23 and a channel ham on 24-47 of a (2, 5, 7, 48) NHWC map; S = 2 forces the per-image
    views of a channel half; R = 40 is larger than D"""
    from hipnet import nmf_train as NT
    low, specs, bases, gy, r64, r32 = _ham_data(S, Rr, steps)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().cuda()
    x = nhwc(low).requires_grad_(True)
    dev_bases = [b.cuda() for b in bases]
    out = NT.hams_train(x, specs, dev_bases, steps)
    dx, = torch.autograd.grad(out, x, nhwc(gy), retain_graph=True)
    torch.cuda.synchronize()
    tag = 'S {} R {} steps {}'.format(S, Rr, steps)
    _hold('hams out ' + tag, out.permute(0, 3, 1, 2), r64[0], r32[0])
    _hold('hams dlow ' + tag, dx.permute(0, 3, 1, 2), r64[1], r32[1])
    # a gradient that is a slice of a wider tensor is read in place; one with strided channels is copied first
    wide = torch.zeros(2, 5, 7, 64, device='cuda')
    wide[..., :48] = nhwc(gy)
    d2, = torch.autograd.grad(out, x, wide[..., :48], retain_graph=True)
    d3, = torch.autograd.grad(out, x, gy.cuda().permute(0, 2, 3, 1))
    assert not wide[..., :48].is_contiguous() and torch.equal(d2, dx) and torch.equal(d3, dx)
    with torch.no_grad():
        plain = NT.hams_train(x.detach(), specs, dev_bases, steps)
    assert torch.equal(plain, out)


def test_hams_train_equals_the_inference_path():
    from hipnet import nmf
    from hipnet import nmf_train as NT
    low, specs, bases, gy, _, _ = _ham_data(2, 8, 6)
    x = low.permute(0, 2, 3, 1).contiguous().cuda()
    out = NT.hams_train(x.clone().requires_grad_(True), specs, [b.cuda() for b in bases], 6)
    want = torch.empty_like(x)
    with torch.no_grad():
        for (sp, c0, ch, S), b in zip(specs, bases):
            nmf.nmf2d(x.permute(0, 3, 1, 2)[:, c0:c0 + ch], b.cuda(), 6, sp, S, out=want.permute(0, 3, 1, 2)[:, c0:c0 + ch])
    assert torch.equal(out, want)


# ---- Conv2d, BatchNorm2d on batch statistics, ReLU -------------------------------------------------------------------------
@pytest.mark.parametrize('ks', [1, 3])
def test_conv_bn_relu_train_statistics(ks):
    """momentum 1.0: the running buffers are the batch mean and the unbiased batch variance themselves"""
    from hipnet import burger_train as BT
    g = torch.Generator().manual_seed(7 + ks)
    B, H, W, ci, co = 2, 5, 7, 40, 24
    conv = torch.nn.Conv2d(ci, co, ks, padding=ks // 2, bias=False)
    bn = torch.nn.BatchNorm2d(co, momentum=1.0)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (ci * ks * ks) ** 0.5)
        bn.weight.copy_(torch.rand(co, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(co, generator=g) * 0.2)
    x = torch.randn(B, ci, H, W, generator=g)
    refs = []
    for dt in (torch.float64, torch.float32):
        z = F.conv2d(x.to(dt), conv.weight.detach().to(dt), padding=ks // 2)
        mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=True)
        y = torch.relu(F.batch_norm(z, None, None, bn.weight.detach().to(dt), bn.bias.detach().to(dt), True, 0.0, bn.eps))
        refs.append((mean, var, y))
    conv, bn = conv.cuda(), bn.cuda()
    xd = torch.zeros(B, H, W, 48, device='cuda')
    xd[..., :ci] = x.permute(0, 2, 3, 1).cuda()
    y = BT.conv_bn_relu_train(xd, conv, bn, ks)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (B, H, W, 32) and not bool(y[..., co:].any())
    _hold('running_mean ks {}'.format(ks), bn.running_mean, refs[0][0], refs[1][0])
    _hold('running_var ks {}'.format(ks), bn.running_var, refs[0][1], refs[1][1])
    _hold('y ks {}'.format(ks), y[..., :co].permute(0, 3, 1, 2), refs[0][2], refs[1][2])
    assert int(bn.num_batches_tracked) == 0


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    from hipnet import burger_train as BT
    from hipnet import nmf_train as NT
    x, c = torch.zeros(2, 5, 7, 48, device='cuda'), torch.ones(1, device='cuda')
    keep = torch.ones(2, 48, device='cuda')
    with pytest.raises(ValueError, match='HIP-device'):
        BT.burger_mix(x.cpu(), x, c, c)
    with pytest.raises(ValueError, match='HIP-device'):
        BT.dropout2d(x, keep.cpu())
    with pytest.raises(ValueError, match='float32 only'):
        BT.burger_mix(x.double(), x, c, c)
    with pytest.raises(ValueError, match='float32 only'):
        NT.hams_train(x.half(), [(True, 0, 48, 1)], [torch.zeros(2, 48, 8, device='cuda')], 6)
    with pytest.raises(ValueError, match='multiple of 16'):
        BT.burger_mix(x[..., :24].contiguous(), x[..., :24].contiguous(), c, c)
    with pytest.raises(ValueError, match='multiple of 16'):
        BT.dropout2d(x[..., :24].contiguous(), keep[:, :24].contiguous())
    with pytest.raises(ValueError, match='one shape'):
        BT.burger_mix(x, x[:1], c, c)
    with pytest.raises(ValueError, match='bases'):
        NT.hams_train(x, [(True, 0, 48, 1)], [torch.zeros(2, 40, 8, device='cuda')], 6)
    with pytest.raises(ValueError, match='disjoint'):
        NT.hams_train(x, [(True, 0, 32, 1), (False, 24, 24, 1)],
                      [torch.zeros(2, 32, 8, device='cuda'), torch.zeros(2, 35, 8, device='cuda')], 6)
    need = BT.mix_scratch(2 * 5 * 7, 48)
    assert need == 2 * 4                                             # 840 float4 over workgroups of 256 threads
    with pytest.raises(RuntimeError, match='scratch of {} doubles'.format(need - 1)):
        BT.mix_backward(x, x, x, x, c, c, scratch=torch.empty(need - 1, dtype=torch.float64, device='cuda'))
    with pytest.raises(RuntimeError, match='C = 24'):
        BT.C.call('hrnet_burger_mix', x.data_ptr(), x.data_ptr(), c.data_ptr(), c.data_ptr(), x.data_ptr(), 70, 24,
                  BT.C.stream_ptr())
