"""The 1x1 convolution on NCHW float32 of csrc/pointwise.hip (process_features of the volumetric model), alone, against
torch.nn.functional.conv2d and its autograd in float64 on the CPU. Every case runs twice, by the convention of
tests/test_v2v_gpu.py and tests/test_v2v_train_gpu.py:
 (a) integer lattice: operands in [-2, 2]; the largest sum here is 4 * 12288 < 2^24, so float32 is exact in any order
     and forward, dx, dw and db must EQUAL the reference;
 (b) real-valued, per element, u = 2^-24 - the gamma_K bounds of an fma chain in any order, plus the additions of the
     partial rows:
        forward  (Cin + 2) u (|w| |x| + |bias|)
        dx       (Cout + 1) u (|w|^T |dy|)
        dw       (N P + parts + 2) u (|dy| |x|^T)
        db       (N P + parts + 2) u sum |dy|
Output buffers are pre-filled with NaN, so an unwritten element shows, and a guard region behind each must stay as it
was. The backward runs with all outputs, then with dx, dw or db passed as NULL: the others do not change by a bit, and
a second full run is bit-identical (no atomics). Each test runs in a spawned child (tests/spawned.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from spawned import spawned

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 1024
SENTINEL = 12345.0

# (N, Cin, Cout, P)
CASES = (
    (1, 3, 1, 1),             # every tail at once
    (1, 4, 16, 16),           # exactly one MFMA tile
    (2, 30, 21, 17),          # Cin % 4 = 2, Cout tail, pixel tail, batch
    (1, 480, 32, 256),        # the model's channels on a 16 x 16 map
    (3, 720, 32, 100),        # w48 width, P not a multiple of 16
    (2, 32, 32, 4096),        # many pixel blocks: several partial rows
    (1, 480, 32, 4096),       # the real map
)


def _draw(rng, shape, lattice):
    a = rng.integers(-2, 3, shape).astype(np.float64) if lattice else rng.normal(0.0, 1.0, shape)
    return torch.from_numpy(a.astype(np.float32).astype(np.float64))


def _out(n):
    """n NaNs followed by a guard; returns (whole buffer, the n-element output view)"""
    buf = torch.full((n + GUARD,), float('nan'), dtype=torch.float32, device='cuda')
    buf[n:] = SENTINEL
    return buf, buf[:n]


def _guard_ok(buf, n):
    return bool((buf[n:] == SENTINEL).all().item())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(what, got, ref, bound, lattice):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), (what, 'unwritten or non-finite elements', int((~np.isfinite(got)).sum()))
    if lattice:
        bad = int((got != ref).sum())
        print(what, 'lattice: {} of {} differ'.format(bad, ref.size))
        assert bad == 0, (what, bad)
    else:
        ratio = (np.abs(got - ref) / np.maximum(bound, 1e-300)).max()
        print(what, 'real: largest |error| / bound = {:.3f}'.format(ratio))
        assert ratio <= 1.0, (what, ratio)


def _reference(x, w, b, dy):
    N, Cin, P = x.shape
    Cout = w.shape[0]
    xs = x.reshape(N, Cin, P, 1).clone().requires_grad_(True)
    ws = w.reshape(Cout, Cin, 1, 1).clone().requires_grad_(True)
    bs = b.clone().requires_grad_(True)
    y = F.conv2d(xs, ws, bs)
    y.backward(dy.reshape(N, Cout, P, 1))
    return (y.detach().reshape(N, Cout, P), xs.grad.reshape(N, Cin, P), ws.grad.reshape(Cout, Cin), bs.grad)


def _backward(C, xd, wd, dyd, shape, parts, want):
    """one hrnet_pointwise_nchw_bwd call with the outputs named in `want`; -> {name: (buffer, view, n)}"""
    N, Cin, Cout, P = shape
    sizes = {'dx': N * Cin * P, 'dw': Cout * Cin, 'db': Cout}
    outs = {k: _out(sizes[k]) + (sizes[k],) for k in want}
    floats = parts * (Cout * Cin + Cout)
    sbuf, scratch = _out(floats)
    ptr = {k: (outs[k][1].data_ptr() if k in outs else None) for k in sizes}
    C.call('hrnet_pointwise_nchw_bwd', C.HR_F32, xd.data_ptr(), wd.data_ptr(), dyd.data_ptr(), ptr['dx'], ptr['dw'],
           ptr['db'], scratch.data_ptr(), floats, N, Cin, Cout, P, C.stream_ptr())
    torch.cuda.synchronize()
    assert _guard_ok(sbuf, floats), 'the guard behind the scratch was written'
    for k, (buf, _v, n) in outs.items():
        assert _guard_ok(buf, n), 'the guard behind {} was written'.format(k)
    return outs


def _case(shape, lattice):
    from hipnet import _capi as C
    N, Cin, Cout, P = shape
    rng = np.random.default_rng((N, Cin, Cout, P, int(lattice)))
    x, w, b, dy = (_draw(rng, s, lattice) for s in ((N, Cin, P), (Cout, Cin), (Cout,), (N, Cout, P)))
    y_ref, dx_ref, dw_ref, db_ref = _reference(x, w, b, dy)
    y_abs, dx_abs, dw_abs, db_abs = _reference(x.abs(), w.abs(), b.abs(), dy.abs())
    assert C.call('hrnet_pointwise_nchw_supported', C.HR_F32, Cin, Cout) == 1
    parts = C.call('hrnet_pointwise_nchw_parts', N, P)
    assert parts >= 1
    if shape == (2, 32, 32, 4096):
        assert parts > 1, parts
    xd, wd, bd, dyd = (t.float().cuda().contiguous() for t in (x, w, b, dy))
    tag = '{} parts {}'.format(shape, parts)

    ybuf, y = _out(N * Cout * P)
    C.call('hrnet_pointwise_nchw', C.HR_F32, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), N, Cin, Cout, P,
           C.stream_ptr())
    torch.cuda.synchronize()
    assert _guard_ok(ybuf, N * Cout * P), 'the guard behind y was written'
    _check('forward ' + tag, y.cpu().numpy().reshape(N, Cout, P), y_ref.numpy(), ((Cin + 2) * U * y_abs).numpy(), lattice)
    # without a bias: the same sums, nothing added
    ybuf0, y0 = _out(N * Cout * P)
    C.call('hrnet_pointwise_nchw', C.HR_F32, xd.data_ptr(), wd.data_ptr(), None, y0.data_ptr(), N, Cin, Cout, P,
           C.stream_ptr())
    torch.cuda.synchronize()
    assert _guard_ok(ybuf0, N * Cout * P)
    nb_ref, nb_abs = y_ref - b[None, :, None], y_abs - b.abs()[None, :, None]
    _check('forward, no bias ' + tag, y0.cpu().numpy().reshape(N, Cout, P), nb_ref.numpy(),
           ((Cin + 2) * U * nb_abs).numpy(), lattice)

    full = _backward(C, xd, wd, dyd, shape, parts, ('dx', 'dw', 'db'))
    K = N * P + parts + 2
    _check('dx ' + tag, full['dx'][1].cpu().numpy().reshape(N, Cin, P), dx_ref.numpy(), ((Cout + 1) * U * dx_abs).numpy(),
           lattice)
    _check('dw ' + tag, full['dw'][1].cpu().numpy().reshape(Cout, Cin), dw_ref.numpy(), (K * U * dw_abs).numpy(), lattice)
    _check('db ' + tag, full['db'][1].cpu().numpy(), db_ref.numpy(), (K * U * db_abs).numpy(), lattice)

    again = _backward(C, xd, wd, dyd, shape, parts, ('dx', 'dw', 'db'))
    for k in ('dx', 'dw', 'db'):
        assert torch.equal(_bits(full[k][1]), _bits(again[k][1])), '{}: two runs differ'.format(k)
    for missing in ('dx', 'dw', 'db'):
        want = tuple(k for k in ('dx', 'dw', 'db') if k != missing)
        part = _backward(C, xd, wd, dyd, shape, parts, want)
        for k in want:
            assert torch.equal(_bits(full[k][1]), _bits(part[k][1])), '{} changed with {} = NULL'.format(k, missing)


@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'x'.join(str(v) for v in s))
@spawned
def test_pointwise_lattice(shape):
    _case(shape, True)


@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'x'.join(str(v) for v in s))
@spawned
def test_pointwise_real(shape):
    _case(shape, False)


@spawned
def test_pointwise_autograd_matches_conv2d():
    """models.triangulation.pointwise_conv_nchw through autograd: the same numbers as the raw calls give, held to the
    same bounds against F.conv2d in float64, and the weight is read in place (an in-place update shows at once)"""
    from models.triangulation import pointwise_conv_nchw
    N, Cin, Cout, H, W = 2, 30, 21, 5, 7
    rng = np.random.default_rng(11)
    x, w, b, dy = (_draw(rng, s, False) for s in ((N, Cin, H * W), (Cout, Cin), (Cout,), (N, Cout, H * W)))
    y_ref, dx_ref, dw_ref, db_ref = _reference(x, w, b, dy)
    y_abs, dx_abs, dw_abs, db_abs = _reference(x.abs(), w.abs(), b.abs(), dy.abs())
    xd = x.float().reshape(N, Cin, H, W).cuda().requires_grad_(True)
    conv = torch.nn.Conv2d(Cin, Cout, 1).cuda()
    with torch.no_grad():
        conv.weight.copy_(w.float().reshape(Cout, Cin, 1, 1))
        conv.bias.copy_(b.float())
    y = pointwise_conv_nchw(xd, conv.weight, conv.bias)
    y.backward(dy.float().reshape(N, Cout, H, W).cuda())
    from hipnet import _capi as C
    K = N * H * W + C.call('hrnet_pointwise_nchw_parts', N, H * W) + 2
    _check('autograd forward', y.detach().cpu().numpy().reshape(N, Cout, -1), y_ref.numpy(),
           ((Cin + 2) * U * y_abs).numpy(), False)
    _check('autograd dx', xd.grad.cpu().numpy().reshape(N, Cin, -1), dx_ref.numpy(), ((Cout + 1) * U * dx_abs).numpy(), False)
    _check('autograd dw', conv.weight.grad.cpu().numpy().reshape(Cout, Cin), dw_ref.numpy(), (K * U * dw_abs).numpy(), False)
    _check('autograd db', conv.bias.grad.cpu().numpy(), db_ref.numpy(), (K * U * db_abs).numpy(), False)
    with torch.no_grad():
        conv.weight.mul_(2.0)
        conv.bias.zero_()
        y2 = pointwise_conv_nchw(xd, conv.weight, conv.bias)
    _check('after an in-place update', y2.cpu().numpy().reshape(N, Cout, -1), (2.0 * (y_ref - b[None, :, None])).numpy(),
           ((Cin + 2) * U * 2.0 * (y_abs - b.abs()[None, :, None])).numpy(), False)
    with pytest.raises(ValueError, match='HIP-device'):
        pointwise_conv_nchw(xd.detach().cpu(), conv.weight, conv.bias)
    with pytest.raises(ValueError, match='no kernel'):
        pointwise_conv_nchw(xd, torch.zeros(65, Cin, 1, 1, device='cuda'))
