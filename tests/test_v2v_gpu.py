"""The 3-D kernels of csrc/conv3d.hip and models.v2v.V2VModel on the device.

Single kernels against torch.nn.functional.conv3d / conv_transpose3d / max_pool3d in float64 on the CPU, every conv
and deconv shape twice:
 (a) integer lattice: x, w, res in [-2, 2], scale 1, integer shift. Every partial sum is an integer below 2^24 (the
     largest K here is 7^3 * 32 = 10 976, so |sum| <= 4 K + small), f32 is exact in any order, and the result must EQUAL
     the reference. One dropped tap of 10 976 is 9e-5 of sum |x||w|, under any rounding bound (K 2^-24 = 6.5e-4).
 (b) real-valued, with the per-element bound (K + 3) u |scale| (|x| conv |w|) + 3 u (|shift| + |res| + |y_ref|),
     K = ks^3 Cin_pad, u = 2^-24: the gamma_K bound of an fmaf chain in any order, plus the epilogue's roundings.
The whole network against the reference's float64 output (tests/golden/v2v.npz) and the float64 restatement
(tests/v2v_ref.py), held to 4 x the error of the same graph run in float32 on the CPU. Each test runs in a spawned
child (tests/spawned.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import v2v_ref as R
import volumetric_ref as VR
from spawned import spawned

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'v2v.npz')
U = 2.0 ** -24

# (ks, N, D, H, W, Cin, Cout, scale?, res?, relu?)
CONV_CASES = (
    (3, 1, 1, 1, 1, 128, 128, True, False, True),
    (3, 2, 2, 2, 2, 128, 128, True, False, True),
    (3, 1, 4, 4, 4, 32, 64, True, True, True),
    (3, 1, 5, 3, 9, 16, 32, True, False, False),
    (3, 1, 8, 8, 8, 32, 32, True, True, True),
    (7, 1, 8, 8, 8, 2, 16, True, False, True),             # Cin padded to 4
    (7, 1, 3, 4, 9, 32, 16, True, False, True),            # extents below the half-width
    (1, 1, 4, 4, 4, 32, 21, False, False, False),          # bias only; Cout padded to 32
    (1, 1, 4, 4, 4, 16, 32, True, False, False),
    (1, 2, 4, 4, 4, 32, 32, True, False, True),
)
# (N, D, H, W, Cin, Cout, add?)
DECONV_CASES = ((1, 1, 1, 1, 128, 128, False), (1, 2, 3, 4, 128, 64, False), (1, 4, 4, 4, 64, 32, True))


def _pad(c, to):
    return (c + to - 1) // to * to


def _ndhwc(a, cp):
    """CPU NCDHW float64 -> device NDHWC f32, channels zero-padded to cp"""
    n, c = a.shape[:2]
    t = torch.zeros((n,) + tuple(a.shape[2:]) + (cp,), dtype=torch.float32)
    t[..., :c] = a.permute(0, 2, 3, 4, 1).float()
    return t.cuda().contiguous()


def _ncdhw(t, c):
    return t.cpu()[..., :c].permute(0, 4, 1, 2, 3).contiguous().numpy()


def _vec(v, cp):
    t = torch.zeros(cp, dtype=torch.float32)
    t[:v.numel()] = v.float()
    return t.cuda()


def _pack(w, cout, cin, ks, transposed):
    from hipnet import _capi as C
    cout_p, cin_p = _pad(cout, 16), _pad(cin, 4)
    wd = w.float().cuda().contiguous()
    out = torch.full((ks ** 3 * cout_p * cin_p,), float('nan'), dtype=torch.float32, device='cuda')
    C.call('hrnet_pack_weights3d', C.HR_F32, wd.data_ptr(), out.data_ptr(), cout, cin, ks, cout_p, cin_p,
           int(transposed), C.stream_ptr())
    return out, cout_p, cin_p


def _draw(rng, shape, lattice):
    a = rng.integers(-2, 3, shape).astype(np.float64) if lattice else rng.normal(0.0, 1.0, shape)
    return torch.from_numpy(a.astype(np.float32).astype(np.float64))       # f32-representable, kept in float64


def _check(what, got, ref, bound, lattice, pads):
    """lattice: equal bits; else |got - ref| <= bound elementwise. pads: the pad channels of the device result."""
    assert (pads == 0).all(), (what, 'pad channels are not zero')
    if lattice:
        bad = int((got.astype(np.float64) != ref).sum())
        print(what, 'lattice: {} of {} differ'.format(bad, ref.size))
        assert bad == 0, (what, bad)
    else:
        ratio = (np.abs(got.astype(np.float64) - ref) / bound).max()
        print(what, 'real: largest |error| / bound = {:.3f}'.format(ratio))
        assert ratio <= 1.0, (what, ratio)


def _conv_case(case, lattice, rng):
    from hipnet import _capi as C
    ks, N, D, H, W, cin, cout, with_scale, with_res, relu = case
    x = _draw(rng, (N, cin, D, H, W), lattice)
    w = _draw(rng, (cout, cin, ks, ks, ks), lattice)
    if not lattice:
        w = (w / np.sqrt(cin * ks ** 3)).float().double()
    res = _draw(rng, (N, cout, D, H, W), lattice) if with_res else None
    if lattice:
        scale = torch.ones(cout, dtype=torch.float64) if with_scale else None
        shift = torch.from_numpy(rng.integers(-3, 4, cout).astype(np.float64))
    else:
        scale = torch.from_numpy(rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout)).float().double() \
            if with_scale else None
        shift = torch.from_numpy(rng.normal(0.0, 0.5, cout)).float().double()
    sc = torch.ones(cout, dtype=torch.float64) if scale is None else scale
    bc = (1, cout, 1, 1, 1)
    ref = F.conv3d(x, w, None, 1, ks // 2) * sc.view(bc) + shift.view(bc)
    if res is not None:
        ref = ref + res
    if relu:
        ref = F.relu(ref)
    wp, cout_p, cin_p = _pack(w, cout, cin, ks, False)
    K = ks ** 3 * cin_p
    bound = ((K + 3) * U * sc.abs().view(bc) * F.conv3d(x.abs(), w.abs(), None, 1, ks // 2)
             + 3 * U * (shift.abs().view(bc) + (0 if res is None else res.abs()) + ref.abs())).numpy()
    assert C.call('hrnet_conv3d_supported', C.HR_F32, cin_p, cout_p, ks) == 1
    xd = _ndhwc(x, cin_p)
    rd = None if res is None else _ndhwc(res, cout_p)
    sd, hd = (None if scale is None else _vec(scale, cout_p)), _vec(shift, cout_p)
    y = torch.full((N, D, H, W, cout_p), float('nan'), dtype=torch.float32, device='cuda')
    C.call('hrnet_conv3d', C.HR_F32, xd.data_ptr(), wp.data_ptr(), C.ptr(sd), hd.data_ptr(), C.ptr(rd), y.data_ptr(),
           N, D, H, W, cin_p, cout_p, ks, int(relu), C.stream_ptr())
    torch.cuda.synchronize()
    pads = y.cpu()[..., cout:].numpy()                     # zero rows of the packed weight, zero shift: exact zeros
    _check('conv3d ks{} {}'.format(ks, case[1:7]), _ncdhw(y, cout), ref.numpy(), bound, lattice, pads)


@spawned
def test_conv3d_every_shape_on_the_lattice_and_in_reals():
    """achieved on one MI355X: every lattice run equals the reference; largest |error| / bound of the real-valued runs
    0.009 for ks 3, 0.003 for ks 7, 0.21 for ks 1 (K = 16: the epilogue's roundings dominate)."""
    rng = np.random.default_rng(41)
    for case in CONV_CASES:
        for lattice in (True, False):
            _conv_case(case, lattice, rng)
    # refusals of the entry: bf16, an unsupported kernel size, unpadded channels
    from hipnet import _capi as C
    t = torch.zeros(64, device='cuda')
    for dtype, cin, cout, ks, msg in ((C.HR_BF16, 32, 32, 3, 'only f32'), (C.HR_F32, 32, 32, 5, 'ks = 5'),
                                      (C.HR_F32, 30, 32, 3, 'Cin = 30'), (C.HR_F32, 32, 24, 3, 'Cout = 24')):
        with pytest.raises(RuntimeError, match=msg):
            C.call('hrnet_conv3d', dtype, t.data_ptr(), t.data_ptr(), None, t.data_ptr(), None, t.data_ptr(), 1, 1, 1,
                   1, cin, cout, ks, 0, C.stream_ptr())


def _deconv_case(case, lattice, rng):
    from hipnet import _capi as C
    N, D, H, W, cin, cout, with_add = case
    x = _draw(rng, (N, cin, D, H, W), lattice)
    w = _draw(rng, (cin, cout, 2, 2, 2), lattice)
    if not lattice:
        w = (w / np.sqrt(cin)).float().double()
    add = _draw(rng, (N, cout, 2 * D, 2 * H, 2 * W), lattice) if with_add else None
    if lattice:
        scale = torch.ones(cout, dtype=torch.float64)
        shift = torch.from_numpy(rng.integers(-3, 4, cout).astype(np.float64))
    else:
        scale = torch.from_numpy(rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout)).float().double()
        shift = torch.from_numpy(rng.normal(0.0, 0.5, cout)).float().double()
    bc = (1, cout, 1, 1, 1)
    ref = F.relu(F.conv_transpose3d(x, w, None, 2, 0) * scale.view(bc) + shift.view(bc))
    if add is not None:
        ref = ref + add                                    # after the ReLU: x = upsample(x) + skip_x
    wp, cout_p, cin_p = _pack(w, cout, cin, 2, True)
    bound = ((cin_p + 3) * U * scale.abs().view(bc) * F.conv_transpose3d(x.abs(), w.abs(), None, 2, 0)
             + 3 * U * (shift.abs().view(bc) + (0 if add is None else add.abs()) + ref.abs())).numpy()
    xd = _ndhwc(x, cin_p)
    ad = None if add is None else _ndhwc(add, cout_p)
    sd, hd = _vec(scale, cout_p), _vec(shift, cout_p)
    y = torch.full((N, 2 * D, 2 * H, 2 * W, cout_p), float('nan'), dtype=torch.float32, device='cuda')
    C.call('hrnet_deconv3d_k2s2', C.HR_F32, xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), C.ptr(ad),
           y.data_ptr(), N, D, H, W, cin_p, cout_p, 1, C.stream_ptr())
    torch.cuda.synchronize()
    _check('deconv3d {}'.format(case[:6]), _ncdhw(y, cout), ref.numpy(), bound, lattice, y.cpu()[..., cout:].numpy())


@spawned
def test_deconv3d_every_shape_on_the_lattice_and_in_reals():
    """achieved on one MI355X: every lattice run equals the reference; real-valued, largest |error| / bound 0.057."""
    rng = np.random.default_rng(43)
    for case in DECONV_CASES:
        for lattice in (True, False):
            _deconv_case(case, lattice, rng)


@spawned
def test_packed_weights_layout():
    """[tap][Cout_pad][Cin_pad] with zero pads, from OIDHW and from IODHW"""
    rng = np.random.default_rng(47)
    for cout, cin, ks, transposed in ((21, 2, 3, False), (16, 32, 7, False), (32, 64, 2, True), (5, 3, 1, False)):
        shape = (cin, cout, ks, ks, ks) if transposed else (cout, cin, ks, ks, ks)
        w = torch.from_numpy(rng.normal(0, 1, shape).astype(np.float32))
        wp, cout_p, cin_p = _pack(w, cout, cin, ks, transposed)
        got = wp.cpu().view(ks ** 3, cout_p, cin_p)
        want = torch.zeros(ks ** 3, cout_p, cin_p)
        oi = w.permute(1, 0, 2, 3, 4) if transposed else w
        want[:, :cout, :cin] = oi.reshape(cout, cin, ks ** 3).permute(2, 0, 1)
        assert torch.equal(got, want), (cout, cin, ks, transposed)


@spawned
def test_maxpool3d_all_negative_and_odd_extents():
    from hipnet import _capi as C
    rng = np.random.default_rng(53)
    for N, D, H, W, Cn in ((1, 2, 2, 2, 32), (2, 4, 6, 8, 64), (1, 64, 2, 2, 128)):
        x = torch.from_numpy(-rng.uniform(0.5, 2.0, (N, Cn, D, H, W)).astype(np.float32))
        ref = F.max_pool3d(x.double(), 2, 2).numpy()
        assert (ref < 0).all()                             # a maximum that starts from zero would show
        xd = _ndhwc(x.double(), Cn)
        y = torch.full((N, D // 2, H // 2, W // 2, Cn), float('nan'), dtype=torch.float32, device='cuda')
        C.call('hrnet_maxpool3d', C.HR_F32, xd.data_ptr(), y.data_ptr(), N, D, H, W, Cn, C.stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_ncdhw(y, Cn).astype(np.float64), ref), (N, D, H, W, Cn)
    t = torch.zeros(4096, device='cuda')
    for D, H, W in ((3, 2, 2), (2, 5, 2), (2, 2, 7), (1, 2, 2)):
        with pytest.raises(RuntimeError, match='maxpool3d'):
            C.call('hrnet_maxpool3d', C.HR_F32, t.data_ptr(), t.data_ptr() + 8192, 1, D, H, W, 32, C.stream_ptr())


def _fixture():
    z = np.load(GOLD)
    keys = [str(k) for k in z['keys']]
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(z['shapes'], z['ndims'])]
    return z, keys, shapes


def _model(cin, cout, seed):
    """(eval-mode model on the device with the recipe's parameters, the float64 state dict)"""
    from models.v2v import V2VModel
    model = V2VModel(cin, cout)
    sd0 = model.state_dict()
    fill = R.fill_state_dict([(k, tuple(v.shape)) for k, v in sd0.items()], seed)
    model.load_state_dict({k: torch.from_numpy(np.asarray(fill[k])).to(sd0[k].dtype) for k in sd0}, strict=True)
    return model.cuda().eval(), fill


@spawned
def test_whole_network_against_the_reference_fixture():
    """max|y_dev - y64| / max|y64| against 4 x e_ref, e_ref = max|y32 - y64| / max|y64| of the reference's own float32
    CPU run (the fixture: e_ref = 2.54e-6, bound 1.02e-5). Achieved on one MI355X: 2.90e-6."""
    z, keys, shapes = _fixture()
    model, _ = _model(2, 2, int(z['seed']))
    assert set(model.state_dict()) == set(keys)
    top = np.abs(z['y64']).max()
    e_ref = np.abs(z['y32'].astype(np.float64) - z['y64']).max() / top
    x = torch.from_numpy(z['x']).cuda()
    with torch.no_grad():
        y = model(x)
        torch.cuda.synchronize()
        y1 = y.cpu().numpy()
        err = np.abs(y1.astype(np.float64) - z['y64']).max() / top
        print('fixture (1, 2 -> 2, 32^3): device {:.3e}, e_ref {:.3e}, bound {:.3e}'.format(err, e_ref, 4 * e_ref))
        assert y.dtype == torch.float32 and y1.shape == (1, 2, 32, 32, 32)
        assert err <= 4 * e_ref, (err, e_ref)
        # a second forward: the same bits, and nothing new but the result (cached plan, cached buffers)
        plan = model._plans[(1, 2, 32, 32, 32)]
        ptrs = [b.data_ptr() for b in plan.buffers]
        y2 = model(x)
        assert model._plans[(1, 2, 32, 32, 32)] is plan and [b.data_ptr() for b in plan.buffers] == ptrs
        assert np.array_equal(y2.cpu().numpy(), y1)
        # other dtypes and strides are converted
        y3 = model(x.double().permute(0, 1, 4, 3, 2).contiguous().permute(0, 1, 4, 3, 2))
        assert np.array_equal(y3.cpu().numpy(), y1)
        # captured after the warm-up above, replayed twice: the eager bits
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yg = model(x)
        for _ in range(2):
            yg.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(yg.cpu().numpy(), y1)
        # new parameters are noticed: the packed copies are rebuilt
        packed = model._packed
        model.output_layer.bias.add_(1.0)
        y4 = model(x)
        assert model._packed is not packed
        assert np.abs(y4.cpu().numpy().astype(np.float64) - 1.0 - z['y64']).max() / top <= 4 * e_ref + 2 * U
    # refusals on the device: gradients
    with pytest.raises(NotImplementedError, match='backward are not built'):
        model(x)
    model.train()
    with pytest.raises(NotImplementedError, match='training-mode'):
        with torch.no_grad():
            model(x)


@spawned
def test_whole_network_at_the_workload_widths():
    """(1, 32 -> 21, 32^3) against the float64 restatement; e_ref is the restatement run in float32 on the CPU, the
    device is held to 4 x e_ref. Achieved on one MI355X: 2.84e-6 (e_ref 1.70e-6, bound 6.81e-6; max|y| 15.7)."""
    model, fill = _model(32, 21, 77)
    x = np.random.default_rng(78).normal(0.0, 1.0, (1, 32, 32, 32, 32)).astype(np.float32)
    y64 = R.forward(fill, x)
    y32 = R.forward(fill, x, torch.float32)
    top = np.abs(y64).max()
    e_ref = np.abs(y32.astype(np.float64) - y64).max() / top
    with torch.no_grad():
        y = model(torch.from_numpy(x).cuda()).cpu().numpy()
    err = np.abs(y.astype(np.float64) - y64).max() / top
    print('restatement (1, 32 -> 21, 32^3): max|y| {:.3f}, device {:.3e}, e_ref {:.3e}, bound {:.3e}'.format(
        top, err, e_ref, 4 * e_ref))
    assert y.shape == (1, 21, 32, 32, 32) and 0.1 <= top <= 100.0
    assert err <= 4 * e_ref, (err, e_ref)


@spawned
def test_the_chain_unproject_v2v_integrate():
    """unproject_heatmaps -> V2VModel -> integrate_tensor_3d_with_coordinates at (B, V, C, H, W) = (1, 2, 4, 16, 16),
    32^3 voxels, J = 3, against the float64 restatements. The key points (error: max-abs over max|coord|) are held to
    4 x the error of the same chain in float32 on the CPU: the float64 unprojection rounded to float32, the V2V
    restatement in float32, a float32 softmax and expectation. Achieved on one MI355X: 5.91e-6 (float32 on the CPU
    4.37e-6, bound 1.75e-5)."""
    from utils.volumetric import build_coord_volumes, integrate_tensor_3d_with_coordinates, unproject_heatmaps
    rng = np.random.default_rng(91)
    B, V, Cn, H, W, S, J, mult = 1, 2, 4, 16, 16, 32, 3, 4.0
    coord = build_coord_volumes(torch.tensor([[10.0, -5.0, 20.0]]), 300.0, S).numpy()
    proj = VR.ring_cameras(V, 1200.0, 50.0, (8.0, 8.0), target=(10.0, -5.0, 20.0))[None].astype(np.float32)
    feat = rng.normal(0.0, 1.0, (B, V, Cn, H, W)).astype(np.float32)
    model, fill = _model(Cn, J, 93)
    # float64
    vol64 = VR.unproject(feat, proj, coord, 'sum')
    y64 = R.forward(fill, vol64)
    kp64, _ = VR.integrate(y64, coord, True, mult)
    # float32 on the CPU
    y32 = torch.from_numpy(R.forward(fill, vol64.astype(np.float32), torch.float32))
    p32 = torch.softmax((torch.tensor(mult, dtype=torch.float32) * y32).reshape(B, J, -1), dim=2)
    kp32 = torch.einsum('bjn,bnc->bjc', p32, torch.from_numpy(coord).reshape(B, -1, 3)).numpy()
    assert kp32.dtype == np.float32
    scale = np.abs(coord).max()
    e_ref = np.abs(kp32.astype(np.float64) - kp64).max() / scale
    with torch.no_grad():
        cv = torch.from_numpy(coord).cuda()
        vol = unproject_heatmaps(torch.from_numpy(feat).cuda(), torch.from_numpy(proj).cuda(), cv, 'sum')
        kp, _ = integrate_tensor_3d_with_coordinates(model(vol), cv, softmax=True, multiplier=mult)
        torch.cuda.synchronize()
    err = np.abs(kp.cpu().numpy().astype(np.float64) - kp64).max() / scale
    print('chain: key points device {:.3e}, float32 on the CPU {:.3e}, bound {:.3e}'.format(err, e_ref, 4 * e_ref))
    assert (np.abs(vol64) > 0).mean() > 0.5                # the cameras see the box
    assert err <= 4 * e_ref, (err, e_ref)
