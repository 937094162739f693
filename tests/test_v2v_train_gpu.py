"""The training kernels of csrc/conv3d_train.hip and V2VModel(trainable=True) on the device.

Single kernels against torch.nn.functional / autograd in float64 on the CPU, every convolution-like shape twice, by the
convention of tests/test_v2v_gpu.py:
 (a) integer lattice: every operand in [-2, 2], so every partial sum is an integer below 2^24 (the longest sum here,
     the 5120 voxels of the several-splits case, stays under 4 * 5120), f32 is exact in any order and any split, and the
     result must EQUAL the reference;
 (b) real-valued, with the per-element bound (K + S + 2) u (|a| * |b|)  - the gamma_K bound of an fmaf chain of K
     products in any order, S more additions for the partial sums of S splits, u = 2^-24 - where K is the number of
     voxels summed for a weight gradient (N D H W, whatever the tap) and taps * Cout_pad for an input gradient;
     (|a| * |b|) is the same contraction of the absolute values. With `accumulate` one more rounding on |init| + |ref|.
Blocks and the whole network go through autograd against tests/v2v_train_ref.py in float64, held to 4 x the error of
the same case in float32 on the CPU. Each test runs in a spawned child (tests/spawned.py)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import v2v_ref as R
import v2v_train_ref as TR
import volumetric_ref as VR
from spawned import spawned

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _pad(c, to):
    return (c + to - 1) // to * to


def _ndhwc(a, cp):
    """CPU NCDHW float64 -> device NDHWC f32, channels zero-padded to cp"""
    n, c = a.shape[:2]
    t = torch.zeros((n,) + tuple(a.shape[2:]) + (cp,), dtype=torch.float32)
    t[..., :c] = a.permute(0, 2, 3, 4, 1).float()
    return t.cuda().contiguous()


def _ncdhw(t, c):
    return t.cpu()[..., :c].permute(0, 4, 1, 2, 3).contiguous().double().numpy()


def _draw(rng, shape, lattice):
    a = rng.integers(-2, 3, shape).astype(np.float64) if lattice else rng.normal(0.0, 1.0, shape)
    return torch.from_numpy(a.astype(np.float32).astype(np.float64))


def _check(what, got, ref, bound, lattice):
    got = np.asarray(got, dtype=np.float64)
    if lattice:
        bad = int((got != ref).sum())
        print(what, 'lattice: {} of {} differ'.format(bad, ref.size))
        assert bad == 0, (what, bad)
    else:
        ratio = (np.abs(got - ref) / np.maximum(bound, 1e-300)).max()
        print(what, 'real: largest |error| / bound = {:.3f}'.format(ratio))
        assert ratio <= 1.0, (what, ratio)


def _query(N, D, H, W, cin_p, cout_p, ks, deconv):
    from hipnet import _capi as C
    nbytes, nsplit, per = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)
    C.call('hrnet_conv3d_wgrad_scratch', C.HR_F32, N, D, H, W, cin_p, cout_p, ks, deconv, ctypes.byref(nbytes),
           ctypes.byref(nsplit), ctypes.byref(per))
    return nbytes.value, nsplit.value, per.value


def _wgrad_case(case, lattice, rng, accumulate=False, deconv=False):
    """dW of Conv3d (OIDHW) or of ConvTranspose3d(2, 2) (IODHW); N, D, H, W are x's"""
    from hipnet import _capi as C
    ks, N, D, H, W, cin, cout = case
    cin_p, cout_p = _pad(cin, 4), _pad(cout, 16)
    up = 2 if deconv else 1
    x = _draw(rng, (N, cin, D, H, W), lattice)
    dz = _draw(rng, (N, cout, up * D, up * H, up * W), lattice)
    wshape = (cin, cout, 2, 2, 2) if deconv else (cout, cin, ks, ks, ks)

    def grad(a, b):
        w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose3d(a, w, None, 2, 0) if deconv else F.conv3d(a, w, None, 1, ks // 2)
        y.backward(b)
        return w.grad
    ref = grad(x, dz)
    init = _draw(rng, wshape, lattice) if accumulate else torch.zeros(wshape, dtype=torch.float64)
    ref = ref + init
    nbytes, nsplit, per = _query(N, D, H, W, cin_p, cout_p, ks, int(deconv))
    K = N * D * H * W
    bound = ((K + nsplit + 2) * U * grad(x.abs(), dz.abs()) + U * (init.abs() + ref.abs())).numpy()
    xd, dzd = _ndhwc(x, cin_p), _ndhwc(dz, cout_p)
    scratch = torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device='cuda')
    dw = init.float().cuda().contiguous() if accumulate else torch.full(wshape, float('nan'), dtype=torch.float32,
                                                                       device='cuda')
    C.call('hrnet_conv3d_wgrad', C.HR_F32, xd.data_ptr(), dzd.data_ptr(), scratch.data_ptr(), nbytes, dw.data_ptr(), N,
           D, H, W, cin_p, cout_p, cin, cout, ks, int(deconv), int(accumulate), C.stream_ptr())
    torch.cuda.synchronize()
    _check('{} ks{} {} splits {}{}'.format('deconv wgrad' if deconv else 'wgrad', ks, case[1:], nsplit,
                                           ' accumulate' if accumulate else ''), dw.cpu().numpy(), ref.numpy(), bound,
           lattice)
    return nsplit, per


# (ks, N, D, H, W, Cin, Cout)
WGRAD_CASES = (
    (3, 1, 3, 5, 7, 32, 32),           # 105 voxels: no multiple of the wave's 64, nor of the step of 16
    (7, 1, 3, 4, 9, 32, 16),           # extents below the half-width
    (3, 2, 2, 2, 2, 128, 128),         # N = 2
    (3, 1, 1, 1, 1, 128, 128),
    (7, 2, 3, 4, 5, 4, 16),            # the 4-channel step
    (7, 1, 2, 3, 4, 2, 16),            # Cin padded to 4
    (3, 1, 2, 3, 5, 16, 32),
    (1, 1, 2, 3, 5, 16, 32),
    (3, 1, 2, 3, 5, 32, 48),           # a channel-block tail: 48 = 3 blocks of 16
    (1, 1, 4, 4, 4, 32, 21),           # Cout padded to 32
    (3, 1, 2, 2, 3, 64, 128),
)
SPLIT_CASE = (3, 1, 16, 16, 20, 16, 32)    # 5120 voxels


@spawned
def test_weight_gradient_every_shape_on_the_lattice_and_in_reals():
    """achieved on one MI355X: every lattice run equals float64; real-valued, largest |error| / bound 0.20
    (128 -> 128 at 1^3: K = 1, the single product's rounding against a bound of 3 u)."""
    rng = np.random.default_rng(141)
    for case in WGRAD_CASES:
        for lattice in (True, False):
            _wgrad_case(case, lattice, rng)
    for lattice in (True, False):
        nsplit, per = _wgrad_case(SPLIT_CASE, lattice, rng)
        # several splits with a ragged last one: by the query's own answer the last split is shorter than the others
        last = 16 * 16 * 20 - (nsplit - 1) * per
        print('splits of the 5120 voxels: {} of {}, the last one {}'.format(nsplit, per, last))
        assert nsplit >= 3 and 0 < last < per, (nsplit, per, last)
    for lattice in (True, False):
        _wgrad_case(WGRAD_CASES[0], lattice, rng, accumulate=True)
        _wgrad_case(SPLIT_CASE, lattice, rng, accumulate=True)


def _dgrad_case(case, lattice, rng):
    """the input gradient of Conv3d: hrnet_conv3d on dz with the weights of hrnet_pack_weights3d_dgrad, + res"""
    from hipnet import _capi as C
    ks, N, D, H, W, cin, cout = case
    cin_p, cout_p = _pad(cin, 4), _pad(cout, 16)
    gin_p = _pad(cin_p, 16)
    dz = _draw(rng, (N, cout, D, H, W), lattice)
    w = _draw(rng, (cout, cin, ks, ks, ks), lattice)
    prev = _draw(rng, (N, cin, D, H, W), lattice)                        # the gradient summed so far
    if not lattice:
        w = (w / np.sqrt(cout * ks ** 3)).float().double()
    ref = F.conv_transpose3d(dz, w, None, 1, ks // 2) + prev
    K = ks ** 3 * cout_p
    bound = ((K + 3) * U * F.conv_transpose3d(dz.abs(), w.abs(), None, 1, ks // 2) + 3 * U * (prev.abs() + ref.abs())).numpy()
    wd = torch.full((ks ** 3 * gin_p * cout_p,), float('nan'), dtype=torch.float32, device='cuda')
    wdev = w.float().cuda().contiguous()
    C.call('hrnet_pack_weights3d_dgrad', C.HR_F32, wdev.data_ptr(), wd.data_ptr(), cout, cin, ks, cout_p, gin_p,
           C.stream_ptr())
    zeros = torch.zeros(gin_p, dtype=torch.float32, device='cuda')
    dzd, pd = _ndhwc(dz, cout_p), _ndhwc(prev, gin_p)
    dx = torch.full((N, D, H, W, gin_p), float('nan'), dtype=torch.float32, device='cuda')
    C.call('hrnet_conv3d', C.HR_F32, dzd.data_ptr(), wd.data_ptr(), None, zeros.data_ptr(), pd.data_ptr(), dx.data_ptr(),
           N, D, H, W, cout_p, gin_p, ks, 0, C.stream_ptr())
    torch.cuda.synchronize()
    assert (dx.cpu()[..., cin:] == 0).all(), ('pad channels of the input gradient', case)
    _check('dgrad ks{} {}'.format(ks, case[1:]), _ncdhw(dx, cin), ref.numpy(), bound, lattice)


@spawned
def test_input_gradient_every_shape_on_the_lattice_and_in_reals():
    """achieved on one MI355X: every lattice run equals float64; real-valued, largest |error| / bound 0.10 (ks 1:
    K = 32, the epilogue's roundings dominate)."""
    rng = np.random.default_rng(143)
    for case in WGRAD_CASES + (SPLIT_CASE,):
        for lattice in (True, False):
            _dgrad_case(case, lattice, rng)


def _deconv_dgrad_case(case, lattice, rng, accumulate):
    from hipnet import _capi as C
    N, D, H, W, cin, cout = case
    cin_p, cout_p = _pad(cin, 16), _pad(cout, 16)
    dz = _draw(rng, (N, cout, 2 * D, 2 * H, 2 * W), lattice)
    w = _draw(rng, (cin, cout, 2, 2, 2), lattice)
    if not lattice:
        w = (w / np.sqrt(8 * cout)).float().double()
    init = _draw(rng, (N, cin, D, H, W), lattice) if accumulate else torch.zeros((N, cin, D, H, W), dtype=torch.float64)
    ref = F.conv3d(dz, w, None, 2, 0) + init             # d conv_transpose / d input: the strided convolution
    K = 8 * cout_p
    bound = ((K + 3) * U * F.conv3d(dz.abs(), w.abs(), None, 2, 0) + 2 * U * (init.abs() + ref.abs())).numpy()
    wd = torch.full((8 * cin_p * cout_p,), float('nan'), dtype=torch.float32, device='cuda')
    wdev = w.float().cuda().contiguous()
    C.call('hrnet_pack_weights3d', C.HR_F32, wdev.data_ptr(), wd.data_ptr(), cin, cout, 2, cin_p, cout_p, 0,
           C.stream_ptr())
    dzd = _ndhwc(dz, cout_p)
    dx = _ndhwc(init, cin_p) if accumulate else torch.full((N, D, H, W, cin_p), float('nan'), dtype=torch.float32,
                                                           device='cuda')
    C.call('hrnet_deconv3d_k2s2_dgrad', C.HR_F32, dzd.data_ptr(), wd.data_ptr(), dx.data_ptr(), N, D, H, W, cin_p, cout_p,
           int(accumulate), C.stream_ptr())
    torch.cuda.synchronize()
    assert (dx.cpu()[..., cin:] == 0).all()
    _check('deconv dgrad {}{}'.format(case, ' accumulate' if accumulate else ''), _ncdhw(dx, cin), ref.numpy(), bound,
           lattice)


# (N, D, H, W, Cin, Cout): the INPUT volume of the deconvolution
DECONV_CASES = ((2, 3, 4, 5, 32, 16), (1, 1, 1, 1, 128, 128), (1, 2, 3, 3, 64, 32))


@spawned
def test_deconvolution_both_gradients_on_the_lattice_and_in_reals():
    """achieved on one MI355X: every lattice run equals float64; real-valued, largest |error| / bound 0.02 for the input
    gradient, 0.48 for the weight gradient (128 -> 128 at 1^3 with accumulate: one product, two roundings)."""
    rng = np.random.default_rng(147)
    for case in DECONV_CASES:
        for lattice in (True, False):
            for accumulate in (False, True):
                _deconv_dgrad_case(case, lattice, rng, accumulate)
                _wgrad_case((2,) + case, lattice, rng, accumulate=accumulate, deconv=True)


@spawned
def test_maxpool_backward_sends_the_gradient_to_the_first_maximum():
    """distinct values, an all-equal window (element 0), the maximum repeated in elements 1, 2, 4 and 7 (element 1), an
    all-negative window, and a lattice volume full of ties: the bits of float64 torch on the CPU"""
    from hipnet import _capi as C
    rng = np.random.default_rng(149)
    Cn = 4
    win = np.zeros((4, 8))
    win[0] = rng.permutation(8) - 3.0                                     # distinct
    win[1] = 1.5                                                          # all equal
    win[2] = [0.0, 2.0, 2.0, -1.0, 2.0, 1.0, 0.5, 2.0]                    # the maximum in elements 1, 2, 4, 7
    win[3] = -(rng.permutation(8) + 1.0)                                  # all negative
    x = np.zeros((1, Cn, 2, 2, 8))
    for k in range(4):
        x[0, :, :, :, 2 * k:2 * k + 2] = win[k].reshape(2, 2, 2)
    g = rng.integers(1, 4, (1, Cn, 1, 1, 4)).astype(np.float64)
    xt = torch.from_numpy(x).requires_grad_(True)
    F.max_pool3d(xt, 2, 2).backward(torch.from_numpy(g))
    ref = xt.grad.numpy()
    assert ref[0, 0, 0, 0, 2] != 0 and ref[0, 0, 0, 0, 5] != 0            # elements 0 and 1: the CPU's rule
    assert np.count_nonzero(ref) == 4 * Cn

    def run(xa, ga, init=None):
        N, Cc, D, H, W = xa.shape
        xd, gd = _ndhwc(torch.from_numpy(xa), Cc), _ndhwc(torch.from_numpy(ga), Cc)
        dx = torch.full((N, D, H, W, Cc), float('nan'), dtype=torch.float32, device='cuda') if init is None \
            else _ndhwc(torch.from_numpy(init), Cc)
        C.call('hrnet_maxpool3d_bwd', C.HR_F32, xd.data_ptr(), gd.data_ptr(), dx.data_ptr(), N, D, H, W, Cc,
               int(init is not None), C.stream_ptr())
        torch.cuda.synchronize()
        return _ncdhw(dx, Cc)
    assert np.array_equal(run(x, g), ref)
    for shape in ((2, 32, 4, 6, 8), (1, 128, 2, 2, 2)):
        xa = rng.integers(-2, 3, shape).astype(np.float64)                # ties in almost every window
        ga = rng.integers(-2, 3, (shape[0], shape[1], shape[2] // 2, shape[3] // 2, shape[4] // 2)).astype(np.float64)
        xt = torch.from_numpy(xa).requires_grad_(True)
        F.max_pool3d(xt, 2, 2).backward(torch.from_numpy(ga))
        assert np.array_equal(run(xa, ga), xt.grad.numpy()), shape
        init = rng.integers(-2, 3, shape).astype(np.float64)
        assert np.array_equal(run(xa, ga, init), xt.grad.numpy() + init), shape


def _bn_chain(rows, Cc):
    """the longest f32 chain of the BatchNorm sums: a thread's rows, then the row lanes of its workgroup (the
    workgroups are added in float64)"""
    from hipnet import _capi as C
    parts = C.call('hrnet_bn3d_parts', rows)
    per = -(-rows // parts)
    lanes = 256 // (Cc // 4)
    return -(-per // lanes) + lanes, parts


@spawned
def test_batchnorm_statistics_against_float64():
    """mean and biased variance of z [rows][C] against float64, with L = the longest f32 chain (_bn_chain):
      |mean - mean64| <= dm := (L + 2) u mean|z| + u |mean64|           (gamma_L on the sum, one rounding of the quotient)
      |var - var64|   <= (L + 8) u (var64 + dm^2) + dm^2                 (a sum of squares of z - mean, each with three
                         roundings, around a mean that is off by at most dm: sum (z - m')^2 = sum (z - m)^2 + rows dm^2)
    plus 4 u (var + eps) for the rounding of invstd, from which the test recovers the variance. A channel with mean 100
    and deviation 1e-2 is in every case: E[z^2] - E[z]^2 in f32 would miss its variance of 1e-4 by about 1e4 u = 6e-4.
    Achieved on one MI355X: largest error / bound 0.08 (mean), 0.12 (variance)."""
    from hipnet import _capi as C
    rng = np.random.default_rng(151)
    eps, mom = 1e-5, 0.1
    worst = [0.0, 0.0]
    for N, D, H, W, Cc, creal in ((2, 1, 1, 1, 16, 16), (1, 3, 5, 7, 16, 16), (2, 8, 8, 9, 32, 21), (1, 1, 1, 2, 128, 128),
                                  (3, 7, 11, 13, 48, 48)):
        rows = N * D * H * W
        z = rng.normal(0.0, 1.0, (rows, Cc)) * rng.uniform(0.2, 3.0, Cc) + rng.normal(0.0, 2.0, Cc)
        z[:, 1] = 100.0 + 1e-2 * rng.normal(0.0, 1.0, rows)
        z[:, creal:] = 0.0
        z = z.astype(np.float32)
        z64 = z.astype(np.float64)
        gamma = np.zeros(Cc, np.float32); gamma[:creal] = rng.uniform(0.5, 1.5, creal)
        beta = np.zeros(Cc, np.float32); beta[:creal] = rng.uniform(-0.3, 0.3, creal)
        rm0, rv0 = rng.normal(0, 0.2, creal).astype(np.float32), rng.uniform(0.5, 1.5, creal).astype(np.float32)
        mean64, var64 = z64.mean(0), z64.var(0)
        L, parts = _bn_chain(rows, Cc)
        zd = torch.from_numpy(z).cuda()
        vec = torch.full((4, Cc), float('nan'), dtype=torch.float32, device='cuda')
        scratch = torch.full((2 * parts * Cc,), float('nan'), dtype=torch.float32, device='cuda')
        rm, rv = torch.from_numpy(rm0).cuda(), torch.from_numpy(rv0).cuda()
        nbt = torch.tensor(5, dtype=torch.int64, device='cuda')
        gd, bd = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
        C.call('hrnet_bn3d_stats', C.HR_F32, zd.data_ptr(), gd.data_ptr(), bd.data_ptr(), scratch.data_ptr(),
               vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), rm.data_ptr(), rv.data_ptr(),
               nbt.data_ptr(), N, D, H, W, Cc, creal, mom, eps, C.stream_ptr())
        torch.cuda.synchronize()
        mean, invstd, scale, shift = (v.double().numpy() for v in vec.cpu())
        dm = (L + 2) * U * np.abs(z64).mean(0) + U * np.abs(mean64)
        dv = (L + 8) * U * (var64 + dm ** 2) + dm ** 2
        var = 1.0 / invstd ** 2 - eps
        r_mean = (np.abs(mean - mean64) / np.maximum(dm, 1e-300))[:creal].max()
        r_var = (np.abs(var - var64) / (dv + 4 * U * (var64 + eps)))[:creal].max()
        print('bn3d_stats rows {} C {}: chain {}, parts {}, mean {:.3f} of its bound, variance {:.3f}'.format(
            rows, Cc, L, parts, r_mean, r_var))
        worst = [max(worst[0], r_mean), max(worst[1], r_var)]
        assert r_mean <= 1.0 and r_var <= 1.0, (rows, Cc, r_mean, r_var)
        assert (mean[creal:] == 0).all() and (scale[creal:] == 0).all() and (shift[creal:] == 0).all()
        # scale, shift and the running statistics restate the kernel's own mean and invstd, a few roundings apart
        assert np.abs(scale - gamma * invstd).max() <= 2 * U * np.abs(gamma * invstd).max()
        assert (np.abs(shift - (beta - mean * scale)) <= 2 * U * (np.abs(beta) + np.abs(mean * scale)) + 1e-45).all()
        want_rm = (1 - mom) * rm0.astype(np.float64) + mom * mean[:creal]
        want_rv = (1 - mom) * rv0.astype(np.float64) + mom * var[:creal] * rows / (rows - 1)
        assert np.abs(rm.cpu().double().numpy() - want_rm).max() <= 4 * U * np.abs(want_rm).max() + 1e-12
        assert (np.abs(rv.cpu().double().numpy() - want_rv) <= 8 * U * (np.abs(want_rv) + eps * rows)).all()
        assert int(nbt.item()) == 6
    t = torch.zeros(64, device='cuda')
    with pytest.raises(RuntimeError, match='Expected more than 1 value per channel when training'):
        C.call('hrnet_bn3d_stats', C.HR_F32, *([t.data_ptr()] * 11), 1, 1, 1, 1, 16, 16, mom, eps, C.stream_ptr())


@spawned
def test_batchnorm_backward_with_relu_residual_and_add():
    """lattice z, res, add and dy with dyadic mean, invstd, gamma and beta: every product and sum of the FORWARD is exact
    in f32, so the sign that decides the ReLU mask is the float64 one. Three forms: y = relu(bn(z)) masked by the saved
    y, y = relu(bn(z) + res) (the masked gradient also goes to res: written, then added to), and y = relu(bn(z)) + add
    (the mask is recomputed from z; the saved y would be wrong). The routed gradient must EQUAL float64; dz, dgamma and
    dbeta are held to (L + 8) u times the same expression in absolute values, L the longest f32 chain; the conv's
    bias gradient is the zero it is. Achieved on one MI355X: largest error / bound 0.03."""
    from hipnet import _capi as C
    rng = np.random.default_rng(157)
    for N, D, H, W, Cc, creal in ((2, 3, 4, 5, 16, 16), (1, 3, 5, 7, 32, 21), (4, 1, 1, 1, 128, 128)):
        rows = N * D * H * W
        L, parts = _bn_chain(rows, Cc)
        for form in ('relu', 'res', 'add'):
            z = rng.integers(-2, 3, (rows, Cc)).astype(np.float64)
            dy = rng.integers(-2, 3, (rows, Cc)).astype(np.float64)
            other = rng.integers(-2, 3, (rows, Cc)).astype(np.float64)
            z[:, creal:] = 0; dy[:, creal:] = 0; other[:, creal:] = 0
            mean = rng.choice([-0.5, 0.0, 0.25, 1.0], Cc)
            invstd = rng.choice([0.5, 1.0, 2.0], Cc)
            gamma = rng.choice([0.5, 1.0, 1.5], Cc); gamma[creal:] = 0
            beta = rng.choice([-0.25, 0.0, 0.125], Cc); beta[creal:] = 0
            scale, shift = gamma * invstd, beta - mean * gamma * invstd
            pre = z * scale + shift
            if form == 'res':
                y = np.maximum(pre + other, 0)
                g = dy * (y > 0)
            else:
                g = dy * (pre > 0)
                y = np.maximum(pre, 0) + (other if form == 'add' else 0)
            xhat = (z - mean) * invstd
            mg, mgx = g.mean(0), (g * xhat).mean(0)
            ref_dz = scale * (g - mg - xhat * mgx)
            b_dz = (L + 8) * U * np.abs(scale) * (np.abs(g) + np.abs(g).mean(0) + np.abs(xhat) * np.abs(g * xhat).mean(0))
            f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
            zd, dyd, yd = f32(z), f32(dy), f32(y)
            vec = [f32(v) for v in (scale, shift, mean, invstd)]
            scratch = torch.full(((2 * parts + 2) * Cc,), float('nan'), dtype=torch.float32, device='cuda')
            dz = torch.full((rows, Cc), float('nan'), dtype=torch.float32, device='cuda')
            init = rng.integers(-2, 3, (rows, Cc)).astype(np.float64)
            dother = f32(init) if form == 'res' else None
            dgamma, dbeta, dbias = (torch.full((creal,), float('nan'), dtype=torch.float32, device='cuda') for _ in '123')
            C.call('hrnet_bn3d_bwd', C.HR_F32, dyd.data_ptr(), zd.data_ptr(), None if form == 'add' else yd.data_ptr(),
                   vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), scratch.data_ptr(),
                   dz.data_ptr(), C.ptr(dother), dgamma.data_ptr(), dbeta.data_ptr(), dbias.data_ptr(), N, D, H, W, Cc,
                   creal, int(form == 'add'), 1, 0, C.stream_ptr())
            torch.cuda.synchronize()
            if form == 'res':
                assert np.array_equal(dother.cpu().double().numpy(), init + g), (rows, Cc, 'res: accumulated')
                C.call('hrnet_bn3d_bwd', C.HR_F32, dyd.data_ptr(), zd.data_ptr(), yd.data_ptr(), vec[0].data_ptr(),
                       vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), scratch.data_ptr(), dz.data_ptr(),
                       dother.data_ptr(), None, None, None, N, D, H, W, Cc, creal, 0, 0, 0, C.stream_ptr())
                torch.cuda.synchronize()
                assert np.array_equal(dother.cpu().double().numpy(), g), (rows, Cc, 'res: written')
            got = dz.cpu().double().numpy()
            assert (got[:, creal:] == 0).all(), 'pad channels of dz'
            ratio = (np.abs(got - ref_dz) / np.maximum(b_dz, 1e-300))[:, :creal].max()
            r_g = np.abs(dgamma.cpu().double().numpy() - (g * xhat).sum(0)[:creal]).max()   # lattice sums: exact
            r_b = np.abs(dbeta.cpu().double().numpy() - g.sum(0)[:creal]).max()
            print('bn3d_bwd rows {} C {} {}: dz {:.3f} of its bound, dgamma off by {}, dbeta by {}'.format(
                rows, Cc, form, ratio, r_g, r_b))
            assert ratio <= 1.0 and r_g == 0 and r_b == 0, (rows, Cc, form, ratio, r_g, r_b)
            assert (dbias.cpu().numpy() == 0).all()
    # a layer without BatchNorm: only the bias sum
    dy = rng.integers(-2, 3, (210, 32)).astype(np.float32)
    dyd = torch.from_numpy(dy).cuda()
    scratch = torch.zeros(4 * 32 * 2, device='cuda')
    dbias = torch.full((21,), 2.0, device='cuda')
    C.call('hrnet_bn3d_bwd', C.HR_F32, dyd.data_ptr(), *([None] * 6), scratch.data_ptr(), None, None, None, None,
           dbias.data_ptr(), 2, 3, 5, 7, 32, 21, 0, 0, 1, C.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(dbias.cpu().numpy(), 2.0 + dy.sum(0)[:21])


def _block_case(name, make, walk, xshape, add_shape, pool, rng):
    from models.v2v import Pool3DBlock, train_blocks
    blk = make()
    sd = TR.block_state(blk, rng)
    blk.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(blk.state_dict()[k].dtype) for k, v in sd.items()})
    x = rng.normal(0.0, 1.0, xshape).astype(np.float32)
    add = None if add_shape is None else rng.normal(0.0, 1.0, add_shape).astype(np.float32)
    psd = {'b.' + k: v for k, v in sd.items()}
    with torch.no_grad():
        yshape = tuple(walk(TR.TrainNet(psd), torch.from_numpy(x).double(),
                            None if add is None else torch.from_numpy(add).double()).shape)
    gout = rng.normal(0.0, 1.0, yshape).astype(np.float32)
    r64 = TR.run(psd, walk, x, gout, add)
    r32 = TR.run(psd, walk, x, gout, add, torch.float32)
    blk = blk.cuda().train()
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    ad = None if add is None else torch.from_numpy(add).cuda().requires_grad_(True)
    y = train_blocks(([Pool3DBlock(2)] if pool else []) + [blk], xd, ad)
    y.backward(torch.from_numpy(gout).cuda())
    torch.cuda.synchronize()
    dev = {'y': y.detach(), 'dx': xd.grad}
    if ad is not None:
        dev['dadd'] = ad.grad
    for k, p in blk.named_parameters():
        dev['grad:b.' + k] = p.grad
    for k, b in blk.named_buffers():
        dev['b.' + k] = b
    dev = {k: v.cpu().double().numpy() for k, v in dev.items()}
    assert set(dev) == set(r64)
    return TR.compare(name, dev, r64, r32, psd.keys())


@spawned
def test_blocks_through_autograd_against_float64():
    """training mode, BatchNorm weight in [0.5, 1.5], bias in +-0.3, conv biases in +-0.1: y, dx, the gradient of the
    added tensor, every parameter gradient and the running statistics after the step. Per tensor
    max|dev - f64| / max|f64| <= 4 x the largest such error of the same case in float32 on the CPU (over the tensors of
    the case: two legitimate f32 summation orders differ per tensor by up to 3.5 x). A conv bias under a BatchNorm has
    gradient zero: |dbias| <= 4 x max|dbias| of the float32 run. Achieved on one MI355X: see DESIGN.md, "V2V training"."""
    from models.v2v import Basic3DBlock, Res3DBlock, Upsample3DBlock
    rng = np.random.default_rng(163)
    res = lambda net, t, a: net.res(t, 'b')
    basic = lambda net, t, a: net.basic(t, 'b')
    cases = (
        ('Res3DBlock(16,32) (2,16,4,6,10)', lambda: Res3DBlock(16, 32), res, (2, 16, 4, 6, 10), None, False),
        ('Res3DBlock(32,32) (2,32,3,5,7)', lambda: Res3DBlock(32, 32), res, (2, 32, 3, 5, 7), None, False),
        ('Res3DBlock(128,128) (4,128,1,1,1)', lambda: Res3DBlock(128, 128), res, (4, 128, 1, 1, 1), None, False),
        ('Res3DBlock(128,128) (1,128,2,2,2)', lambda: Res3DBlock(128, 128), res, (1, 128, 2, 2, 2), None, False),
        ('Basic3DBlock(4,16,7) (2,4,3,4,9)', lambda: Basic3DBlock(4, 16, 7), basic, (2, 4, 3, 4, 9), None, False),
        ('Basic3DBlock(32,32,1) (2,32,3,4,5)', lambda: Basic3DBlock(32, 32, 1), basic, (2, 32, 3, 4, 5), None, False),
        ('Upsample3DBlock(32,16) + add (2,32,3,4,5)', lambda: Upsample3DBlock(32, 16, 2, 2),
         lambda net, t, a: net.upsample(t, 'b', a), (2, 32, 3, 4, 5), (2, 16, 6, 8, 10), False),
        ('Pool3DBlock, Res3DBlock(32,64) (2,32,4,6,6)', lambda: Res3DBlock(32, 64),
         lambda net, t, a: net.res(net.pool(t), 'b'), (2, 32, 4, 6, 6), None, True),
    )
    for case in cases:
        _block_case(*case, rng)


def _model_state(model, seed):
    sd0 = model.state_dict()
    fill = R.fill_state_dict([(k, tuple(v.shape)) for k, v in sd0.items()], seed)
    fill = {k: (np.asarray(v, dtype=np.float32).astype(np.float64) if np.asarray(v).dtype.kind == 'f' else v)
            for k, v in fill.items()}
    model.load_state_dict({k: torch.from_numpy(np.asarray(fill[k])).to(sd0[k].dtype) for k in sd0}, strict=True)
    return fill


@spawned
def test_whole_network_trains():
    """V2VModel(4, 3, trainable=True) at (2, 4, 32, 32, 64), the smallest input whose bottom level has more than two
    values per channel, one forward and backward with a random output gradient. A STRUCTURAL check: per tensor the
    max-abs error over max|f64| is held to 4 x the largest per-tensor error of the float32 CPU run, which ReLU and
    argmax flips put at 2e-2 .. 4e-2 - a missing path or a wrong order shows, a rounding error does not (the kernel
    and block tests hold those). Conv biases under a BatchNorm as in the block tests. The float64 reference takes
    about 12 s and the float32 one 2 s on 16 CPU threads; that is the cost of this test.
    Then: a second identical forward and backward gives the same bits; five Adam(lr = 1e-3) steps on a fixed batch
    lower an MSE loss; .eval() under no_grad then runs on the updated running statistics and meets the float64 eval
    restatement within the forward criterion (4 x the restatement's float32 error)."""
    from models.v2v import V2VModel
    rng = np.random.default_rng(167)
    model = V2VModel(4, 3, trainable=True)
    fill = _model_state(model, 169)
    shape = (2, 4, 32, 32, 64)
    x = rng.normal(0.0, 1.0, shape).astype(np.float32)
    gout = rng.normal(0.0, 1.0, (2, 3, 32, 32, 64)).astype(np.float32)
    r64 = TR.run(fill, TR.whole, x, gout)
    r32 = TR.run(fill, TR.whole, x, gout, None, torch.float32)
    model = model.cuda().train()

    def step():
        for p in model.parameters():
            p.grad = None
        xd = torch.from_numpy(x).cuda().requires_grad_(True)
        y = model(xd)
        y.backward(torch.from_numpy(gout).cuda())
        torch.cuda.synchronize()
        out = {'y': y.detach(), 'dx': xd.grad}
        out.update({'grad:' + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
        return {k: v.cpu().numpy() for k, v in out.items()}
    first = step()
    dev = {k: v.astype(np.float64) for k, v in first.items()}
    dev.update({k: b.cpu().double().numpy() for k, b in model.named_buffers()})
    assert set(dev) == set(r64)
    TR.compare('whole network (2, 4 -> 3, 32 x 32 x 64)', dev, r64, r32, fill.keys())
    # gradients accumulate into an existing .grad
    w = model.output_layer.weight
    kept = w.grad.clone()
    model(torch.from_numpy(x).cuda()).backward(torch.from_numpy(gout).cuda())
    # (the running statistics moved between the two forwards, the batch statistics did not: the same gradient)
    assert torch.equal(w.grad, kept + kept)
    # equal bits in a second run from the same state
    _model_state(model, 169)
    a = step()
    _model_state(model, 169)
    b = step()
    for k in a:
        assert np.array_equal(a[k], b[k]), ('not reproducible', k)
        assert np.array_equal(a[k], first[k]), ('not reproducible after a reload', k)
    # frozen parameters get no gradient
    for p in model.front_layers.parameters():
        p.requires_grad_(False)
    c = step()
    assert all(p.grad is None for p in model.front_layers.parameters())
    assert set(a) - set(c) == {'grad:' + k for k, _ in model.named_parameters() if k.startswith('front_layers.')}
    assert np.array_equal(c['grad:output_layer.weight'], a['grad:output_layer.weight'])
    assert np.array_equal(c['dx'], a['dx'])
    for p in model.front_layers.parameters():
        p.requires_grad_(True)
    # five Adam steps on a fixed batch lower an MSE loss
    _model_state(model, 169)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    xd, target = torch.from_numpy(x).cuda(), torch.from_numpy(gout).cuda() * 0.1
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(model(xd), target)
        losses.append(float(loss))
        if len(losses) <= 5:
            loss.backward()
            opt.step()
    print('MSE over five Adam steps:', ' '.join('{:.5f}'.format(v) for v in losses))
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
    # eval on the updated running statistics
    model.eval()
    sd = {k: v.detach().cpu().double().numpy() if v.is_floating_point() else v.cpu().numpy()
          for k, v in model.state_dict().items()}
    assert int(sd['front_layers.0.block.1.num_batches_tracked']) == 7 + 6
    with torch.no_grad():
        ye = model(xd).cpu().double().numpy()
    y64, y32 = R.forward(sd, x), R.forward(sd, x, torch.float32)
    e_ref, err = TR.rel_err(y32, y64), TR.rel_err(ye, y64)
    print('eval after training: device {:.3e}, e_ref {:.3e}, bound {:.3e}'.format(err, e_ref, 4 * e_ref))
    assert err <= 4 * e_ref, (err, e_ref)
    with pytest.raises(NotImplementedError, match='eval mode with a gradient required'):
        model(xd)
    model.train()
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        model(xd[:1, :, :, :, :32])


@spawned
def test_eval_after_a_training_forward_without_an_optimiser_step():
    """eval under no_grad, then training-mode forwards that change no parameter (under no_grad: recalibrating the
    BatchNorm statistics; and with a backward but no optimiser step), then eval again: the second eval must run on the
    UPDATED running statistics, which the kernels write through their addresses without moving a version counter.
    Held, like every eval forward, to 4 x the float32 error of the float64 restatement on the model's buffers; that
    the statistics moved at all is asserted on the outputs of the two restatements. Also with the mode flipped by
    hand (`training = True`), which does not go through train(). Last, the two refusals of a backward whose forward's
    state is gone: a parameter modified in between, and a later forward of the same shape."""
    from models.v2v import V2VModel
    rng = np.random.default_rng(173)
    model = V2VModel(4, 3, trainable=True)
    _model_state(model, 175)
    model = model.cuda()
    x = rng.normal(0.0, 1.0, (2, 4, 32, 32, 64)).astype(np.float32)   # as test_whole_network_trains: four values at the bottom
    xd = torch.from_numpy(x).cuda()

    def eval_check(what):
        sd = {k: v.detach().cpu().double().numpy() if v.is_floating_point() else v.cpu().numpy()
              for k, v in model.state_dict().items()}
        with torch.no_grad():
            ye = model(xd).cpu().double().numpy()
        y64, y32 = R.forward(sd, x), R.forward(sd, x, torch.float32)
        e_ref, err = TR.rel_err(y32, y64), TR.rel_err(ye, y64)
        print('{}: device {:.3e}, e_ref {:.3e}, bound {:.3e}'.format(what, err, e_ref, 4 * e_ref))
        assert err <= 4 * e_ref, (what, err, e_ref)
        return y64
    model.eval()
    y_a = eval_check('eval before any training forward')
    model.train()
    with torch.no_grad():
        model(xd)
    model.eval()
    y_b = eval_check('eval after a training forward under no_grad')
    assert TR.rel_err(y_b, y_a) > 1e-3                                    # the statistics did move
    model.training = True                                                 # by hand: train() is not called
    model(xd).sum().backward()                                            # a backward, no optimiser step
    model.training = False
    y_c = eval_check('eval after a forward and backward with the mode flipped by hand')
    assert TR.rel_err(y_c, y_b) > 1e-3
    assert int(model.front_layers[0].block[1].num_batches_tracked) == 7 + 2
    # a parameter modified in place between a forward and its backward: refused, as autograd refuses for a saved tensor
    model.train()
    y = model(xd)
    with torch.no_grad():
        model.output_layer.bias.add_(1.0)
    with pytest.raises(RuntimeError, match='between this forward and its backward'):
        y.sum().backward()
    # and a backward after a later forward of the same shape
    y1 = model(xd)
    model(xd)
    with pytest.raises(RuntimeError, match='a later forward of the same input shape'):
        y1.sum().backward()


@spawned
def test_gradients_flow_through_the_chain_unproject_v2v_integrate():
    """unproject_heatmaps -> V2VModel(trainable=True) -> integrate_tensor_3d_with_coordinates -> sum at the shapes of
    test_the_chain_unproject_v2v_integrate, batch 2 for the BatchNorm: finite, non-zero gradients reach the feature maps
    and the first convolution's weight"""
    from models.v2v import V2VModel
    from utils.volumetric import build_coord_volumes, integrate_tensor_3d_with_coordinates, unproject_heatmaps
    rng = np.random.default_rng(191)
    B, V, Cn, H, W, S, J, mult = 2, 2, 4, 16, 16, 32, 3, 4.0
    cv = build_coord_volumes(torch.tensor([[10.0, -5.0, 20.0], [12.0, -4.0, 18.0]]), 300.0, S).cuda()
    proj = VR.ring_cameras(V, 1200.0, 50.0, (8.0, 8.0), target=(10.0, -5.0, 20.0))[None].astype(np.float32)
    proj = torch.from_numpy(np.repeat(proj, B, 0)).cuda()
    feat = torch.from_numpy(rng.normal(0.0, 1.0, (B, V, Cn, H, W)).astype(np.float32)).cuda().requires_grad_(True)
    model = V2VModel(Cn, J, trainable=True)
    _model_state(model, 193)
    model = model.cuda().train()
    vol = unproject_heatmaps(feat, proj, cv, 'sum')
    kp, _ = integrate_tensor_3d_with_coordinates(model(vol), cv, softmax=True, multiplier=mult)
    kp.sum().backward()
    torch.cuda.synchronize()
    for what, g in (('feature maps', feat.grad), ('front_layers.0.block.0.weight', model.front_layers[0].block[0].weight.grad)):
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, what
        print('chain: max|d sum(key points) / d {}| = {:.3e}'.format(what, float(g.abs().max())))
