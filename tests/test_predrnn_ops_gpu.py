"""The kernels of csrc/predrnn.hip, one by one, against float64 on the CPU (tests/predrnn_ref.py's NHWC restatements):
hrnet_sample_stats, hrnet_stlstm_gates, hrnet_stlstm_out, hrnet_maxpool2d_2x2 through the checked ops of hipnet.predrnn.

Statistics: mean and rstd each within 2^-23 relative of the float64 value - what sums in double rounded to float once
guarantee with a factor two to spare (the rounding is 2^-24), and what a float32 E[x^2] - mean^2 misses by three orders of
magnitude at mean 50, sigma 1. Gates and out: within bound(e_ref) = 4 e_ref + 2^-23 of the float64 result over its largest
value, e_ref the same measure of the float32 CPU restatement. The pool is exact."""
import numpy as np
import pytest
import torch

import predrnn_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CANARY = 777.0


@pytest.fixture(scope='module')
def P():
    from hipnet import predrnn
    return predrnn


def _dev(t):
    return t.float().to(DEV).contiguous()


# ---- statistics ------------------------------------------------------------------------------------------------------
STAT_SHAPES = [(1, 1, 4), (17, 17, 28), (40, 40, 28)]        # 4 elements (less than a wave); odd; 44 800: six workgroups


@pytest.fixture(scope='module')
def stat_maps():
    """three maps of B = 3 samples, N(50, 1) scaled per sample (1, 1/4, 3): float32 tensors and their float64 statistics"""
    rng = np.random.RandomState(R.SEED)
    maps, want = [], []
    for shape in STAT_SHAPES:
        x = (50.0 + rng.standard_normal((3,) + shape)) * np.array([1.0, 0.25, 3.0]).reshape(3, 1, 1, 1)
        x = torch.tensor(x, dtype=torch.float32)
        maps.append(x)
        want.append(R.sample_stats(x.double()).numpy())
    return maps, np.stack(want)


def test_stats_three_maps_in_one_launch(P, stat_maps):
    maps, want = stat_maps
    assert P.stats_scratch_bytes(3, [m[0].numel() for m in maps]) == 3 * (1 + 1 + 6) * 16
    dev = [_dev(m) for m in maps]
    got = P.sample_stats(dev)
    again = P.sample_stats(dev)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (3, 3, 2) and torch.equal(got, again)
    err = np.abs(got.cpu().double().numpy() - want) / np.abs(want)
    print('sample_stats relative errors: mean {:.2e} rstd {:.2e} (bound {:.2e})'.format(
        err[..., 0].max(), err[..., 1].max(), 2.0 ** -23))
    assert err.max() <= 2.0 ** -23
    # the naive float32 form is not within reach of this bound: the test would see it
    x = maps[2]
    naive = 1.0 / torch.sqrt((x * x).reshape(3, -1).mean(1) - x.reshape(3, -1).mean(1) ** 2 + 1e-5)
    assert (np.abs(naive.double().numpy() - want[2, :, 1]) / want[2, :, 1]).max() > 100 * 2.0 ** -23


@pytest.mark.parametrize('pick', [(0,), (1,), (2,), (2, 0), (1, 2)])
def test_stats_do_not_depend_on_the_company(P, stat_maps, pick):
    maps, want = stat_maps
    all3 = P.sample_stats([_dev(m) for m in maps])
    got = P.sample_stats([_dev(maps[i]) for i in pick])
    for k, i in enumerate(pick):
        assert torch.equal(got[k], all3[i])


def test_stats_of_a_constant_map(P):
    x = torch.full((2, 3, 5, 12), 0.3, dtype=torch.float32)
    x[1] = -7.25
    got = P.sample_stats([_dev(x)]).cpu().double().numpy()[0]
    assert np.array_equal(got[:, 0], x[:, 0, 0, 0].double().numpy())
    assert (np.abs(got[:, 1] - 1.0 / np.sqrt(1e-5)) * np.sqrt(1e-5)).max() <= 2.0 ** -23


def test_stats_refusals(P):
    x = torch.zeros((2, 3, 3, 4), device=DEV)
    with pytest.raises(ValueError, match='HIP-device'):
        P.sample_stats([x.cpu()])
    with pytest.raises(ValueError, match='one to 3'):
        P.sample_stats([x, x, x, x])
    with pytest.raises(ValueError, match='multiple of 4'):
        P.sample_stats([torch.zeros((2, 3, 3, 3), device=DEV)])
    with pytest.raises(ValueError, match='B = 2'):
        P.sample_stats([x, torch.zeros((3, 3, 3, 4), device=DEV)])
    with pytest.raises(NotImplementedError, match='inference only'):
        P.sample_stats([x.clone().requires_grad_(True)])


# ---- gates and out ---------------------------------------------------------------------------------------------------
def _cell_inputs(nh, H, W, B, hc_mode, seed):
    rng = np.random.RandomState(seed)
    n = lambda *s: torch.tensor(rng.standard_normal(s), dtype=torch.float32)
    d = {'xc': n(B, H, W, 7 * nh) * 0.7 + 0.2, 'hc': n(B, H, W, 4 * nh) * 1.3 - 0.4, 'mc': n(B, H, W, 3 * nh) + 2.0,
         'c_t': n(B, H, W, nh), 'm_t': n(B, H, W, nh) * 0.5,
         'ln': [(1.0 if i % 2 == 0 else 0.0) + 0.1 * n(H, W, k * nh) for i, k in enumerate((7, 7, 4, 4, 3, 3))],
         'oc': n(B, H, W, nh) * 2.0 + 1.0, 'wo': 1.0 + 0.1 * n(H, W, nh), 'bo': 0.1 * n(H, W, nh), 'last': n(B, H, W, nh)}
    if hc_mode == 'bias':            # t = 0: conv_h of a zero map is its bias, one value per channel
        d['hc'] = (n(4 * nh) * 0.1).reshape(1, 1, 1, -1).expand(B, H, W, 4 * nh).contiguous()
    elif hc_mode == 'constant':      # ... and all biases equal: variance 0, rstd = 1 / sqrt(eps)
        d['hc'] = torch.full((B, H, W, 4 * nh), 0.0625)
    return d


def _ref(d, nh, dtype):
    t = lambda v: v.to(dtype)
    c, m, o = R.gates(t(d['xc']), t(d['hc']), t(d['mc']), [t(v) for v in d['ln']], t(d['c_t']), t(d['m_t']), nh)
    h = R.out_gate(t(d['oc']), t(d['wo']), t(d['bo']), o, t(d['last']))
    return [v.double().numpy() for v in (c, m, o, h)]


def _run_cell_ops(P, d, nh, aliased, extra=4):
    """(c_new, m_new, o_pre, h_new, the memory map) from the device; the memory map has `extra` canary channels"""
    B, H, W, _ = d['xc'].shape
    xc, hc, mc = _dev(d['xc']), _dev(d['hc']), _dev(d['mc'])
    ln = [_dev(v) for v in d['ln']]
    mem = torch.full((B, H, W, 2 * nh + extra), CANARY, dtype=torch.float32, device=DEV)
    st = P.sample_stats([xc, hc, mc])
    if aliased:
        mem[..., :nh] = _dev(d['c_t'])
        mem[..., nh:2 * nh] = _dev(d['m_t'])
        _, o_pre = P.stlstm_gates(xc, hc, mc, st, ln, mem, mem, mem, nh, c_off=0, m_off=nh)
    else:
        # the states as slices of wider maps at offsets of their own
        c_t = torch.full((B, H, W, nh + 8), CANARY, dtype=torch.float32, device=DEV)
        c_t[..., 4:4 + nh] = _dev(d['c_t'])
        m_t = torch.full((B, H, W, 2 * nh), CANARY, dtype=torch.float32, device=DEV)
        m_t[..., nh:] = _dev(d['m_t'])
        _, o_pre = P.stlstm_gates(xc, hc, mc, st, ln, c_t, m_t, mem, nh, c_off=4, m_off=nh)
    oc = _dev(d['oc'])
    h = P.stlstm_out(oc, P.sample_stats([oc]), _dev(d['wo']), _dev(d['bo']), o_pre, _dev(d['last']))
    torch.cuda.synchronize()
    return mem[..., :nh].cpu(), mem[..., nh:2 * nh].cpu(), o_pre.cpu(), h.cpu(), mem.cpu()


GATE_CASES = [(nh, hw, B, 'random') for nh in (4, 12, 64) for hw in ((1, 1), (3, 5), (17, 17)) for B in (1, 3)]
GATE_CASES += [(4, (1, 1), 1, 'bias'), (12, (3, 5), 3, 'bias'), (64, (17, 17), 1, 'bias'),
               (4, (1, 1), 1, 'constant'), (12, (3, 5), 3, 'constant'), (64, (17, 17), 1, 'constant')]


@pytest.mark.parametrize('nh, hw, B, hc_mode', GATE_CASES)
def test_gates_and_out(P, nh, hw, B, hc_mode):
    d = _cell_inputs(nh, hw[0], hw[1], B, hc_mode, R.SEED + nh + 7 * hw[0] + B)
    ref64, ref32 = _ref(d, nh, torch.float64), _ref(d, nh, torch.float32)
    plain = _run_cell_ops(P, d, nh, aliased=False)
    alias = _run_cell_ops(P, d, nh, aliased=True)
    for name, got, got_a, r64, r32 in zip(('c_new', 'm_new', 'o_pre', 'h_new'), plain, alias, ref64, ref32):
        e_ref, err = R.rel(r32, r64), R.rel(got.double().numpy(), r64)
        print('{} nh {} map {} B {} hc {}: err {:.2e} e_ref {:.2e} bound {:.2e}'.format(
            name, nh, hw, B, hc_mode, err, e_ref, R.bound(e_ref)))
        assert err <= R.bound(e_ref), name
        assert torch.equal(got, got_a), name + ': the aliased call differs'
    for mem in (plain[4], alias[4]):
        assert bool((mem[..., 2 * nh:] == CANARY).all()), 'the channels behind 2 nh were written'


def test_gates_refusals(P):
    nh, B, H, W = 4, 1, 2, 2
    d = _cell_inputs(nh, H, W, B, 'random', 1)
    xc, hc, mc = _dev(d['xc']), _dev(d['hc']), _dev(d['mc'])
    ln = [_dev(v) for v in d['ln']]
    st = P.sample_stats([xc, hc, mc])
    mem = torch.zeros((B, H, W, 2 * nh), device=DEV)
    keep = mem.clone()
    with pytest.raises(ValueError, match='HIP-device'):
        P.stlstm_gates(xc.cpu(), hc, mc, st, ln, mem, mem, mem, nh, m_off=nh)
    with pytest.raises(ValueError, match='hc'):
        P.stlstm_gates(xc, mc, mc, st, ln, mem, mem, mem, nh, m_off=nh)
    with pytest.raises(ValueError, match='m_off must be nh'):
        P.stlstm_gates(xc, hc, mc, st, ln, mem, mem, mem, nh, m_off=0)
    with pytest.raises(ValueError, match='c_off must be 0'):
        P.stlstm_gates(xc, hc, mc, st, ln, mem, mem, mem, nh, c_off=nh, m_off=nh)
    with pytest.raises(ValueError, match='wx'):
        P.stlstm_gates(xc, hc, mc, st, ln[::-1], mem, mem, mem, nh, m_off=nh)
    with pytest.raises(NotImplementedError, match='inference only'):
        P.stlstm_gates(xc.clone().requires_grad_(True), hc, mc, st, ln, mem, mem, mem, nh, m_off=nh)
    # an overlap that is not the element-for-element one is the C entry's to refuse: a view of mem shifted by one pixel
    flat = torch.zeros(B * H * W * 2 * nh + 2 * nh, device=DEV)
    shifted, base = flat[2 * nh:].view(B, H, W, 2 * nh), flat[:B * H * W * 2 * nh].view(B, H, W, 2 * nh)
    with pytest.raises(RuntimeError, match='overlaps mem'):
        P.stlstm_gates(xc, hc, mc, st, ln, shifted, base, base, nh, m_off=nh)
    torch.cuda.synchronize()
    assert torch.equal(mem, keep) and float(flat.abs().max()) == 0.0


# ---- pool ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H, W, c, x_off, ldx, y_off, ldy', [(2, 2, 4, 0, 4, 0, 4), (6, 10, 8, 4, 16, 8, 20),
                                                             (6, 10, 56, 0, 56, 0, 56), (2, 2, 4, 8, 12, 4, 8)])
def test_maxpool2x2(P, H, W, c, x_off, ldx, y_off, ldy):
    rng = np.random.RandomState(R.SEED + H + c)
    x = torch.tensor(rng.standard_normal((2, H, W, ldx)), dtype=torch.float32)
    out = torch.full((2, H // 2, W // 2, ldy), CANARY, dtype=torch.float32, device=DEV)
    got = P.maxpool2x2(_dev(x), c, x_off, out=out, y_off=y_off)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    want = torch.full((2, H // 2, W // 2, ldy), CANARY)
    want[..., y_off:y_off + c] = R.maxpool2x2(x[..., x_off:x_off + c])
    assert torch.equal(out.cpu(), want)
    if x_off == 0 and c == ldx:
        assert torch.equal(P.maxpool2x2(_dev(x)).cpu(), R.maxpool2x2(x))


def test_maxpool2x2_refusals(P):
    x = torch.zeros((1, 4, 4, 8), device=DEV)
    with pytest.raises(ValueError, match='even'):
        P.maxpool2x2(torch.zeros((1, 3, 4, 8), device=DEV))
    with pytest.raises(ValueError, match='multiples of 4'):
        P.maxpool2x2(x, 3)
    with pytest.raises(ValueError, match='expected \\(1, 2, 2, ld\\)'):
        P.maxpool2x2(x, out=torch.zeros((1, 4, 4, 8), device=DEV))
    with pytest.raises(ValueError, match='HIP-device'):
        P.maxpool2x2(x.cpu())


def test_pack_ln_round_trip(P):
    t = torch.arange(2 * 3 * 5, dtype=torch.float32).reshape(2, 3, 5)
    p = P.pack_ln(t.to(DEV))
    assert tuple(p.shape) == (3, 5, 2) and p.is_contiguous() and float(p[1, 2, 1]) == float(t[1, 1, 2])
    assert torch.equal(P.unpack_ln(p).cpu(), t)
