"""The BatchNorm statistic sums the conv epilogues gather, held to bounds that see one tile (tests/bn_bounds.py).

Every producer of the conv family - forward batch sums as per-walk rows (hrnet_conv2d, hrnet_conv2d_sum) and as float
atomics into sums[8][2][C] (hrnet_conv2d_bnref, hrnet_conv2d_sum stats_atomic) on the tile-walking body and the LDS
ring, backward-statistics rows (hrnet_conv2d_bwdstats: bn_relu, sum_mask and unmasked, the stride-2 four-parity form,
both routes) - against an f64 sum over the operands the device saw. The data are of one sign per channel, so a missing,
doubled or wrong tile moves a channel's sum by more than twice the bound; every case asserts that, with the tile of
its own launch geometry. test_every_statistics_instantiation_of_a_training_step_has_a_case ties the cases to the
kernel instantiations a w32 bf16 B=64 training step records."""
import ctypes
import re

import pytest
import torch

import bn_bounds as B

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


def _hh():
    import hip_helpers as hh
    return hh


def _C():
    from hipnet import _capi as C
    return C


class _ring(object):
    """hrnet_conv_ring_enable(on) for a block, restored afterwards"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev = _C().call('hrnet_conv_ring_enable', self.on)
        return self

    def __exit__(self, *exc):
        _C().call('hrnet_conv_ring_enable', 1 if self.prev != 0 else 0)


def _walk(N, Ho, Wo, Cout, ks, stride, bs=False, s2d=False):
    out = (ctypes.c_int * 5)()
    _C().call('hrnet_conv_tile_walk', N, Ho, Wo, Cout, ks, stride, 1 if bs else 0, 1 if s2d else 0, out)
    return dict(th=out[0], tw=out[1], bn=out[2], tpw=out[3], gx=out[4])


def _name(dtype_id, N, Ho, Wo, Cin, Cout, ks, stride, upz, mode):
    buf = ctypes.create_string_buffer(160)
    _C().call('hrnet_conv_kernel_name', dtype_id, N, Ho, Wo, Cin, Cout, ks, stride, upz, mode, buf, 160)
    return buf.value.decode()


def _mode(bs, bias, upz, acc, stats, affine, relu):
    return _C().call('hrnet_conv_mode', int(bs), int(bias), int(upz), int(acc), int(stats), int(affine), int(relu))


def _ring_geometry(name, N, H, W, Cout):
    """tile (ti images x th x tw, from the instantiation's name) and an upper bound on the tiles one workgroup walks:
    conv_ring.hip aims every grid at >= 256 workgroups (256 x workgroups per CU) or gives each workgroup one tile"""
    m = re.match(r'conv_ring_kernel<(\d+), (\d+), (\d+), (\d+), \d+, \d+, \d+, \d+, (true|false)>', name)
    assert m, name
    th, tw, ti, nb = (int(m.group(k)) for k in (1, 2, 3, 4))
    total = -(-N // ti) * -(-H // th) * -(-W // tw)
    tpw = max(1, -(-(total * -(-Cout // nb)) // 256))
    return dict(th=th, tw=tw, ti=ti, tpw=tpw, gx=total)     # gx: an upper bound on the walks (atomic adds per copy)


def _check_terms(label, terms, got, D, geo):
    """got [2][C] device sums; terms [(label, t, e)] of bn_bounds"""
    for k, (lab, t, e) in enumerate(terms):
        B.check('{} {} (D={})'.format(label, lab, D), got[k], t.sum((0, 2, 3)), B.channel_bound(t, e, D),
                B.tile_sums(t, geo['th'], geo['tw'], geo.get('ti', 1)))


# ---- forward batch sums ---------------------------------------------------------------------------------------------
FWD_CASES = [
    # N, H, W, Cin, Cout, ks, stride, input BatchNorm + ReLU, bias
    (3, 20, 37, 32, 32, 3, 1, True, False),      # tiles overhang the map on both axes
    (5, 13, 21, 64, 48, 3, 2, True, True),       # stride 2, bias, partial tiles
    (7, 24, 40, 32, 64, 1, 1, True, True),       # 1x1 with bias
    (71, 48, 48, 32, 32, 3, 1, True, False),     # odd tile count: the last walk is short
    (64, 64, 64, 32, 32, 3, 1, True, False),     # the w32 layer shapes at B=64
    (64, 32, 32, 64, 64, 3, 1, True, False),
    (64, 16, 16, 128, 128, 3, 1, True, False),
    (64, 8, 8, 256, 256, 3, 1, True, False),
    (64, 64, 64, 64, 256, 1, 1, True, False),    # layer1 1x1 pair (and its 64 -> 64)
    (64, 64, 64, 256, 64, 1, 1, True, False),
    (64, 64, 64, 64, 64, 1, 1, True, False),
    (64, 8, 8, 256, 128, 1, 1, True, False),
    (64, 64, 64, 32, 32, 3, 2, True, False),     # fuse-layer down paths
    (64, 64, 64, 32, 64, 3, 2, True, False),
    (8, 64, 64, 480, 480, 1, 1, False, True),    # the 480-channel head layer (bias)
    (20, 96, 72, 48, 48, 3, 1, True, False),     # w48 geometry: partial tiles
]
# (a 480 -> 480 1x1 launch without per-walk rows goes to the GEMM kernel, which writes no statistics in the step)
ATOMIC_CASES = [c[:8] + (False,) for c in FWD_CASES if c[3] != 480]
RING_FWD_CASES = [c for c in ATOMIC_CASES if c[5] == 3 and c[6] == 1 and c[3] in (32, 64, 128, 256)]


def _fwd_ref(case, dtype, affine=None):
    N, H, W, Cin, Cout, ks, stride, aff, bias = case
    aff = aff if affine is None else affine
    d = B.fwd_data(N, H, W, Cin, Cout, ks, stride, aff, bias, dtype, seed=100 + N + H + Cin + Cout + ks + stride)
    y, e = B.fwd_reference(d, ks, stride, dtype)
    return d, B.fwd_terms(y, e)


def fwd_rows_name(case, dtype_id):
    N, H, W, Cin, Cout, ks, stride, aff, bias = case
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    with _ring(0):      # (per-walk rows are never the ring's: it adds by atomics)
        n = _name(dtype_id, N, Ho, Wo, Cin, Cout, ks, stride, 0, _mode(0, bias, 0, 0, 1, aff, aff))
    # the name query reports the GEMM kernel for the 480-channel head, but a launch with per-walk rows stays on the
    # tile-walking body (conv.hip: the GEMM takes atomic statistics or none), whose name the query cannot give
    return None if n == 'gemm_pw_kernel' else n


@pytest.mark.parametrize('dtype', [F32, BF])
@pytest.mark.parametrize('case', FWD_CASES)
def test_forward_statistics_rows(dtype, case):
    """hrnet_conv2d: one (sum y, sum y^2) row per pixel walk of the tile-walking body"""
    hh, C = _hh(), _C()
    N, H, W, Cin, Cout, ks, stride, aff, bias = case
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    geo = _walk(N, Ho, Wo, Cout, ks, stride)
    d, terms = _fwd_ref(case, dtype)
    wp, cop, _ = hh.pack_weights(d['w'], dtype)
    assert cop == Cout
    name = fwd_rows_name(case, hh.dt_id(dtype))
    assert name is None and Cin == 480 or name.startswith('conv_fwd') and not name.startswith('conv_fwds'), name
    y, st = hh.conv2d(hh.nhwc(d['x'], dtype), wp, N, H, W, Cin, Cout, ks, stride, dtype,
                      in_scale=d['sc'].to(hh.DEV) if aff else None, in_shift=d['sh'].to(hh.DEV) if aff else None,
                      bias=d['bias'].to(hh.DEV) if bias else None, in_relu=aff, stats=True)
    assert st.shape[0] == geo['gx']
    hh.sync()
    _check_terms('{} {}'.format(name, case), terms, st.double().sum(0).cpu(), B.walk_chain(geo['th'], geo['tw'], geo['tpw']), geo)


def bnref_name(case, ring):
    N, H, W, Cin, Cout, ks, stride, _, bias = case
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    with _ring(ring):
        return _name(1, N, Ho, Wo, Cin, Cout, ks, stride, 0, _mode(0, 0, 0, 0, 1, 0, 0))


@pytest.mark.parametrize('case,route', [(c, 'walk') for c in ATOMIC_CASES] + [(c, 'ring') for c in RING_FWD_CASES])
def test_forward_statistics_atomic_sums(case, route):
    """hrnet_conv2d_bnref out_sums: float atomics into sums[8][2][C] (raw input), on the tile-walking body and,
    for the shapes it serves, the LDS ring"""
    hh, C = _hh(), _C()
    N, H, W, Cin, Cout, ks, stride, _, bias = case
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    d, terms = _fwd_ref(case, BF, affine=False)
    wp, _, _ = hh.pack_weights(d['w'], BF)
    xd = hh.nhwc(d['x'], BF)
    on = 1 if route == 'ring' else 0
    name = bnref_name(case, on)
    with _ring(on):
        served = C.call('hrnet_conv_ring_supported', 1, N, H, W, Cin, Cout)
        assert (served > 0) == (route == 'ring') and name.startswith('conv_ring_kernel<') == (route == 'ring'), name
        y = torch.empty(N, Ho, Wo, Cout, dtype=BF, device=hh.DEV)
        sums = torch.zeros(8, 2, Cout, dtype=torch.float32, device=hh.DEV)
        C.call('hrnet_conv2d_bnref', 1, xd.data_ptr(), wp.data_ptr(), None, None, None, 0.0, 0.0, None, y.data_ptr(),
               sums.data_ptr(), N, H, W, Cin, Ho, Wo, Cout, ks, stride, 0, C.stream_ptr())
        hh.sync()
    if route == 'ring':
        geo = _ring_geometry(name, N, H, W, Cout)
        D = B.ring_chain(geo['ti'], geo['th'], geo['tw'], geo['tpw'], -(-geo['gx'] // 8))
    else:
        geo = _walk(N, Ho, Wo, Cout, ks, stride)
        D = B.walk_chain(geo['th'], geo['tw'], geo['tpw'], -(-geo['gx'] // 8))
    _check_terms('{} {}'.format(name, case), terms, sums.double().sum(0).cpu(), D, geo)


SUM_CASES = [
    # N, H, W, Cin, Cout, ks: conv of a = relu(bn(x) + x2) (hrnet_conv2d_sum)
    (3, 20, 37, 32, 32, 3),
    (64, 64, 64, 32, 32, 3),
    (64, 32, 32, 64, 64, 3),
    (64, 8, 8, 256, 256, 3),
    (64, 32, 32, 64, 32, 1),
    (64, 16, 16, 128, 32, 1),
    (64, 64, 64, 256, 64, 1),
    (64, 8, 8, 256, 32, 1),
]


def sum_name(case):
    N, H, W, Cin, Cout, ks = case
    return _name(1, N, H, W, Cin, Cout, ks, 1, 0, 5)


@pytest.mark.parametrize('atomic', [0, 1])
@pytest.mark.parametrize('case', SUM_CASES)
def test_residual_sum_conv_statistics(atomic, case):
    """hrnet_conv2d_sum: the output statistics as per-walk rows and as float atomics"""
    hh, C = _hh(), _C()
    N, H, W, Cin, Cout, ks = case
    d = B.fwd_data(N, H, W, Cin, Cout, ks, 1, True, False, BF, seed=7 + N + H + Cin + Cout + ks, residual=True)
    y_ref, e = B.fwd_reference(d, ks, 1, BF)
    terms = B.fwd_terms(y_ref, e)
    name = sum_name(case)
    assert name.startswith('conv_fwds_kernel<'), name
    geo = _walk(N, H, W, Cout, ks, 1)
    wp, _, _ = hh.pack_weights(d['w'], BF)
    xd, x2d = hh.nhwc(d['x'], BF), hh.nhwc(d['x2'], BF)
    side = torch.empty(N, H, W, Cin, dtype=BF, device=hh.DEV)
    y = torch.empty(N, H, W, Cout, dtype=BF, device=hh.DEV)
    rows = 8 if atomic else C.call('hrnet_conv_tiles', N, H, W, Cout, ks, 1)
    assert atomic or rows == geo['gx']
    st = torch.zeros(rows, 2, Cout, dtype=torch.float32, device=hh.DEV)
    scd, shd = d['sc'].to(hh.DEV), d['sh'].to(hh.DEV)
    C.call('hrnet_conv2d_sum', 1, xd.data_ptr(), x2d.data_ptr(), wp.data_ptr(), scd.data_ptr(), shd.data_ptr(), None, None, None, 0.0, 0.0, side.data_ptr(), y.data_ptr(), st.data_ptr(), atomic,
           N, H, W, Cin, Cout, ks, C.stream_ptr())
    hh.sync()
    D = B.walk_chain(geo['th'], geo['tw'], geo['tpw'], -(-geo['gx'] // 8) if atomic else 0)
    _check_terms('{} {} atomic={}'.format(name, case, atomic), terms, st.double().sum(0).cpu(), D, geo)


# ---- backward-statistics rows -------------------------------------------------------------------------------------
BS_CASES = [
    # forward-conv view: N, H, W, Cin, Cout, ks, stride (the launch writes the gradient of x and its rows)
    (3, 20, 37, 32, 32, 3, 1),        # overhanging tiles
    (5, 26, 22, 32, 64, 3, 2),        # four-parity stride-2 gradient, odd tile count
    (64, 32, 32, 64, 64, 3, 1),
    (64, 16, 16, 128, 32, 1, 1),      # w32 layer shapes at B=64
    (64, 32, 32, 64, 32, 1, 1),
    (64, 8, 8, 256, 32, 1, 1),
    (64, 32, 32, 32, 128, 3, 2),
    (64, 16, 16, 64, 256, 3, 2),
    (64, 16, 16, 128, 128, 3, 1),     # served by the ring as well
    (64, 8, 8, 256, 256, 3, 1),
]
BS_MODES = ['bn_relu', 'sum_mask', 'unmasked']


def bs_name(case, dtype_id, ring):
    N, H, W, Cin, Cout, ks, stride = case
    upz = 1 if stride == 2 else 0
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    with _ring(ring):
        return _name(dtype_id, N, H, W, Cout, Cin, ks, stride, upz, _mode(1, 0, upz, 1, 1, 0, 0))


def _bs_params():
    out = []
    for case in BS_CASES:
        for mode in BS_MODES:
            for dtype in (F32, BF):
                out.append((case, mode, dtype, 'walk'))
            if case[5] == 3 and case[6] == 1 and case[3] >= 96:
                out.append((case, mode, BF, 'ring'))
    return out


@pytest.mark.parametrize('case,mode,dtype,route', _bs_params())
def test_backward_statistics_rows(case, mode, dtype, route):
    """hrnet_conv2d_bwdstats: (sum dz, sum dz*y) per pixel walk, dz = (dgrad + old gradient) * mask"""
    hh, C = _hh(), _C()
    N, H, W, Cin, Cout, ks, stride = case
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    upz = 1 if stride == 2 else 0
    d = B.bs_data(N, H, W, Cin, Cout, ks, stride, mode, dtype, seed=300 + N + H + Cin + Cout + ks + stride)
    terms = B.bs_reference(d, ks, stride)
    wd, _, _ = hh.pack_weights(d['w'], dtype, mode=1)
    on = 1 if route == 'ring' else 0
    name = bs_name(case, hh.dt_id(dtype), on)
    with _ring(on):
        assert C.call('hrnet_conv_route', hh.dt_id(dtype), N, H, W, Cout, Cin, ks, stride) == (2 if on else 1), route
        assert name.startswith('conv_ring_kernel<' if on else 'conv_bs_kernel<'), name
        rows_n = C.call('hrnet_conv_rows_bwdstats', hh.dt_id(dtype), N, H, W, Cout, Cin, ks, stride)
        rows = torch.full((rows_n, 2, Cin), float('nan'), device=hh.DEV)
        gx = hh.nhwc(d['prev'], dtype)
        yd = hh.nhwc(d['yraw'], dtype)
        md = hh.nhwc(d['m'], dtype) if mode == 'sum_mask' else None
        scd = d['sc'].to(hh.DEV) if mode == 'bn_relu' else None
        shd = d['sh'].to(hh.DEV) if mode == 'bn_relu' else None
        C.call('hrnet_conv2d_bwdstats', hh.dt_id(dtype), hh.nhwc(d['dy'], dtype).data_ptr(), wd.data_ptr(), gx.data_ptr(),
               rows.data_ptr(), yd.data_ptr(), C.ptr(md), C.ptr(scd), C.ptr(shd), N, Ho, Wo, Cout, H, W, Cin, ks, stride,
               upz, 1, C.stream_ptr())
        hh.sync()
    if on:
        geo = _ring_geometry(name, N, H, W, Cin)
        assert -(-geo['gx'] // rows_n) <= geo['tpw'], (geo, rows_n)       # the walk-length bound holds
        D = B.ring_chain(geo['ti'], geo['th'], geo['tw'], geo['tpw'])
    else:
        geo = _walk(N, H, W, Cin, ks, stride, True, upz == 1)
        assert geo['gx'] == rows_n
        D = B.walk_chain(geo['th'], geo['tw'], geo['tpw'])
    _check_terms('{} {} {}'.format(name, case, mode), terms, rows.double().sum(0).cpu(), D, geo)


# ---- fused backward rows ------------------------------------------------------------------------------------------
FUSED_CASES = [
    # N, H, W, Cin, Cout: the BasicBlock 3x3 convs (hrnet_conv3x3_bwd_fused with coef, addend, output mask and rows)
    (3, 20, 37, 32, 32),          # overhanging tiles
    (64, 64, 64, 32, 32),         # the w32 branch layers at B=64
    (64, 32, 32, 64, 64),
    (64, 64, 64, 64, 64),
]


def fused_name(dtype_id, Cin, Cout):
    buf = ctypes.create_string_buffer(160)
    _C().call('hrnet_bwd_fused_kernel_name', dtype_id, Cin, Cout, buf, 160)
    return buf.value.decode()


def _fused_params():
    C = _C()
    return [(c, dt) for c in FUSED_CASES for dt in (F32, BF) if C.call('hrnet_bwd_fused_supported', C.dtype_id(dt), c[3], c[4])]


@pytest.mark.parametrize('case,dtype', _fused_params())
def test_fused_backward_rows(case, dtype):
    """hrnet_conv3x3_bwd_fused rows[nsplit][2][Cin]: (sum dx, sum dx*bs_y) of the masked input gradient, every split
    walking the tiles split, split + nsplit, ..."""
    hh, C = _hh(), _C()
    N, H, W, Cin, Cout = case
    did = hh.dt_id(dtype)
    name = fused_name(did, Cin, Cout)
    m = re.match(r'bwd_fused_kernel<[^,]+, (\d+), (\d+), (\d+),', name)
    assert m, name
    th, nw = int(m.group(2)), int(m.group(3))     # tile th x 16 pixels, nw waves
    d = B.fused_data(N, H, W, Cin, Cout, dtype, seed=500 + N + H + Cin + Cout)
    terms = B.fused_reference(d, dtype)
    ns = C.call('hrnet_bwd_fused_splits', did, N, H, W, Cin, Cout)
    tiles = N * -(-H // th) * -(-W // 16)
    dev = hh.DEV
    wT, _, _ = hh.pack_weights(d['w'], dtype, mode=1)
    dzd, yd, xd = hh.nhwc(d['dz'], dtype), hh.nhwc(d['y'], dtype), hh.nhwc(d['x'], dtype)
    addd, bsd = hh.nhwc(d['addend'], dtype), hh.nhwc(d['bs_y'], dtype)
    coef, scd, shd = d['coef'].contiguous().to(dev), d['sc'].to(dev), d['sh'].to(dev)
    dx = torch.empty(N, H, W, Cin, dtype=dtype, device=dev)
    rows = torch.full((ns, 2, Cin), float('nan'), device=dev)
    slabs = torch.zeros(ns, Cout, 9, Cin, device=dev)
    C.call('hrnet_conv3x3_bwd_fused', did, dzd.data_ptr(), yd.data_ptr(), coef.data_ptr(), xd.data_ptr(), scd.data_ptr(),
           shd.data_ptr(), 1, wT.data_ptr(), dx.data_ptr(), addd.data_ptr(), 1, rows.data_ptr(), bsd.data_ptr(),
           slabs.data_ptr(), N, H, W, Cin, Cout, C.stream_ptr())
    hh.sync()
    geo = dict(th=th, tw=16, tpw=-(-tiles // ns))
    _check_terms('{} {}'.format(name, case), terms, rows.double().sum(0).cpu(), B.walk_chain(th, 16, geo['tpw'], wp_max=nw), geo)


# ---- coverage -----------------------------------------------------------------------------------------------------
# statistics producers of the step that this module does not reach yet (tracked as their own work: the 1x1 fused
# backward rows, the head kernels, the BatchNorm-backward reductions): listed by what they are, so that any OTHER
# instantiation without a case fails the coverage test
NOT_YET = {'bwd_pw_kernel<256, 64>', 'bwd_pw_kernel<64, 256>', 'bwd_pw_kernel<64, 64>', 'head_mix', 'head_bwd',
           'bn_bwd_reduce', 'pool_reduce'}


def _plan_statistics_names():
    """kernel instantiation of every op that writes BatchNorm statistics in a w32 bf16 B=64 training step (the
    queries bench.py uses); the forward rows of HRNET_DETERMINISTIC=1 never take the ring, so they are named with the
    routing off. Producers without an instantiation query are named by their op."""
    import bench
    from hipnet import _capi as C
    model, _, _ = bench.build_model('bf16', 'RHD_HRNet_w32_max_hmloss_v1.yaml')
    model = model.cuda().train()
    plan = model.hip().plan(64, 256, 256, True, True)
    buf = ctypes.create_string_buffer(160)
    names = {}
    for prog in (plan.fwd, plan.bwd):
        for op in prog.ops:
            k = int(op.kind)
            if k == C.OP_CONV and op.p[6]:
                bs, atomic = bool(op.p[7]), op.i[13] != 0
                mode = _mode(bs, bool(op.p[4]), op.i[10], op.i[12], 1, bool(op.p[2]), op.i[11])
                on = 1 if (atomic or (bs and op.i[17] == 2)) else 0
                with _ring(on):
                    n = _name(op.i[0], op.i[1], op.i[5], op.i[6], op.i[4], op.i[7], op.i[8], op.i[9], op.i[10], mode)
                names.setdefault(n, tuple(op.i[:11]))
            elif k == C.OP_CONV_SUM and op.p[8]:
                names.setdefault(_name(op.i[0], op.i[1], op.i[2], op.i[3], op.i[4], op.i[5], op.i[6], 1, 0, 5), tuple(op.i[:8]))
            elif k in (C.OP_BWD_FUSED, C.OP_BWD_PW) and op.p[9]:        # p[9]: the rows of the next BatchNorm
                C.call('hrnet_bwd_fused_kernel_name' if k == C.OP_BWD_FUSED else 'hrnet_bwd_pw_kernel_name',
                       op.i[0], op.i[4], op.i[5], buf, 160)
                names.setdefault(buf.value.decode(), tuple(op.i[:8]))
            elif k == C.OP_HEAD_MIX and op.p[4]:
                names.setdefault('head_mix', tuple(op.i[:15]))
            elif k == C.OP_HEAD_BWD and op.i[6] == 1:
                names.setdefault('head_bwd', tuple(op.i[:8]))
            elif k == C.OP_BN_BWD_REDUCE or (k == C.OP_EW_TABLE and op.i[2] == C.OP_BN_BWD_REDUCE):
                names.setdefault('bn_bwd_reduce', tuple(op.i[:6]))
            elif k == C.OP_POOL_REDUCE or (k == C.OP_EW_TABLE and op.i[2] == C.OP_POOL_REDUCE):
                names.setdefault('pool_reduce', tuple(op.i[:6]))
    del plan, model
    return names


def test_every_statistics_instantiation_of_a_training_step_has_a_case(monkeypatch):
    hh = _hh()
    reached = set()
    for case in FWD_CASES:
        for dt in (F32, BF):
            reached.add(fwd_rows_name(case, hh.dt_id(dt)))
    for case in ATOMIC_CASES:
        reached.add(bnref_name(case, 0))
    for case in RING_FWD_CASES:
        reached.add(bnref_name(case, 1))
    for case in SUM_CASES:
        reached.add(sum_name(case))
    for case, mode, dtype, route in _bs_params():
        reached.add(bs_name(case, hh.dt_id(dtype), 1 if route == 'ring' else 0))
    for case, dtype in _fused_params():
        reached.add(fused_name(hh.dt_id(dtype), case[3], case[4]))
    need = {}
    for det in ('0', '1'):
        monkeypatch.setenv('HRNET_DETERMINISTIC', det)
        need.update(_plan_statistics_names())
    torch.cuda.empty_cache()
    missing = {n: shape for n, shape in need.items() if n not in reached}
    print('statistics producers of the step: {}, with a case: {}, not yet covered: {}'.format(
        len(need), len(need) - len(missing), sorted(missing)))
    assert set(missing) <= NOT_YET, 'statistics-writing instantiations without a case: {}'.format(
        {n: v for n, v in missing.items() if n not in NOT_YET})
