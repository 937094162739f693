"""The 2-D backbone contraction kernels held per element (tests/contraction_refs.py): conv_body.h in its six modes and
seven tile shapes, the LDS ring, gemm_pw, wgrad in its slab and float-atomic forms, bwd_fused and bwd_pw, every one
through its C entry point and once more as the recorded op (hrnet_program_run), which must give the same bits.

Every case runs on the integer lattice, where the stored bits must EQUAL the float64 reference, and in reals, where
every element must stay inside its derived bound; `largest |error| / bound` is printed per case. Outputs sit between
NaN guards that must stay untouched, pad channels must be exactly zero, and every launch runs twice into the same
buffers (an accumulating one with its prior contents restored) with equal bits. Each case asserts the instantiation it
means through hrnet_conv_mode / hrnet_conv_tile_walk / the *_kernel_name and *_supported queries.

Not covered, and why: hrnet_conv2d_bnref, the in_sums prologue and the HrBnBwdRef form (coefficients built on the device
from invstd are not known to the bit); ring instantiations 5 and 6 and the fused-backward variants 1 and 2, which only
process-wide measurement knobs read once at start-up select, not a per-test switch.

Worst ratios measured on one MI355X are in the docstrings of the tests."""
import ctypes
import os
import re

import pytest
import torch

import contraction_refs as R

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'bf16': torch.bfloat16}
DEV = 'cuda:0'
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'hrnet-hand-pose-estimation_amd', 'csrc')


def _C():
    from hipnet import _capi as C
    return C


def _did(dtype):
    return _C().dtype_id(TD[dtype])


class _ring(object):
    """hrnet_conv_ring_enable(on) (and optionally hrnet_conv_ring_sum_enable) for a block, restored afterwards"""

    def __init__(self, on, ring_sum=None):
        self.on, self.ring_sum = on, ring_sum

    def __enter__(self):
        self.prev = _C().call('hrnet_conv_ring_enable', self.on)
        if self.ring_sum is not None:
            self.prev_sum = _C().call('hrnet_conv_ring_sum_enable', self.ring_sum)
        return self

    def __exit__(self, *exc):
        _C().call('hrnet_conv_ring_enable', 1 if self.prev != 0 else 0)
        if self.ring_sum is not None:
            _C().call('hrnet_conv_ring_sum_enable', self.prev_sum)


# ---- tensors ----------------------------------------------------------------------------------------------------
def _nhwc(t, dtype):
    """CPU NCHW float64 (values of the device dtype) -> device NHWC"""
    return None if t is None else t.permute(0, 2, 3, 1).contiguous().to(TD[dtype]).to(DEV)


def _vec(v):
    return None if v is None else v.contiguous().float().to(DEV)


def _nchw64(t):
    return t.float().cpu().double().permute(0, 3, 1, 2).contiguous()


def _pack(w, dtype, mode, cout_pad, cin_pad):
    C = _C()
    co, ci, ks, _ = w.shape
    wd = w.float().to(DEV).contiguous()
    out = torch.full((cout_pad * ks * ks * cin_pad,), float('nan'), dtype=TD[dtype], device=DEV)
    C.call('hrnet_pack_weights', _did(dtype), wd.data_ptr(), out.data_ptr(), co, ci, ks, cout_pad, cin_pad, mode, C.stream_ptr())
    return out


class _Out(object):
    """an output tensor between two NaN guards (at least one row of the tensor each), optionally holding a prior"""

    def __init__(self, shape, tdtype, prior=None):
        n = 1
        for s in shape:
            n *= s
        row = shape[-1] * (shape[-2] if len(shape) > 1 else 1)
        self.g = -(-max(row, 64) // 64) * 64
        self.n, self.prior = n, prior
        self.buf = torch.full((n + 2 * self.g,), float('nan'), dtype=tdtype, device=DEV)
        self.view = self.buf[self.g:self.g + n].view(shape)
        self.reset()

    def reset(self):
        if self.prior is None:
            self.view.fill_(float('nan'))
        else:
            self.view.copy_(self.prior.reshape(self.view.shape))

    def ptr(self):
        return self.view.data_ptr()

    def bits(self):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[:self.g]).all()) and bool(torch.isnan(self.buf[self.g + self.n:]).all()), 'guard rows touched'
        v = self.view.contiguous()
        return v.view(torch.int16 if v.element_size() == 2 else torch.int32).cpu().clone()


WORST = {}


def _check(fam, what, got, ref, bound):
    """lattice (bound None): equal; reals: |got - ref| <= bound per element. Prints and records the ratio per family."""
    assert not bool(torch.isnan(got).any()), (what, 'NaN in the output')
    if bound is None:
        bad = int((got != ref).sum())
        print('{:10s} {} lattice: {} of {} differ'.format(fam, what, bad, ref.numel()))
        assert bad == 0, (what, bad, (got != ref).nonzero()[0].tolist())
        return 0.0
    err = (got - ref).abs()
    ratio = float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())
    WORST[fam] = max(WORST.get(fam, 0.0), ratio)
    print('{:10s} {} real: largest |error| / bound = {:.4f}'.format(fam, what, ratio))
    assert ratio <= 1.0, (what, ratio)
    return ratio


def _op(kind, ints, ptrs):
    C = _C()
    op = C.HrOp()
    op.kind = kind
    for k, v in enumerate(ints):
        op.i[k] = int(v)
    for k, t in enumerate(ptrs):
        op.p[k] = t if isinstance(t, int) or t is None else C.ptr(t)
    return op


def _run_op(op):
    C = _C()
    C.call('hrnet_program_run', ctypes.byref(op), 1, C.stream_ptr())


def _walk(N, Ho, Wo, Cout, ks, stride, bs=False, s2d=False):
    out = (ctypes.c_int * 5)()
    tiles = _C().call('hrnet_conv_tile_walk', N, Ho, Wo, Cout, ks, stride, int(bs), int(s2d), out)
    return dict(tile=(out[0], out[1], out[2]), tpw=out[3], gx=out[4], tiles=tiles)


def _conv_name(did, N, Ho, Wo, Cin, Cout, ks, stride, upz, mode):
    buf = ctypes.create_string_buffer(160)
    _C().call('hrnet_conv_kernel_name', did, N, Ho, Wo, Cin, Cout, ks, stride, upz, mode, buf, 160)
    return buf.value.decode()


def _name(fn, *args):
    buf = ctypes.create_string_buffer(160)
    _C().call(fn, *(args + (buf, 160)))
    return buf.value.decode()


def _mode(bs, bias, upz, acc, stats, affine, relu):
    return _C().call('hrnet_conv_mode', int(bs), int(bias), int(upz), int(acc), int(stats), int(affine), int(relu))


def _three_runs(out, direct, op, extra=()):
    """direct call twice and the recorded op once into the same buffers: equal bits (`extra`: further _Out's)"""
    bits = []
    for run in (direct, direct, (lambda: _run_op(op)) if op is not None else None):
        if run is None:
            continue
        out.reset()
        for e in extra:
            e.reset()
        run()
        bits.append([out.bits()] + [e.bits() for e in extra])
    for b in bits[1:]:
        for x, y in zip(bits[0], b):
            assert torch.equal(x, y), 'a second run, or the recorded op, gives other bits'


# ---- 1. hrnet_conv2d forward; 4. the ring's forward; 5. gemm_pw ---------------------------------------------------------
def conv_name_of(case, dtype, ring):
    f = R.FORMS[case.form]
    Ho, Wo = R.out_hw(case.H, case.W, case.ks, case.stride)
    with _ring(ring):
        return _conv_name(_did(dtype), case.N, Ho, Wo, case.cin, case.cout, case.ks, case.stride, 0,
                          _mode(0, f['bias'], 0, f['acc'], f['stats'], f['affine'], f['relu']))


def _run_conv(fam, case, dtype, ring=0, name_prefix=None):
    C = _C()
    c, f, did = case, R.FORMS[case.form], _did(dtype)
    Ho, Wo = R.out_hw(c.H, c.W, c.ks, c.stride)
    assert _mode(0, f['bias'], 0, f['acc'], f['stats'], f['affine'], f['relu']) == f['mode'], case
    name = conv_name_of(case, dtype, ring)
    if name_prefix:
        assert name.startswith(name_prefix), (name, name_prefix)
    for lattice in (True, False):
        d = R.conv_data(case, dtype, lattice)
        xd = _nhwc(d['x'], dtype)
        wp = _pack(d['w'][:c.cout_real, :c.cin_real], dtype, 0, c.cout, c.cin)
        scd, shd, bd = _vec(d['sc']), _vec(d['sh']), _vec(d['bias'])
        st = None
        if f['stats']:
            st = torch.zeros(C.call('hrnet_conv_tiles', c.N, Ho, Wo, c.cout, c.ks, c.stride), 2, c.cout, device=DEV)
        out = _Out((c.N, Ho, Wo, c.cout), TD[dtype], _nhwc(d['prior'], dtype))
        ints = (did, c.N, c.H, c.W, c.cin, Ho, Wo, c.cout, c.ks, c.stride, 0, int(f['relu']), int(f['acc']))
        op = _op(C.OP_CONV, ints, (xd, wp, scd, shd, bd, out.ptr(), st))

        def direct():
            C.call('hrnet_conv2d', did, xd.data_ptr(), wp.data_ptr(), C.ptr(scd), C.ptr(shd), C.ptr(bd), out.ptr(), C.ptr(st),
                   c.N, c.H, c.W, c.cin, Ho, Wo, c.cout, c.ks, c.stride, 0, int(f['relu']), int(f['acc']), C.stream_ptr())
        with _ring(ring):
            _three_runs(out, direct, op)
        got = _nchw64(out.view)
        assert float(got[:, c.cout_real:].abs().sum()) == 0, 'pad channels are not zero'
        _check(fam, '{} {} {}'.format(name, tuple(case), dtype), got, d['ref'], d['bound'])


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('case', R.CONV_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_conv2d_forward_every_mode_and_tile(case, dtype):
    """hrnet_conv2d on the tile-walking body: CONV_FWD, CONV_FWDB, CONV_GENERIC, CONV_DG on tiles 0 - 4.
    Measured on one MI355X: every lattice run equal; largest |error| / bound in reals: f32 0.157, bf16 0.995
    (bf16: the store's half ulp, which reaches v |ref| just above a power of two, is nearly the whole bound; the
    f32-stored outputs of the same MFMA path - slab sums 0.038, rows 0.003 below - show the contraction's own share)."""
    Ho, Wo = R.out_hw(case.H, case.W, case.ks, case.stride)
    wk = _walk(case.N, Ho, Wo, case.cout, case.ks, case.stride)
    tile = R.CONV_TILE[case]
    if tile is not None:
        assert wk['tile'] == R.TILES[tile], (case, wk)
    if case.N >= 130:
        assert wk['tpw'] >= 2 and wk['gx'] < wk['tiles'], wk            # several tiles per workgroup
        if case.N == 513:
            assert wk['tiles'] % wk['tpw'] != 0                          # the last workgroup walks fewer
    mode_names = {2: 'conv_fwd_kernel<', 4: 'conv_fwdb_kernel<', 0: 'conv_kernel<', 3: 'conv_dg_kernel<'}
    _run_conv('conv_' + dtype, case, dtype, 0, mode_names[R.FORMS[case.form]['mode']])


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_conv2d_forward_at_the_narrowest_input(dtype):
    """Cin at the 16-byte minimum: 8 channels in bf16, 4 in f32"""
    _run_conv('conv_' + dtype, R.MIN_CIN_CASES[dtype], dtype, 0, 'conv_fwd_kernel<')


@pytest.mark.parametrize('case,rid,on', R.RING_FWD_CASES, ids=lambda v: '-'.join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_ring_forward(case, rid, on):
    """conv_ring.hip behind hrnet_conv2d, instantiations 1 - 4 (3 also on a 20 x 37 map under hrnet_conv_ring_enable(2)).
    Measured on one MI355X: every lattice run equal; largest |error| / bound 0.971."""
    with _ring(on):
        assert _C().call('hrnet_conv_ring_supported', 1, case.N, case.H, case.W, case.cin, case.cout) == rid
    _run_conv('ring', case, 'bf16', on, 'conv_ring_kernel<')


def _g_bm():
    with open(os.path.join(CSRC, 'gemm_pw.hip')) as f:
        return int(re.search(r'constexpr int G_BM = (\d+)', f.read()).group(1))


@pytest.mark.parametrize('bias', [0, 1])
@pytest.mark.parametrize('ch', R.GEMM_CHANNELS)
def test_gemm_pw(ch, bias):
    """gemm_pw.hip behind hrnet_conv2d (bf16, 1x1, Cin and Cout >= 256, no statistics): 1 pixel, a block minus 1, a block
    plus 1, three blocks and a remainder. Measured on one MI355X: lattice equal; largest |error| / bound 0.977."""
    bm = _g_bm()
    assert bm == 128          # (tests/test_contraction_refs_cpu.py checks the lattice conditions at these pixel counts)
    for m, r in R.GEMM_PIXELS:
        _run_conv('gemm_pw', R.gemm_case(ch, bias, m * bm + r), 'bf16', 1, 'gemm_pw_kernel')


# ---- 3. hrnet_conv2d_sum ----------------------------------------------------------------------------------------------
def sum_name_of(case, dtype, ring):
    with _ring(1 if ring else 0, 1 if ring else 0):
        return _conv_name(_did(dtype), case.N, case.H, case.W, case.cin, case.cout, case.ks, 1, 0, 5)


def _run_sum(fam, case, dtype, ring):
    C = _C()
    c, did = case, _did(dtype)
    name = sum_name_of(case, dtype, ring)
    assert name.startswith('conv_ring_kernel<') and name.endswith('false, true>') if ring else name.startswith('conv_fwds_kernel<'), name
    for lattice in (True, False):
        d = R.sum_data(case, dtype, lattice)
        xd, x2d = _nhwc(d['x'], dtype), _nhwc(d['x2'], dtype)
        wp = _pack(d['w'], dtype, 0, c.cout, c.cin)
        scd, shd = _vec(d['sc']), _vec(d['sh'])
        rows = 8 if ring else C.call('hrnet_conv_tiles', c.N, c.H, c.W, c.cout, c.ks, 1)
        st = torch.zeros(rows, 2, c.cout, device=DEV)
        y = _Out((c.N, c.H, c.W, c.cout), TD[dtype])
        side = _Out((c.N, c.H, c.W, c.cin), TD[dtype])
        op = _op(C.OP_CONV_SUM, (did, c.N, c.H, c.W, c.cin, c.cout, c.ks, int(ring)),
                 (xd, wp, scd, shd, None, None, None, y.ptr(), st, x2d, side.ptr()))

        def direct():
            C.call('hrnet_conv2d_sum', did, xd.data_ptr(), x2d.data_ptr(), wp.data_ptr(), scd.data_ptr(), shd.data_ptr(), None,
                   None, None, 0.0, 0.0, side.ptr(), y.ptr(), st.data_ptr(), int(ring), c.N, c.H, c.W, c.cin, c.cout, c.ks,
                   C.stream_ptr())
        with _ring(1 if ring else 0, 1 if ring else 0):
            _three_runs(y, direct, op, extra=(side,))
        what = '{} {} {}'.format(name, tuple(case), dtype)
        _check(fam, what + ' y', _nchw64(y.view), d['ref'], d['bound'])
        # side = a: known to the bit on the lattice and in bf16; in f32 reals two roundings of the prologue and the add
        _check(fam, what + ' side', _nchw64(side.view), d['a'], d['e_side'])


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('case', R.SUM_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_conv2d_sum(case, dtype):
    """CONV_FWDS on the tile-walking body: y and `side`, the BatchNorm term as scale / shift.
    Measured on one MI355X: lattice equal; largest |error| / bound y 0.140 (f32) and 0.995 (bf16), `side` 0.633 (f32; equal
    bits in bf16); on the ring y 0.965."""
    if case.N >= 130:
        wk = _walk(case.N, case.H, case.W, case.cout, case.ks, 1)
        assert wk['tpw'] >= 2, wk
    _run_sum('conv_sum', case, dtype, False)


@pytest.mark.parametrize('case,rid', R.RING_SUM_CASES, ids=lambda v: '-'.join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_conv2d_sum_on_the_ring(case, rid):
    """the residual-sum form of ring instantiations 1 and 2 under hrnet_conv_ring_sum_enable(1), restored afterwards"""
    with _ring(1, 1):
        assert _C().call('hrnet_conv_ring_supported', 1, case.N, case.H, case.W, case.cin, case.cout) == rid
    _run_sum('ring', case, 'bf16', True)


# ---- 2. input gradients; 4. the ring's input gradient ---------------------------------------------------------------------
def _dgrad_flags(case):
    """(bs, upz, in_relu, store_masked)"""
    return case.form.startswith('bs_'), int(case.stride == 2), int(case.form == 'zs'), int(case.form.endswith('+m'))


def dgrad_name_of(case, dtype, ring):
    bs, upz, relu, _ = _dgrad_flags(case)
    with _ring(ring):
        return _conv_name(_did(dtype), case.N, case.H, case.W, case.cout, case.cin, case.ks, case.stride, upz,
                          _mode(bs, 0, upz, case.acc, bs, 0, relu))


def _run_dgrad(fam, case, dtype, ring=0, name_prefix=None):
    C = _C()
    c, did = case, _did(dtype)
    bs, upz, relu, store_masked = _dgrad_flags(case)
    Ho, Wo = R.out_hw(c.H, c.W, c.ks, c.stride)
    name = dgrad_name_of(case, dtype, ring)
    assert name.startswith(name_prefix), (name, name_prefix)
    for lattice in (True, False):
        d = R.dgrad_data(case, dtype, lattice)
        dyd = _nhwc(d['dy'], dtype)
        wT = _pack(d['w'], dtype, 1, c.cout, c.cin)
        out = _Out((c.N, c.H, c.W, c.cin), TD[dtype], _nhwc(d['prior'], dtype))
        with _ring(ring):
            if bs:
                nrows = C.call('hrnet_conv_rows_bwdstats', did, c.N, c.H, c.W, c.cout, c.cin, c.ks, c.stride)
                rows = torch.zeros(nrows, 2, c.cin, device=DEV)
                byd, bmd = _nhwc(d['bs_y'], dtype), _nhwc(d.get('bs_mask'), dtype)
                bscd, bshd = _vec(d.get('bs_sc')), _vec(d.get('bs_sh'))
                ints = (did, c.N, Ho, Wo, c.cout, c.H, c.W, c.cin, c.ks, c.stride, upz, 0, c.acc, 0, store_masked)
                op = _op(C.OP_CONV, ints, (dyd, wT, None, None, None, out.ptr(), rows, byd, bmd, bscd, bshd))

                def direct():
                    C.call('hrnet_conv2d_bwdstats', did, dyd.data_ptr(), wT.data_ptr(), out.ptr(), rows.data_ptr(), byd.data_ptr(),
                           C.ptr(bmd), C.ptr(bscd), C.ptr(bshd), c.N, Ho, Wo, c.cout, c.H, c.W, c.cin, c.ks, c.stride, upz, c.acc,
                           C.stream_ptr())
                # (the masked store is a slot of the recorded op only)
                _three_runs(out, (lambda: _run_op(op)) if store_masked else direct, op)
            else:
                ints = (did, c.N, Ho, Wo, c.cout, c.H, c.W, c.cin, c.ks, c.stride, upz, relu, c.acc)
                op = _op(C.OP_CONV, ints, (dyd, wT, None, None, None, out.ptr(), None))

                def direct():
                    C.call('hrnet_conv2d', did, dyd.data_ptr(), wT.data_ptr(), None, None, None, out.ptr(), None, c.N, Ho, Wo,
                           c.cout, c.H, c.W, c.cin, c.ks, c.stride, upz, relu, c.acc, C.stream_ptr())
                _three_runs(out, direct, op)
        _check(fam, '{} {} {}'.format(name, tuple(case), dtype), _nchw64(out.view), d['ref'], d['bound'])


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('case', R.DGRAD_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_input_gradient(case, dtype):
    """hrnet_conv2d with mode-1 weights (CONV_DG; stride 2: the four-parity S2D tiles 6 and 7, and the zero-stuffed form
    through CONV_GENERIC) and hrnet_conv2d_bwdstats (CONV_BS: the dx it stores, masked or not), accumulate on and off.
    Measured on one MI355X: lattice equal; largest |error| / bound f32 0.145, bf16 0.995."""
    bs, upz, relu, _ = _dgrad_flags(case)
    s2d = upz and not relu
    wk = _walk(case.N, case.H, case.W, case.cin, case.ks, case.stride, bs, s2d)
    if s2d:
        assert wk['tile'] == R.TILES[7 if case.cin >= 64 else 6], wk
    if case.N >= 130:
        assert wk['tpw'] >= 2, wk
    prefix = 'conv_bs_kernel<' if bs else 'conv_kernel<' if relu else 'conv_dg_kernel<'
    _run_dgrad('dgrad_' + dtype, case, dtype, 0, prefix)
    if s2d:
        assert ', 3, 4, ' in dgrad_name_of(case, dtype, 0)        # the S2D instantiation (template stride 4)


@pytest.mark.parametrize('case,rid,on', R.RING_DGRAD_CASES, ids=lambda v: '-'.join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_ring_input_gradient(case, rid, on):
    """the ring's input gradient: accumulating, plain (the forward instantiation) and with backward statistics"""
    with _ring(on):
        assert _C().call('hrnet_conv_ring_supported', 1, case.N, case.H, case.W, case.cout, case.cin) == rid
        if case.form.startswith('bs_'):
            assert _C().call('hrnet_conv_route', 1, case.N, case.H, case.W, case.cout, case.cin, 3, 1) == 2
    _run_dgrad('ring', case, 'bf16', on, 'conv_ring_kernel<')


# ---- 6. weight gradients ----------------------------------------------------------------------------------------------------
def wgrad_name_of(case, dtype):
    Ho, Wo = R.out_hw(case.H, case.W, case.ks, case.stride)
    return _name('hrnet_wgrad_kernel_name', _did(dtype), Ho, Wo, case.cout, case.cin, case.ks, case.stride)


def _oihw(slab_sum, ks):
    """[Cout][taps][Cin] -> [Cout][Cin][ks][ks]"""
    co, taps, ci = slab_sum.shape
    return slab_sum.permute(0, 2, 1).reshape(co, ci, ks, ks)


def _run_wgrad(case, dtype, kflat=False):
    C = _C()
    c, did = case, _did(dtype)
    Ho, Wo = R.out_hw(c.H, c.W, c.ks, c.stride)
    name = wgrad_name_of(case, dtype)
    m = re.match(r'wgrad_kernel<[^,]+, (\d+), (\d+), (\d+), (\d+), (\d+),', name)
    want = R.WG_TILES[10 if (c.wg == 11 and dtype == 'f32') else c.wg]
    assert (int(m.group(1)), int(m.group(2))) == (c.ks, c.stride) and tuple(int(m.group(k)) for k in (3, 4, 5)) == want, name
    ns = C.call('hrnet_wgrad_splits', did, c.N, Ho, Wo, c.cout, c.cin, c.ks, c.stride)
    if case == R.WGRAD_UNEVEN:
        tiles = C.call('hrnet_wgrad_tiles', did, c.N, Ho, Wo, c.cout, c.cin, c.ks, c.stride)
        assert ns > 1 and tiles % ns != 0, (tiles, ns)            # an uneven tile count per split
    fam = 'wgrad_' + dtype
    gks = 3 if kflat else c.ks
    gci = 3 if kflat else c.cin_real
    for lattice in (True, False):
        d = R.wgrad_data(case, dtype, lattice)
        xd, dyd = _nhwc(d['x'], dtype), _nhwc(d['dy'], dtype)
        scd, shd = _vec(d['sc']), _vec(d['sh'])
        slabs = _Out((ns, c.cout, c.ks * c.ks, c.cin), torch.float32)
        ints = (did, c.N, c.H, c.W, c.cin, Ho, Wo, c.cout, c.ks, c.stride, int(c.affine), ns)
        op = _op(C.OP_WGRAD, ints, (xd, dyd, scd, shd, slabs.ptr()))

        def direct():
            C.call('hrnet_conv2d_wgrad', did, xd.data_ptr(), dyd.data_ptr(), C.ptr(scd), C.ptr(shd), slabs.ptr(), c.N, c.H, c.W,
                   c.cin, Ho, Wo, c.cout, c.ks, c.stride, int(c.affine), ns, C.stream_ptr())
        _three_runs(slabs, direct, op)
        what = '{} {} {} ns={}'.format(name, tuple(case), dtype, ns)
        total = _oihw(slabs.view.cpu().double().sum(0), c.ks)
        assert float(total[c.cout_real:].abs().sum()) == 0 and float(total[:, c.cin_real:].abs().sum()) == 0, 'pad channels'
        _check(fam, what + ' slab sum', total[:c.cout_real, :c.cin_real], d['ref'], d['bound'])
        # hrnet_wgrad_reduce adding to a gradient that already holds values
        ref, prior = d['ref'], d['prior']
        if kflat:
            ref, prior = R.kflat_to_oihw(ref.reshape(c.cout_real, -1), 3, 3), prior.reshape(c.cout_real, -1)[:, :27].reshape(c.cout_real, 3, 3, 3)
        bound = None if lattice else d['bound'].reshape(ref.shape) if not kflat else R.kflat_to_oihw(d['bound'].reshape(c.cout_real, -1), 3, 3)
        if bound is not None:
            bound = bound + (d['P'] + 3) * R.U * prior.abs()
        grad = _Out((c.cout_real, gci, gks, gks), torch.float32, prior.float().to(DEV))

        def reduce_():
            C.call('hrnet_wgrad_reduce', slabs.ptr(), grad.ptr(), ns, c.cout, c.cin, gks, c.cout_real, gci, int(kflat), 1,
                   C.stream_ptr())
        _three_runs(grad, reduce_, None)
        reduced = grad.bits()
        _check(fam, what + ' reduce', grad.view.cpu().double(), ref + prior, bound)
        if kflat:
            continue
        # the float-atomic form adds into the gradient itself: on the lattice the same bits as slabs + reduce
        ints = ints + (1, c.cout_real, c.cin_real)
        aop = _op(C.OP_WGRAD, ints, (xd, dyd, scd, shd, grad.ptr()))
        for _ in range(2):
            grad.reset()
            _run_op(aop)
            if lattice:
                assert torch.equal(grad.bits(), reduced), 'the atomic gradient differs from slabs + reduce on the lattice'
            _check(fam, what + ' atomic', grad.view.cpu().double(), ref + prior, bound)


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('case', R.WGRAD_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_weight_gradient_slabs_reduce_and_atomics(case, dtype):
    """hrnet_conv2d_wgrad + hrnet_wgrad_reduce (accumulating) and the atomic HR_OP_WGRAD, every choose_wg id.
    Measured on one MI355X: lattice equal, the atomic form bit for bit the slab form; largest |error| / bound f32
    0.270 (slab sums 0.255), bf16 0.248 (slab sums 0.038; the rest is the accumulating reduce's one rounding of the prior)."""
    _run_wgrad(case, dtype)


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_weight_gradient_of_the_flattened_stem(dtype):
    """kflat: the slab's K index is (tap, ci) of the im2col'ed stem; the reduce scatters it to [64][3][3][3]"""
    _run_wgrad(R.WGRAD_STEM, dtype, kflat=True)


# ---- 7. and 8. the fused backward launches --------------------------------------------------------------------------------
def fused_name_of(case, dtype):
    fn = 'hrnet_bwd_pw_kernel_name' if case.ks == 1 else 'hrnet_bwd_fused_kernel_name'
    return _name(fn, _did(dtype), case.cin, case.cout)


def _run_fused(case, dtype):
    C = _C()
    c, did = case, _did(dtype)
    pw = c.ks == 1
    P = c.N * c.H * c.W
    if pw:
        assert C.call('hrnet_bwd_pw_supported', did, c.cin, c.cout) == 1
        ns = C.call('hrnet_bwd_pw_splits', did, P, c.cin, c.cout)
        tiles = -(-P // 64)
    else:
        assert C.call('hrnet_bwd_fused_supported', did, c.cin, c.cout) == 1
        ns = C.call('hrnet_bwd_fused_splits', did, c.N, c.H, c.W, c.cin, c.cout)
    name = fused_name_of(case, dtype)
    if pw:
        assert name == 'bwd_pw_kernel<{}, {}>'.format(c.cout, c.cin), name
    else:
        m = re.match(r'bwd_fused_kernel<([^,]+), (\d+), (\d+),', name)
        assert int(m.group(2)) == (32 if c.cout <= 32 else 64 if c.cout <= 64 else 128), name
        tiles = c.N * -(-c.H // int(m.group(3))) * -(-c.W // 16)
    if c.N >= 5 and c.H >= 16:
        assert tiles > ns, (tiles, ns)                    # several tiles per walk
    fam = ('bwd_pw' if pw else 'bwd_fused_' + dtype)
    kind = C.OP_BWD_PW if pw else C.OP_BWD_FUSED
    for lattice in (True, False):
        d = R.fused_data(case, dtype, lattice)
        dzd, yd, xd = _nhwc(d['dz'], dtype), _nhwc(d['y'], dtype), _nhwc(d['x'], dtype)
        addd, bsd = _nhwc(d['addend'], dtype), _nhwc(d['bsy'], dtype)
        coef = None if d['coef'] is None else _vec(d['coef'].reshape(-1))
        scd, shd = _vec(d['sc']), _vec(d['sh'])
        wT = _pack(d['w'], dtype, 1, c.cout, c.cin)
        dx = _Out((c.N, c.H, c.W, c.cin), TD[dtype])
        rows = _Out((ns, 2, c.cin), torch.float32) if c.rows else None
        slabs = _Out((ns, c.cout, c.ks * c.ks, c.cin), torch.float32)
        extra = (slabs,) + ((rows,) if rows else ())
        rp = rows.ptr() if rows else None

        def ptrs(dxp, addp, dst):
            return (dzd, yd if coef is not None else None, coef, xd, scd, shd, wT, dxp, addp, rp, bsd, dst)

        def ints(atomic):
            return (did, c.N, c.H, c.W, c.cin, c.cout, int(c.affine), int(c.mask), atomic, c.cout, c.cin)

        def direct():
            args = (did, dzd.data_ptr(), C.ptr(yd) if coef is not None else None, C.ptr(coef), xd.data_ptr(), C.ptr(scd), C.ptr(shd),
                    int(c.affine), wT.data_ptr(), dx.ptr(), C.ptr(addd), int(c.mask), rp, C.ptr(bsd), slabs.ptr())
            if pw:
                C.call('hrnet_conv1x1_bwd_fused', *(args + (P, c.cin, c.cout, C.stream_ptr())))
            else:
                C.call('hrnet_conv3x3_bwd_fused', *(args + (c.N, c.H, c.W, c.cin, c.cout, C.stream_ptr())))
        _three_runs(dx, direct, _op(kind, ints(0), ptrs(dx.ptr(), addd, slabs.ptr())), extra=extra)
        what = '{} {} {} ns={}'.format(name, tuple(case), dtype, ns)
        dx_bits = dx.bits()
        _check(fam, what + ' dx', _nchw64(dx.view), d['dx'], d.get('b_dx'))
        total = _oihw(slabs.view.cpu().double().sum(0), c.ks)
        _check(fam, what + ' slab sum', total, d['gw'], d.get('b_gw'))
        bound = None if lattice else d['b_gw'] + (P + 3) * R.U * d['prior'].abs()
        grad = _Out((c.cout, c.cin, c.ks, c.ks), torch.float32, d['prior'].float().to(DEV))
        C.call('hrnet_wgrad_reduce', slabs.ptr(), grad.ptr(), ns, c.cout, c.cin, c.ks, c.cout, c.cin, 0, 1, C.stream_ptr())
        reduced = grad.bits()
        _check(fam, what + ' reduce', grad.view.cpu().double(), d['gw'] + d['prior'], bound)
        if rows:
            rows_bits = rows.bits()
            # (bwd_pw_kernel<64, 256> sums the tile as stored, the others the f32 values in front of the store)
            _check(fam, what + ' rows', rows.view.cpu().double().sum(0), d['rows'],
                   d.get('b_rows_stored' if pw and c.cin == 256 else 'b_rows'))
        # the atomic weight-gradient form: dx and rows keep their bits, the gradient equals slabs + reduce on the lattice
        dx.reset()
        grad.reset()
        if rows:
            rows.reset()
        _run_op(_op(kind, ints(1), ptrs(dx.ptr(), addd, grad.ptr())))
        assert torch.equal(dx.bits(), dx_bits) and (rows is None or torch.equal(rows.bits(), rows_bits))
        if lattice:
            assert torch.equal(grad.bits(), reduced), 'the atomic gradient differs from slabs + reduce on the lattice'
        _check(fam, what + ' atomic', grad.view.cpu().double(), d['gw'] + d['prior'], bound)
        # in place: dx is the addend's own buffer
        if c.addend:
            inplace = _Out((c.N, c.H, c.W, c.cin), TD[dtype], addd)
            _run_op(_op(kind, ints(0), ptrs(inplace.ptr(), inplace.ptr(), slabs.ptr())))
            assert torch.equal(inplace.bits(), dx_bits), 'the in-place form gives other bits'


def _fused_params():
    return [(c, dt) for c in R.FUSED_CASES for dt in R.DTYPES if dt == 'bf16' or c.cout <= 32]


@pytest.mark.parametrize('case,dtype', _fused_params(), ids=lambda v: '-'.join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_conv3x3_bwd_fused(case, dtype):
    """hrnet_conv3x3_bwd_fused: dx, slabs then reduce, the atomic gradient, the rows, the in-place form; f32 with Cout <= 32,
    bf16 on the 32, 64 and 128 output-channel instantiations. Measured on one MI355X: lattice equal; largest |error| /
    bound f32: dx 0.019, gradient 0.265, rows 0.004; bf16: dx 0.981, gradient 0.247, rows 0.003."""
    _run_fused(case, dtype)


@pytest.mark.parametrize('case', R.PW_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_conv1x1_bwd_fused(case):
    """hrnet_conv1x1_bwd_fused on its three shapes (64 -> 256, 256 -> 64, 64 -> 64).
    Measured on one MI355X: lattice equal; largest |error| / bound dx 0.995, gradient 0.248, rows 0.255 - the rows
    of bwd_pw_kernel<64, 256> against the bound of the STORED tile, which is what that instantiation sums (held to the
    bound of the f32 values, as the other two are, it reads 10.3: contraction_refs.fused_data)."""
    _run_fused(case, 'bf16')


def test_worst_ratios_report():
    """prints the worst |error| / bound per kernel family over the cases that ran before it in this process"""
    for fam in sorted(WORST):
        print('worst ratio {:16s} {:.4f}'.format(fam, WORST[fam]))
    assert all(v <= 1.0 for v in WORST.values())


# ---- coverage ---------------------------------------------------------------------------------------------------------------
# instantiations of a training step without a case here: none
NOT_YET = set()


def _plan_contraction_names():
    """kernel instantiation of every HR_OP_CONV, HR_OP_CONV_SUM, HR_OP_WGRAD, HR_OP_BWD_FUSED and HR_OP_BWD_PW a w32 bf16
    B=64 training plan records, by the queries bench.py uses"""
    import bench
    C = _C()
    model, _, _ = bench.build_model('bf16', 'RHD_HRNet_w32_max_hmloss_v1.yaml')
    model = model.cuda().train()
    plan = model.hip().plan(64, 256, 256, True, True)
    names = {}
    for prog in (plan.fwd, plan.bwd):
        for op in prog.ops:
            k, i, p = int(op.kind), op.i, op.p
            if k == C.OP_CONV:
                bs, raw = bool(p[7]), not (p[2] or p[11] or i[11])
                mode = _mode(bs, bool(p[4]), i[10], i[12], bool(p[6]), bool(p[2]) or bool(p[11]), i[11])
                # (conv.hip ring_serves: what the switch being on can send to the ring)
                if i[8] != 3 or i[9] != 1 or i[10] or p[4] or i[17] == 1:
                    on = 0
                elif bs or (raw and i[12] and not p[6]):
                    on = 1
                else:
                    on = 0 if (i[12] or (p[6] and not i[13])) else 1
                with _ring(on):
                    n = _conv_name(i[0], i[1], i[5], i[6], i[4], i[7], i[8], i[9], i[10], mode)
                names.setdefault(n, tuple(i[:14]))
            elif k == C.OP_CONV_SUM:
                with _ring(1):
                    names.setdefault(_conv_name(i[0], i[1], i[2], i[3], i[4], i[5], i[6], 1, 0, 5), tuple(i[:8]))
            elif k == C.OP_WGRAD:
                names.setdefault(_name('hrnet_wgrad_kernel_name', i[0], i[5], i[6], i[7], i[4], i[8], i[9]), tuple(i[:13]))
            elif k in (C.OP_BWD_FUSED, C.OP_BWD_PW):
                fn = 'hrnet_bwd_fused_kernel_name' if k == C.OP_BWD_FUSED else 'hrnet_bwd_pw_kernel_name'
                names.setdefault(_name(fn, i[0], i[4], i[5]), tuple(i[:9]))
    del plan, model
    return names


def _reached():
    out = set()
    for dt in R.DTYPES:
        out.update(conv_name_of(c, dt, 0) for c in R.CONV_CASES)
        out.add(conv_name_of(R.MIN_CIN_CASES[dt], dt, 0))
        out.update(sum_name_of(c, dt, False) for c in R.SUM_CASES)
        out.update(dgrad_name_of(c, dt, 0) for c in R.DGRAD_CASES)
        out.update(wgrad_name_of(c, dt) for c in R.WGRAD_CASES + (R.WGRAD_STEM,))
    out.update(conv_name_of(c, 'bf16', on) for c, _, on in R.RING_FWD_CASES)
    out.update(sum_name_of(c, 'bf16', True) for c, _ in R.RING_SUM_CASES)
    out.update(dgrad_name_of(c, 'bf16', on) for c, _, on in R.RING_DGRAD_CASES)
    out.update(conv_name_of(R.gemm_case(ch, b, 129), 'bf16', 1) for ch in R.GEMM_CHANNELS for b in (0, 1))
    out.update(fused_name_of(c, dt) for c, dt in _fused_params())
    out.update(fused_name_of(c, 'bf16') for c in R.PW_CASES)
    return out


def test_every_contraction_instantiation_of_a_training_step_has_a_case(monkeypatch):
    """Found in the w32 bf16 B=64 plan with HRNET_DETERMINISTIC 0 and 1 on one MI355X: 49 instantiations (30
    of the tile-walking body - conv_fwd 9, conv_dg 8, conv_fwds 7, conv_bs 5, conv_fwdb 1, no CONV_GENERIC launch - 6 of
    the ring, gemm_pw, 7 of wgrad, 2 of bwd_fused, 3 of bwd_pw), every one with a case"""
    reached = _reached()
    need = {}
    for det in ('0', '1'):
        monkeypatch.setenv('HRNET_DETERMINISTIC', det)
        need.update(_plan_contraction_names())
    torch.cuda.empty_cache()
    missing = {n: shape for n, shape in need.items() if n not in reached}
    for n in sorted(need):
        print('step instantiation {} {}'.format('    ' if n in reached else 'MISS', n), need[n])
    print('contraction instantiations of the step: {}, with a case: {}, without: {}'.format(
        len(need), len(need) - len(missing), sorted(missing)))
    assert set(missing) <= NOT_YET, 'instantiations without a case: {}'.format({n: v for n, v in missing.items() if n not in NOT_YET})
