"""GPU parity of the fused backward kernels at the shapes where their prologue can go wrong.

hrnet_conv3x3_bwd_fused and hrnet_conv1x1_bwd_fused request the first tile, the weights and the inputs of the
BatchNorm-backward coefficients together and wait once; the row sums of the coefficients are fetched in batches of
HR_BNBWD_UB = 8 rows per thread. What that can break, and what is held here:

  row tables    nrows in {1, NRG - 1, NRG + 1, 256} for the row-group count NRG = threads / padded channels of every
                instantiation (3x3: 16, 8 and 4; 1x1: 4 and 1), with and without `accumulate`, a ragged channel
                count (Cout 16 and 48: the padded channels' coefficients must be zero) and more than one batch per
                thread. (The 1x1 launcher takes nrows * Cout <= 8192: its largest table is 128 / 32 rows, not 256.)
  tiles         one tile under a grid of 8 x ncb workgroups (the surplus ones pass the top of the kernel and leave),
                one partial tile, a walk of exactly two tiles (the prologue's loads meet the in-loop prefetch)
  forms         `coef` given, from rows, none - each with and without the input affine; both bf16 instantiations of
                the benchmark, the 128-channel one and the fp32 one
  1x1           1, 63, 65 and 64 * nsplit + 1 pixels for the three served shapes

Every case is launched twice into fresh buffers: dx, statistics rows, slabs (and dgamma / dbeta) must be bit-identical.
References: torch fp32 autograd on the CPU (fp32 2e-4, bf16 3e-2, as tests/test_bwd_fused_gpu.py and
tests/test_bwd_pw_gpu.py), hrnet_bn_bwd_finalize on the same rows for the coefficients, and the launch with those
finalized coefficients for the from-rows form (dx / dW 1e-5 fp32, 2e-3 bf16; dgamma / dbeta rtol 2e-6, atol 1e-5)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_bwd_fused_gpu import TOL, _h, _q

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
TOL_ROWS_FORM = {F32: 1e-5, BF16: 2e-3}


def _launch(ks, dt, t, coef, ref, affine, ns, N, H, W, Cin, Cout, dtype):
    """one launch into fresh NaN-filled outputs"""
    from hipnet import _capi as C
    d = t['dz'].device
    slabs = torch.full((ns, Cout, ks * ks, Cin), float('nan'), device=d)
    rows = torch.full((ns, 2, Cin), float('nan'), device=d)
    dx = torch.full((N, H, W, Cin), float('nan'), dtype=dtype, device=d)
    rp = ctypes.addressof(ref) if ref is not None else None
    cp = coef.data_ptr() if coef is not None else None
    y = t['y'].data_ptr() if (coef is not None or ref is not None) else None
    sc, sh = (t['sc'].data_ptr(), t['sh'].data_ptr()) if affine else (None, None)
    if ks == 3:
        C.call('hrnet_conv3x3_bwd_fused_bnref', dt, t['dz'].data_ptr(), y, cp, rp, t['x'].data_ptr(), sc, sh,
               1 if affine else 0, t['wT'].data_ptr(), dx.data_ptr(), t['add'].data_ptr(), 1, rows.data_ptr(),
               t['bsy'].data_ptr(), slabs.data_ptr(), N, H, W, Cin, Cout, C.stream_ptr())
    else:
        C.call('hrnet_conv1x1_bwd_fused_bnref', dt, t['dz'].data_ptr(), y, cp, rp, t['x'].data_ptr(), sc, sh,
               1 if affine else 0, t['wT'].data_ptr(), dx.data_ptr(), t['add'].data_ptr(), 1, rows.data_ptr(),
               t['bsy'].data_ptr(), slabs.data_ptr(), N * H * W, Cin, Cout, C.stream_ptr())
    torch.cuda.synchronize()
    return dx, rows, slabs


def _same(a, b):
    assert not torch.isnan(a.float()).any()
    assert torch.equal(a, b)


def _case(ks, dtype, N, H, W, Cin, Cout, form, affine, nrows=5, accumulate=1, tiles_per_walk=None):
    hh = _h()
    from hipnet import _capi as C
    dt = hh.dt_id(dtype)
    d = hh.DEV
    P = N * H * W
    if ks == 3:
        assert C.call('hrnet_bwd_fused_supported', dt, Cin, Cout) == 1
        ns = C.call('hrnet_bwd_fused_splits', dt, N, H, W, Cin, Cout)
        th = 8 if Cout > 64 else 16
        tiles = N * ((H + th - 1) // th) * ((W + 15) // 16)
    else:
        assert C.call('hrnet_bwd_pw_supported', dt, Cin, Cout) == 1
        ns = C.call('hrnet_bwd_pw_splits', dt, P, Cin, Cout)
        tiles = (P + 63) // 64
    if tiles_per_walk is not None:
        assert tiles == tiles_per_walk * ns
    g = torch.Generator().manual_seed(17 + Cin + 3 * Cout + N + nrows)
    w = _q(torch.randn(Cout, Cin, ks, ks, generator=g) / np.sqrt(Cin * ks * ks), dtype)
    x = _q(torch.randn(N, Cin, H, W, generator=g), dtype)
    dz = _q(torch.randn(N, Cout, H, W, generator=g), dtype)
    dz = dz * (torch.rand(dz.shape, generator=g) < 0.6)
    y = _q(torch.randn(N, Cout, H, W, generator=g), dtype)
    addend = _q(torch.randn(N, Cin, H, W, generator=g), dtype)
    bsy = _q(torch.randn(N, Cin, H, W, generator=g), dtype)
    sc, sh = torch.rand(Cin, generator=g) + 0.5, torch.rand(Cin, generator=g) - 0.5
    t = {'wT': hh.pack_weights(w, dtype, mode=1)[0], 'sc': sc.to(d), 'sh': sh.to(d)}
    t['dz'], t['y'], t['x'], t['add'], t['bsy'] = (hh.nhwc(v, dtype) for v in (dz, y, x, addend, bsy))
    coef, ref, keep = None, None, None
    if form == 'coef':
        coef = torch.cat([torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2,
                          torch.randn(Cout, generator=g) * 0.1]).to(d)
    elif form == 'rows':
        # rows of the size the statistics epilogues leave: sums over `count` elements of O(1) values
        rows_in = (torch.randn(nrows, 2, Cout, generator=g) * np.sqrt(P / nrows)).to(d)
        gamma, mean = (torch.rand(Cout, generator=g) + 0.5).to(d), torch.randn(Cout, generator=g).to(d)
        invstd = (torch.rand(Cout, generator=g) + 0.5).to(d)
        keep = (rows_in, gamma, mean, invstd)
        coef = torch.zeros(3 * Cout, device=d)                      # the finalize launch on the same rows
        dg_f, db_f = torch.full((Cout,), 0.25, device=d), torch.full((Cout,), -0.5, device=d)
        C.call('hrnet_bn_bwd_finalize', rows_in.data_ptr(), nrows, Cout, float(P), gamma.data_ptr(), mean.data_ptr(),
               invstd.data_ptr(), dg_f.data_ptr(), db_f.data_ptr(), coef.data_ptr(), accumulate, C.stream_ptr())
    # ---- reference: torch fp32 autograd on the CPU ----
    a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if affine else x
    a = _q(a, dtype).requires_grad_(True)
    gy = dz
    if coef is not None:
        cA, cB, cC = coef.cpu().view(3, Cout)
        gy = cA.view(1, -1, 1, 1) * dz + cB.view(1, -1, 1, 1) * y + cC.view(1, -1, 1, 1)
    gy = _q(gy, dtype)
    wr = w.clone().requires_grad_(True)
    F.conv2d(a, wr, None, padding=ks // 2).backward(gy)
    v = (a.grad + addend) * (a.detach() > 0)
    want_rows = torch.stack([v.double().sum((0, 2, 3)), (v.double() * bsy.double()).sum((0, 2, 3))])
    # ---- device: the form under test, twice ----
    outs = []
    for _ in range(2):
        dcoef = coef if form == 'coef' else None
        if form == 'rows':
            dg, db = torch.full((Cout,), 0.25, device=d), torch.full((Cout,), -0.5, device=d)
            ref = C.HrBnBwdRef()
            ref.rows, ref.gamma, ref.save_mean, ref.save_invstd = (k.data_ptr() for k in keep)
            ref.dgamma, ref.dbeta, ref.count, ref.nrows, ref.accumulate = dg.data_ptr(), db.data_ptr(), float(P), nrows, accumulate
            outs.append(_launch(ks, dt, t, None, ref, affine, ns, N, H, W, Cin, Cout, dtype) + (dg, db))
        else:
            outs.append(_launch(ks, dt, t, dcoef, None, affine, ns, N, H, W, Cin, Cout, dtype))
    for p, q in zip(*outs):
        _same(p, q)
    dx, rows, slabs = outs[0][:3]
    gw = torch.zeros(Cout, Cin, ks, ks, device=d)
    C.call('hrnet_wgrad_reduce', slabs.data_ptr(), gw.data_ptr(), ns, Cout, Cin, ks, Cout, Cin, 0, 0, C.stream_ptr())
    got = hh.from_nhwc(dx)
    tol = TOL[dtype]
    tol_dx = tol if dtype == F32 else tol + 2.0 ** -8 * float(addend.abs().max() / v.abs().max())
    print('dx', hh.rel_err(got, v), 'dW', hh.rel_err(gw.cpu(), wr.grad))
    assert hh.rel_err(got, v) <= tol_dx
    assert hh.rel_err(gw.cpu(), wr.grad) <= tol
    r = rows.double().sum(0).cpu()
    assert float((r[0] - want_rows[0]).abs().max()) <= 2 * tol * v.double().abs().sum((0, 2, 3)).max().item()
    assert float((r[1] - want_rows[1]).abs().max()) <= 2 * tol * (v.double() * bsy.double()).abs().sum((0, 2, 3)).max().item()
    if form == 'rows':
        # against the finalize-launch form (same f64 formula, another order of the row sum)
        dx_c, _, slabs_c = _launch(ks, dt, t, coef, None, affine, ns, N, H, W, Cin, Cout, dtype)
        dg, db = outs[0][3:]
        print('dgamma', float((dg - dg_f).abs().max()), 'dbeta', float((db - db_f).abs().max()))
        np.testing.assert_allclose(dg.cpu().numpy(), dg_f.cpu().numpy(), rtol=2e-6, atol=1e-5)
        np.testing.assert_allclose(db.cpu().numpy(), db_f.cpu().numpy(), rtol=2e-6, atol=1e-5)
        assert hh.rel_err(dx.float().cpu(), dx_c.float().cpu()) <= TOL_ROWS_FORM[dtype]
        assert hh.rel_err(slabs.sum(0).cpu(), slabs_c.sum(0).cpu()) <= TOL_ROWS_FORM[dtype]


# dtype, Cin, Cout, NRG of the instantiation that serves them (512 threads / padded output channels)
ROW_LAYERS_3X3 = [(BF16, 32, 32, 16), (F32, 32, 32, 16), (BF16, 64, 64, 8), (BF16, 32, 16, 16), (BF16, 48, 48, 8),
                  (BF16, 128, 128, 4)]


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('which', ['one', 'nrg-1', 'nrg+1', '256'])
@pytest.mark.parametrize('layer', ROW_LAYERS_3X3, ids=lambda l: '{}-{}-{}'.format(str(l[0])[6:], l[1], l[2]))
def test_conv3x3_row_tables(layer, which, accumulate):
    dtype, Cin, Cout, nrg = layer
    nrows = {'one': 1, 'nrg-1': nrg - 1, 'nrg+1': nrg + 1, '256': 256 if 256 * Cout <= 16384 else 16384 // Cout}[which]
    _case(3, dtype, 1, 16, 16, Cin, Cout, 'rows', False, nrows=nrows, accumulate=accumulate)


# Cin, Cout, NRG (256 threads / output channels)
ROW_LAYERS_1X1 = [(64, 64, 4), (256, 64, 4), (64, 256, 1)]


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('which', ['one', 'nrg-1', 'nrg+1', 'max'])
@pytest.mark.parametrize('layer', ROW_LAYERS_1X1, ids=lambda l: '{}-{}'.format(l[0], l[1]))
def test_conv1x1_row_tables(layer, which, accumulate):
    Cin, Cout, nrg = layer
    nrows = {'one': 1, 'nrg-1': max(nrg - 1, 1), 'nrg+1': nrg + 1, 'max': 8192 // Cout}[which]
    if which == 'nrg-1' and nrg == 1:
        nrows = 9           # (no table of 0 rows: one row past the first batch of eight instead)
    _case(1, BF16, 1, 9, 7, Cin, Cout, 'rows', False, nrows=nrows, accumulate=accumulate)


INST_3X3 = [(BF16, 32, 32), (BF16, 64, 64), (BF16, 128, 128), (F32, 32, 32)]
_inst_id = lambda l: '{}-{}'.format(str(l[0])[6:], l[2])


@pytest.mark.parametrize('affine', [False, True])
@pytest.mark.parametrize('form', ['coef', 'rows', 'none'])
@pytest.mark.parametrize('inst', INST_3X3, ids=_inst_id)
def test_conv3x3_forms_on_one_tile(inst, form, affine):
    """(1,16,16): one tile in total under a grid of 8 x ncb workgroups - the surplus ones leave at the top"""
    dtype, Cin, Cout = inst
    _case(3, dtype, 1, 16, 16, Cin, Cout, form, affine, tiles_per_walk=None if Cout > 64 else 1)


@pytest.mark.parametrize('inst', INST_3X3, ids=_inst_id)
def test_conv3x3_one_partial_tile(inst):
    dtype, Cin, Cout = inst
    if Cout > 64:
        _case(3, dtype, 1, 5, 12, Cin, Cout, 'rows', True, tiles_per_walk=1)     # (8x16 tiles)
    else:
        _case(3, dtype, 1, 20, 12, Cin, Cout, 'rows', True)


@pytest.mark.parametrize('inst', INST_3X3, ids=_inst_id)
def test_conv3x3_walk_of_two_tiles(inst):
    """every walk has exactly two tiles: the prologue's loads, then one in-loop prefetch, then none"""
    dtype, Cin, Cout = inst
    N, H, W = {32: (8, 64, 128), 64: (32, 32, 32), 128: (24, 16, 16)}[Cout]
    _case(3, dtype, N, H, W, Cin, Cout, 'rows', True, tiles_per_walk=2)


@pytest.mark.parametrize('pixels', [1, 63, 65, 64 * 256 + 1])
@pytest.mark.parametrize('layer', ROW_LAYERS_1X1, ids=lambda l: '{}-{}'.format(l[0], l[1]))
def test_conv1x1_pixel_counts(layer, pixels):
    """64 * nsplit + 1 pixels (nsplit = 256): workgroup 0 walks a full tile and then a tile of one pixel"""
    Cin, Cout, _ = layer
    hh = _h()
    from hipnet import _capi as C
    if pixels > 64:
        ns = C.call('hrnet_bwd_pw_splits', hh.dt_id(BF16), pixels, Cin, Cout)
        assert pixels == 65 or pixels == 64 * ns + 1
    for form in ('coef', 'rows', 'none'):
        _case(1, BF16, 1, 1, pixels, Cin, Cout, form, Cin <= 64)
