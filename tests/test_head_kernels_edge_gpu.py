"""The head kernels of csrc/head_mix.hip at the smallest shapes at which their paths can go wrong
(tests/test_head_mix_gpu.py holds the full w32 head shape).

Transposed upsampling (hrnet_upsample_bilinear_t, tile form): bf16 runs on the matrix pipe - the contraction over the
pixels of an image row is an MFMA whose weights are exact in bf16, the contraction over rows f32 FMAs - on a grid that
walks (tile, 64-channel chunk) jobs. Checked against the CPU autograd of F.interpolate, against the streamed form of
the same entry point, and with G = 1, where every output is the sum of its row of the upsampling matrix: per axis the
weights of low-resolution index h are (r + 1/2)/s and 1 - (r + 1/2)/s over 2s full-resolution indices, s in all; at a
clamped border the s/2 indices that exist on the outer side carry 1 each instead of the s that sum to s/2, so the sum
stays s (the columns of an interpolation matrix whose rows sum to 1 share H = s * hs evenly). Every output is s * s.

The walk's grid is min(jobs, 512) rounded up to a multiple of 8: the cases below have fewer jobs than that (workgroups
with one job and, through the rounding, with none); test_upsample_t_walk_with_several_jobs_per_workgroup sets the grid
to 8 through HRNET_UPT_GRID, which the library honours under HRNET_MEASURE=1 - read once per process, hence the child
process.

Mix / backward modes 0, 1, 2 (hrnet_head_mix, hrnet_head_bwd): one workgroup per (pixel tile, 96-channel chunk), no
walk - their job count is their grid. Reference: the fp32 kernel of the same entry point on the same bf16-rounded
operands, to the tolerances of tests/test_head_mix_gpu.py."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from spawned import spawned

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


def _h():
    import hip_helpers as hh
    return hh


def _C():
    from hipnet import _capi as C
    return C


def _pp(tensors):
    arr = (ctypes.c_void_p * max(1, len(tensors)))()
    for k, t in enumerate(tensors):
        arr[k] = t.data_ptr()
    return arr


def _ip(vals):
    return (ctypes.c_int * max(1, len(vals)))(*vals)


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------- transposed upsampling

UPT_CASES = [
    # N, H, W, C, output sizes
    (1, 8, 8, 8, [(1, 1)]),                               # scale 8, ONE output pixel: both border rules on both axes,
                                                          # image smaller than a tile
    (2, 16, 16, 40, [(8, 8), (4, 4), (2, 2)]),            # one tile; 40 channels fill neither a chunk nor a fragment
    (1, 32, 32, 8, [(16, 16), (8, 8), (4, 4)]),           # footprints across interior tile edges on both axes
    (3, 24, 40, 96, [(12, 20), (6, 10), (3, 5)]),         # overhanging tiles, non-square, 36 jobs on a grid of 40
    (2, 32, 32, 8, [(16, 16), (8, 8), (4, 4)]),           # 8 jobs: equal to the grid, no idle workgroup
]
_UPT_REF = {}


def _upt_ref(case):
    """(G as the device holds it [N][C][H][W] f32, autograd references), computed once per case"""
    if case not in _UPT_REF:
        N, H, W, Cc, sizes = UPT_CASES[case]
        g = torch.Generator().manual_seed(41 + H + Cc)
        G = torch.randn(N, Cc, H, W, generator=g).to(BF).float()
        refs = []
        for hs, ws in sizes:
            x = torch.zeros(N, Cc, hs, ws, requires_grad=True)
            F.interpolate(x, size=(H, W), mode='bilinear', align_corners=False).backward(G)
            refs.append(x.grad)
        _UPT_REF[case] = (G, refs)
    return _UPT_REF[case]


def _upt_run(G, sizes, streamed):
    hh, C = _h(), _C()
    N, Cc, H, W = G.shape
    gd = hh.nhwc(G, BF)
    outs = [torch.full((N, hs, ws, Cc), float('nan'), dtype=BF, device=hh.DEV) for hs, ws in sizes]
    C.call('hrnet_upsample_bilinear_t', C.dtype_id(BF), gd.data_ptr(), _pp(outs), _ip([h for h, _ in sizes]),
           _ip([w for _, w in sizes]), len(sizes), N, H, W, Cc, 0, streamed, C.stream_ptr())
    hh.sync()
    return [hh.from_nhwc(o) for o in outs]


def _upt_check(case):
    N, H, W, Cc, sizes = UPT_CASES[case]
    G, refs = _upt_ref(case)
    tile, stream = _upt_run(G, sizes, 0), _upt_run(G, sizes, 1)
    for k, ref in enumerate(refs):
        tol = 2.0 ** -8 * float(ref.abs().max())          # one output rounding
        e_ref = float((tile[k] - ref).abs().max())
        e_str = float((tile[k] - stream[k]).abs().max())
        print('upsample_t case {} out {}: |tile - autograd| {:.3e} |tile - streamed| {:.3e} bound {:.3e}'.format(
            case, sizes[k], e_ref, e_str, tol))
        assert e_ref <= tol, (case, sizes[k], e_ref, tol)
        assert e_str <= tol, (case, sizes[k], e_str, tol)


def _upt_check_ones(case):
    N, H, W, Cc, sizes = UPT_CASES[case]
    got = _upt_run(torch.ones(N, Cc, H, W), sizes, 0)
    for (hs, ws), o in zip(sizes, got):
        s = H // hs
        assert tuple(o.shape) == (N, Cc, hs, ws)
        assert torch.equal(o, torch.full_like(o, float(s * s))), (case, (hs, ws), float(o.min()), float(o.max()))


@pytest.mark.parametrize('case', range(len(UPT_CASES)))
def test_upsample_t_tile_form_at_edge_shapes(case):
    _upt_check(case)


@pytest.mark.parametrize('case', range(len(UPT_CASES)))
def test_upsample_t_of_ones_is_the_row_sum_of_the_upsampling_matrix(case):
    """random signs could hide a wrong or missing weight; G = 1 cannot. The closed form itself (s per axis) is held
    against autograd once, for the case with every border rule"""
    _upt_check_ones(case)
    if case == 0:
        x = torch.zeros(1, 1, 1, 1, requires_grad=True)
        F.interpolate(x, size=(8, 8), mode='bilinear', align_corners=False).backward(torch.ones(1, 1, 8, 8))
        assert float(x.grad) == 64.0


@spawned
def test_upsample_t_walk_with_several_jobs_per_workgroup():
    """a grid of 8 workgroups (HRNET_UPT_GRID under HRNET_MEASURE, read once per process: a child process): case 3 has
    36 jobs then, five for most workgroups, four and one for the last two, so that a workgroup stages a region while
    its next job's loads are in flight and re-uses the staging area; case 4 has as many jobs as workgroups, case 0
    leaves seven workgroups idle"""
    os.environ['HRNET_MEASURE'] = '1'
    os.environ['HRNET_UPT_GRID'] = '8'
    for case in (0, 3, 4):
        _upt_check(case)
        _upt_check_ones(case)


# ---------------------------------------------------------------- mix and backward modes

MIX_SHAPES = [
    # N, H, W, K, Cout
    (3, 8, 8, 32, 96),        # every tile partial
    (1, 24, 40, 48, 104),     # K with a half-empty second K step; Cout ends inside a sub-block and a 96-channel chunk
    (5, 16, 16, 16, 40),      # five jobs
]


def _mix_operands(shape, nup):
    N, H, W, K, Cout = shape
    g = torch.Generator().manual_seed(7 + H + Cout + nup)
    x0 = torch.randn(N, H, W, K, generator=g).to(BF)
    w0 = (torch.randn(Cout, K, generator=g) / K ** 0.5).to(BF)
    bias = torch.randn(Cout, generator=g) * 0.1
    ts = [torch.randn(N, H >> j, W >> j, Cout, generator=g).to(BF) for j in range(1, nup + 1)]
    return x0, w0, bias, ts


def _mix_run(shape, nup, rows_mode, DT, ops):
    hh, C = _h(), _C()
    N, H, W, K, Cout = shape
    x0, w0, bias, ts = ops
    xd, wd, bd = x0.to(DT).to(hh.DEV), w0.to(DT).to(hh.DEV), bias.to(hh.DEV)
    td = [t.to(DT).to(hh.DEV) for t in ts]
    y = torch.full((N, H, W, Cout), float('nan'), dtype=DT, device=hh.DEV)
    nrows = C.call('hrnet_head_mix_rows', N, H, W)
    stats = torch.zeros((nrows if rows_mode else 8), 2, Cout, dtype=F32, device=hh.DEV)
    C.call('hrnet_head_mix', C.dtype_id(DT), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(),
           stats.data_ptr(), rows_mode, _pp(td), _ip([H >> j for j in range(1, nup + 1)]),
           _ip([W >> j for j in range(1, nup + 1)]), nup, N, H, W, K, Cout, 0, C.stream_ptr())
    hh.sync()
    return y, stats


@pytest.mark.parametrize('rows_mode', [0, 1])
@pytest.mark.parametrize('nup', [0, 3])
@pytest.mark.parametrize('shape', MIX_SHAPES)
def test_head_mix_forward_at_edge_shapes(shape, nup, rows_mode):
    N, H, W, K, Cout = shape
    ops = _mix_operands(shape, nup)
    y, stats = _mix_run(shape, nup, rows_mode, BF, ops)
    ref, rstats = _mix_run(shape, nup, rows_mode, F32, ops)
    ref = ref.cpu()
    scale = float(ref.abs().max())
    err = float((y.float().cpu() - ref).abs().max())
    print('head_mix {} nup {} rows {}: err {:.3e} bound {:.3e}'.format(shape, nup, rows_mode, err, 1.2e-2 * scale))
    assert err <= 1.2e-2 * scale, (err, scale)
    # the statistics are those of the f32 values each kernel formed before its store
    cnt = N * H * W
    s, r = stats.sum(0).cpu() / cnt, rstats.sum(0).cpu() / cnt
    assert torch.allclose(s[0], r[0], atol=2e-3 * scale)
    assert torch.allclose(s[1], r[1], rtol=2e-2, atol=1e-4 * scale * scale)
    if rows_mode:
        y2, stats2 = _mix_run(shape, nup, rows_mode, BF, ops)
        assert torch.equal(y.view(torch.int16), y2.view(torch.int16)) and torch.equal(stats, stats2)


BWD_VARIANTS = [
    # inner_relu, BatchNorm affine in front of the ReLU mask
    (1, True),
    (1, False),       # null bn_scale / bn_shift: the mask is [y > 0]
    (0, False),       # no mask at all
]


def _bwd_run(shape, mode, relu, affine, DT, ops):
    hh, C = _h(), _C()
    N, H, W, K, Cout = shape
    dy, wT, y, sc, sf, coef = ops
    dd, wd, yd = dy.to(DT).to(hh.DEV), wT.to(DT).to(hh.DEV), y.to(DT).to(hh.DEV)
    scd = sc.to(hh.DEV) if affine else None
    sfd = sf.to(hh.DEV) if affine else None
    cfd = coef.to(hh.DEV).contiguous()
    if mode == 1:
        out = torch.full((C.call('hrnet_head_mix_rows', N, H, W), 2, Cout), float('nan'), device=hh.DEV)
    else:
        out = torch.full((N, H, W, Cout), float('nan'), dtype=DT, device=hh.DEV)
    C.call('hrnet_head_bwd', C.dtype_id(DT), mode, dd.data_ptr(), wd.data_ptr(), yd.data_ptr(), out.data_ptr(),
           _ptr(scd), _ptr(sfd), cfd.data_ptr() if mode == 2 else None, relu, N, H, W, K, Cout, C.stream_ptr())
    hh.sync()
    return out


@pytest.mark.parametrize('variant', BWD_VARIANTS)
@pytest.mark.parametrize('shape', MIX_SHAPES)
def test_head_backward_modes_at_edge_shapes(shape, variant):
    N, H, W, K, Cout = shape
    relu, affine = variant
    g = torch.Generator().manual_seed(13 + H + Cout)
    dy = torch.randn(N, H, W, K, generator=g).to(BF)
    wT = (torch.randn(Cout, K, generator=g) / K ** 0.5).to(BF)
    y = torch.randn(N, H, W, Cout, generator=g).to(BF)
    sc = torch.rand(Cout, generator=g) + 0.5
    sf = torch.randn(Cout, generator=g) * 0.3
    coef = torch.randn(3, Cout, generator=g)
    ops = (dy, wT, y, sc, sf, coef)
    # sum |dz| per channel, the scale of the row sums' bound (f32 sums of exact products in another order)
    dz = dy.float() @ wT.float().t()
    yf = y.float()
    if relu:
        dz = torch.where((yf * sc + sf if affine else yf) > 0, dz, torch.zeros(()))
    tol = 1e-4 * float(dz.abs().sum((0, 1, 2)).max())
    rows = _bwd_run(shape, 1, relu, affine, BF, ops)
    rref = _bwd_run(shape, 1, relu, affine, F32, ops)
    r, rr = rows.double().sum(0).cpu(), rref.double().sum(0).cpu()
    e1, e2 = float((r[0] - rr[0]).abs().max()), float((r[1] - rr[1]).abs().max())
    print('head_bwd {} relu {} affine {}: row-sum err {:.3e} {:.3e} bound {:.3e}'.format(shape, relu, affine, e1, e2, tol))
    assert e1 <= tol and e2 <= 3 * tol, (e1, e2, tol)
    assert torch.equal(rows, _bwd_run(shape, 1, relu, affine, BF, ops))            # rows: bit-reproducible
    out = _bwd_run(shape, 2, relu, affine, BF, ops).float().cpu()
    oref = _bwd_run(shape, 2, relu, affine, F32, ops).cpu()
    scale = float(oref.abs().max())
    err = float((out - oref).abs().max())
    print('head_bwd mode 2: err {:.3e} bound {:.3e}'.format(err, 1.2e-2 * scale))
    assert err <= 1.2e-2 * scale, (err, scale)
