"""CPU self-test of tests/bn_bounds.py on the shapes and data of tests/test_bn_sums_gpu.py (every case, in the dtypes
the GPU module runs): the bound holds for correct
f32 arithmetic (torch f32 convolutions, f32 row sums in blocked and in shuffled order), and it catches a dropped tile, a
doubled tile and one row's sum(dz*y) perturbed the way trap 4 did (10.09 stored where 8.75 was right).
Only host-side library queries are made (launch geometry, kernel names): no GPU."""
import pytest
import torch

import bn_bounds as B
import test_bn_sums_gpu as G

BF, F32 = torch.bfloat16, torch.float32
TRAP4 = 10.09 / 8.75


def _rows_f32(t32, geo, gen):
    """per-channel f64 sum of per-walk f32 sums of t32 [N, C, H, W]: (blocked: f32 tile sums, then the walk's tiles
    added one after the other in f32; shuffled: the walk's pixels in a random order, summed in f32)"""
    tv = B.tile_view(t32, geo['th'], geo['tw'], geo.get('ti', 1))        # [tiles, pix, C] f32
    tiles, pix, C = tv.shape
    tpw = geo['tpw']
    walks = -(-tiles // tpw)
    tv = torch.cat([tv, tv.new_zeros(walks * tpw - tiles, pix, C)]).view(walks, tpw, pix, C)
    ts = tv.sum(2)                                                       # f32 per tile
    acc = ts[:, 0].clone()
    for k in range(1, tpw):
        acc = acc + ts[:, k]
    blocked = acc.double().sum(0)
    flat = tv.reshape(walks, tpw * pix, C)
    shuffled = flat[:, torch.randperm(tpw * pix, generator=gen)].sum(1).double().sum(0)
    return blocked, shuffled


def _assert_catches(label, t, bound, geo, trap4=False):
    """half the smallest tile's share exceeds the bound, and the injected defects leave it"""
    tiles = B.tile_sums(t, geo['th'], geo['tw'], geo.get('ti', 1))
    want = t.sum((0, 2, 3))
    tmin = tiles.abs().min(0)
    assert bool((2 * bound <= tmin.values).all()), label
    k = tmin.indices
    one = tiles.gather(0, k.view(1, -1)).flatten()
    assert bool(((want - one) - want).abs().gt(bound).all()), label + ': a dropped tile passes'
    assert bool(((want + one) - want).abs().gt(bound).all()), label + ': a doubled tile passes'
    if trap4:
        tpw = geo['tpw']
        n = tiles.shape[0]
        rows = torch.cat([tiles, tiles.new_zeros(-(-n // tpw) * tpw - n, tiles.shape[1])]).view(-1, tpw, tiles.shape[1]).sum(1)
        small = rows.abs().min(0).values
        assert bool(((TRAP4 - 1) * small > bound).all()), label + ': the trap-4 row passes'


def _geo_fwd(case):
    N, H, W, Cin, Cout, ks, stride, _, _ = case
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    return G._walk(N, Ho, Wo, Cout, ks, stride)


def _holds_and_catches(label, terms, t32s, geos, trap4=False):
    """terms [(label, t, e)], t32s the same terms in f32 arithmetic, geos [(geometry, D)]"""
    gen = torch.Generator().manual_seed(5)
    for (lab, t, et), t32 in zip(terms, t32s):
        for geo, D in geos:
            bound = B.channel_bound(t, et, D)
            want = t.sum((0, 2, 3))
            for got in _rows_f32(t32, geo, gen):
                assert bool(((got - want).abs() <= bound).all()), (lab, label, float(((got - want).abs() / bound).max()))
            _assert_catches('{} {} D={}'.format(lab, label, D), t, bound, geo, trap4=trap4 and lab.endswith('*y'))


@pytest.mark.parametrize('dtype', [F32, BF])
@pytest.mark.parametrize('case', G.FWD_CASES)
def test_forward_bound_holds_and_sees_one_tile(case, dtype):
    N, H, W, Cin, Cout, ks, stride, aff, bias = case
    d = B.fwd_data(N, H, W, Cin, Cout, ks, stride, aff, bias, dtype, seed=100 + N + H + Cin + Cout + ks + stride)
    y, e = B.fwd_reference(d, ks, stride, dtype)
    terms = B.fwd_terms(y, e)
    # the f32 arithmetic of a correct kernel: the same staged operands, an f32 convolution, f32 sums
    x = d['x'].double()
    if aff:
        a, _ = B.stage(x * d['sc'].double().view(1, -1, 1, 1) + d['sh'].double().view(1, -1, 1, 1), dtype, relu=True)
    else:
        a = x
    y32 = torch.nn.functional.conv2d(a.float(), d['w'], d.get('bias'), stride=stride, padding=ks // 2)
    geos = [(_geo_fwd(case), 0)]
    if case[:8] + (False,) in G.RING_FWD_CASES:
        gr = G._ring_geometry(G.bnref_name(case[:8] + (False,), 1), N, H, W, Cout)
        geos.append((gr, 1))
    gen = torch.Generator().manual_seed(5)
    for (lab, t, et), t32 in zip(terms, (y32, y32 * y32)):
        for geo, ring in geos:
            for atomic in (0, 1):
                aw = -(-geo['gx'] // 8) if atomic else 0
                D = (B.ring_chain(geo['ti'], geo['th'], geo['tw'], geo['tpw'], aw) if ring else
                     B.walk_chain(geo['th'], geo['tw'], geo['tpw'], aw))
                bound = B.channel_bound(t, et, D)
                want = t.sum((0, 2, 3))
                for got in _rows_f32(t32, geo, gen):
                    assert bool(((got - want).abs() <= bound).all()), (lab, case, float(((got - want).abs() / bound).max()))
                _assert_catches('{} {} ring={}'.format(lab, case, ring), t, bound, geo)


@pytest.mark.parametrize('dtype', [F32, BF])
@pytest.mark.parametrize('mode', G.BS_MODES)
@pytest.mark.parametrize('case', G.BS_CASES)
def test_backward_rows_bound_holds_and_sees_one_tile(case, mode, dtype):
    N, H, W, Cin, Cout, ks, stride = case
    d = B.bs_data(N, H, W, Cin, Cout, ks, stride, mode, dtype, seed=300 + N + H + Cin + Cout + ks + stride)
    terms = B.bs_reference(d, ks, stride)
    v32 = torch.nn.grad.conv2d_input((N, Cin, H, W), d['w'], d['dy'], stride=stride, padding=ks // 2) + d['prev']
    if mode == 'bn_relu':
        keep = torch.addcmul(d['sh'].view(1, -1, 1, 1), d['yraw'], d['sc'].view(1, -1, 1, 1)) > 0
    elif mode == 'sum_mask':
        keep = d['m'] > 0
    else:
        keep = torch.ones_like(v32, dtype=torch.bool)
    dz32 = torch.where(keep, v32, torch.zeros_like(v32))
    geos = [(G._walk(N, H, W, Cin, ks, stride, True, stride == 2), 0)]
    if ks == 3 and stride == 1 and Cin >= 96:
        geos.append((G._ring_geometry(G.bs_name(case, 1, 1), N, H, W, Cin), 1))
    gen = torch.Generator().manual_seed(6)
    for (lab, t, et), t32 in zip(terms, (dz32, dz32 * d['yraw'])):
        for geo, ring in geos:
            D = B.ring_chain(geo['ti'], geo['th'], geo['tw'], geo['tpw']) if ring else B.walk_chain(geo['th'], geo['tw'], geo['tpw'])
            bound = B.channel_bound(t, et, D)
            want = t.sum((0, 2, 3))
            for got in _rows_f32(t32, geo, gen):
                assert bool(((got - want).abs() <= bound).all()), (lab, case, mode, float(((got - want).abs() / bound).max()))
            _assert_catches('{} {} {} ring={}'.format(lab, case, mode, ring), t, bound, geo, trap4=lab == 'sum dz*y')


@pytest.mark.parametrize('case', G.SUM_CASES)
def test_residual_sum_bound_holds_and_sees_one_tile(case):
    N, H, W, Cin, Cout, ks = case
    d = B.fwd_data(N, H, W, Cin, Cout, ks, 1, True, False, BF, seed=7 + N + H + Cin + Cout + ks, residual=True)
    y, e = B.fwd_reference(d, ks, 1, BF)
    a, _ = B.stage(d['x'].double() * d['sc'].double().view(1, -1, 1, 1) + d['sh'].double().view(1, -1, 1, 1), BF,
                   relu=True, addend=d['x2'])
    y32 = torch.nn.functional.conv2d(a.float(), d['w'], None, padding=ks // 2)
    geo = G._walk(N, H, W, Cout, ks, 1)
    geos = [(geo, B.walk_chain(geo['th'], geo['tw'], geo['tpw'], aw)) for aw in (0, -(-geo['gx'] // 8))]
    _holds_and_catches(str(case), B.fwd_terms(y, e), (y32, y32 * y32), geos)


@pytest.mark.parametrize('case,dtype', G._fused_params())
def test_fused_backward_bound_holds_and_sees_one_tile(case, dtype):
    N, H, W, Cin, Cout = case
    name = G.fused_name(G._C().dtype_id(dtype), Cin, Cout)
    th = int(name.split(', ')[2])
    d = B.fused_data(N, H, W, Cin, Cout, dtype, seed=500 + N + H + Cin + Cout)
    terms = B.fused_reference(d, dtype)
    A, Bc, Cc = (d['coef'][k].view(1, -1, 1, 1) for k in range(3))
    g = torch.addcmul(torch.addcmul(Cc, Bc, d['y']), A, d['dz']).to(dtype).float()
    dx = torch.nn.grad.conv2d_input(d['x'].shape, d['w'], g, padding=1) + d['addend']
    a = torch.relu(torch.addcmul(d['sh'].view(1, -1, 1, 1), d['x'], d['sc'].view(1, -1, 1, 1))).to(dtype)
    dx = torch.where(a > 0, dx, torch.zeros_like(dx))
    ns = G._C().call('hrnet_bwd_fused_splits', G._C().dtype_id(dtype), N, H, W, Cin, Cout)
    geo = dict(th=th, tw=16, tpw=-(-(N * -(-H // th) * -(-W // 16)) // ns))
    _holds_and_catches(str(case), terms, (dx, dx * d['bs_y']), [(geo, B.walk_chain(th, 16, geo['tpw'], wp_max=8))],
                       trap4=True)
