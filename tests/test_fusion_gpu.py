"""The cross-view fusion kernels (csrc/view_fusion.hip) and their autograd wrapper (models.multiview_pose_hrnet.view_fusion)
on the device against tests/fusion_ref.py, the float64 restatement of the two formulas.

Inputs are seeded: positive H rows (a softmax), W uniform in +-1/sqrt(P), dF of N(0, 1). Tolerances are derived, not
tuned: an f32 dot product of n terms differs from the exact one by at most about n * 2^-24 * sum|a||b|, and every output
is held elementwise to 2 x that (the factor 2 covers the output rounding and the summation order), with n = (V - 1) * P
for F and dH and n = B * K for dW. At every shape below one dropped 4-wide reduction step exceeds the bound.

Shapes: the smallest at which the tiling can go wrong - the plain case; P = 25 (unaligned weight rows, tails in both
dimensions, M = 63); V = 3 and V = 2; P = 1024 (many reduction steps and output tiles); M = 189 (twelve M tiles against
one weight tile); M = 210 (more M tiles than one workgroup holds: the second slice of the grid)."""
import numpy as np
import pytest
import torch

import fusion_ref as R

pytestmark = pytest.mark.gpu

# (B, V, K, h, w)
SHAPES = [(1, 4, 21, 8, 8), (3, 4, 21, 5, 5), (2, 3, 21, 8, 8), (1, 2, 5, 6, 6), (1, 4, 21, 32, 32), (9, 4, 21, 8, 8),
          (10, 2, 21, 8, 8)]
IDS = ['x'.join(map(str, s)) for s in SHAPES]
_CACHE = {}


def _case(shape):
    """inputs, the float64 reference and its gradients, computed once per shape and left unchanged"""
    if shape not in _CACHE:
        B, V, K, h, w = shape
        H, Ws, dF = R.inputs(B, V, K, h * w, seed=sum(s * 31 ** n for n, s in enumerate(shape)))
        Hg = H.clone().requires_grad_(True)
        Wg = [x.clone().requires_grad_(True) for x in Ws]
        F = R.fusion_ref(Hg, Wg)
        grads = torch.autograd.grad(F, [Hg] + Wg, dF)
        _CACHE[shape] = dict(H=H, Ws=Ws, dF=dF, F=F.detach(), dH=grads[0], dWs=list(grads[1:]),
                             F_bound=R.forward_bound(H, Ws), dH_bound=R.dh_bound(dF, Ws), dW_bound=R.dw_bounds(H, dF))
    return _CACHE[shape]


def _dev(shape, c, h_grad=True, w_grad=True):
    B, V, K, h, w = shape
    H = c['H'].float().reshape(B, V, K, h, w).cuda().requires_grad_(h_grad)
    Ws = [x.float().cuda().requires_grad_(w_grad) for x in c['Ws']]
    return H, Ws, c['dF'].float().reshape(B, V, K, h, w).cuda()


def _worst(got, ref, bound):
    """largest |got - ref| / bound; printed before it is asserted on"""
    return float(((got.detach().double().cpu().reshape(ref.shape) - ref).abs() / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_forward_parity(shape):
    from models.multiview_pose_hrnet import view_fusion
    c = _case(shape)
    H, Ws, _ = _dev(shape, c, False, False)
    F = view_fusion(H, Ws)
    assert F.shape == H.shape and F.dtype == torch.float32
    worst = _worst(F, c['F'], c['F_bound'])
    print('forward {}: worst error / bound = {:.3f}'.format(shape, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_backward_parity(shape):
    from models.multiview_pose_hrnet import view_fusion
    c = _case(shape)
    H, Ws, dF = _dev(shape, c)
    view_fusion(H, Ws).backward(dF)
    worst = _worst(H.grad, c['dH'], c['dH_bound'])
    print('dH {}: worst error / bound = {:.3f}'.format(shape, worst))
    assert worst <= 1.0
    for n, w in enumerate(Ws):
        worst = _worst(w.grad, c['dWs'][n], c['dW_bound'][n])
        print('dW[{}] {}: worst error / bound = {:.3f}'.format(n, shape, worst))
        assert worst <= 1.0


def test_one_dropped_step_exceeds_the_bounds():
    """the bounds see a single missing MFMA step: dropping four consecutive reduction terms from the first 16 x 16
    tile of outputs moves at least one of them by more than its bound, at every shape (float64, no device work)"""
    for shape in SHAPES:
        c = _case(shape)
        B, V, K = shape[:3]
        H, Ws, dF = c['H'], c['Ws'], c['dF']
        r = min(16, K)
        miss = 0.2 * (H[0, 1, :r, :4] @ Ws[R.pair_index(0, 1, V)][:16, :4].t()).abs()      # F[0, 0, :r, :16]
        assert (miss > c['F_bound'][0, 0, :r, :16]).any(), shape
        miss = 0.2 * (dF[0, 1, :r, :4] @ Ws[R.pair_index(1, 0, V)][:4, :16]).abs()         # dH[0, 0, :r, :16]
        assert (miss > c['dH_bound'][0, 0, :r, :16]).any(), shape
        rows = min(4, B * K)
        a, h = dF[:, 0].reshape(B * K, -1), H[:, 1].reshape(B * K, -1)
        miss = 0.2 * (a[:rows, :16].t() @ h[:rows, :16]).abs()                             # dW[n(0,1)][:16, :16]
        assert (miss > c['dW_bound'][R.pair_index(0, 1, V)][:16, :16]).any(), shape


def test_unused_pairs_get_no_gradient():
    """the model's layer at V = 3: matrices 6..11 are not used and their .grad stays None, as in torch"""
    from models.multiview_pose_hrnet import Aggregation
    from config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_list(['MODEL.HEATMAP_SIZE', '[8, 8]', 'MODEL.IMAGE_SIZE', '[32, 32]'])
    layer = Aggregation(cfg).cuda()
    shape = SHAPES[2]
    c = _case(shape)
    H, _, dF = _dev(shape, c)
    with torch.no_grad():
        for n in range(6):
            layer.aggre[n].weight.weight.copy_(c['Ws'][n].float())
    layer(H).backward(dF)
    for n in range(12):
        g = layer.aggre[n].weight.weight.grad
        if n < 6:
            assert _worst(g, c['dWs'][n], c['dW_bound'][n]) <= 1.0
        else:
            assert g is None
    assert _worst(H.grad, c['dH'], c['dH_bound']) <= 1.0


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[4]], ids=[IDS[1], IDS[4]])
def test_bit_reproducible(shape):
    from models.multiview_pose_hrnet import view_fusion
    c = _case(shape)
    outs = []
    for _ in range(2):
        H, Ws, dF = _dev(shape, c)
        F = view_fusion(H, Ws)
        F.backward(dF)
        outs.append([F.detach(), H.grad] + [w.grad for w in Ws])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_gradient_subsets():
    from models.multiview_pose_hrnet import view_fusion
    shape = SHAPES[1]
    c = _case(shape)
    H, Ws, dF = _dev(shape, c, True, False)                      # only H
    view_fusion(H, Ws).backward(dF)
    assert _worst(H.grad, c['dH'], c['dH_bound']) <= 1.0 and all(w.grad is None for w in Ws)
    H, Ws, dF = _dev(shape, c, False, True)                      # only the weights
    view_fusion(H, Ws).backward(dF)
    assert H.grad is None
    for n, w in enumerate(Ws):
        assert _worst(w.grad, c['dWs'][n], c['dW_bound'][n]) <= 1.0
    H, Ws, dF = _dev(shape, c, True, True)                       # one weight frozen among the others
    Ws[3].requires_grad_(False)
    view_fusion(H, Ws).backward(dF)
    assert Ws[3].grad is None and _worst(Ws[4].grad, c['dWs'][4], c['dW_bound'][4]) <= 1.0
    assert _worst(H.grad, c['dH'], c['dH_bound']) <= 1.0
    H, Ws, dF = _dev(shape, c, False, False)                     # neither: no graph node
    F = view_fusion(H, Ws)
    assert F.grad_fn is None and not F.requires_grad
    assert _worst(F, c['F'], c['F_bound']) <= 1.0


def test_weights_read_in_place():
    """the forward after an in-place W.mul_(2) follows the formula with the new weights: nothing was packed"""
    from models.multiview_pose_hrnet import view_fusion
    shape = SHAPES[0]
    c = _case(shape)
    H, Ws, _ = _dev(shape, c, False, False)
    assert _worst(view_fusion(H, Ws), c['F'], c['F_bound']) <= 1.0
    for w in Ws:
        w.mul_(2)
    W2 = [2.0 * w for w in c['Ws']]
    assert _worst(view_fusion(H, Ws), R.fusion_ref(c['H'], W2), R.forward_bound(c['H'], W2)) <= 1.0


def test_c_abi_refusals():
    """what the entry points refuse, by return code and message, without launching"""
    import ctypes
    from hipnet import _capi as C
    assert C.call('hrnet_view_fusion_supported', C.HR_F32, 4, 4096) == 1
    assert C.call('hrnet_view_fusion_supported', C.HR_F32, 1, 64) == 0
    assert C.call('hrnet_view_fusion_supported', C.HR_F32, 5, 64) == 0
    assert C.call('hrnet_view_fusion_supported', C.HR_BF16, 4, 64) == 0
    assert C.call('hrnet_view_fusion_supported', C.HR_F32, 4, 0) == 0
    H = torch.zeros(1, 2, 3, 16, device='cuda')
    W = [torch.zeros(16, 16, device='cuda') for _ in range(2)]
    arr = (ctypes.c_void_p * 2)(*[w.data_ptr() for w in W])
    with pytest.raises(RuntimeError, match='both null'):
        C.call('hrnet_view_fusion_bwd', C.HR_F32, H.data_ptr(), arr, H.data_ptr(), None, None, 1, 2, 3, 16, 0.4, 0.2,
               C.stream_ptr())
    with pytest.raises(RuntimeError, match='aliases'):
        C.call('hrnet_view_fusion', C.HR_F32, H.data_ptr(), arr, H.data_ptr(), 1, 2, 3, 16, 0.4, 0.2, C.stream_ptr())
    with pytest.raises(RuntimeError, match='needs f32'):
        C.call('hrnet_view_fusion', C.HR_F32, H.data_ptr(), arr, H.data_ptr(), 1, 5, 3, 16, 0.4, 0.2, C.stream_ptr())
    torch.cuda.synchronize()
