"""hipnet.upsample_slice on the GPU against tests/upsample_slice_ref.py: forward and backward inside the per-element bounds
on NaN- or pattern-prefilled buffers, every output written, accumulate adds, channels outside the slice keep their bits,
two runs give equal bits, and the dyadic cases equal float64 bit for bit."""
import functools

import numpy as np
import pytest
import torch

import upsample_slice_ref as U

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def _run(case, integer):
    """(forward (N, C, H, W), backward written over NaN (N, h, w, Cp), backward added onto a pattern, the pattern), on the CPU"""
    from hipnet import upsample_slice as S
    N, h, w, Cp, c0, C, H, W = case
    src, g = U.inputs(case, integer=integer)
    out = torch.full((N, C, H, W), float('nan'), device=DEV)
    S.forward(_dev(src), out, c0, C)
    pattern = _dev(np.random.RandomState(5).randn(N, h, w, Cp))
    wrote = torch.full((N, h, w, Cp), float('nan'), device=DEV)
    S.backward(_dev(g), wrote, c0, C, False)
    added = pattern.clone()
    S.backward(_dev(g), added, c0, C, True)
    torch.cuda.synchronize()
    return out.cpu(), wrote.cpu(), added.cpu(), pattern.cpu()


def _outside(case, t):
    N, h, w, Cp, c0, C, H, W = case
    return torch.cat([t[..., :c0], t[..., c0 + C:]], dim=3)


@pytest.mark.parametrize('case', U.CASES + U.DYADIC, ids=str)
def test_forward_inside_the_bound_and_every_output_written(case):
    src, _ = U.inputs(case)
    out = _run(case, False)[0]
    assert not bool(torch.isnan(out).any())
    err, bound = (out.double() - U.forward(src, case)).abs(), U.forward_bound(src, case)
    print('worst err / bound', float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize('case', U.CASES + U.DYADIC, ids=str)
def test_backward_inside_the_bound_adds_and_leaves_the_other_channels(case):
    N, h, w, Cp, c0, C, H, W = case
    _, g = U.inputs(case)
    _, wrote, added, pattern = _run(case, False)
    got = wrote[..., c0:c0 + C]
    assert not bool(torch.isnan(got).any())
    err, bound = (got.double() - U.backward(g, case)).abs(), U.backward_bound(g, case)
    print('worst err / bound', float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())
    # accumulate = 1 is one f32 addition of the same sum onto what was there
    assert torch.equal(added[..., c0:c0 + C], pattern[..., c0:c0 + C] + got)
    assert bool(torch.isnan(_outside(case, wrote)).all())
    assert torch.equal(_outside(case, added), _outside(case, pattern))


@pytest.mark.parametrize('case', U.CASES, ids=str)
def test_two_runs_are_bit_equal(case):
    from hipnet import upsample_slice as S
    N, h, w, Cp, c0, C, H, W = case
    src, g = U.inputs(case)
    out, wrote, _, _ = _run(case, False)
    again = S.forward(_dev(src), torch.empty((N, C, H, W), device=DEV), c0, C)
    dagain = S.backward(_dev(g), torch.zeros((N, h, w, Cp), device=DEV), c0, C, False)
    assert torch.equal(again.cpu(), out)
    assert torch.equal(dagain.cpu()[..., c0:c0 + C], wrote[..., c0:c0 + C])


@pytest.mark.parametrize('case', U.DYADIC, ids=str)
def test_dyadic_cases_equal_float64_bit_for_bit(case):
    N, h, w, Cp, c0, C, H, W = case
    src, g = U.inputs(case, integer=True)
    out, wrote, _, _ = _run(case, True)
    assert torch.equal(out.double(), U.forward(src, case))
    assert torch.equal(wrote[..., c0:c0 + C].double(), U.backward(g, case))


def test_autograd_function_and_refusals():
    from hipnet import upsample_slice as S
    case = U.CASES[0]
    N, h, w, Cp, c0, C, H, W = case
    src, g = U.inputs(case)
    x = _dev(src).requires_grad_(True)
    y = S.upsample_slice(x, c0, C, (H, W))
    (y * _dev(g)).sum().backward()
    out, wrote, _, _ = _run(case, False)
    assert torch.equal(y.detach().cpu(), out)
    assert torch.equal(x.grad.cpu()[..., c0:c0 + C], wrote[..., c0:c0 + C])
    assert float(_outside(case, x.grad.cpu()).abs().max()) == 0.0
    with pytest.raises(ValueError, match='do not lie in a row'):
        S.upsample_slice(x.detach(), c0, Cp, (H, W))
    with pytest.raises(ValueError, match='HIP-device'):
        S.upsample_slice(torch.zeros(1, 2, 2, 4), 0, 1, (2, 2))
    with pytest.raises(ValueError, match='expected H, W >= 1'):
        S.upsample_slice(x.detach(), c0, C, (0, 3))
