"""tests/upsample_slice_ref.py checked on the CPU: (a) torch's own float32 result lies inside the per-element bounds on every
case the GPU test uses, (b) an align_corners=False evaluation and a one-channel shift of the slice fall outside them, so
the bounds see what they should, (c) on the dyadic size pairs with integer inputs the float64 result is a float32 number,
so the GPU test may demand bit equality there."""
import pytest
import torch

import upsample_slice_ref as U


@pytest.mark.parametrize('case', U.CASES + U.DYADIC, ids=str)
def test_torch_float32_lies_inside_the_bounds(case):
    src, g = U.inputs(case)
    ref, bound = U.forward(src, case), U.forward_bound(src, case)
    err = (U.forward(src, case, torch.float32).double() - ref).abs()
    print('forward worst err / bound', float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())
    ref, bound = U.backward(g, case), U.backward_bound(g, case)
    err = (U.backward(g, case, torch.float32).double() - ref).abs()
    print('backward worst err / bound', float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize('case', [c for c in U.CASES if (c[1], c[2]) != (c[6], c[7]) and c[1] * c[2] > 1], ids=str)
def test_align_corners_false_falls_outside(case):
    src, g = U.inputs(case)
    assert not bool(((U.forward(src, case, align_corners=False) - U.forward(src, case)).abs()
                     <= U.forward_bound(src, case)).all())
    assert not bool(((U.backward(g, case, align_corners=False) - U.backward(g, case)).abs()
                     <= U.backward_bound(g, case)).all())


@pytest.mark.parametrize('case', U.CASES, ids=str)
def test_a_shifted_slice_falls_outside(case):
    N, h, w, Cp, c0, C, H, W = case
    shift = 1 if c0 + C < Cp else -1
    src, _ = U.inputs(case)
    assert not bool(((U.forward(src, case, shift=shift) - U.forward(src, case)).abs() <= U.forward_bound(src, case)).all())


@pytest.mark.parametrize('case', U.DYADIC, ids=str)
def test_dyadic_pairs_are_exact_in_float32(case):
    src, g = U.inputs(case, integer=True)
    fwd, bwd = U.forward(src, case), U.backward(g, case)
    assert U.exact(fwd) and U.exact(bwd)
    assert torch.equal(U.forward(src, case, torch.float32).double(), fwd)
    assert float(fwd.abs().max()) > 0 and float(bwd.abs().max()) > 0
