"""The hams of pose_hrnet_hamburger in training mode, with their one-step gradient, over the C ABI (csrc/nmf.hip):

    hams_train(low, specs, bases, steps)     every ham of a burger on its channels of one NHWC map

The reference runs the TRAIN_STEPS multiplicative updates under torch.no_grad() (ham.py:48-58); only compute_coef and the
closing bmm carry a gradient (ham.py:90-93, :261-269). So bases_T and coef_T - the factors after TRAIN_STEPS updates, before
compute_coef - are constants, and with Gm = bases_T^T bases_T

    dnum = coef_T * (dY^T bases_T) / (coef_T Gm + 1e-6)     hrnet_nmf_update with dY where X sits
    dX   = bases_T dnum^T                                    hrnet_nmf_reconstruct into the gradient's own strided view

(checked on the CPU in float64 against autograd through the reference's NMF2D in training mode: 1.4e-16 of max|dX|). The
backward of a ham is two launches of the forward's kernels; dY and dX are read and written in place through (ld, batch
stride, orientation), as the forward reads X. A single fused launch would save one (G, N, R) round trip - 8 MB at full
size - against about 6 GFLOP of products, and is not built. The bases get no gradient.

HIP-device float32 tensors only (a CPU tensor is a ValueError: there is no CPU path). Shapes are checked before any device
call. hipnet.nmf stays the inference module and keeps refusing gradients.
"""
import torch

from hipnet import nmf as N
from hipnet.nhwc import check


def _nchw(t, c0, ch):
    """channels [c0, c0 + ch) of an NHWC tensor as a (B, ch, h, w) view"""
    return t.permute(0, 3, 1, 2)[:, c0:c0 + ch]


def _forward(low, specs, bases, steps, keep):
    covered = sum(ch for _, _, ch, _ in specs)
    out = torch.empty_like(low) if covered == low.shape[3] else torch.zeros_like(low)     # pad channels stay zero
    saved = []
    for (spatial, c0, ch, S), b in zip(specs, bases):
        xs, outs = N.paired_views('hams_train', _nchw(low, c0, ch), _nchw(out, c0, ch), spatial, S)
        for (g0, xv), (_, ov) in zip(xs, outs):
            r = N.factorise(xv, b[g0:g0 + xv.shape[0]], steps, ov, keep=keep)
            if keep:
                saved.append(r[1])
    return out, saved


class _HamsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, low, specs, bases, steps):
        out, saved = _forward(low, specs, bases, steps, True)
        ctx.specs, ctx.saved = specs, saved          # neither inputs nor outputs: nothing autograd has to track
        return out

    @staticmethod
    def backward(ctx, gy):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        gy = gy.float()
        if gy.stride(3) != 1 or gy.stride(1) != gy.shape[2] * gy.stride(2):
            gy = gy.contiguous()                     # the kernels read evenly spaced pixels with unit-stride channels
        dlow = torch.zeros(gy.shape, dtype=torch.float32, device=gy.device)
        states = iter(ctx.saved)
        for spatial, c0, ch, S in ctx.specs:
            gs, ds = N.paired_views('hams_train', _nchw(gy, c0, ch), _nchw(dlow, c0, ch), spatial, S)
            for (_, gv), (_, dv) in zip(gs, ds):
                bases_T, coef_T, gm = next(states)
                N.reconstruct(bases_T, N.update_coef(coef_T, bases_T, gv, gm), dv)
        return dlow, None, None, None


def hams_train(low, specs, bases, steps):
    """low (B, h, w, Cp) f32 NHWC, already through its ReLU (non-negative); specs [(spatial, first channel, channels, S)] in
    drawing order; bases: one NORMALISED (B * S, D, R) tensor per ham, D = channels / S (spatial) or h * w (not); steps =
    TRAIN_STEPS. Returns the cheese input (B, h, w, Cp): each ham writes its own channels, the rest is zero; there is no
    cat. With a gradient required the backward is the one-step gradient above."""
    specs = [(bool(sp), int(c0), int(ch), int(S)) for sp, c0, ch, S in specs]
    bases = list(bases)
    check('hams_train', low=low, **{'bases{}'.format(i): b for i, b in enumerate(bases)})
    if low.ndim != 4 or low.numel() == 0:
        raise ValueError('hams_train: low {}: expected NHWC (B, h, w, Cp), nothing empty'.format(tuple(low.shape)))
    B, h, w, cp = low.shape
    if int(steps) < 0:
        raise ValueError('hams_train: steps = {}: must be at least 0'.format(steps))
    if not specs or len(specs) != len(bases):
        raise ValueError('hams_train: {} hams with {} bases'.format(len(specs), len(bases)))
    end = 0
    for (spatial, c0, ch, S), b in zip(specs, bases):
        if c0 < end or ch < 1 or S < 1 or ch % S or c0 + ch > cp:
            raise ValueError('hams_train: ham on channels [{}, {}) with S = {} of a {}-channel map: the hams take '
                             'ascending, disjoint channel ranges that S divides'.format(c0, c0 + ch, S, cp))
        end = c0 + ch
        D = ch // S if spatial else h * w
        if b.ndim != 3 or b.shape[0] != B * S or b.shape[1] != D or b.shape[2] < 1:
            raise ValueError('hams_train: bases {}: expected ({}, {}, R) for spatial = {}, S = {}'.format(
                tuple(b.shape), B * S, D, spatial, S))
    low = low.contiguous()
    bases = [b.detach().contiguous() for b in bases]
    if torch.is_grad_enabled() and low.requires_grad:
        return _HamsFn.apply(low, specs, bases, int(steps))
    with torch.no_grad():
        return _forward(low.detach(), specs, bases, int(steps), False)[0]
