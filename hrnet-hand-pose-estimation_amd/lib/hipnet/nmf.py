"""NMF ops of pose_hrnet_hamburger over the C ABI (csrc/nmf.hip), forward only,

    product(x, bases)                     hrnet_nmf_product        logits X^T Bs (G, N, R)
    softmax_rows(z)                       hrnet_spatial_softmax_fwd  softmax over R of every row
    gram(a)                               hrnet_nmf_gram           A^T A (G, R, R)
    update_coef(coef, bases, x, gm)       hrnet_nmf_update         coef * (X^T Bs) / (coef gm + eps)
    update_bases(bases, coef, x, gm)      hrnet_nmf_update         bases * (X coef) / (bases gm + eps)
    reconstruct(bases, coef, out)         hrnet_nmf_reconstruct    Bs Cf^T written into the strided view `out`
    nmf2d(x, bases, steps, spatial, S, out=None)                   the whole factorisation on given bases

The feature matrices are a strided view x (G, D, N): element X_g[d, n] at x.stride() = (batch, s_d, s_n) with s_n == 1 or
s_d == 1. Nothing is copied or transposed: the view's pointer, leading dimension, batch stride and orientation go to the
kernels as they are, so a channel half of an NCHW or NHWC tensor is read in place. Bases (G, D, R), coefficients (G, N, R)
and Gram matrices (G, R, R) are dense.

HIP-device float32 tensors only (a CPU tensor is a ValueError: there is no CPU path). Shapes are checked before any device
call. There is no autograd here: an input that requires grad while grad is enabled raises NotImplementedError.
"""
import torch

from hipnet import _capi as C
from hipnet.nhwc import check

OP_UPDATE, OP_GRAM, OP_PRODUCT = (C.VALUES['HR_NMF_' + n] for n in ('UPDATE', 'GRAM', 'PRODUCT'))
EPS = 1e-6                   # the reference's denominator guard (ham.py:250, :257, :267)
MAX_G = 65535


def _no_grad(name, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise NotImplementedError('{}: backward is not built (pose_hrnet_hamburger is inference only): run under '
                                  'torch.no_grad()'.format(name))


def supported(op, a, b=0):
    return bool(C.call('hrnet_nmf_supported', int(op), int(a), int(b)))


def _dense(name, what, t, shape):
    if tuple(t.shape) != tuple(shape):
        raise ValueError('{}: {} {}: expected {}'.format(name, what, tuple(t.shape), tuple(shape)))
    return t.detach().contiguous()


def _view(name, x):
    """(pointer, ld, batch stride, orientation) of a strided (G, D, N) view: orientation 0 is X[d, n] = mem[d * ld + n]"""
    if x.ndim != 3 or x.numel() == 0:
        raise ValueError('{}: x {}: expected (G, D, N), nothing empty'.format(name, tuple(x.shape)))
    G, D, N = x.shape
    if G > MAX_G or not supported(OP_PRODUCT, D, N):
        raise ValueError('{}: x {}: no kernel for this shape (G <= {}, D, N <= 2^24)'.format(name, tuple(x.shape), MAX_G))
    sb, sd, sn = x.stride()
    if N == 1 or sn == 1:
        orient, ld, run = 0, sd, N
    elif D == 1 or sd == 1:
        orient, ld, run = 1, sn, D
    else:
        raise ValueError('{}: x has strides {}: one of the last two must be 1 (the kernels read a row-major matrix or its '
                         'transpose in place)'.format(name, tuple(x.stride())))
    if (D == 1 and orient == 0) or (N == 1 and orient == 1):
        ld = max(ld, run)                    # a single row: its stride is never used
    if ld < run or sb < 0 or (G > 1 and sb < 1):
        raise ValueError('{}: x {} with strides {}: rows overlap'.format(name, tuple(x.shape), tuple(x.stride())))
    return x.data_ptr(), int(ld), int(sb) if G > 1 else 0, orient


def product(x, bases):
    """x (G, D, N) strided, bases (G, D, R) -> X^T bases (G, N, R)"""
    check('product', x=x, bases=bases)
    p, ld, bs, orient = _view('product', x)
    G, D, N = x.shape
    if bases.ndim != 3 or bases.shape[0] != G or bases.shape[1] != D or bases.shape[2] < 1:
        raise ValueError('product: bases {} for x {}: expected ({}, {}, R)'.format(tuple(bases.shape), tuple(x.shape), G, D))
    _no_grad('product', x, bases)
    bases = bases.detach().contiguous()
    R = bases.shape[2]
    out = torch.empty((G, N, R), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        C.call('hrnet_nmf_product', p, ld, bs, 1 - orient, bases.data_ptr(), out.data_ptr(), G, N, D, R, C.stream_ptr())
    return out


def softmax_rows(z, out=None):
    """softmax over the last axis of z (G, N, R): hrnet_spatial_softmax_fwd on G * N rows with temperature 1"""
    check('softmax_rows', z=z, out=out)
    if z.ndim != 3 or z.numel() == 0 or z.shape[0] * z.shape[1] > 0x7fffffff:
        raise ValueError('softmax_rows: z {}: expected (G, N, R), nothing empty'.format(tuple(z.shape)))
    _no_grad('softmax_rows', z)
    z = z.detach().contiguous()
    if out is None:
        out = torch.empty_like(z)
    elif tuple(out.shape) != tuple(z.shape) or not out.is_contiguous() or out.data_ptr() == z.data_ptr():
        raise ValueError('softmax_rows: out {}: expected a dense tensor of z\'s shape, not z itself'.format(tuple(out.shape)))
    one = torch.ones(1, dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        C.call('hrnet_spatial_softmax_fwd', z.data_ptr(), one.data_ptr(), out.data_ptr(), z.shape[0] * z.shape[1],
               z.shape[2], C.stream_ptr())
    return out


def gram_scratch(G, K, R):
    return int(C.call('hrnet_nmf_gram_scratch', int(G), int(K), int(R)))


def gram(a, out=None, scratch=None):
    """a (G, K, R) -> a^T a (G, R, R); scratch: None (allocated here) or a float32 tensor of gram_scratch(G, K, R) values"""
    check('gram', a=a, out=out, scratch=scratch)
    if a.ndim != 3 or a.numel() == 0 or a.shape[0] > MAX_G or not supported(OP_GRAM, a.shape[1], a.shape[2]):
        raise ValueError('gram: a {}: expected (G, K, R), nothing empty, G <= {}'.format(tuple(a.shape), MAX_G))
    _no_grad('gram', a)
    a = a.detach().contiguous()
    G, K, R = a.shape
    if out is None:
        out = torch.empty((G, R, R), dtype=torch.float32, device=a.device)
    elif tuple(out.shape) != (G, R, R) or not out.is_contiguous():
        raise ValueError('gram: out {}: expected a dense ({}, {}, {})'.format(tuple(out.shape), G, R, R))
    need = gram_scratch(G, K, R)
    if scratch is None and need:
        scratch = torch.empty(need, dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        C.call('hrnet_nmf_gram', a.data_ptr(), out.data_ptr(), C.ptr(scratch), 0 if scratch is None else scratch.numel(),
               G, K, R, C.stream_ptr())
    return out


def _update(name, t, f, x, gm, xt_of, M, K, out, eps):
    p, ld, bs, orient = _view(name, x)
    G = x.shape[0]
    if t.ndim != 3 or t.shape[2] < 1:
        raise ValueError('{}: {}: expected three axes'.format(name, tuple(t.shape)))
    R = t.shape[2]
    t, f, gm = _dense(name, 'updated factor', t, (G, M, R)), _dense(name, 'fixed factor', f, (G, K, R)), \
        _dense(name, 'gram', gm, (G, R, R))
    if not eps > 0:
        raise ValueError('{}: eps = {}: must be positive'.format(name, eps))
    if out is None:
        out = torch.empty_like(t)
    elif tuple(out.shape) != (G, M, R) or not out.is_contiguous() or out.data_ptr() in (t.data_ptr(), f.data_ptr(),
                                                                                       gm.data_ptr()):
        raise ValueError('{}: out {}: expected a dense ({}, {}, {}) that is none of the inputs (the update is out of '
                         'place)'.format(name, tuple(out.shape), G, M, R))
    with torch.cuda.device(x.device):
        C.call('hrnet_nmf_update', t.data_ptr(), f.data_ptr(), p, ld, bs, xt_of(orient), gm.data_ptr(), out.data_ptr(), G, M,
               K, R, float(eps), C.stream_ptr())
    return out


def update_coef(coef, bases, x, gm, out=None, eps=EPS):
    """coef (G, N, R) * (X^T bases) / (coef gm + eps) with gm = bases^T bases (G, R, R)"""
    check('update_coef', coef=coef, bases=bases, x=x, gm=gm, out=out)
    _no_grad('update_coef', coef, bases, x, gm)
    if x.ndim != 3:
        raise ValueError('update_coef: x {}: expected (G, D, N)'.format(tuple(x.shape)))
    return _update('update_coef', coef, bases, x, gm, lambda o: 1 - o, x.shape[2], x.shape[1], out, eps)


def update_bases(bases, coef, x, gm, out=None, eps=EPS):
    """bases (G, D, R) * (X coef) / (bases gm + eps) with gm = coef^T coef (G, R, R)"""
    check('update_bases', bases=bases, coef=coef, x=x, gm=gm, out=out)
    _no_grad('update_bases', bases, coef, x, gm)
    if x.ndim != 3:
        raise ValueError('update_bases: x {}: expected (G, D, N)'.format(tuple(x.shape)))
    return _update('update_bases', bases, coef, x, gm, lambda o: o, x.shape[1], x.shape[2], out, eps)


def reconstruct(bases, coef, out):
    """out (G, D, N), a strided view as x is: out_g = bases_g coef_g^T, written in place; returns out"""
    check('reconstruct', bases=bases, coef=coef, out=out)
    p, ld, bs, orient = _view('reconstruct', out)
    G, D, N = out.shape
    if bases.ndim != 3 or bases.shape[2] < 1:
        raise ValueError('reconstruct: bases {}: expected (G, D, R)'.format(tuple(bases.shape)))
    R = bases.shape[2]
    _no_grad('reconstruct', bases, coef)
    bases, coef = _dense('reconstruct', 'bases', bases, (G, D, R)), _dense('reconstruct', 'coef', coef, (G, N, R))
    with torch.cuda.device(out.device):
        C.call('hrnet_nmf_reconstruct', bases.data_ptr(), coef.data_ptr(), p, ld, bs, orient, G, D, N, R, C.stream_ptr())
    return out


def factorise(x, bases, steps, out, keep=False):
    """the iteration of NMF2D in eval mode (ham.py:49-58, :244-269, :93) on x (G, D, N), bases (G, D, R), both as above;
    the reconstruction goes to the view `out` (G, D, N). 3 + 4 steps + 2 launches, plus one per split Gram matrix.
    keep: return (out, (bases_T, coef_T, Gm)) - the factors after `steps` updates, BEFORE the closing coefficient update,
    and Gm = bases_T^T bases_T: what the one-step gradient of hipnet.nmf_train reads (the closing update writes to the
    spare buffer, so coef_T is intact; with steps = 0 bases_T is the caller's tensor)."""
    G, D, N = x.shape
    R = bases.shape[2]
    dev = x.device
    need = max(gram_scratch(G, D, R), gram_scratch(G, N, R))
    scratch = torch.empty(need, dtype=torch.float32, device=dev) if need else None
    gm = torch.empty((G, R, R), dtype=torch.float32, device=dev)
    spare_c = product(x, bases)
    coef = softmax_rows(spare_c)
    own = [torch.empty_like(bases) for _ in range(min(int(steps), 2))]     # the caller's bases are never written
    for k in range(int(steps)):
        coef, spare_c = update_coef(coef, bases, x, gram(bases, gm, scratch), spare_c), coef
        bases = update_bases(bases, coef, x, gram(coef, gm, scratch), own[k % 2])
    last = update_coef(coef, bases, x, gram(bases, gm, scratch), spare_c)
    reconstruct(bases, last, out)
    return (out, (bases, coef, gm)) if keep else out


def group_view(name, x, spatial, S):
    """the (B * S, D, N) matrices of NMF2D (ham.py:66-74) as views of x (B, C, H, W), any strides whose pixels are evenly
    spaced: a list of (first group, view) pairs - one view when the groups are evenly spaced in memory, one per image
    otherwise (a channel half of a wider tensor with S > 1)"""
    if x.ndim != 4 or x.numel() == 0:
        raise ValueError('{}: x {}: expected (B, C, H, W), nothing empty'.format(name, tuple(x.shape)))
    B, Cc, H, W = x.shape
    S = int(S)
    if S < 1 or Cc % S:
        raise ValueError('{}: S = {} does not divide the {} channels'.format(name, S, Cc))
    sb, sc, sh, sw = x.stride()
    if H > 1 and W > 1 and sh != W * sw:
        raise ValueError('{}: x has strides {}: the pixels of a channel must be evenly spaced (stride(2) == W * '
                         'stride(3))'.format(name, tuple(x.stride())))
    sp = sw if W > 1 else (sh if H > 1 else 1)
    Dc, P = Cc // S, H * W
    size, strides = ((Dc, P), (sc, sp)) if spatial else ((P, Dc), (sp, sc))
    if B == 1 or S == 1 or sb == S * Dc * sc:
        gs = sb if S == 1 else Dc * sc
        return [(0, x.as_strided((B * S,) + size, (gs,) + strides, x.storage_offset()))]
    return [(b * S, x.as_strided((S,) + size, (Dc * sc,) + strides, x.storage_offset() + b * sb)) for b in range(B)]


def paired_views(name, a, b, spatial, S):
    """group_view of two tensors of one shape, cut alike: when one is evenly spaced and the other is not, both go image
    by image"""
    va, vb = group_view(name, a, spatial, S), group_view(name, b, spatial, S)
    if len(va) != len(vb):
        per = lambda t: [(i * int(S), v) for i in range(t.shape[0]) for _, v in group_view(name, t[i:i + 1], spatial, S)]
        va, vb = per(a), per(b)
    return va, vb


def nmf2d(x, bases, steps, spatial, S, out=None):
    """NMF2D in eval mode on given bases: x (B, C, H, W), any strides (NCHW, channels-last, a channel slice), non-negative;
    bases (B * S, D, R) with D = C / S (spatial) or H * W (not), already normalised; steps = EVAL_STEPS. Returns the
    reconstruction in x's shape: `out` if given (any such strides, written in place), a new NCHW tensor otherwise."""
    check('nmf2d', x=x, bases=bases, out=out)
    _no_grad('nmf2d', x, bases)
    xs = group_view('nmf2d', x, spatial, S)
    G, D, N = x.shape[0] * int(S), xs[0][1].shape[1], xs[0][1].shape[2]
    if bases.ndim != 3 or bases.shape[0] != G or bases.shape[1] != D or bases.shape[2] < 1:
        raise ValueError('nmf2d: bases {}: expected ({}, {}, R) for x {}, spatial = {}, S = {}'.format(
            tuple(bases.shape), G, D, tuple(x.shape), bool(spatial), S))
    if int(steps) < 0:
        raise ValueError('nmf2d: steps = {}: must be at least 0'.format(steps))
    if out is None:
        out = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != tuple(x.shape):
        raise ValueError('nmf2d: out {}: expected x\'s shape {}'.format(tuple(out.shape), tuple(x.shape)))
    xs, outs = paired_views('nmf2d', x, out, spatial, S)
    bases = bases.detach().contiguous()
    for (g0, xv), (_, ov) in zip(xs, outs):
        factorise(xv.detach(), bases[g0:g0 + xv.shape[0]], steps, ov)
    return out


def draw_bases(G, D, R):
    """the reference's draw (ham.py:233-237) on the HOST: torch.rand((G, D, R)) from the global CPU generator, float32, not
    yet normalised"""
    return torch.rand((int(G), int(D), int(R)))


def normalise_bases(bases):
    """L2-normalise along D (F.normalize(bases, dim=1), ham.py:239): one torch op on the device"""
    return torch.nn.functional.normalize(bases, dim=1)
