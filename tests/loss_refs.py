"""Float64 references of the small kernels of csrc/loss.hip, the bounds they are compared under and the inputs of
tests/test_loss_kernels_gpu.py. Nothing here imports GPU code: tests/test_loss_refs_cpu.py pins the references to the
fixtures and the oracle the project already trusts, and checks the planted inputs, on a machine without a GPU.

Every reference is written once over torch tensors and runs in the dtype of its inputs: in float64 it is the reference,
in float32 it is "the same operation run by torch in float32", whose deviation from the float64 run (dev32) sets the
bound (tests/test_structure_loss_gpu.py's convention):

    max |ours - ref64| <= max(2 * dev32, floor) * max |ref64|          element-wise outputs, floor = 4 * 2^-24
    |ours - ref64|     <= max(2 * dev32, floor) * sum |terms|          a reduced scalar, floor = sum_floor(n, ...)

and never looser than what tests/test_kernels_gpu.py asks of the same kernel (the `cap` arguments below).

Planted elements: every input of a reduction carries, at planted_indices(n) - index 0, the last index and the three
indices around every multiple of 64 (so of 256 too) - a term so large that losing or doubling it moves the result by
at least 100 times the bound. A wrong stride, a dropped tail or a wave boundary counted twice cannot hide in the noise.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24                       # unit roundoff of float32
FLOOR = 4 * U
PER_MAP_SHAPES = [(1, 1), (1, 63), (8, 8), (5, 13), (13, 5), (15, 17), (16, 16), (1, 257), (257, 1), (64, 48), (64, 64)]
PER_MAP_BK = (1, 3, 257)


def sum_floor(n, per_term):
    """relative floor (of sum |terms|) for a float32 sum of n terms.

    Any summation of n terms makes n - 1 additions, and however they are arranged some term passes through at least
    ceil(log2 n) of them (the balanced tree is the shallowest arrangement). Each addition rounds a partial sum that is
    at most sum |terms| by at most 2^-24 of it, so ceil(log2 n) * 2^-24 * sum |terms| is the worst case of the best
    possible order; no kernel is asked for less. per_term counts the roundings made on every term before it is added
    and on the result after the sum (a difference, a product, a square root, the final division)."""
    return (math.ceil(math.log2(max(int(n), 2))) + per_term) * U


def planted_indices(n):
    idx = {0, n - 1}
    for m in range(64, n + 1, 64):
        idx.update((m - 1, m, m + 1))
    return np.array(sorted(i for i in idx if 0 <= i < n), dtype=np.int64)


def assert_planted(terms, idx, bound_rel, what):
    """terms: the float64 terms of one reduction (1-D). Losing or doubling terms[i] moves the sum by |terms[i]|; each
    planted one must be worth 100 bounds, the bound being bound_rel * sum |terms|"""
    terms = np.abs(np.asarray(terms, dtype=np.float64)).ravel()
    need = 100.0 * bound_rel * terms.sum()
    least = terms[idx].min()
    assert least >= need and least > 0, '{}: planted term {:.3e} < 100 bounds = {:.3e}'.format(what, least, need)
    return least / max(terms.sum(), 1e-300)


# ---- bounds ---------------------------------------------------------------------------------------------------------

def _f64(a):
    return a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)


def elementwise_allowed(ref64, ref32, floor=FLOOR, cap=None, per_row=False, scale=None):
    """(allowed absolute error, dev32) of an element-wise output; cap = the absolute bound of the older test.
    per_row: every row of a 2-D output is a quantity of its own, with its own scale and dev32 (arrays come back).
    scale: what the errors are relative to, max |ref64| unless the caller has a reason for another (one per row)"""
    ref64, ref32 = _f64(ref64), _f64(ref32)
    if not per_row:
        ref64, ref32 = ref64.reshape(1, -1), ref32.reshape(1, -1)
    if scale is not None:
        scale = _f64(scale).reshape(ref64.shape[0])
    else:
        scale = np.abs(ref64).max(1) if ref64.shape[1] else np.zeros(ref64.shape[0])
    dev32 = np.abs(ref32 - ref64).max(1) / np.where(scale > 0, scale, 1.0) if ref64.shape[1] else scale
    allowed = np.maximum(2 * dev32, floor) * scale
    if cap is not None:
        allowed = np.minimum(allowed, cap)
    return (allowed, dev32) if per_row else (float(allowed[0]), float(dev32[0]))


def check(name, ours, ref64, ref32, floor=FLOOR, cap=None, per_row=False, scale=None):
    """element-wise output against the float64 reference; prints the measured figure next to its bound (of the row
    that comes closest to its bound when every row has its own)"""
    ours, r64 = _f64(ours), _f64(ref64)
    assert ours.shape == r64.shape, (name, ours.shape, r64.shape)
    assert np.isfinite(ours).all(), (name, 'non-finite output')
    allowed, dev32 = elementwise_allowed(r64, ref32, floor, cap, per_row, scale)
    if per_row:
        errs = np.abs(ours - r64).max(1)
        k = int(np.argmax(errs - allowed))
        err, bound, dev = float(errs[k]), float(allowed[k]), float(dev32[k])
        ok = bool((errs <= allowed).all())
    else:
        err, bound, dev = (float(np.abs(ours - r64).max()) if r64.size else 0.0), allowed, dev32
        ok = err <= bound
    print('{:58s} abs err {:.3e} bound {:.3e} (dev32 {:.2e})'.format(name, err, bound, dev))
    assert ok, (name, err, bound)
    return err


def sums_allowed(ref64, ref32, abs_terms, floor, cap=None):
    """allowed absolute error of each reduced scalar: max(2 dev32, floor) * sum |terms| (abs_terms, already divided as
    the result is), capped by the older test's absolute bound"""
    r64, r32, s = _f64(ref64), _f64(ref32), _f64(abs_terms)
    allowed = np.maximum(2 * np.abs(r32 - r64), floor * s)
    return allowed if cap is None else np.minimum(allowed, _f64(cap))


def check_sums(name, ours, ref64, ref32, abs_terms, floor, cap=None):
    """reduced scalars (one or a vector, each held to its own bound); prints the worst one relative to sum |terms|"""
    ours, r64, s = _f64(ours).ravel(), _f64(ref64).ravel(), _f64(abs_terms).ravel()
    assert ours.shape == r64.shape == s.shape, (name, ours.shape, r64.shape, s.shape)
    assert np.isfinite(ours).all(), (name, 'non-finite output')
    allowed = sums_allowed(r64, _f64(ref32).ravel(), s, floor, None if cap is None else _f64(cap).ravel())
    err = np.abs(ours - r64)
    k = int(np.argmax(err - allowed))
    den = s[k] if s[k] > 0 else 1.0
    print('{:58s} rel err {:.3e} bound {:.3e} (of sum|terms|, worst of {})'.format(name, err[k] / den, allowed[k] / den,
                                                                                  ours.size))
    assert (err <= allowed).all(), (name, k, err[k], allowed[k])
    return err[k] / den


def same_bits(a, b):
    a, b = np.ascontiguousarray(_f32(a)), np.ascontiguousarray(_f32(b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _f32(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _grad(fn, x, gout):
    x = x.detach().clone().requires_grad_(True)
    y = fn(x)
    y.backward(torch.as_tensor(gout, dtype=y.dtype).reshape(y.shape))
    return x.grad


# ---- references (torch, in the dtype of their inputs) ---------------------------------------------------------------

def heatmap_terms(pred, gt, mode):
    d = pred - gt
    return d * d if mode == 0 else d.abs()


def heatmap_loss(pred, gt, mode):
    """pred, gt [BK, HW] -> (per-map sums [BK], their mean)"""
    partial = heatmap_terms(pred, gt, mode).sum(-1)
    return partial, partial.sum() / pred.shape[0]


def heatmap_loss_grad(pred, gt, mode, gout):
    """d (gout * loss) / d pred; torch's abs has sign(0) = 0"""
    return _grad(lambda p: heatmap_loss(p, gt, mode)[1], pred, gout)


def joints_terms(pred, gt, vis):
    n = torch.norm(pred - gt, dim=-1)
    return n if vis is None else n * vis


def joints_loss(pred, gt, vis):
    """pred, gt [B, K, 2]; vis [B, K] of any real weights or None: sum(norm * vis) / max(1, sum vis), or sum / K"""
    s = joints_terms(pred, gt, vis).sum()
    return s / pred.shape[1] if vis is None else s / torch.clamp(vis.sum(), min=1.0)


def joints_denominator(pred, vis):
    return float(pred.shape[1]) if vis is None else max(1.0, float(vis.double().sum()))


def joints_loss_grad(pred, gt, vis, gout):
    """torch.norm's backward is 0 at a zero difference"""
    return _grad(lambda p: joints_loss(p, gt, vis), pred, gout)


def decode_expectation(hms):
    """hms [BK, H, W] -> [BK, 2] = (sum h * x, sum h * y), x the column, y the row"""
    xs = torch.arange(hms.shape[2], dtype=hms.dtype)
    ys = torch.arange(hms.shape[1], dtype=hms.dtype)
    return torch.stack(((hms * xs[None, None, :]).sum((1, 2)), (hms * ys[None, :, None]).sum((1, 2))), dim=1)


def decode_expectation_abs_terms(hms):
    return decode_expectation(hms.abs())


def decode_expectation_grad(gpreds, h, w):
    """gpreds [BK, 2] -> d sum(gpreds * preds) / d hms [BK, H, W], by autograd through the forward"""
    z = torch.zeros(gpreds.shape[0], h, w, dtype=gpreds.dtype)
    return _grad(lambda m: (decode_expectation(m) * gpreds).sum(), z, 1.0)


def decode_argmax(hms, inference_style):
    """hms numpy [BK, H, W] -> (preds [BK, 2] float32, maxima [BK]). numpy.argmax: the first maximal flat index, a NaN
    counts as maximal. Training style takes % H and // H, inference style % W and // W and zeroes where max is not > 0"""
    hms = np.asarray(hms)
    bk, h, w = hms.shape
    flat = hms.reshape(bk, -1)
    idx = np.argmax(flat, axis=1)
    mx = flat[np.arange(bk), idx]
    d = w if inference_style else h
    preds = np.stack((idx % d, idx // d), axis=1).astype(np.float32)
    if inference_style:
        preds[~(mx > 0)] = 0.0
    return preds, mx


def softmax(x, t):
    """x [BK, HW], t a 0-d tensor of x's dtype"""
    return torch.softmax(x * t, dim=-1)


def softmax_grads(x, t, gout):
    """(out, dx, dtemp per map): the temperature gets one copy per map so that autograd keeps the maps' shares apart"""
    xr = x.detach().clone().requires_grad_(True)
    tv = t.detach().reshape(1).expand(x.shape[0]).clone().requires_grad_(True)
    out = torch.softmax(xr * tv[:, None], dim=-1)
    out.backward(gout)
    return out.detach(), xr.grad, tv.grad


def softmax_dtemp_abs_terms(x, out, gout):
    """dtemp = sum_i out_i (g_i - dot) x_i with dot = sum_j g_j out_j: written out it is the sum of the 2 HW terms
    out_i g_i x_i and -dot out_i x_i, and their absolute sum is what its rounding errors scale with"""
    dot = (gout * out).sum(-1, keepdim=True)
    return (out * gout * x).abs().sum(-1) + (dot * out * x).abs().sum(-1)


def adam_step(p, g, m, v, step, lr, b1, b2, eps, wd, gscale):
    """one Adam step with L2 weight decay added to the scaled gradient (torch.optim.Adam) from the state (p, m, v)
    that step - 1 steps left; torch tensors or numpy arrays, hyper-parameters python floats. -> (p, m, v)"""
    gi = g * gscale + wd * p
    m2 = b1 * m + (1.0 - b1) * gi
    v2 = b2 * v + (1.0 - b2) * gi * gi
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = v2 ** 0.5 / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m2 / denom), m2, v2


def f32(x):
    """the float32 value a C `float` argument takes, as a python float"""
    return float(np.float32(x))


def normalize_u8(img, mean, std, dtype):
    """img uint8 [N, H, W, 3], mean / std three floats -> [N, 3, H, W] = (v / 255 - mean) / std"""
    x = img.to(dtype) / 255.0
    m, s = torch.tensor(mean, dtype=dtype), torch.tensor(std, dtype=dtype)
    return ((x - m) / s).permute(0, 3, 1, 2).contiguous()


# ---- inputs ---------------------------------------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def heatmap_case(bk, hw, seed=0):
    """pred, gt float32 [bk, hw]: differences of ~0.1, +-3 at the planted indices of a map, the planted maps 1.5 times
    as large, and exact zeros of pred - gt (L1 gradient 0) at every index 7 mod 11 that is not planted"""
    rng = _rng(1, bk, hw, seed)
    gt = rng.random((bk, hw)).astype(np.float32)
    d = (rng.standard_normal((bk, hw)) * 0.1).astype(np.float32)
    pi = planted_indices(hw)
    d[:, pi] = np.where(np.arange(len(pi)) % 2 == 0, 3.0, -3.0).astype(np.float32)
    d[planted_indices(bk)] *= 1.5
    zeros = np.setdiff1d(np.arange(7, hw, 11), pi)
    d[:, zeros] = 0.0
    pred = (gt + d).astype(np.float32)
    pred[:, zeros] = gt[:, zeros]
    return pred, gt, zeros


JOINTS_SHAPES = [(1, 1), (1, 21), (5, 51), (16, 16), (1, 257), (16, 21), (37, 21)]     # B * K = 1 ... 777
JOINTS_VIS = ('none', 'mixed', 'zero', 'frac')


def joints_case(b, k, vis_mode, seed=0):
    """pred, gt [b, k, 2], vis [b, k] or None: errors of ~1 pixel, ~25 pixels at the planted points (which are visible
    with weight 1 in the 'mixed' case), pred == gt at every point 5 mod 9 that is not planted"""
    rng = _rng(2, b, k, JOINTS_VIS.index(vis_mode), seed)
    n = b * k
    gt = (rng.random((n, 2)) * 64).astype(np.float32)
    d = rng.standard_normal((n, 2)).astype(np.float32)
    pi = planted_indices(n)
    ang = rng.random(len(pi)) * 2 * np.pi
    d[pi] = (25.0 * np.stack((np.cos(ang), np.sin(ang)), 1)).astype(np.float32)
    zeros = np.setdiff1d(np.arange(5, n, 9), pi)
    pred = (gt + d).astype(np.float32)
    pred[zeros] = gt[zeros]
    if vis_mode == 'none':
        vis = None
    elif vis_mode == 'mixed':
        vis = (rng.random(n) < 0.6).astype(np.float32)
        vis[pi] = 1.0
    elif vis_mode == 'zero':
        vis = np.zeros(n, np.float32)
    else:
        vis = (0.25 + 0.75 * rng.random(n)).astype(np.float32)
    return pred.reshape(b, k, 2), gt.reshape(b, k, 2), None if vis is None else vis.reshape(b, k), zeros


def expectation_case(bk, h, w, seed=0):
    """maps [bk, h, w] of ~1e-3 .. 1e-2 with 0.2 at the planted flat indices (index 0 has x = y = 0: it is planted all
    the same, a kernel that doubles it is caught at index 1 of the next stripe)"""
    rng = _rng(3, bk, h, w, seed)
    hm = (rng.random((bk, h * w)) * 0.01 + 0.001).astype(np.float32)
    hm[:, planted_indices(h * w)] = 0.2
    return hm.reshape(bk, h, w)


SOFTMAX_TEMPS = (1.0, 1.7, 0.01, 50.0, -2.0)
ROW_PLAIN, ROW_SHIFTED, ROW_EQUAL, ROW_ONE_HOT = 0, 1, 2, 3


def softmax_row_kinds(bk, shape_index):
    """row 0 is always a plain planted row; the others go round shifted / all-equal / near-one-hot / plain, starting
    at a kind that depends on the shape so that BK = 3 sees all of them over the shapes"""
    cycle = (ROW_SHIFTED, ROW_EQUAL, ROW_ONE_HOT, ROW_PLAIN)
    return np.array([ROW_PLAIN] + [cycle[(k + shape_index) % 4] for k in range(bk - 1)])


def softmax_case(bk, hw, temp, shape_index=0, seed=0):
    """x, gout float32 [bk, hw]. The logits z = x * temp: plain rows are N(0, 1) with 2.5 at the planted indices (each
    then holds > 1e-3 of the row's mass); shifted rows are plain rows moved to +1e4 or -1e4 with every 5th unplanted
    logit at -1e4 or below (exp overflows or the row sums to 0 without the max subtraction); all-equal rows; near-one-hot rows (one logit
    12 above the rest). gout is N(0, 1), +-1.5 at the planted indices"""
    rng = _rng(4, bk, hw, int(round(abs(temp) * 100)), seed)
    z = rng.standard_normal((bk, hw))
    pi = planted_indices(hw)
    z[:, pi] = 2.5
    kinds = softmax_row_kinds(bk, shape_index)
    for r in range(bk):
        if kinds[r] == ROW_SHIFTED:
            low = np.setdiff1d(np.arange(3, hw, 5), pi)
            up = r % 2 == 1
            z[r] += 1e4 if up else -1e4
            z[r, low] = -1e4 if up else -1e4 - 60.0
        elif kinds[r] == ROW_EQUAL:
            z[r] = 0.75
        elif kinds[r] == ROW_ONE_HOT:
            z[r] = rng.standard_normal(hw)
            z[r, (r * 37) % hw] += 12.0
    x = (z / temp).astype(np.float32)
    g = rng.standard_normal((bk, hw))
    g[:, pi] = np.where(np.arange(len(pi)) % 2 == 0, 1.5, -1.5)
    return x, g.astype(np.float32), kinds


ARGMAX_SCENARIOS = ('plain', 'one_nan', 'nan_other_stripe', 'two_nans', 'all_nan', 'all_neg_inf', 'pos_inf', 'all_equal',
                    'tie_next', 'tie_64', 'tie_256', 'tie_cross', 'never_positive', 'all_zero', 'neg_zero_tie')


def argmax_case(bk, h, w, seed=0):
    """maps [bk, h, w]; map k holds scenario k mod 15 (ARGMAX_SCENARIOS), 'plain' where the map is too small for it.
    Ties are placed at i > 0: (i, i+1) neighbouring threads, (i, i+64) neighbouring waves, (i, i+256) one thread's
    first and second element, and 'tie_cross' (i+1, i+256): the lower flat index sits in the HIGHER thread"""
    rng = _rng(5, bk, h, w, seed)
    hw = h * w
    hm = rng.standard_normal((bk, hw)).astype(np.float32)
    names = []
    for k in range(bk):
        s = ARGMAX_SCENARIOS[k % len(ARGMAX_SCENARIOS)]
        m = hm[k]
        i = 1 + int(rng.integers(0, max(1, min(hw - 1, 200))))          # 1 .. 200
        top = np.float32(5.0 + rng.random())
        done = True
        if s == 'one_nan' and hw > 1:
            m[int(rng.integers(1, hw))] = np.nan
        elif s == 'nan_other_stripe' and hw > 2:
            q = int(rng.integers(0, hw - 1))
            m[q] = 100.0                                                # a finite maximum earlier, in another thread
            m[q + 1 + int(rng.integers(0, min(hw - q - 1, 255)))] = np.nan
        elif s == 'two_nans' and hw > 2:
            a, b = sorted(rng.choice(hw, 2, replace=False))
            m[a] = m[b] = np.nan
        elif s == 'all_nan':
            m[:] = np.nan
        elif s == 'all_neg_inf':
            m[:] = -np.inf
        elif s == 'pos_inf' and hw > 1:
            m[int(rng.integers(1, hw))] = np.inf
        elif s == 'all_equal':
            m[:] = 0.5
        elif s == 'tie_next' and i + 1 < hw:
            m[i] = m[i + 1] = top
        elif s == 'tie_64' and i + 64 < hw:
            m[i] = m[i + 64] = top
        elif s == 'tie_256' and i + 256 < hw:
            m[i] = m[i + 256] = top
        elif s == 'tie_cross' and i + 256 < hw:
            m[i + 1] = m[i + 256] = top
        elif s == 'never_positive':
            m[:] = -np.abs(m) - 0.01
        elif s == 'all_zero':
            m[:] = 0.0
        elif s == 'neg_zero_tie' and hw > 2:
            m[:] = -np.abs(m) - 0.01
            m[hw - 1] = 0.0
            m[hw // 2] = -0.0                                           # -0 == +0: the first of the two wins
        else:
            done = s == 'plain'
        names.append(s if done else 'plain')
    return hm.reshape(bk, h, w), names


def targets_case(bk, h, w, seed=0):
    """pose [bk, 2], vis [bk] (<= 0, fractional > 0 and 1): the four corners, coordinates in (-1, 0) (int() puts them at
    0, on the map), exactly w / h (off the map), w - 0.01, far outside, between min(h, w) and max(h, w) (on the map in
    one direction only), and uniform ones over a frame of 8 pixels around the map"""
    rng = _rng(6, bk, h, w, seed)
    special = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (-0.7, 3.2), (3.2, -0.7), (-0.7, -0.99), (w, 2), (2, h),
               (w - 0.01, h - 0.01), (w - 0.01, 0.5), (1e4, 1e4), (-1e4, 5), (5, -1e4), (min(h, w) + 1.5, min(h, w) + 1.5),
               (max(h, w) - 1, 1), (1, max(h, w) - 1), (-1.0, 4), (4, -1.0), (0.999, 0.001)]
    pose = np.stack((rng.random(bk) * (w + 16) - 8, rng.random(bk) * (h + 16) - 8), 1)
    vis = np.ones(bk)
    for k in range(bk):
        if k < len(special) or bk == 1:
            pose[k] = special[(k + seed) % len(special)]
        else:
            vis[k] = (1.0, 0.3, 0.0, -1.0, 1e-6, 2.5)[k % 6]
    return pose.astype(np.float32), vis.astype(np.float32)


U8_CASES = [(1, 1, 1), (3, 5, 17), (1, 1, 257), (3, 16, 16), (1, 1, 2097153)]          # N * H * W = 1, 255, 257, 768, 2^21 + 1
U8_CONSTANTS = (((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), ((0.1, 0.5, 0.9), (0.5, 1.7, 0.3)))


def u8_case(n, h, w):
    """uint8 [n, h, w, 3]: channel c of pixel p holds (p + 85 c + p // 256) mod 256, every byte value in each channel
    once 256 pixels are there, and no channel equal to another"""
    p = np.arange(n * h * w, dtype=np.int64)
    img = np.stack([(p + 85 * c + p // 256) % 256 for c in range(3)], 1).astype(np.uint8)
    return img.reshape(n, h, w, 3)


ADAM_BETAS_EPS = (0.9, 0.999, 1e-8)
ADAM_POOL = 509                                   # prime: a tiled state repeats at no power-of-two stride
_ADAM_WALKS = {}                                  # (grad_scale, weight_decay, lr) -> [steps made, p, m, v, snapshots]


def adam_pool_state(step, gscale, wd, lr):
    """(p, m, v) float64 [ADAM_POOL] after step - 1 float64 reference steps from p ~ N(0, 1), m = v = 0, the gradient of
    step t being row t mod 64 of a fixed N(0, 1) table with zero column means. One walk per (gscale, wd, lr), continued when a later step is
    asked for; the hyper-parameters are the float32 values the C ABI receives"""
    b1, b2, eps = (f32(x) for x in ADAM_BETAS_EPS)
    rng = _rng(7, 0)
    p0 = rng.standard_normal(ADAM_POOL)
    table = rng.standard_normal((64, ADAM_POOL))
    table -= table.mean(0)          # no net gradient over a cycle: p stays O(1), where float32 still resolves 1e-6
    walk = _ADAM_WALKS.setdefault((gscale, wd, lr), [0, p0, np.zeros(ADAM_POOL), np.zeros(ADAM_POOL), {1: None}])
    if walk[4].get(1) is None:
        walk[4][1] = (p0.copy(), walk[2].copy(), walk[3].copy())
    while walk[0] < step - 1:
        t = walk[0] + 1
        walk[1], walk[2], walk[3] = adam_step(walk[1], table[t % 64], walk[2], walk[3], t, f32(lr), b1, b2, eps, f32(wd),
                                              f32(gscale))
        walk[0] = t
        if t + 1 in (2, 1000, 100000) or t + 1 == step:
            walk[4][t + 1] = (walk[1].copy(), walk[2].copy(), walk[3].copy())
    return walk[4][step]


def adam_case(n, step, gscale, wd, lr, seed=0):
    """float32 (p, g, m, v) [n]: the pool state tiled over n, a fresh N(0, 1) gradient, and at every index 3 mod 7 other
    than the first and the last a zero gradient with zero moments (with wd = 0 the denominator there is eps alone)"""
    rng = _rng(8, n, step, seed)
    pp, pm, pv = (a.astype(np.float32) for a in adam_pool_state(step, gscale, wd, lr))
    reps = -(-n // ADAM_POOL)
    p, m, v = (np.tile(a, reps)[:n].copy() for a in (pp, pm, pv))
    g = rng.standard_normal(n, dtype=np.float32)
    g[0], g[n - 1] = 1.5, -1.5                      # the ends move by far more than any bound
    z = np.arange(3, n - 1, 7)
    g[z] = 0.0
    m[z] = 0.0
    v[z] = 0.0
    return p, g, m, v, z


# ---- what a kernel has to give for one input: (ref64, ref32, sum |terms|, floor[, cap]) per compared quantity -------

def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def heatmap_expected(pred, gt, mode):
    """the per-map sums (each a sum of HW terms: a difference and, for L2, a square before the sum -> 2 roundings) and
    the loss (BK * HW terms, and the division by BK -> 3). The older test holds the loss to 1e-5 of itself"""
    bk, hw = pred.shape
    p64, g64, p32, g32 = _t(pred, torch.float64), _t(gt, torch.float64), _t(pred, torch.float32), _t(gt, torch.float32)
    part64, loss64 = heatmap_loss(p64, g64, mode)
    part32, loss32 = heatmap_loss(p32, g32, mode)
    terms = heatmap_terms(p64, g64, mode)
    return {'terms': terms.numpy(),
            'partial': (part64, part32, terms.sum(-1), sum_floor(hw, 2)),
            'loss': (loss64, loss32, terms.sum() / bk, sum_floor(bk * hw, 3), 1e-5 * abs(float(loss64)))}


def joints_expected(pred, gt, vis):
    """the loss: B * K terms, each a difference, a two-term sum of squares (2), a square root and a weight (2) -> 5, the
    division (1), and the denominator's own sum of B * K weights, which scales the result (ceil(log2 n) more).
    The older test holds it to 1e-5 * max(loss, 1)"""
    n = pred.shape[0] * pred.shape[1]
    a64 = [_t(a, torch.float64) for a in (pred, gt, vis)]
    a32 = [_t(a, torch.float32) for a in (pred, gt, vis)]
    loss64, loss32 = joints_loss(*a64), joints_loss(*a32)
    terms = joints_terms(*a64)
    den = joints_denominator(a64[0], a64[2])
    floor = sum_floor(n, 6) + (sum_floor(n, 0) if vis is not None else 0.0)
    return {'terms': terms.numpy().ravel(), 'denominator': den,
            'loss': (loss64, loss32, terms.abs().sum() / den, floor, 1e-5 * max(abs(float(loss64)), 1.0))}


def expectation_expected(hm):
    """each coordinate a sum of H * W products h * x (1 rounding each; fused in the kernel). The older test: 1e-5 of
    the largest coordinate"""
    h64, h32 = _t(hm, torch.float64), _t(hm, torch.float32)
    ref64, ref32 = decode_expectation(h64), decode_expectation(h32)
    cap = torch.full_like(ref64, 1e-5 * float(ref64.abs().max()))
    return {'preds': (ref64, ref32, decode_expectation_abs_terms(h64), sum_floor(hm.shape[1] * hm.shape[2], 1), cap)}


def softmax_expected(x, gout, temp):
    """out (every map a quantity of its own; older test: 1e-6 absolute); every row sum of out, a sum of HW terms each
    rounded by the exp and the normalisation (2); dtemp per map (softmax_dtemp_abs_terms: 2 HW terms of three factors,
    their `dot` and `out` factors carrying the error of a sum of HW terms and of the forward: ceil(log2 2HW) +
    ceil(log2 HW) + 6).

    dx_i = t out_i (g_i - sum_j g_j out_j) is element-wise in name only: each element is a sum of the HW + 1 terms
    t out_i g_i and -t out_i g_j out_j, which cancel where out_i is near 1, and `out` reaches the backward kernel
    rounded to float32. With max |dx| as the scale and 4 * 2^-24 as the floor no float32 kernel can pass a map that
    is near one-hot: the float32 rounding of g_j out_j alone moves dx_j by |t| 2^-24 |g_j|, while max |dx| of the case
    (set by the plain rows, out <= 0.2) is about 0.4 |t|. So dx is held as reduced scalars are: every map relative to
    its largest sum |terms| = |t| max_i out_i (|g_i| + sum_j |g_j out_j|), floor sum_floor(HW + 1, 3) (two products
    before the sum and t after it), and never looser than the older test (1e-5 * max(1, max |dx|)). 'dx_plain' is the
    max |dx| / 4 * 2^-24 comparison, printed by the test next to it and not asserted"""
    hw = x.shape[1]
    out = {}
    for dt in (torch.float64, torch.float32):
        xs, gs, ts = _t(x, dt), _t(gout, dt), torch.tensor(f32(temp), dtype=dt)
        out[dt] = softmax_grads(xs, ts, gs)
    o64, dx64, dt64 = out[torch.float64]
    o32, dx32, dt32 = out[torch.float32]
    x64, g64 = _t(x, torch.float64), _t(gout, torch.float64)
    return {'out': (o64, o32, FLOOR, 1e-6, True), 'dx': (dx64, dx32, sum_floor(hw + 1, 3), 1e-5 * max(1.0, float(dx64.abs().max())), True,
                   abs(f32(temp)) * (o64 * (g64.abs() + (g64 * o64).abs().sum(-1, keepdim=True))).max(-1).values),
            'dx_plain': (dx64, dx32, FLOOR, None),
            'rowsum': (o64.sum(-1), o32.sum(-1), o64.sum(-1), sum_floor(hw, 2)),
            'dtemp': (dt64, dt32, softmax_dtemp_abs_terms(x64, o64, g64), sum_floor(2 * hw, 6) + sum_floor(hw, 0)),
            'mass': o64.numpy(), 'dot_terms': (g64 * o64).numpy(), 'dtemp_terms': (o64 * (g64 - (g64 * o64).sum(-1, keepdim=True)) * x64).numpy()}


ADAM_HYPER = dict(b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8))


def adam_expected(p, g, m, v, step, gscale, wd, lr):
    """(p, m, v) after the step, element-wise; the older test holds p to 1e-6 absolute. The hyper-parameters are the
    float32 values the C ABI receives, so both sides step with the same numbers"""
    res = {}
    for dt in (torch.float64, torch.float32):
        res[dt] = adam_step(_t(p, dt), _t(g, dt), _t(m, dt), _t(v, dt), step, f32(lr), ADAM_HYPER['b1'], ADAM_HYPER['b2'],
                            ADAM_HYPER['eps'], f32(wd), f32(gscale))
    (p64, m64, v64), (p32, m32, v32) = res[torch.float64], res[torch.float32]
    return {'p': (p64, p32, FLOOR, 1e-6), 'm': (m64, m32, FLOOR, None), 'v': (v64, v32, FLOOR, None)}
