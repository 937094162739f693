"""Restatement of the reference's HamNet head (lib/models/pose_hrnet_hamburger.py:56-84, hamburger/burger.py:183-201
HamburgerV2Plus, hamburger/ham.py:63-110 and :244-269 NMF2D in eval mode, hamburger/bread.py ConvBNReLU) in plain torch
tensor ops, in the dtype of its inputs: the CPU yardstick of the HIP path. It follows the reference's own route - NCHW,
view / transpose, bmm - so it shares nothing with the device path's NHWC layout and strided reads.

fill_state_dict(keys_and_shapes, seed) draws every tensor from numpy.random.RandomState(seed) in SORTED key order, so no
weights are stored anywhere: BatchNorm running variances in [0.5, 2) and about a third of the gammas negative, non-zero
biases, coef_ham and coef_shortcut in [0.5, 1.5) (the reference's ZERO_HAM start, coef_ham = 0, would hide the whole ham).

err = rel(dev, ref64) = max|dev - ref64| / max|ref64|; a device result must stay within bound(e_ref) =
4 * e_ref + 2 * 2^-24, e_ref being the same measure of this restatement run in float32 on the CPU.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from swin_ref import bound, rel, to_torch  # noqa: F401  (the error rule is the project's one)

SEED = 20261019
EPS = 1e-6
ALIGN = 256
# cin: feature channels; size: feature map; emb: MODEL.EMB_DIM; R, S, steps (EVAL_STEPS), dual (DUAL_HAM), spatial (SPATIAL,
# read without dual), cheese (CHEESE_FACTOR)
CASE_A = dict(cin=480, size=(16, 16), emb=32, R=16, S=1, dual=True, spatial=True, cheese=1, steps=6, batch=2, joints=21)
CASE_B = dict(cin=480, size=(5, 7), emb=24, R=8, S=1, dual=True, spatial=True, cheese=1, steps=6, batch=1, joints=21)
CASE_C = dict(cin=480, size=(8, 8), emb=16, R=48, S=2, dual=False, spatial=False, cheese=2, steps=6, batch=2, joints=21)
FULL = dict(cin=480, size=(64, 64), emb=512, R=512, S=1, dual=True, spatial=True, cheese=1, steps=6, batch=1, joints=21)
CASES = dict(a=CASE_A, b=CASE_B, c=CASE_C)


# ---- the state dict ----------------------------------------------------------------------------------------------------
def channels(cfg):
    """(C of the hamburger, C / f after the cheese)"""
    c = cfg['S'] * cfg['emb'] * (2 if cfg['dual'] else 1)
    return c, c // (cfg['cheese'] * (2 if cfg['dual'] else 1))


def _bn(prefix, c):
    return [(prefix + 'weight', (c,)), (prefix + 'bias', (c,)), (prefix + 'running_mean', (c,)),
            (prefix + 'running_var', (c,)), (prefix + 'num_batches_tracked', ())]


def head_keys(cfg):
    """the state-dict entries of HamNet without backbone.*, in the reference's order, with shapes"""
    e, cin, j = cfg['emb'], cfg['cin'], cfg['joints']
    c, mid = channels(cfg)
    return ([('trainable_temp', ()), ('squeeze.conv.weight', (e, cin, 3, 3))] + _bn('squeeze.bn.', e) +
            [('hamburger.coef_shortcut', (1,)), ('hamburger.coef_ham', (1,)),
             ('hamburger.lower_bread.0.weight', (c, e, 1, 1)), ('hamburger.lower_bread.0.bias', (c,)),
             ('hamburger.cheese.conv.weight', (mid, c, 1, 1))] + _bn('hamburger.cheese.bn.', mid) +
            [('hamburger.upper_bread.weight', (e, mid, 1, 1)), ('align.conv.weight', (ALIGN, e, 3, 3))] +
            _bn('align.bn.', ALIGN) + [('fc.1.weight', (j, ALIGN, 1, 1)), ('fc.1.bias', (j,))])


def fill_state_dict(keys_and_shapes, seed=SEED):
    """numpy arrays (float64; num_batches_tracked int64) drawn from numpy.random.RandomState(seed) in SORTED key order:
    convolutions N(0, 1 / sqrt(fan_in)); biases N(0, 0.1); BatchNorm: |gamma| U(0.5, 1.5) with a third negative, beta
    N(0, 0.2), running_mean N(0, 0.3), running_var U(0.5, 2); coef_ham, coef_shortcut U(0.5, 1.5); trainable_temp
    U(0.8, 1.5)."""
    rng = np.random.RandomState(seed)
    bn = {k.rsplit('.', 1)[0] for k, _ in keys_and_shapes if k.endswith('running_var')}
    out = {}
    for key, shape in sorted(keys_and_shapes):
        shape = tuple(int(s) for s in shape)
        stem, leaf = key.rsplit('.', 1) if '.' in key else ('', key)
        if leaf == 'num_batches_tracked':
            v = np.zeros((), dtype=np.int64)
        elif key == 'trainable_temp':
            v = rng.uniform(0.8, 1.5, shape)
        elif leaf in ('coef_ham', 'coef_shortcut'):
            v = rng.uniform(0.5, 1.5, shape)
        elif stem in bn:
            if leaf == 'weight':
                v = rng.uniform(0.5, 1.5, shape) * np.where(rng.uniform(size=shape) < 1.0 / 3.0, -1.0, 1.0)
            elif leaf == 'running_var':
                v = rng.uniform(0.5, 2.0, shape)
            else:
                v = rng.normal(0.0, 0.3 if leaf == 'running_mean' else 0.2, shape)
        elif len(shape) == 4:
            v = rng.normal(0.0, 1.0 / math.sqrt(float(np.prod(shape[1:]))), shape)
        else:
            v = rng.normal(0.0, 0.1, shape)
        out[key] = v
    return out


def inputs(cfg, seed=SEED):
    """N(0, 1) rounded to float16 values (exact in every wider format; the fixture stores them as float16), float64"""
    rng = np.random.RandomState(seed + 1)
    return rng.normal(0.0, 1.0, (cfg['batch'], cfg['cin']) + tuple(cfg['size'])).astype(np.float16).astype(np.float64)


def ham_list(cfg):
    """[(spatial, first channel, channels)] in the reference's drawing order (burger.py:188-194)"""
    c, _ = channels(cfg)
    return [(True, 0, c // 2), (False, c // 2, c // 2)] if cfg['dual'] else [(bool(cfg['spatial']), 0, c)]


def bases_shapes(cfg, batch=None):
    B, hw = cfg['batch'] if batch is None else batch, cfg['size'][0] * cfg['size'][1]
    return [(B * cfg['S'], ch // cfg['S'] if spatial else hw, cfg['R']) for spatial, _, ch in ham_list(cfg)]


def draw_bases(cfg, seed, batch=None):
    """torch.rand in the reference's order after torch.manual_seed(seed): float32 CPU tensors, not normalised"""
    torch.manual_seed(seed)
    return [torch.rand(shape) for shape in bases_shapes(cfg, batch)]


# ---- the ops -----------------------------------------------------------------------------------------------------------
def product(X, bases):
    """X (G, D, N), bases (G, D, R) -> X^T bases (G, N, R) (ham.py:51)"""
    return torch.bmm(X.transpose(1, 2), bases)


def gram(a):
    return torch.bmm(a.transpose(1, 2), a)


def update(t, f, xop, gm, eps=EPS):
    """t * (xop f) / (t gm + eps) (ham.py:246-257)"""
    return t * torch.bmm(xop, f) / (torch.bmm(t, gm) + eps)


def update_coef(coef, bases, X, eps=EPS):
    return update(coef, bases, X.transpose(1, 2), gram(bases), eps)


def update_bases(bases, coef, X, eps=EPS):
    return update(bases, coef, X, gram(coef), eps)


def normalise(bases):
    """F.normalize(bases, dim=1) (ham.py:239)"""
    return bases / bases.norm(dim=1, keepdim=True).clamp_min(1e-12)


def factorise(X, bases, steps):
    """X (G, D, N), normalised bases (G, D, R) -> bases coef^T (G, D, N) (ham.py:49-58, :87-93)"""
    coef = torch.softmax(product(X, bases), dim=-1)
    for _ in range(steps):
        coef = update_coef(coef, bases, X)
        bases = update_bases(bases, coef, X)
    coef = update_coef(coef, bases, X)
    return torch.bmm(bases, coef.transpose(1, 2))


def nmf2d(x, bases, steps, spatial, S):
    """NMF2D.forward in eval mode on given, normalised bases: x (B, C, H, W) NCHW (ham.py:63-99)"""
    B, C, H, W = x.shape
    if spatial:
        X = x.reshape(B * S, C // S, H * W)
    else:
        X = x.reshape(B * S, C // S, H * W).transpose(1, 2)
    out = factorise(X, bases, steps)
    return (out if spatial else out.transpose(1, 2)).reshape(B, C, H, W)


def conv_bn_relu(x, P, prefix, eps=1e-5):
    w = P[prefix + 'conv.weight']
    y = F.conv2d(x, w, padding=w.shape[2] // 2)
    n = prefix + 'bn.'
    y = (y - P[n + 'running_mean'].reshape(1, -1, 1, 1)) / torch.sqrt(P[n + 'running_var'].reshape(1, -1, 1, 1) + eps)
    return torch.relu(y * P[n + 'weight'].reshape(1, -1, 1, 1) + P[n + 'bias'].reshape(1, -1, 1, 1))


def burger(x, P, cfg, bases):
    """HamburgerV2Plus.forward (burger.py:183-201); bases: one tensor per ham, not normalised"""
    h = 'hamburger.'
    y = torch.relu(F.conv2d(x, P[h + 'lower_bread.0.weight'], P[h + 'lower_bread.0.bias']))
    parts = [nmf2d(y[:, c0:c0 + ch], normalise(b.to(y.dtype)), cfg['steps'], spatial, cfg['S'])
             for (spatial, c0, ch), b in zip(ham_list(cfg), bases)]
    y = conv_bn_relu(torch.cat(parts, dim=1), P, h + 'cheese.')
    y = F.conv2d(y, P[h + 'upper_bread.weight'])
    return torch.relu(P[h + 'coef_ham'] * y + P[h + 'coef_shortcut'] * x)


def head(x, P, cfg, bases):
    """NCHW features -> heat maps (B, J, h, w) (pose_hrnet_hamburger.py:73-82)"""
    y = conv_bn_relu(x, P, 'squeeze.')
    y = burger(y, P, cfg, bases)
    y = conv_bn_relu(y, P, 'align.')
    y = F.conv2d(y, P['fc.1.weight'], P['fc.1.bias'])
    return torch.softmax(y.flatten(2) * P['trainable_temp'], dim=2).reshape(y.shape)


def run(cfg, dtype, bases, seed=SEED, x=None):
    """the case's heat maps as a float64 numpy array; bases: float32 tensors or arrays, not normalised"""
    P = to_torch(fill_state_dict(head_keys(cfg), seed), dtype)
    x = torch.tensor(inputs(cfg, seed) if x is None else np.asarray(x), dtype=dtype)
    with torch.no_grad():
        y = head(x, P, cfg, [torch.as_tensor(np.asarray(b)) for b in bases])
    return y.double().numpy()
