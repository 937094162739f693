"""Restatement of the reference's HamNet head in TRAINING mode (lib/models/pose_hrnet_hamburger.py:56-84,
hamburger/burger.py:183-201, hamburger/ham.py:48-110 and :244-269, hamburger/bread.py ConvBNReLU on batch statistics) in
plain torch tensor ops, in the dtype of its inputs, differentiated by autograd on the CPU: the yardstick of the HIP training
path. It follows tests/hamburger_ref's route (NCHW, view / transpose, bmm) and shares its cases, state dicts and error
rule.

What training mode changes: every BatchNorm normalises with the batch mean and the biased batch variance and moves its
running statistics by momentum 3e-4 (the variance unbiased; num_batches_tracked is NOT incremented: the reference's
SyncBN calls F.batch_norm directly); Dropout2d multiplies by a given keep mask (B, 256) of values in {0, 1 / 0.9}; a ham
runs TRAIN_STEPS multiplicative updates under no_grad (ham.py:48-58) and only compute_coef and the closing bmm carry a
gradient (ham.py:90-93, :261-269).

ham_grad is that gradient in closed form: with bases_T, coef_T the factors after TRAIN_STEPS updates and Gm = bases_T^T
bases_T,   dnum = coef_T * (dY^T bases_T) / (coef_T Gm + 1e-6),   dX = bases_T dnum^T.

loss(): the mean over images and joints of the distance between the soft-argmax of a heat map and a seeded target.
"""
import numpy as np
import torch
import torch.nn.functional as F

import hamburger_ref as R
from hamburger_ref import bound, rel, to_torch  # noqa: F401

SEED = 11
TRAIN_STEPS = 6
MOMENTUM = 3e-4               # bread.py:17
DROP_P = 0.1
BN_PREFIXES = ('squeeze.bn.', 'hamburger.cheese.bn.', 'align.bn.')


def draw_keep(cfg, seed=SEED):
    """the keep mask of Dropout2d(0.1): (B, 256) float32 values in {0, 1 / 0.9}"""
    rng = np.random.RandomState(seed + 2)
    return ((rng.uniform(size=(cfg['batch'], R.ALIGN)) >= DROP_P) / (1.0 - DROP_P)).astype(np.float32)


def draw_targets(cfg, seed=SEED):
    """(B, J, 2) target positions (x, y) inside the map, float64"""
    rng = np.random.RandomState(seed + 3)
    h, w = cfg['size']
    return rng.uniform(0.0, 1.0, (cfg['batch'], cfg['joints'], 2)) * np.array([w - 1.0, h - 1.0])


def loss(hm, targets):
    """hm (B, J, h, w), targets (B, J, 2) -> mean distance between sum_p hm[p] * (x_p, y_p) and the target"""
    B, J, h, w = hm.shape
    ys, xs = torch.arange(h, dtype=hm.dtype), torch.arange(w, dtype=hm.dtype)
    px = (hm.sum(dim=2) * xs).sum(dim=2)
    py = (hm.sum(dim=3) * ys).sum(dim=2)
    return (torch.stack([px, py], dim=2) - targets).norm(dim=2).mean()


# ---- the hams ------------------------------------------------------------------------------------------------------------
def local_inference(X, bases, steps):
    """(bases_T, coef_T): ham.py:48-58, no gradient"""
    with torch.no_grad():
        X = X.detach()
        coef = torch.softmax(R.product(X, bases), dim=-1)
        for _ in range(steps):
            coef = R.update_coef(coef, bases, X)
            bases = R.update_bases(bases, coef, X)
    return bases, coef


def factorise_train(X, bases, steps):
    """X (G, D, N) with gradient, normalised bases (G, D, R) -> bases_T compute_coef(X, bases_T, coef_T)^T"""
    bases_T, coef_T = local_inference(X, bases, steps)
    coef = R.update_coef(coef_T, bases_T, X)               # compute_coef: the gradient enters through X^T bases_T alone
    return torch.bmm(bases_T, coef.transpose(1, 2))


def ham_grad(X, bases, steps, dY):
    """the closed-form gradient of factorise_train with respect to X for the output gradient dY (G, D, N)"""
    bases_T, coef_T = local_inference(X, bases, steps)
    gm = R.gram(bases_T)
    dnum = coef_T * torch.bmm(dY.transpose(1, 2), bases_T) / (torch.bmm(coef_T, gm) + R.EPS)
    return torch.bmm(bases_T, dnum.transpose(1, 2))


def group(x, spatial, S):
    B, C, H, W = x.shape
    X = x.reshape(B * S, C // S, H * W)
    return X if spatial else X.transpose(1, 2)


def ungroup(X, shape, spatial):
    return (X if spatial else X.transpose(1, 2)).reshape(shape)


def nmf2d_train(x, bases, steps, spatial, S):
    """NMF2D.forward in training mode on given, normalised bases: x (B, C, H, W) NCHW (ham.py:63-99)"""
    return ungroup(factorise_train(group(x, spatial, S), bases, steps), x.shape, spatial)


# ---- the head ------------------------------------------------------------------------------------------------------------
def conv_bn_relu_train(x, P, prefix, stats, eps=1e-5):
    w = P[prefix + 'conv.weight']
    y = F.conv2d(x, w, padding=w.shape[2] // 2)
    mean, var = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
    n = y.numel() // y.shape[1]
    stats[prefix + 'bn.'] = (mean.detach(), var.detach() * (n / (n - 1.0)))
    y = (y - mean.reshape(1, -1, 1, 1)) / torch.sqrt(var.reshape(1, -1, 1, 1) + eps)
    return torch.relu(y * P[prefix + 'bn.weight'].reshape(1, -1, 1, 1) + P[prefix + 'bn.bias'].reshape(1, -1, 1, 1))


def burger_train(x, P, cfg, bases, stats, steps):
    h = 'hamburger.'
    y = torch.relu(F.conv2d(x, P[h + 'lower_bread.0.weight'], P[h + 'lower_bread.0.bias']))
    parts = [nmf2d_train(y[:, c0:c0 + ch], R.normalise(b.to(y.dtype)), steps, spatial, cfg['S'])
             for (spatial, c0, ch), b in zip(R.ham_list(cfg), bases)]
    y = conv_bn_relu_train(torch.cat(parts, dim=1), P, h + 'cheese.', stats)
    y = F.conv2d(y, P[h + 'upper_bread.weight'])
    return torch.relu(P[h + 'coef_ham'] * y + P[h + 'coef_shortcut'] * x)


def head_train(x, P, cfg, bases, keep, steps=TRAIN_STEPS):
    """NCHW features -> (heat maps (B, J, h, w), {BatchNorm prefix: (batch mean, unbiased batch variance)})"""
    stats = {}
    y = conv_bn_relu_train(x, P, 'squeeze.', stats)
    y = burger_train(y, P, cfg, bases, stats, steps)
    y = conv_bn_relu_train(y, P, 'align.', stats)
    y = y * keep.to(y.dtype).reshape(keep.shape[0], -1, 1, 1)
    y = F.conv2d(y, P['fc.1.weight'], P['fc.1.bias'])
    return torch.softmax(y.flatten(2) * P['trainable_temp'], dim=2).reshape(y.shape), stats


def param_keys(cfg):
    """the head's parameters (what an optimiser steps), in state-dict order"""
    return [k for k, _ in R.head_keys(cfg) if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]


def run_train(cfg, dtype, bases, keep, targets, seed=SEED, steps=TRAIN_STEPS):
    """one training step of the case, differentiated on the CPU: dict(loss, hm, grads {key or 'features': array}, running
    {prefix + 'running_mean' / 'running_var': array after the step}, batch {prefix: (mean, unbiased var)}), float64 numpy"""
    state = R.fill_state_dict(R.head_keys(cfg), seed)
    P = to_torch(state, dtype)
    keys = param_keys(cfg)
    for k in keys:
        P[k].requires_grad_(True)
    x = torch.tensor(R.inputs(cfg, seed), dtype=dtype, requires_grad=True)
    hm, stats = head_train(x, P, cfg, [torch.as_tensor(np.asarray(b)) for b in bases],
                           torch.as_tensor(np.asarray(keep)), steps)
    value = loss(hm, torch.tensor(np.asarray(targets), dtype=dtype))
    grads = torch.autograd.grad(value, [x] + [P[k] for k in keys])
    out = dict(loss=float(value.detach().double()), hm=hm.detach().double().numpy(),
               grads={k: g.double().numpy() for k, g in zip(['features'] + keys, grads)}, running={}, batch={})
    for prefix, (mean, var) in stats.items():
        out['batch'][prefix] = (mean.double().numpy(), var.double().numpy())
        for name, new in (('running_mean', mean), ('running_var', var)):
            old = P[prefix + name].detach()
            out['running'][prefix + name] = ((1.0 - MOMENTUM) * old + MOMENTUM * new).double().numpy()
    return out
