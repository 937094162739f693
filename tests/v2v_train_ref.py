"""Training-mode references for V2V on the CPU, from torch.nn.functional and autograd, in float64 unless told
otherwise: the restatement of tests/v2v_ref.py with every BatchNorm3d on batch statistics (momentum 0.1, biased variance
for the normalisation, unbiased for running_var), its parameters as autograd leaves, and the recipes the device tests
share: a block's parameters, one forward and backward of a block or of the whole network, and the error metric."""
import numpy as np
import torch
import torch.nn.functional as F

import v2v_ref as R

MOMENTUM = 0.1


class TrainNet(R.Net):
    """R.Net in training mode: parameters require gradients, running statistics are private copies that a forward
    updates"""

    def __init__(self, sd, dtype=torch.float64):
        super().__init__(sd, dtype)
        self.sd = {k: v.clone() for k, v in self.sd.items()}
        for k, v in self.sd.items():
            if self.is_param(k):
                v.requires_grad_(True)

    @staticmethod
    def is_param(k):
        return k.rsplit('.', 1)[1] in ('weight', 'bias')

    def _bn(self, x, p):
        g = self.sd
        g[p + '.num_batches_tracked'] += 1
        return F.batch_norm(x, g[p + '.running_mean'], g[p + '.running_var'], g[p + '.weight'], g[p + '.bias'], True,
                            MOMENTUM, R.EPS)

    def upsample(self, x, p, add=None):
        y = super().upsample(x, p)
        return y if add is None else y + add


def block_state(module, rng):
    """float64 numpy state dict for a block: conv weights normal(0, 1.4 / sqrt(fan_in)), conv biases in +-0.1,
    BatchNorm weight in [0.5, 1.5], bias in +-0.3, running_mean normal(0, 0.2), running_var in [0.5, 1.5]; every value
    float32-representable"""
    out = {}
    for k, v in module.state_dict().items():
        shp, leaf = tuple(v.shape), k.rsplit('.', 1)[1]
        bn = k.rsplit('.', 1)[0] + '.running_mean' in module.state_dict()
        if leaf == 'num_batches_tracked':
            out[k] = np.array(3, dtype=np.int64)
            continue
        if leaf == 'running_mean':
            a = rng.normal(0.0, 0.2, shp)
        elif leaf == 'running_var':
            a = rng.uniform(0.5, 1.5, shp)
        elif len(shp) == 5:
            transposed = 'ConvTranspose' in type(dict(module.named_modules())[k.rsplit('.', 1)[0]]).__name__
            fan_in = shp[0] if transposed else shp[1] * shp[2] * shp[3] * shp[4]
            a = rng.normal(0.0, 1.4 / np.sqrt(fan_in), shp)
        elif bn:
            a = rng.uniform(0.5, 1.5, shp) if leaf == 'weight' else rng.uniform(-0.3, 0.3, shp)
        else:
            a = rng.uniform(-0.1, 0.1, shp)
        out[k] = a.astype(np.float32).astype(np.float64)
    return out


def run(sd, walk, x, gout, add=None, dtype=torch.float64):
    """one training-mode forward and backward on the CPU. walk(net, x, add) -> y drives a TrainNet over `sd`.
    -> dict of float64 numpy arrays: 'y', 'dx', 'dadd' (if add), 'grad:<key>' per parameter, and '<key>' per buffer
    after the step"""
    net = TrainNet(sd, dtype)
    xt = torch.as_tensor(x).to(dtype).requires_grad_(True)
    at = None if add is None else torch.as_tensor(add).to(dtype).requires_grad_(True)
    y = walk(net, xt, at)
    y.backward(torch.as_tensor(gout).to(dtype))
    out = {'y': y.detach(), 'dx': xt.grad}
    if at is not None:
        out['dadd'] = at.grad
    for k, v in net.sd.items():
        if net.is_param(k):
            out['grad:' + k] = v.grad
        else:
            out[k] = v.detach()
    return {k: v.double().numpy() for k, v in out.items()}


def whole(net, x, add=None):
    return net(x)


def bias_under_bn(keys):
    """the keys of conv / deconv biases that sit under a BatchNorm: '<seq>.<i>.bias' with '<seq>.<i+1>.running_mean'"""
    out = set()
    for k in keys:
        head, leaf = k.rsplit('.', 1)
        if leaf != 'bias' or '.' not in head:
            continue
        seq, i = head.rsplit('.', 1)
        if i.isdigit() and '{}.{}.running_mean'.format(seq, int(i) + 1) in keys:
            out.add(k)
    return out


def rel_err(got, ref):
    top = np.abs(ref).max()
    return np.abs(np.asarray(got, dtype=np.float64) - ref).max() / (top if top > 0 else 1.0)


def compare(what, dev, r64, r32, state_keys, factor=4.0):
    """dev / r64 / r32: dicts as run() returns. Every tensor's max-abs error over max|f64| is held to factor x the
    LARGEST such error of the float32 CPU run over the tensors of the case; the gradient of a conv bias under a
    BatchNorm (mathematically zero) is held to factor x max|that gradient| of the float32 run instead.
    -> (largest device error, e_ref)"""
    zero = {'grad:' + k for k in bias_under_bn(set(state_keys))}
    names = [k for k in r64 if k not in zero and not k.endswith('num_batches_tracked')]
    e_ref = max(rel_err(r32[k], r64[k]) for k in names)
    worst = 0.0
    for k in names:
        e = rel_err(dev[k], r64[k])
        worst = max(worst, e)
        assert e <= factor * e_ref, (what, k, e, e_ref)
    for k in zero:
        lim = factor * np.abs(r32[k]).max()
        assert np.abs(dev[k]).max() <= lim, (what, k, np.abs(dev[k]).max(), lim)
    for k in r64:
        if k.endswith('num_batches_tracked'):
            assert int(dev[k]) == int(r64[k]), (what, k)
    print('{}: device {:.3e}, e_ref {:.3e}, bound {:.3e} ({} tensors, {} zero biases)'.format(
        what, worst, e_ref, factor * e_ref, len(names), len(zero)))
    return worst, e_ref
