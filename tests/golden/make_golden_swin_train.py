"""Writes tests/golden/swin_train.npz: the reference's SwinPose head (lib/models/swin_transformer.py) in TRAINING mode, in
float64 on the CPU, at swin_ref.CASE_A, differentiated by torch.autograd. Run it where the reference checkout is:

    python tests/golden/make_golden_swin_train.py <reference checkout>

The reference file is loaded as tests/golden/make_golden_swin.py loads it, except that timm's DropPath is stood in by a
module that multiplies each sample by a RECORDED factor (flag / keep_prob, swin_train_ref.factors): a block's DropPath is
called twice per forward, for the attention branch and then for the MLP branch. The state dict, the inputs and the targets
come from swin_ref.fill_state_dict / inputs and swin_train_ref.targets with SEED_TRAIN, so nothing but results is stored.

Two runs: 'all' (every flag kept: only the 1 / keep_prob scales act) and 'drop' (the flags of seed 5, some dropped). Per run
r: r/loss (swin_train_ref.loss), r/factors (blocks, 2, B), r/dx_head (the gradient of the input features, channels 0 - 7),
r/dx_sums, r/names, r/sums (names, 2): sum and sum of squares of every parameter gradient and of dx, and r/full/<name> for
the gradients of at most 4096 elements; r/mean<s>, r/var<s>: the BatchNorm running statistics after the step. float64.

It asserts that tests/swin_train_ref agrees with the reference to 1e-10 on every stored quantity.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden_swin as G  # noqa: E402
import swin_ref as R  # noqa: E402
import swin_train_ref as TR  # noqa: E402

SEED_TRAIN = 11
FULL = 4096


class RecordedDropPath(nn.Module):
    made = []

    def __init__(self, p):
        super().__init__()
        self.p, self.pair, self.calls = p, None, 0
        RecordedDropPath.made.append(self)

    def forward(self, x):
        f = torch.as_tensor(self.pair[self.calls % 2], dtype=x.dtype)
        self.calls += 1
        return x * f.reshape(-1, *([1] * (x.ndim - 1)))


def load_reference(root):
    G._stub('timm')
    G._stub('timm.models')
    G._stub('timm.models.layers', DropPath=RecordedDropPath, to_2tuple=lambda v: (v, v), trunc_normal_=lambda *a, **k: None)
    soft = G._stub('refmodels.pose_hrnet_softmax', get_pose_net=lambda config, is_train=True: G._PassThrough())
    G._stub('refmodels', pose_hrnet_softmax=soft, __path__=[])
    spec = importlib.util.spec_from_file_location('refmodels.swin_transformer',
                                                  os.path.join(root, 'lib', 'models', 'swin_transformer.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules['refmodels.swin_transformer'] = mod
    spec.loader.exec_module(mod)
    return mod


def sums(g):
    g = np.asarray(g, dtype=np.float64)
    return np.array([g.sum(), (g * g).sum()])


def restatement(state, x, fac, target):
    P = R.to_torch(state, torch.float64)
    names = [k for k, v in P.items() if v.dtype == torch.float64 and not k.endswith(('running_mean', 'running_var'))]
    for k in names:
        P[k].requires_grad_(True)
    xx = torch.tensor(x).requires_grad_(True)
    hm, stats = TR.head(xx, P, R.CASE_A, fac)
    loss = TR.loss(hm, torch.tensor(target))
    grads = torch.autograd.grad(loss, [xx] + [P[k] for k in names], allow_unused=True)
    return float(loss), grads[0].numpy(), {k: g for k, g in zip(names, grads[1:])}, stats


def main(root):
    mod = load_reference(root)
    cfg = R.CASE_A
    state = R.fill_state_dict(R.head_keys(cfg), SEED_TRAIN)
    x, target = R.inputs(cfg, SEED_TRAIN), TR.targets(cfg, 16, SEED_TRAIN)
    out = {'seed': np.int64(SEED_TRAIN)}
    for tag, keep_all in (('all', True), ('drop', False)):
        fac = TR.factors(cfg['depths'], cfg['batch'], 0.2, seed=5, keep_all=keep_all)
        RecordedDropPath.made = []
        model = mod.SwinPose(G.config(cfg, True)).double()
        model.load_state_dict(R.to_torch(state, torch.float64), strict=True)
        model.train(True)
        assert model.training and model.decoder[2].training and model.swinTransformer.layers[3].training
        rates = TR.drop_path_rates(cfg['depths'], 0.2)
        made = RecordedDropPath.made
        assert [m.p for m in made] == [r for r in rates if r > 0]                  # block 0 has rate 0: an Identity
        for m, pair in zip(made, [p for p, r in zip(fac, rates) if r > 0]):
            m.pair = pair
        assert all(np.all(np.asarray(f) == 1) for p, r in zip(fac, rates) if r == 0 for f in p)
        xx = torch.tensor(x).requires_grad_(True)
        hm = model(xx)[0]
        assert all(m.calls == 2 for m in made)
        loss = TR.loss(hm, torch.tensor(target))
        loss.backward()
        grads = {k: p.grad for k, p in model.named_parameters()}
        rl, rdx, rg, rstats = restatement(state, x, fac, target)
        tol = 1e-10
        assert abs(rl - float(loss)) <= tol * abs(float(loss)), (rl, float(loss))
        assert R.rel(rdx, xx.grad.numpy()) <= tol, R.rel(rdx, xx.grad.numpy())
        names, table = ['dx'], [sums(xx.grad.numpy())]
        for k, g in grads.items():
            unused = g is None or float(g.abs().max()) == 0
            if unused:                                                              # norm0 - norm2: computed and discarded
                assert k.startswith(('swinTransformer.norm0', 'swinTransformer.norm1', 'swinTransformer.norm2')), k
                assert rg[k] is None or float(rg[k].abs().max()) == 0
                continue
            g = g.numpy()
            scale = np.abs(g).max()
            # the biases under a BatchNorm and the last bias under the softmax have a gradient of rounding noise
            noise = scale < 1e-12
            if not noise:
                assert R.rel(rg[k].numpy(), g) <= tol, (k, R.rel(rg[k].numpy(), g))
                names.append(k)
                table.append(sums(g))
                if g.size <= FULL:
                    out['{}/full/{}'.format(tag, k)] = g
        for s in range(cfg['steps']):
            bn = model.decoder[4 * s + 2]
            old_m, old_v = (torch.tensor(state['decoder.{}.running_{}'.format(4 * s + 2, n)]) for n in ('mean', 'var'))
            assert R.rel((0.9 * old_m + 0.1 * rstats[s][0]).detach().numpy(), bn.running_mean.numpy()) <= tol
            assert R.rel((0.9 * old_v + 0.1 * rstats[s][1]).detach().numpy(), bn.running_var.numpy()) <= tol
            assert int(bn.num_batches_tracked) == 1
            out['{}/mean{}'.format(tag, s)] = bn.running_mean.numpy().copy()
            out['{}/var{}'.format(tag, s)] = bn.running_var.numpy().copy()
        out.update({tag + '/loss': np.float64(float(loss)), tag + '/factors': np.asarray(fac, dtype=np.float64),
                    tag + '/dx_head': xx.grad.numpy()[:, :8].copy(), tag + '/names': np.array(names),
                    tag + '/sums': np.stack(table)})
        print('{}: loss {:.6g}, {} gradients ({} in full), dropped flags {}'.format(
            tag, float(loss), len(names), sum(1 for k in out if k.startswith(tag + '/full/')),
            int(sum((np.asarray(f) == 0).sum() for p in fac for f in p))))
    path = os.path.join(HERE, 'swin_train.npz')
    np.savez_compressed(path, **out)
    print('wrote {} ({} bytes)'.format(path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1000000


if __name__ == '__main__':
    main(sys.argv[1])
