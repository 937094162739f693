"""Writes tests/golden/hamburger_train.npz: one training step of the reference's HamNet head
(lib/models/pose_hrnet_hamburger.py with lib/models/hamburger/) in TRAINING mode on the CPU, in float64, differentiated by
autograd.

    python tests/golden/make_golden_hamburger_train.py <reference checkout>

The reference is loaded as tests/golden/make_golden_hamburger.py loads it: the pass-through backbone, torch.rand recorded
(_RecordedRand), and here model.fc[0] - the Dropout2d - replaced by a module that multiplies by the recorded keep mask.
Cases A, B and C of tests/hamburger_ref, state dicts of fill_state_dict(seed 11), the soft-argmax distance loss of
tests/hamburger_train_ref on seeded targets. The reference is read only when this script runs.

It asserts that tests/hamburger_train_ref agrees with the reference to 1e-10 (loss, every gradient, the running
statistics) and that num_batches_tracked stays 0. Stored per case c in (a, b, c) - results only, no weights, no code:
  c/bases0 [, c/bases1] (float32, as drawn), c/keep (float32), c/targets, c/loss,
  c/sums: (sum, sum of squares) of every gradient, rows in the order of c/names ('features', then the parameters),
  c/grad/<name>: the gradients of at most 4096 elements in full, c/grad/features: channels 0-7 of the feature gradient,
  c/running/<key>: the running statistics after the step, c/tracked: num_batches_tracked after the step (three values),
  c/e32: the error of the float32 restatement per name (rows as c/names; the loss last).
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import hamburger_ref as R  # noqa: E402
import hamburger_train_ref as T  # noqa: E402
from make_golden_hamburger import _RecordedRand, config, load_reference  # noqa: E402

FULL_LIMIT = 4096


class _Keep(nn.Module):
    def __init__(self, keep):
        super(_Keep, self).__init__()
        self.keep = keep

    def forward(self, x):
        return x * self.keep.to(x.dtype).reshape(x.shape[0], -1, 1, 1)


def main(root):
    mod = load_reference(root)
    out = {'seed': np.int64(T.SEED)}
    for tag, cfg in sorted(R.CASES.items()):
        state = R.fill_state_dict(R.head_keys(cfg), T.SEED)
        keep, targets = T.draw_keep(cfg), T.draw_targets(cfg)
        model = mod.HamNet(config(cfg), False).double().train()
        model.load_state_dict(R.to_torch(state, torch.float64), strict=True)
        model.fc[0] = _Keep(torch.from_numpy(keep))
        x = torch.tensor(R.inputs(cfg, T.SEED), dtype=torch.float64, requires_grad=True)
        torch.manual_seed(T.SEED + ord(tag))
        with _RecordedRand() as rec:
            hm = model(x)[0]
        bases = [b.numpy() for b in rec.draws]
        assert [b.shape for b in bases] == R.bases_shapes(cfg), [b.shape for b in bases]
        value = T.loss(hm, torch.tensor(targets))
        value.backward()
        names = ['features'] + T.param_keys(cfg)
        params = dict(model.named_parameters())
        ref = {'features': x.grad.numpy()}
        ref.update({k: params[k].grad.numpy() for k in names[1:]})
        sd = model.state_dict()
        r64 = T.run_train(cfg, torch.float64, bases, keep, targets)
        r32 = T.run_train(cfg, torch.float32, bases, keep, targets)
        assert abs(r64['loss'] - value.item()) <= 1e-10 * abs(value.item()), (r64['loss'], value.item())
        scale = max(np.abs(ref[k]).max() for k in names if k != 'fc.1.bias')
        for k in names:
            # fc.1.bias: zero by the softmax's shift invariance - rounding noise on both sides
            e = np.abs(r64['grads'][k] - ref[k]).max() / scale if k == 'fc.1.bias' else R.rel(r64['grads'][k], ref[k])
            assert e <= 1e-10, (tag, k, e)
        tracked = []
        for prefix in T.BN_PREFIXES:
            for leaf in ('running_mean', 'running_var'):
                assert R.rel(r64['running'][prefix + leaf], sd[prefix + leaf].numpy()) <= 1e-10, (tag, prefix + leaf)
                out['{}/running/{}'.format(tag, prefix + leaf)] = sd[prefix + leaf].numpy()
            tracked.append(int(sd[prefix + 'num_batches_tracked']))
        assert tracked == [0, 0, 0], tracked
        e32 = [R.rel(r32['grads'][k], ref[k]) for k in names] + [abs(r32['loss'] - value.item()) / abs(value.item())]
        print('{}: loss {:.6g}; float32 restatement: loss {:.2g}, gradients at most {:.2g} ({})'.format(
            tag, value.item(), e32[-1], max(e for k, e in zip(names, e32) if k != 'fc.1.bias'),
            max((e, k) for k, e in zip(names, e32) if k != 'fc.1.bias')[1]))
        out.update({tag + '/keep': keep, tag + '/targets': targets, tag + '/loss': np.float64(value.item()),
                    tag + '/names': np.array(names), tag + '/tracked': np.array(tracked, dtype=np.int64),
                    tag + '/sums': np.array([[ref[k].sum(), (ref[k] ** 2).sum()] for k in names]),
                    tag + '/e32': np.array(e32), tag + '/grad/features': ref['features'][:, :8].copy()})
        for i, b in enumerate(bases):
            out['{}/bases{}'.format(tag, i)] = b.astype(np.float32)
        for k in names[1:]:
            if ref[k].size <= FULL_LIMIT:
                out['{}/grad/{}'.format(tag, k)] = ref[k]
    path = os.path.join(HERE, 'hamburger_train.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1000000


if __name__ == '__main__':
    main(sys.argv[1])
