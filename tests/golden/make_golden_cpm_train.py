"""Writes tests/golden/cpm_train.npz: the gradients of the reference's Convolutional Pose Machine (lib/models/CPM.py) under
its HeatmapLoss (lib/core/loss.py), by the reference modules' own float64 autograd.

    python tests/golden/make_golden_cpm_train.py <reference checkout>

Both reference files are loaded by path (they import numpy and torch only). The state dict is cpm_ref.fill_state_dict's
(never stored). Cases and inputs: tests/cpm_train_ref.CASES / inputs (float16-valued image, centre map and target).

Stored per case c: c/img, c/center, c/target (float16), c/loss (two float64: the last stage alone, all six stages),
c/gmax (2, 80): max |g| per tensor in state-dict order, c/gsamples (2, 80, 1024): the gradient at seeded flat indices
(tests/cpm_train_ref.sample_index: drawn with replacement per tensor from the seed, not stored), and for case p c/trajectory: the losses of six Adam steps
(torch.optim.Adam, float64, lr below) on the fixed batch, last-stage loss. `keys`, `seed`, `lr`. No weights, no code.

It asserts that the restatement of tests/cpm_train_ref.py, run with its OWN decisions, matches the reference's autograd to
1e-10 on both losses and on every gradient (over max |g| of the tensor), and that the float64 trajectory ends below 0.8
of its first loss: the margin under which the device test's `last < first` is safe.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cpm_ref as R  # noqa: E402
import cpm_train_ref as TR  # noqa: E402

LR = 1e-4
SAMPLES = 1024


def load(root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_run(ref, loss_mod, state, img, cm, tgt, weights):
    model = ref.CPM(R.K_JOINTS).double().train()
    model.load_state_dict(R.to_torch(state, torch.float64), strict=True)
    crit = loss_mod.HeatmapLoss()
    outs = model(torch.tensor(img), torch.tensor(cm))
    loss = sum(crit(o, torch.tensor(tgt)) * w for o, w in zip(outs, weights) if w)
    loss.backward()
    return float(loss.detach()), {k: p.grad.numpy() for k, p in model.named_parameters()}, model


def main():
    ref = load(sys.argv[1], ('lib', 'models', 'CPM.py'), 'ref_cpm')
    loss_mod = load(sys.argv[1], ('lib', 'core', 'loss.py'), 'ref_loss')
    state = R.fill_state_dict(R.K_JOINTS, R.SEED)
    keys = [k for k, _ in R.keys_and_shapes()]
    out = {'keys': np.array(keys), 'seed': np.int64(R.SEED), 'lr': np.float64(LR)}
    for case in sorted(TR.CASES):
        img, cm, tgt = TR.inputs(case)
        index = TR.sample_index(case, [state[k].size for k in keys], SAMPLES)
        losses, gmax, samples = [], [], []
        for weights in (TR.LAST_STAGE, TR.ALL_STAGES):
            l_ref, g_ref, _ = reference_run(ref, loss_mod, state, img, cm, tgt, weights)
            l_mine, g_mine = TR.loss_and_grads(state, img, cm, tgt, weights, torch.float64)
            worst = max(R.rel(g_mine[k], g_ref[k]) for k in keys)
            print('case {} weights {}: loss {:.12g} (restatement off by {:.2e}), worst gradient {:.2e}'.format(
                case, weights, l_ref, abs(l_mine - l_ref) / abs(l_ref), worst))
            assert abs(l_mine - l_ref) <= 1e-10 * abs(l_ref) and worst <= 1e-10
            losses.append(l_ref)
            gmax.append([np.abs(g_ref[k]).max() for k in keys])
            samples.append([g_ref[k].reshape(-1)[index[i]] for i, k in enumerate(keys)])
        out.update({case + '/img': img.astype(np.float16), case + '/center': cm.astype(np.float16),
                    case + '/target': tgt.astype(np.float16), case + '/loss': np.array(losses), case + '/gmax': np.array(gmax),
                    case + '/gsamples': np.array(samples)})
    img, cm, tgt = TR.inputs('p')
    model = ref.CPM(R.K_JOINTS).double().train()
    model.load_state_dict(R.to_torch(state, torch.float64), strict=True)
    opt, crit, traj = torch.optim.Adam(model.parameters(), lr=LR), loss_mod.HeatmapLoss(), []
    for _ in range(6):
        opt.zero_grad()
        loss = crit(model(torch.tensor(img), torch.tensor(cm))[-1], torch.tensor(tgt))
        loss.backward()
        opt.step()
        traj.append(float(loss.detach()))
    print('trajectory', traj)
    assert traj[-1] < 0.8 * traj[0], traj
    out['p/trajectory'] = np.array(traj)
    path = os.path.join(HERE, 'cpm_train.npz')
    np.savez_compressed(path, **out)
    print('wrote {} ({} bytes)'.format(path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
