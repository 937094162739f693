"""Writes tests/golden/hamburger.npz and tests/golden/hamburger_state_keys.npz: the reference's HamNet
(lib/models/pose_hrnet_hamburger.py with lib/models/hamburger/) in eval mode on the CPU, in float64, on random inputs.

    python tests/golden/make_golden_hamburger.py <reference checkout>

The reference files are loaded by path as the package `refmodels`, with stand-ins for the two sibling modules that
pose_hrnet_hamburger imports: pose_hrnet_softmax (a dummy backbone that passes the features through) and pose_resnet. The
hamburger package itself (burger, ham, bread, its sync_bn) is the reference's own. The state dict is filled by
tests/hamburger_ref.fill_state_dict (seed below, sorted key order), never stored.

The reference draws its bases with torch.rand((B * S, D, R)) in float32 from the global CPU generator and would then
multiply them with a float64 map; while the model runs, torch.rand is wrapped so that each draw is recorded and handed on
as the same values in float64. The draws are float32 values, so the device gets the reference's bases exactly. Case C
also needs Tensor.view to fall back to reshape (see _RecordedRand): the reference's ham.py:99 raises with SPATIAL false
and S > 1.

  case A  the whole head on 480-channel 16x16 features: E = 32, R = 16, dual, S = 1, B = 2.
  case B  5x7 features (H W = 35, the channel ham's D, is a multiple of nothing): E = 24, R = 8, dual, B = 1.
  case C  a single ham with SPATIAL false, S = 2, CHEESE_FACTOR 2, E = 16, R = 48 (R > D), 8x8 features, B = 2.

Stored per case c in (a, b, c): c/x (float16: the inputs are float16 values), c/bases0 [, c/bases1] (float32, as drawn, not
normalised), c/y64 (the reference's heat maps), c/e32 (error of the float32 RESTATEMENT against c/y64), `seed`. The key
file holds, per case and for the full-size v2 configuration (`full`), the names and shapes (padded with 0 to four entries)
of the reference HamNet.state_dict() without its backbone.* entries, in the reference's order. No weights, no code.

It asserts that tests/hamburger_ref agrees with the reference's float64 run to 1e-12 of max|y| and lists the same keys.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hamburger_ref as R  # noqa: E402


class _PassThrough(nn.Module):
    def forward(self, x):
        return None, x, None


def load_reference(root):
    pkg = types.ModuleType('refmodels')
    pkg.__path__ = [os.path.join(root, 'lib', 'models')]
    sys.modules['refmodels'] = pkg
    for name in ('pose_hrnet_softmax', 'pose_resnet'):
        m = types.ModuleType('refmodels.' + name)
        m.get_pose_net = lambda config, is_train=True: _PassThrough()
        sys.modules['refmodels.' + name] = m
        setattr(pkg, name, m)
    return importlib.import_module('refmodels.pose_hrnet_hamburger')


def config(cfg):
    ns = types.SimpleNamespace
    return ns(DATASET=ns(NUM_JOINTS=cfg['joints']),
              MODEL=ns(HEATMAP_SIZE=list(cfg['size']), BACKBONE_NAME='pose_hrnet_softmax', BACKBONE_MODEL_PATH='',
                       EXTRA=ns(STAGE4=ns(NUM_CHANNELS=[32, 64, 128, 256])), EMB_DIM=cfg['emb'], VERSION='V2+',
                       HAM_TYPE='NMF', S=cfg['S'], R=cfg['R'], DUAL_HAM=cfg['dual'], SPATIAL=cfg['spatial'],
                       CHEESE_FACTOR=cfg['cheese'], ZERO_HAM=True, TRAIN_STEPS=6, EVAL_STEPS=cfg['steps'], INV_T=1, ETA=0.9,
                       RAND_INIT=True, BETA=0.1, TRAINABLE_SOFTMAX=True))


def table(model):
    return [(k, tuple(v.shape)) for k, v in model.state_dict().items() if not k.startswith('backbone.')]


def pack(keys):
    return (np.array([k for k, _ in keys]), np.array([list(s) + [0] * (4 - len(s)) for _, s in keys], dtype=np.int64))


class _RecordedRand(object):
    """torch.rand, recorded: the float32 draw is kept and returned as float64. Tensor.view falls back to reshape where it
    raises: ham.py:99 views a transposed product as (B, C, H, W), which no stride pattern allows when SPATIAL is false
    and S > 1 (case C; the reference's own yamls have S = 1) - reshape is what the statement means."""

    def __init__(self):
        self.draws, self.rand, self.view = [], torch.rand, torch.Tensor.view

    def __enter__(self):
        def rand(*a, **k):
            v = self.rand(*a, **k)
            assert v.dtype == torch.float32
            self.draws.append(v.clone())
            return v.double()

        def view(t, *shape):
            try:
                return self.view(t, *shape)
            except RuntimeError:
                return t.reshape(*shape)
        torch.rand, torch.Tensor.view = rand, view
        return self

    def __exit__(self, *exc):
        torch.rand, torch.Tensor.view = self.rand, self.view


def main(root):
    mod = load_reference(root)
    out, keyfile = {'seed': np.int64(R.SEED)}, {}
    for tag, cfg in sorted(R.CASES.items()):
        x = R.inputs(cfg)
        state = R.fill_state_dict(R.head_keys(cfg))
        model = mod.HamNet(config(cfg), False).double().eval()
        keys = table(model)
        assert keys == R.head_keys(cfg), 'the restatement lists other keys or shapes than the reference'
        model.load_state_dict(R.to_torch(state, torch.float64), strict=True)
        torch.manual_seed(R.SEED + ord(tag))
        with torch.no_grad(), _RecordedRand() as rec:
            y = model(torch.tensor(x, dtype=torch.float64))[0].numpy()
        bases = [b.numpy() for b in rec.draws]
        assert [b.shape for b in bases] == R.bases_shapes(cfg), [b.shape for b in bases]
        again = R.draw_bases(cfg, R.SEED + ord(tag))
        assert all(np.array_equal(a.numpy(), b) for a, b in zip(again, bases)), 'the restatement draws in another order'
        r64, r32 = R.run(cfg, torch.float64, bases), R.run(cfg, torch.float32, bases)
        assert R.rel(r64, y) <= 1e-12, R.rel(r64, y)
        print('{}: y {}, max {:.3g}; restatement float64 {:.2g}, float32 {:.2g}'.format(
            tag, y.shape, np.abs(y).max(), R.rel(r64, y), R.rel(r32, y)))
        out.update({tag + '/x': x.astype(np.float16), tag + '/y64': y, tag + '/e32': np.float64(R.rel(r32, y))})
        for i, b in enumerate(bases):
            out['{}/bases{}'.format(tag, i)] = b.astype(np.float32)
        keyfile[tag + '/keys'], keyfile[tag + '/shapes'] = pack(keys)
    keys = table(mod.HamNet(config(R.FULL), False))
    assert keys == R.head_keys(R.FULL), 'full'
    keyfile['full/keys'], keyfile['full/shapes'] = pack(keys)
    for name, data in (('hamburger.npz', out), ('hamburger_state_keys.npz', keyfile)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **data)
        print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
