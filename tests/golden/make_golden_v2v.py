"""Writes tests/golden/v2v.npz: the reference's own V2VModel(2, 2) in eval mode on one (1, 2, 32, 32, 32) input, in
float64 and in float32 on the CPU, for tests/test_v2v_cpu.py and tests/test_v2v_gpu.py.

    python tests/golden/make_golden_v2v.py <reference checkout>

Imports numpy, torch, tests/v2v_ref.py (for the recipe that fills the state dict, fill_state_dict: written out there,
drawn from numpy.random.default_rng(seed) in sorted key order) and, by path, the reference's lib/models/v2v.py. 32 is
the smallest extent that reaches the 1^3 bottom level. Only inputs and outputs are stored, no code and no weights
(11.8 M parameters): a test regenerates them from the seed with the same recipe.

- seed, x (1, 2, 32, 32, 32) float32 from normal(0, 1)
- y64: the float64 run on x widened; y32: the float32 run with the state dict rounded to float32
- keys, shapes: the state dict's keys (in the reference's order) and shapes (padded with 0 to five entries, ndim kept
  in ndims)
Asserted and printed: max|y64| lies in [0.1, 100]; between 10 % and 90 % of every ReLU's outputs are nonzero (counted
by running tests/v2v_ref.py's restatement on the same state dict, which is also held to y64 here to 1e-10 of max|y|)."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import v2v_ref as R  # noqa: E402

SEED = 20


def main(ref):
    spec = importlib.util.spec_from_file_location('ref_v2v', os.path.join(ref, 'lib', 'models', 'v2v.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    model = mod.V2VModel(2, 2).eval()
    sd0 = model.state_dict()
    keys = list(sd0.keys())
    shapes = [tuple(v.shape) for v in sd0.values()]
    sd = R.fill_state_dict(zip(keys, shapes), SEED)
    x = np.random.default_rng(SEED + 1).normal(0.0, 1.0, (1, 2, 32, 32, 32)).astype(np.float32)

    def run(dtype):
        m = mod.V2VModel(2, 2).to(dtype)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(sd0[k].dtype if not sd0[k].is_floating_point()
                                                                 else dtype) for k, v in sd.items()}, strict=True)
        m.eval()
        with torch.no_grad():
            return m(torch.from_numpy(x).to(dtype)).numpy()
    y64, y32 = run(torch.float64), run(torch.float32)
    assert y64.dtype == np.float64 and y32.dtype == np.float32
    top = np.abs(y64).max()
    net = R.Net(sd)
    with torch.no_grad():
        mine = net(x).numpy()
    on = net.relu_on
    print('parameters', sum(int(np.prod(s)) for k, s in zip(keys, shapes) if 'running' not in k and 'tracked' not in k))
    print('max|y64| {:.4f}  restatement {:.2e}  e_ref = max|y32 - y64| / max|y64| = {:.3e}'.format(
        top, np.abs(mine - y64).max() / top, np.abs(y32 - y64).max() / top))
    print('ReLUs {}: nonzero fraction min {:.3f} max {:.3f}'.format(len(on), min(on), max(on)))
    assert 0.1 <= top <= 100.0, top
    assert np.abs(mine - y64).max() <= 1e-10 * top
    assert 0.1 <= min(on) and max(on) <= 0.9, (min(on), max(on))
    ndims = np.array([len(s) for s in shapes], dtype=np.int64)
    shp = np.zeros((len(shapes), 5), dtype=np.int64)
    for i, s in enumerate(shapes):
        shp[i, :len(s)] = s
    out = os.path.join(HERE, 'v2v.npz')
    np.savez_compressed(out, seed=np.int64(SEED), x=x, y64=y64, y32=y32, keys=np.array(keys), shapes=shp, ndims=ndims)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
