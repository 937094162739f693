"""Writes tests/golden/poseformer.npz: the head of the reference's PoseTransformer (lib/models/pose_hrnet_transformer.py)
in eval mode - Spatial_forward_features, forward_features, head - on random poses, in float64 and float32, at
(S, F, J) = (4, 9, 21), (2, 5, 21) and (1, 1, 21).

    python tests/golden/make_golden_poseformer.py <reference checkout>

The reference file is loaded by path with stand-ins for what it imports and this machine may lack: timm (DropPath is the
identity in eval mode, the other names are unused), einops (its two rearrange patterns are a permute and a reshape),
models.pose_hrnet_softmax (a dummy backbone with stage3, stage4, last_layer) and utils.heatmap_decoding. The state dict
is filled by tests/poseformer_ref.fill_state_dict (seed below, sorted key order), never stored.

Stored per shape tag t = s<S>f<F>j<J>: t/p (poses), t/g (cotangent), t/y64, t/y32 (the reference's outputs), t/dp64 (the
float64 gradient of sum(y * g) with respect to the poses), t/grad/<key> (float64 parameter gradients of
poseformer_ref.STORED, large matrices subsampled by poseformer_ref.sample) and t/gmax/<key> (max |gradient| of the whole
tensor), t/keys and t/shapes (the head's state-dict keys in the reference's order, shapes padded with 0 to three
entries), t/e32 = (forward, pose gradient, worst stored parameter gradient) error of the float32 RESTATEMENT against
float64, and `seed`. No weights, no code.

It asserts that tests/poseformer_ref.head agrees with the reference's float64 run to 1e-10 of max|y| (forward and pose
gradient).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import poseformer_ref as R  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _rearrange(x, pattern, **kw):
    pattern = ' '.join(pattern.split())
    if pattern == 'b c f p -> (b f) p c':
        b, c, f, p = x.shape
        return x.permute(0, 2, 3, 1).reshape(b * f, p, c)
    if pattern == '(b f) w c -> b f (w c)':
        bf, w, c = x.shape
        return x.reshape(bf // kw['f'], kw['f'], w * c)
    raise ValueError(pattern)


class _DummyBackbone(nn.Module):
    def __init__(self):
        super().__init__()
        self.stage3 = nn.Identity()
        self.stage4 = nn.Identity()
        self.last_layer = nn.Identity()


def load_reference(root):
    ident = lambda *a, **k: None
    _stub('timm')
    _stub('timm.data', IMAGENET_DEFAULT_MEAN=(0,) * 3, IMAGENET_DEFAULT_STD=(1,) * 3)
    _stub('timm.models')
    _stub('timm.models.helpers', load_pretrained=ident)
    _stub('timm.models.layers', DropPath=lambda p: nn.Identity(), to_2tuple=lambda v: (v, v), trunc_normal_=ident)
    _stub('timm.models.registry', register_model=lambda f: f)
    _stub('einops', rearrange=_rearrange, repeat=ident)
    soft = _stub('models.pose_hrnet_softmax', get_pose_net=lambda cfg, is_train=True: _DummyBackbone())
    _stub('models', pose_hrnet_softmax=soft)
    _stub('utils')
    _stub('utils.heatmap_decoding', get_final_preds=ident)
    spec = importlib.util.spec_from_file_location('ref_pose_hrnet_transformer',
                                                  os.path.join(root, 'lib', 'models', 'pose_hrnet_transformer.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def config(F, J):
    ns = types.SimpleNamespace
    return ns(DATASET=ns(SEQ_IDX=list(range(F)), NUM_JOINTS=J),
              MODEL=ns(BACKBONE_NAME='pose_hrnet_softmax', BACKBONE_MODEL_PATH='', HEATMAP_SOFTMAX=True,
                       INIT_WEIGHTS=False))


def reference_run(mod, state, p, g, dtype, F, J):
    model = mod.PoseTransformer(config(F, J), is_train=False).to(dtype).eval()
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items() if not k.startswith('backbone.')]
    model.load_state_dict({k: torch.tensor(v, dtype=dtype) for k, v in state.items()}, strict=True)
    pt = torch.tensor(p, dtype=dtype, requires_grad=True)
    x = pt.permute(0, 3, 1, 2)
    y = model.head(model.forward_features(model.Spatial_forward_features(x))).view(p.shape[0], J, 2)
    (y * torch.tensor(g, dtype=dtype)).sum().backward()
    grads = {k: q.grad.double().numpy() for k, q in model.named_parameters() if k in R.STORED}
    return y.detach().double().numpy(), pt.grad.double().numpy(), grads, keys


def main(root):
    mod = load_reference(root)
    out = {'seed': np.int64(R.SEED)}
    for S, F, J in R.SHAPES:
        t = R.tag(S, F, J)
        state = R.fill_state_dict(R.head_keys(F, J), R.SEED)
        p, g = R.inputs(S, F, J)
        y64, dp64, g64, keys = reference_run(mod, state, p, g, torch.float64, F, J)
        y32, _, _, _ = reference_run(mod, state, p, g, torch.float32, F, J)
        assert keys == R.head_keys(F, J), 'the restatement lists other keys or shapes than the reference'
        assert sum(int(np.prod(s)) for _, s in keys) == (14552276 if F == 9 else sum(int(np.prod(s)) for _, s in keys))
        ry, rdp, rg = R.run(p, g, state, torch.float64)
        ymax = np.abs(y64).max()
        assert np.abs(ry - y64).max() <= 1e-10 * ymax and R.rel(rdp, dp64) <= 1e-10, (R.rel(ry, y64), R.rel(rdp, dp64))
        for k in R.STORED:
            denom = np.abs(g64['weighted_mean.weight']).max() if k == 'weighted_mean.bias' else None
            assert R.rel(rg[k], g64[k], denom) <= 1e-9, (k, R.rel(rg[k], g64[k], denom))
        fy, fdp, fg = R.run(p, g, state, torch.float32)
        worst = max(R.rel(fg[k], g64[k], np.abs(g64['weighted_mean.weight']).max() if k == 'weighted_mean.bias' else None)
                    for k in R.STORED)
        e32 = (R.rel(fy, y64), R.rel(fdp, dp64), worst)
        print('{}: max|y| {:.3g}, {} entries; float32 restatement vs float64: forward {:.2g}, pose gradient {:.2g}, worst '
              'stored parameter gradient {:.2g}; reference float32 forward {:.2g}'.format(
                  t, ymax, len(keys), e32[0], e32[1], e32[2], R.rel(y32, y64)))
        out.update({t + '/p': p, t + '/g': g, t + '/y64': y64, t + '/y32': y32.astype(np.float32), t + '/dp64': dp64,
                    t + '/e32': np.array(e32), t + '/keys': np.array([k for k, _ in keys]),
                    t + '/shapes': np.array([list(s) + [0] * (3 - len(s)) for _, s in keys], dtype=np.int64)})
        for k in R.STORED:
            out[t + '/grad/' + k] = R.sample(g64[k])
            out[t + '/gmax/' + k] = np.float64(np.abs(g64[k]).max())
    path = os.path.join(HERE, 'poseformer.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
