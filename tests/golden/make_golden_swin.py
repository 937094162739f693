"""Writes tests/golden/swin.npz: the reference's SwinPose (lib/models/swin_transformer.py) in eval mode, in float64 and
float32, on random inputs.

    python tests/golden/make_golden_swin.py <reference checkout>

The reference file is loaded by path with stand-ins for what it imports and this machine may lack: timm (DropPath is the
identity in eval mode, to_2tuple, a no-op trunc_normal_) and its sibling module pose_hrnet_softmax (a dummy backbone with a
stage4 that passes the features through). The state dict is filled by tests/swin_ref.fill_state_dict (seed below, sorted key
order), never stored.

  case A  the full head, SwinPose.forward behind the pass-through backbone: Cin 480, features 16x16, PATCH_SIZE 2,
          EMB_DIM 48, DEPTHS [2, 2, 2, 2], B = 2. Token maps 8, 4, 2, 1 (every stage padded, the shifted blocks of the
          4x4, 2x2 and 1x1 maps have one window over the whole padded map), decoder of four steps, 1 -> 16.
  case B  SwinTransformer alone, last output: Cin 3, image 41x25, PATCH_SIZE 4, EMB_DIM 96, DEPTHS [2, 2, 2, 2], B = 1.
          Patch-embed padding, an 11x7 token map (two windows in a column), odd merges.

Stored per case c in (a, b): c/x (float16: the inputs are float16 values), c/y64, c/y32 (the reference's outputs; case B as
tokens (B, H W, C)), c/e32 (error of the float32 RESTATEMENT against c/y64), c/keys, c/shapes (state-dict keys in the
reference's order, shapes padded with 0 to four entries); full/keys, full/shapes and full_nb/keys, full_nb/shapes: the key
table of the full-size model (EMB_DIM 96, DEPTHS [2, 2, 18, 2], PATCH_SIZE 2, 64x64 heat maps) with the backbone (without
its backbone.* entries) and without it; `seed`. No weights, no code.

It asserts that tests/swin_ref agrees with the reference's float64 run to 1e-10 of max|y| and lists the same keys.
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
import swin_ref as R  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _PassThrough(nn.Module):
    def __init__(self):
        super().__init__()
        self.stage4 = nn.Identity()

    def forward(self, x):
        return None, x, None


def load_reference(root):
    _stub('timm')
    _stub('timm.models')
    _stub('timm.models.layers', DropPath=lambda p: nn.Identity(), to_2tuple=lambda v: (v, v),
          trunc_normal_=lambda *a, **k: None)
    soft = _stub('refmodels.pose_hrnet_softmax', get_pose_net=lambda config, is_train=True: _PassThrough())
    _stub('refmodels', pose_hrnet_softmax=soft, __path__=[])
    spec = importlib.util.spec_from_file_location('refmodels.swin_transformer',
                                                  os.path.join(root, 'lib', 'models', 'swin_transformer.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules['refmodels.swin_transformer'] = mod
    spec.loader.exec_module(mod)
    return mod


def config(cfg, backbone):
    ns = types.SimpleNamespace
    hm = cfg['size'][0] if backbone else 64       # with a backbone the features have the heat maps' size
    return ns(DATASET=ns(NUM_JOINTS=cfg['joints']),
              MODEL=ns(IMAGE_SIZE=[256, 256], HEATMAP_SIZE=[hm, hm], BACKBONE_NAME='pose_hrnet_softmax' if backbone else '',
                       BACKBONE_MODEL_PATH='', PATCH_SIZE=cfg['patch'], EMB_DIM=cfg['emb'], DEPTHS=list(cfg['depths']),
                       ABSOLUTE_POSITION_ENCODING=False, FF_TYPE='mlp', TRAINABLE_SOFTMAX=True,
                       EXTRA=ns(STAGE4=ns(NUM_CHANNELS=[32, 64, 128, 256]))))


def table(model):
    return [(k, tuple(v.shape)) for k, v in model.state_dict().items() if not k.startswith('backbone.')]


def pack(keys):
    return (np.array([k for k, _ in keys]), np.array([list(s) + [0] * (4 - len(s)) for _, s in keys], dtype=np.int64))


def main(root):
    mod = load_reference(root)
    out = {'seed': np.int64(R.SEED)}
    # case A
    cfg = R.CASE_A
    x = R.inputs(cfg)
    state = R.fill_state_dict(R.head_keys(cfg))
    ys = {}
    for dtype in (torch.float64, torch.float32):
        model = mod.SwinPose(config(cfg, True)).to(dtype).eval()
        keys = table(model)
        assert keys == R.head_keys(cfg), 'the restatement lists other keys or shapes than the reference'
        model.load_state_dict(R.to_torch(state, dtype), strict=True)
        with torch.no_grad():
            ys[dtype] = model(torch.tensor(x, dtype=dtype))[0].double().numpy()
    r64, r32 = R.run(cfg, torch.float64), R.run(cfg, torch.float32)
    assert R.rel(r64, ys[torch.float64]) <= 1e-10, R.rel(r64, ys[torch.float64])
    print('a: y {}, max {:.3g}; float32 restatement {:.2g}, reference float32 {:.2g}'.format(
        r64.shape, np.abs(r64).max(), R.rel(r32, ys[torch.float64]), R.rel(ys[torch.float32], ys[torch.float64])))
    k, s = pack(keys)
    out.update({'a/x': x.astype(np.float16), 'a/y64': ys[torch.float64], 'a/y32': ys[torch.float32].astype(np.float32),
                'a/e32': np.float64(R.rel(r32, ys[torch.float64])), 'a/keys': k, 'a/shapes': s})
    # case B
    cfg = R.CASE_B
    x = R.inputs(cfg)
    state = R.fill_state_dict(R.head_keys(cfg))
    ys = {}
    for dtype in (torch.float64, torch.float32):
        model = mod.SwinTransformer(pretrain_img_size=256, patch_size=cfg['patch'], in_chans=cfg['cin'],
                                    embed_dim=cfg['emb'], depths=list(cfg['depths']), ape=False,
                                    feed_forward='mlp').to(dtype)
        model.eval()                                                          # (the reference's train() returns None)
        keys = [('swinTransformer.' + a, b) for a, b in table(model)]
        assert keys == R.head_keys(cfg)[1:], 'the restatement lists other keys or shapes than the reference'
        model.load_state_dict({a[len('swinTransformer.'):]: b for a, b in R.to_torch(state, dtype).items()
                               if a.startswith('swinTransformer.')}, strict=True)
        with torch.no_grad():
            y = model(torch.tensor(x, dtype=dtype))[-1]                       # (B, C, H, W)
        ys[dtype] = y.flatten(2).transpose(1, 2).double().numpy()
    r64, r32 = R.run(cfg, torch.float64), R.run(cfg, torch.float32)
    assert R.rel(r64, ys[torch.float64]) <= 1e-10, R.rel(r64, ys[torch.float64])
    print('b: y {}, max {:.3g}; float32 restatement {:.2g}, reference float32 {:.2g}'.format(
        r64.shape, np.abs(r64).max(), R.rel(r32, ys[torch.float64]), R.rel(ys[torch.float32], ys[torch.float64])))
    k, s = pack(keys)
    out.update({'b/x': x.astype(np.float16), 'b/y64': ys[torch.float64], 'b/y32': ys[torch.float32].astype(np.float32),
                'b/e32': np.float64(R.rel(r32, ys[torch.float64])), 'b/keys': k, 'b/shapes': s})
    # the full-size key tables
    for tag, cfg, backbone in (('full', R.FULL, True), ('full_nb', R.FULL_NO_BACKBONE, False)):
        keys = table(mod.SwinPose(config(cfg, backbone)))
        assert keys == R.head_keys(cfg), tag
        out[tag + '/keys'], out[tag + '/shapes'] = pack(keys)
        print('{}: {} entries, {} values'.format(tag, len(keys), sum(int(np.prod(s)) for _, s in keys)))
    path = os.path.join(HERE, 'swin.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
