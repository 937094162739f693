"""Writes tests/golden/ftl.npz: the head of the reference's FTLMultiviewNet (lib/models/FTL_encoder_decoder.py) in float64
and float32 on small widths.

    python tests/golden/make_golden_ftl.py <reference checkout>

The reference's file is loaded by path as a member of a stand-in package: `utils`, `utils.heatmap_decoding`, `utils.misc`
and the sibling model modules it imports are stand-ins in sys.modules (this machine has no kornia and no cv2, and none of
them is run). The backbone is a stub that returns the given features; the module's get_final_preds is this project's CPU
decode (ftl_ref.expectation); DLT_sii_pytorch is a no-op, since the reference's call has its arguments swapped and cannot
run. The reference hard-codes 240 (= 480 / 2) as the encoder's output width, so at the small widths recorded here its
encoder_head is rebuilt from the reference's OWN conv_block with C / 2 in that place. Everything else is the reference's
own constructor and its own forward.

The state dict is ftl_ref.fill_state_dict (sorted key order) and the inputs ftl_ref.inputs; neither is stored beyond the
features (float16 values) and the cameras. For B = 2 the reference's rows after the distribution are view-major (v * B + b):
they are permuted to slot order b * V + v before recording, and pose2d is decoded from the permuted maps (at B = 1 it is
asserted equal to what the reference returns).

Stored per case c (ftl_ref.CASES): c/feat, c/ext, c/K; c/<stage> for the stages of ftl_ref.STAGES in float64 (the channels
ftl_ref.kept keeps); c/pose2d (float64 run), c/pose2d32 (float32 run); c/e32 (rel(y32, y64) per stage, on the whole maps);
`<width>_<V>/keys` and `/shapes` (the head's state-dict entries in the reference's order); `seed`. No weights, no code.

Asserted: ftl_ref agrees with the reference's float64 run to 1e-12 of max|y| per stage and lists the same keys and shapes;
e32 < 1e-5 for every stage of every unit-scale case (a condition on the inputs: at MHP scale features of order 1 are divided
by ~600 and shifted by t ~ 300, and float32 loses its digits in the reference's own arithmetic, so only the unit-scale set
makes a wrong tap, slice or view show); 5e-8 < e32 everywhere, so that float32 was really run. The seed is fixed: the
script fails if the reference does not meet these.
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
import ftl_ref as R  # noqa: E402


class StubBackbone(nn.Module):
    def forward(self, x):
        return None, x


def load_reference(root):
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    backbone = lambda name: module(name, get_pose_net=lambda config, is_train=True: StubBackbone())
    utils = module('utils')
    utils.heatmap_decoding = module('utils.heatmap_decoding', get_final_preds=lambda hm, use_softmax=True: R.expectation(hm))
    utils.misc = module('utils.misc', DLT_sii_pytorch=lambda proj, pts: torch.zeros(pts.shape[0], 3, dtype=pts.dtype))
    pkg = module('ref_models')
    pkg.__path__ = []
    for name in ('pose_hrnet_softmax', 'pose_hrnet_volumetric', 'pose_hrnet'):
        setattr(pkg, name, backbone('ref_models.' + name))
    spec = importlib.util.spec_from_file_location('ref_models.FTL_encoder_decoder',
                                                  os.path.join(root, 'lib', 'models', 'FTL_encoder_decoder.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def config(channels, V):
    ns = types.SimpleNamespace
    return ns(MODEL=ns(BACKBONE_NAME='pose_hrnet_softmax', BACKBONE_MODEL_PATH='',
                       EXTRA=ns(STAGE4=ns(NUM_CHANNELS=list(channels)))),
              DATASET=ns(NUM_VIEWS=V, NUM_JOINTS=R.K_JOINTS))


def build(ref, channels, V, dtype, state):
    model = ref.FTLMultiviewNet(config(channels, V), device='cpu')
    C = sum(channels)
    model.encoder_head = ref.conv_block(n_layers=2, channel_lst=[C, C, C // 2], kernel_size_lst=[3, 3], stride_lst=[2, 2],
                                        padding_lst=[2, 2])
    model = model.to(dtype).eval()
    model.load_state_dict(R.to_torch(state, dtype), strict=True)
    return model


def run_reference(ref, case, dtype, state):
    channels, V, B, _, _ = R.CASES[case]
    feat, ext, K = R.inputs(case)
    model = build(ref, channels, V, dtype, state)
    got = {}
    hooks = [getattr(model, s).register_forward_hook(lambda m, i, o, s=s: got.__setitem__(s, o.detach()))
             for s in R.STAGES[:4]]
    with torch.no_grad():
        hm, pose2d, _ = model(torch.tensor(feat, dtype=dtype).reshape(B, V, *feat.shape[1:]), torch.tensor(ext, dtype=dtype),
                              torch.tensor(K, dtype=dtype).expand(B, 3, 3))
    for h in hooks:
        h.remove()
    got['heatmaps'] = hm
    for s in ('channel_expansion', 'decoder', 'heatmaps'):          # view-major rows v * B + b -> slot order b * V + v
        y = got[s]
        got[s] = y.reshape(V, B, *y.shape[1:]).transpose(0, 1).reshape(y.shape)
    mine = R.expectation(got['heatmaps']).reshape(B, V, -1, 2)
    if B == 1:
        assert torch.equal(mine, pose2d), case
    got['pose2d'] = mine
    return {k: v.double().numpy() for k, v in got.items()}


def main():
    ref = load_reference(sys.argv[1])
    out = {'seed': np.int64(R.SEED)}
    for case in sorted(R.CASES):
        channels, V, B, size, kind = R.CASES[case]
        state = R.fill_state_dict(channels, V, kind=kind)
        y64, y32 = run_reference(ref, case, torch.float64, state), run_reference(ref, case, torch.float32, state)
        mine = R.run(case, torch.float64, state=state)
        agree = {s: R.rel(mine[s], y64[s]) for s in R.STAGES}
        e32 = np.array([R.rel(y32[s], y64[s]) for s in R.STAGES])
        pix = np.abs(y32['pose2d'] - y64['pose2d']).max()
        print('case {} ({}, V {}, B {}, {}, {}): restatement {:.1e}, e32 {}, pose2d32 off by {:.2e} px, max hm {:.3f}'.format(
            case, sum(channels), V, B, size, kind, max(agree.values()), ' '.join('%.2e' % e for e in e32), pix, y64['heatmaps'].max()))
        assert max(agree.values()) < 1e-12 and R.rel(mine['pose2d'], y64['pose2d']) < 1e-12, (case, agree)
        assert e32.min() > 5e-8, (case, e32)
        assert kind != 'unit' or e32.max() < 1e-5, (case, e32)
        feat, ext, K = R.inputs(case)
        out.update({case + '/feat': feat.astype(np.float16), case + '/ext': ext, case + '/K': K, case + '/e32': e32,
                    case + '/pose2d': y64['pose2d'], case + '/pose2d32': y32['pose2d']})
        out.update({case + '/' + s: R.kept(s, y64[s]) for s in R.STAGES})
        tag = '{}_{}'.format(sum(channels), V)
        if tag + '/keys' not in out:
            model = build(ref, channels, V, torch.float64, state)
            table = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
            assert table == R.keys_and_shapes(channels, V), 'key table'
            out[tag + '/keys'] = np.array([k for k, _ in table])
            out[tag + '/shapes'] = np.array([list(s) + [0] * (4 - len(s)) for _, s in table], dtype=np.int64)
    path = os.path.join(HERE, 'ftl.npz')
    np.savez_compressed(path, **out)
    print('wrote {} ({} bytes), seed {}'.format(path, os.path.getsize(path), R.SEED))


if __name__ == '__main__':
    main()
