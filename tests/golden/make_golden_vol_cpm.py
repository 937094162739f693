"""Writes tests/golden/vol_cpm_state_keys.npz: the state_dict keys and shapes of the reference's CPM_volumetric backbone
(with MODEL.VOL_CONFIDENCES true and false) and of its whole VolumetricTriangulationNet_CPM, for tests/test_vol_cpm_cpu.py,
and pins tests/vol_cpm_ref.py against the reference's own module.

    python tests/golden/make_golden_vol_cpm.py <reference checkout>   (or HRNET_REFERENCE)

Runs on the CPU. Imports, by path, the reference's lib/models/CPM_volumetric.py (torch only) and lib/models/v2v.py, with
this project's CfgNode on this project's vol_CPM yaml. The reference's whole model (lib/models/triangulation.py) cannot be
imported here (kornia, cv2 and yacs are absent), so its key list is composed by the rules of triangulation.py:491-534:
`backbone.` + the backbone's keys (the reference builds it with VOL_CONFIDENCES as the yaml has it: true),
`process_features.0.weight` (32, 128, 1, 1) and `.bias` (32,), `volume_net.` + the keys of V2VModel(32, NUM_JOINTS).
Names and shapes only: no code, no weights.

- backbone_conf_keys, _shapes, _ndims: VOL_CONFIDENCES true (the shipped yaml; GlobalAveragePoolingHead(128, 32))
- backbone_keys, ...: VOL_CONFIDENCES false
- model_keys, ...: the whole model, VOL_CONFIDENCES true
- <case>/agree: at cpm_ref.CASES b and c, the largest error of tests/vol_cpm_ref.backbone against the reference's float64
  forward over its seven tensors (relative to each tensor's largest value), and <case>/commuted: the same of
  features_commuted against the reference's order (up-sample 128 channels, then the 1x1 convolution)
shapes are padded with 0 to five entries, ndim kept in *_ndims.

It asserts that the restatement agrees with the reference to 1e-10 on every tensor (the reference's seventh output is the
up-sampled feature map; the restatement's stride-8 one is up-sampled here to compare) and that the commuted feature path
agrees with the reference's order to 1e-12."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(REPO, 'hrnet-hand-pose-estimation_amd')
sys.path.insert(0, os.path.join(PKG, 'lib'))
sys.path.insert(0, os.path.dirname(HERE))

import cpm_ref as R  # noqa: E402
import vol_cpm_ref as VC  # noqa: E402
from config import get_cfg_defaults  # noqa: E402

YAML = os.path.join(PKG, 'experiments', 'MHP', 'MHP_VolTriangulation_CPM_v1.yaml')
HM = {'b': 6, 'c': 4}            # the reference's up-sampled maps are square: MODEL.HEATMAP_SIZE[0] on both axes


def _load(ref, name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _table(pairs):
    keys = np.array([k for k, _s in pairs])
    ndims = np.array([len(s) for _k, s in pairs], dtype=np.int64)
    shapes = np.zeros((len(pairs), 5), dtype=np.int64)
    for i, (_k, s) in enumerate(pairs):
        shapes[i, :len(s)] = s
    return keys, shapes, ndims


def _cfg(conf=True, hm=64):
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    cfg.MODEL.VOL_CONFIDENCES = conf
    cfg.MODEL.HEATMAP_SIZE = [hm, hm]
    return cfg


def main(ref):
    if not hasattr(np, 'int'):
        np.int = int
    backbone = _load(ref, 'ref_cpm_volumetric', 'lib/models/CPM_volumetric.py')
    v2v = _load(ref, 'ref_v2v', 'lib/models/v2v.py')
    out, pairs = {}, {}
    for name, conf in (('backbone_conf', True), ('backbone', False)):
        model = backbone.get_pose_net(_cfg(conf), is_train=False)
        pairs[name] = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        out[name + '_keys'], out[name + '_shapes'], out[name + '_ndims'] = _table(pairs[name])
    assert pairs['backbone'] == R.keys_and_shapes(R.K_JOINTS)
    net = v2v.V2VModel(32, R.K_JOINTS)
    whole = [('backbone.' + k, s) for k, s in pairs['backbone_conf']]
    whole += [('process_features.0.weight', (32, VC.INTER, 1, 1)), ('process_features.0.bias', (32,))]
    whole += [('volume_net.' + k, tuple(v.shape)) for k, v in net.state_dict().items()]
    out['model_keys'], out['model_shapes'], out['model_ndims'] = _table(whole)

    state = R.fill_state_dict(R.K_JOINTS, R.SEED)
    w, b = (torch.tensor(a) for a in VC.process_weights())
    for case, hm in sorted(HM.items()):
        img, cm = (torch.tensor(a) for a in R.inputs(case))
        torch.manual_seed(0)
        model = backbone.get_pose_net(_cfg(True, hm), is_train=False).double().eval()
        res = model.load_state_dict(R.to_torch(state, torch.float64), strict=False)
        assert not res.unexpected_keys and all(k.startswith('vol_confidences.') for k in res.missing_keys)
        with torch.no_grad():
            want = model(img, cm)
            low, heat, feat = VC.backbone(R.to_torch(state, torch.float64), img, cm, (hm, hm))
            mine = list(low) + [heat, VC.upsample(feat, (hm, hm))]
            agree = max(R.rel(m.numpy(), t.numpy()) for m, t in zip(mine, want[:7]))
            commuted = R.rel(VC.features_commuted(feat, w, b, (hm, hm)).numpy(),
                             VC.features_reference(feat, w, b, (hm, hm)).numpy())
            # the reference's own order on ITS up-sampled tensor is features_reference on the stride-8 one
            assert R.rel(torch.nn.functional.conv2d(want[6], w, b).numpy(),
                         VC.features_reference(feat, w, b, (hm, hm)).numpy()) <= 1e-10
        print('case {}: restatement {:.2e}, commuted feature path {:.2e}'.format(case, agree, commuted))
        assert agree <= 1e-10 and commuted <= 1e-12, (case, agree, commuted)
        assert want[7] is not None and tuple(want[5].shape[2:]) == (hm, hm)
        out[case + '/agree'], out[case + '/commuted'] = np.float64(agree), np.float64(commuted)
    path = os.path.join(HERE, 'vol_cpm_state_keys.npz')
    np.savez_compressed(path, **out)
    print('backbone {} keys, with the confidence head {}, whole model {}'.format(
        len(pairs['backbone']), len(pairs['backbone_conf']), len(whole)))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ['HRNET_REFERENCE'])
