"""Host side of the volumetric model on the CPM backbone (MODEL.NAME vol_CPM): the new C ABI entries, exported and bound from
the header; the state_dict keys, shapes and order of CPM_volumetric and of VolumetricTriangulationNet_CPM against the
reference's (tests/golden/vol_cpm_state_keys.npz, written by tests/golden/make_golden_vol_cpm.py); the frozen set; every
refusal of the backbone, the model and the tools before any device work; the refusals of `vol` and of evaluate_3D stay; the
commuted feature path (1x1 convolution, then up-sampling) equals the reference's order in float64. No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import cpm_ref as R
import mhp_tree
import vol_cpm_ref as VC

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = os.path.join(HERE, 'golden', 'vol_cpm_state_keys.npz')
YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_VolTriangulation_CPM_v1.yaml')
VOL_YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_VolTriangulation_w32_v1.yaml')
NEW = ('hrnet_upsample_slice_nchw', 'hrnet_upsample_slice_nchw_bwd', 'hrnet_upsample_slice_nchw_supported')


def _tools():
    tools = os.path.join(mhp_tree.PKG, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import evaluate_3D
    import evaluate_vol
    import train_vol
    return train_vol, evaluate_vol, evaluate_3D


def _cfg(opts=(), data='.', yaml=YAML):
    return mhp_tree.config(data, list(opts), yaml)


def _table(z, name):
    keys = [str(k) for k in z[name + '_keys']]
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(z[name + '_shapes'], z[name + '_ndims'])]
    return keys, shapes


def test_abi_entries_are_exported_and_bound_from_the_header():
    import ctypes
    from hipnet import _capi as C
    assert C.ABI_VERSION == 2 and C.call('hrnet_abi_version') == 2
    for name in NEW:
        assert name in C.EXPORTED and hasattr(C.lib(), name), name
    assert len(C._SIGS['hrnet_upsample_slice_nchw']) == 11 and len(C._SIGS['hrnet_upsample_slice_nchw_bwd']) == 12
    assert C._SIGS['hrnet_upsample_slice_nchw_supported'] == [ctypes.c_int] * 3
    assert 'hrnet_upsample_slice_nchw_supported' in C._PLAIN and 'hrnet_upsample_slice_nchw' not in C._PLAIN
    assert C.call('hrnet_upsample_slice_nchw_supported', 56, 32, 22) == 1
    assert C.call('hrnet_upsample_slice_nchw_supported', 8, 3, 5) == 1
    assert C.call('hrnet_upsample_slice_nchw_supported', 8, 3, 6) == 0
    assert C.call('hrnet_upsample_slice_nchw_supported', 8, -1, 2) == 0
    assert C.call('hrnet_upsample_slice_nchw_supported', 8, 0, 0) == 0
    # refused before any launch: no device is needed to be told so
    with pytest.raises(RuntimeError, match='null or aliased'):
        C.call('hrnet_upsample_slice_nchw', None, None, 1, 2, 2, 4, 0, 1, 2, 2, None)
    buf = (ctypes.c_float * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 128
    with pytest.raises(RuntimeError, match='do not lie in a row'):
        C.call('hrnet_upsample_slice_nchw', a, b, 1, 2, 2, 4, 3, 2, 2, 2, None)
    with pytest.raises(RuntimeError, match='H = 0'):
        C.call('hrnet_upsample_slice_nchw', a, b, 1, 2, 2, 4, 0, 1, 0, 2, None)
    with pytest.raises(RuntimeError, match='accumulate = 2'):
        C.call('hrnet_upsample_slice_nchw_bwd', a, b, 1, 2, 2, 4, 0, 1, 2, 2, 2, None)
    with pytest.raises(RuntimeError, match='too many pixels'):
        C.call('hrnet_upsample_slice_nchw_bwd', a, b, 1, 65536, 32768, 4, 0, 1, 2, 2, 0, None)


@pytest.mark.parametrize('conf', [True, False])
def test_backbone_state_dict_is_the_reference(conf):
    from models import CPM_volumetric
    keys, shapes = _table(np.load(KEYS), 'backbone_conf' if conf else 'backbone')
    model = CPM_volumetric.get_pose_net(_cfg(['MODEL.VOL_CONFIDENCES', str(conf)]), is_train=False)
    sd = model.state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert any(k.startswith('vol_confidences.') for k in keys) == conf
    if conf:
        first = keys.index('vol_confidences.features.0.weight')
        assert keys[first - 1] == 'Mconv5_stage6.bias' and sd['vol_confidences.features.0.weight'].shape == (512, 128, 3, 3)
        with pytest.raises(NotImplementedError, match='never run|not built'):
            model.vol_confidences(torch.zeros(1, 128, 4, 4))
    assert model.hm_size == (64, 64)
    assert CPM_volumetric.get_pose_net(_cfg(['MODEL.HEATMAP_SIZE', '[18, 10]']), is_train=False).hm_size == (10, 18)


def test_model_state_dict_and_frozen_set():
    from models.triangulation import VolumetricTriangulationNet_CPM
    keys, shapes = _table(np.load(KEYS), 'model')
    model = VolumetricTriangulationNet_CPM(_cfg(), is_train=True)
    sd = model.state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert list(model._modules) == ['backbone', 'process_features', 'volume_net']
    assert tuple(model.process_features[0].weight.shape) == (32, 128, 1, 1)
    # the reference's freeze (triangulation.py:512-527): the last three layers of stage 6 train
    for k, p in model.named_parameters():
        want = k.startswith(('backbone.Mconv3_stage6.', 'backbone.Mconv4_stage6.', 'backbone.Mconv5_stage6.',
                             'process_features.', 'volume_net.'))
        assert p.requires_grad == want, k
    assert model.backbone.trainable and model.volume_net.trainable
    other = VolumetricTriangulationNet_CPM(_cfg(), is_train=False)
    other.load_state_dict({k: torch.zeros(s, dtype=sd[k].dtype) for k, s in zip(keys, shapes)}, strict=True)
    assert not other.backbone.trainable and not other.volume_net.trainable
    from models import triangulation
    assert isinstance(triangulation.get_pose_net(_cfg(), is_train=False), VolumetricTriangulationNet_CPM)


def test_backbone_checkpoint_is_loaded_non_strictly(tmp_path):
    from models import CPM
    from models.triangulation import VolumetricTriangulationNet_CPM
    torch.manual_seed(3)
    two_d = CPM.CPM(21)
    path = str(tmp_path / 'cpm.pth.tar')
    sd = {'module.' + k: v for k, v in two_d.state_dict().items()}
    torch.save({'state_dict': sd, 'epoch': 4}, path)
    model = VolumetricTriangulationNet_CPM(_cfg(['MODEL.BACKBONE_MODEL_PATH', path]), is_train=True)
    for k, v in two_d.state_dict().items():
        assert torch.equal(model.backbone.state_dict()[k], v), k


def test_model_and_backbone_refusals():
    from models import CPM_volumetric
    from models.triangulation import VolumetricTriangulationNet, VolumetricTriangulationNet_CPM
    for opts, exc, match in ((['MODEL.VOLUME_AGGREGATION_METHOD', 'conf'], NotImplementedError, 'conf'),
                             (['MODEL.VOLUME_AGGREGATION_METHOD', 'conf_norm'], NotImplementedError, 'conf_norm'),
                             (['MODEL.VOLUME_SIZE', '48'], ValueError, 'multiple of 32'),
                             (['MODEL.BACKBONE_NAME', 'pose_hrnet_volumetric'], ValueError, 'BACKBONE_NAME.*CPM_volumetric'),
                             (['MODEL.ALG_CONFIDENCES', 'True'], NotImplementedError, 'ALG_CONFIDENCES'),
                             (['MODEL.VOL_CONFIDENCES', 'False'], ValueError,
                              'VOL_CONFIDENCES false.*stride-8.*geometrically wrong.*both reference yamls')):
        with pytest.raises(exc, match=match):
            VolumetricTriangulationNet_CPM(_cfg(opts), is_train=False)
    # MODEL.NAME vol keeps its backbone: the CPM one is still refused there
    with pytest.raises(ValueError, match='BACKBONE_NAME.*pose_hrnet_volumetric'):
        VolumetricTriangulationNet(_cfg(['MODEL.NAME', 'vol']), is_train=False)
    with pytest.raises(NotImplementedError, match='ALG_CONFIDENCES'):
        CPM_volumetric.get_pose_net(_cfg(['MODEL.ALG_CONFIDENCES', 'True']), is_train=False)
    model = VolumetricTriangulationNet_CPM(_cfg(['MODEL.VOLUME_SIZE', '32']), is_train=False).eval()
    with pytest.raises(ValueError, match='HIP-device'):
        model(torch.zeros(1, 2, 3, 64, 64), torch.zeros(1, 2, 1, 64, 64), torch.zeros(1, 2, 3, 4))
    backbone = CPM_volumetric.get_pose_net(_cfg(), is_train=False)
    with pytest.raises(NotImplementedError, match='training of CPM is not built'):
        backbone.train()(torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 8, 8))
    with pytest.raises(NotImplementedError, match='eval mode with a gradient required'):
        backbone.eval()(torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 8, 8))
    with pytest.raises(NotImplementedError, match='no flat parameter buffer'):
        CPM_volumetric.get_pose_net(_cfg(), is_train=True, trainable=True).hip()
    with torch.no_grad():
        with pytest.raises(ValueError, match='HIP-device'):
            backbone.eval()(torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 8, 8))
        with pytest.raises(ValueError, match='multiples of 8'):
            backbone(torch.zeros(1, 3, 12, 8), torch.zeros(1, 1, 12, 8))


def test_tools_accept_vol_cpm_and_refuse_what_they_cannot_run(tmp_path):
    train_vol, evaluate_vol, evaluate_3D = _tools()
    mhp_tree.write_tree(tmp_path, {'data_1': 1})
    good = _cfg([], tmp_path)
    train_vol.check_config(good)
    evaluate_vol.check_config(good)
    assert good.MODEL.NAME == 'vol_CPM' and good.MODEL.BACKBONE_NAME == 'CPM_volumetric' and good.MODEL.VOL_CONFIDENCES
    assert list(good.DATASET.DATASET) == ['MHP_CPM_mv'] == list(good.DATASET.TEST_DATASET)
    assert good.LOSS.WITH_HEATMAP_LOSS and good.LOSS.HEATMAP_LOSS_FACTOR == 0.1 and not good.MODEL.HEATMAP_SOFTMAX
    assert good.LOSS.WITH_POSE3D_LOSS and good.LOSS.WITH_VOLUMETRIC_CE_LOSS and good.LOSS.VOLUMETRIC_LOSS_FACTOR == 0.01
    assert good.TRAIN.IMAGES_PER_GPU == 8 and good.TRAIN.LR == 1e-4 and list(good.TRAIN.LR_STEP) == [8, 16, 24]
    assert good.TRAIN.PROCESS_FEATURE_LR == 1e-3 and good.TRAIN.VOLUME_NET_LR == 1e-3
    for opts, exc, match in ((['MODEL.VOL_CONFIDENCES', 'False'], ValueError, 'VOL_CONFIDENCES false'),
                             (['MODEL.VOLUME_AGGREGATION_METHOD', 'conf_norm'], NotImplementedError, 'conf_norm'),
                             (['MODEL.VOLUME_SIZE', '40'], ValueError, 'multiple of 32'),
                             (['MODEL.BACKBONE_NAME', 'pose_hrnet_volumetric'], ValueError, 'BACKBONE_NAME'),
                             (['DATASET.DATASET', "['MHP_mv']"], ValueError, r"DATASET.DATASET.*MHP_CPM_mv"),
                             (['DATASET.TEST_DATASET', "['MHP_CPM_kpt']"], ValueError, 'DATASET.TEST_DATASET'),
                             (['LOSS.WITH_POSE3D_LOSS', 'False'], ValueError, 'WITH_POSE3D_LOSS'),
                             (['LOSS.WITH_BONE_LOSS', 'True'], ValueError, 'WITH_BONE_LOSS')):
        with pytest.raises(exc, match=match):
            train_vol.check_config(_cfg(opts, tmp_path))
    with pytest.raises(ValueError, match='WORLD_SIZE 2'):
        train_vol.check_config(good, world=2)
    with pytest.raises(ValueError, match='annotated_frames'):
        train_vol.check_config(_cfg([], tmp_path / 'nowhere'))
    for opts, exc, match in ((['MODEL.VOL_CONFIDENCES', 'False'], ValueError, 'VOL_CONFIDENCES false'),
                             (['MODEL.VOLUME_AGGREGATION_METHOD', 'conf'], NotImplementedError, 'conf'),
                             (['MODEL.NAME', 'CPM'], ValueError, "MODEL.NAME 'CPM'")):
        with pytest.raises(exc, match=match):
            evaluate_vol.check_config(_cfg(opts, tmp_path))
    with pytest.raises(ValueError, match='--model_path'):
        evaluate_vol.main(['--cfg', YAML, 'DATA_DIR', str(tmp_path)])
    # the vol yaml is served as before, and does not get the CPM reader
    vol = _cfg([], tmp_path, VOL_YAML)
    train_vol.check_config(vol)
    evaluate_vol.check_config(vol)
    with pytest.raises(ValueError, match=r"DATASET.DATASET.*\['MHP_mv'\]"):
        train_vol.check_config(_cfg(['DATASET.DATASET', "['MHP_CPM_mv']"], tmp_path, VOL_YAML))
    with pytest.raises(ValueError, match="MODEL.NAME 'pose_hrnet_softmax'.*MODEL.NAME 'vol'"):
        train_vol.check_config(_cfg(['MODEL.NAME', 'pose_hrnet_softmax'], tmp_path, VOL_YAML))
    # the triangulating tool still refuses both
    for name in ('vol', 'vol_CPM'):
        with pytest.raises(ValueError, match="MODEL.NAME '{}' is not built.*evaluate_vol.py".format(name)):
            evaluate_3D.build_model(name)


def test_optimizer_groups_hold_the_three_stage_six_layers():
    from models.triangulation import VolumetricTriangulationNet_CPM
    train_vol = _tools()[0]
    cfg = _cfg()
    model = VolumetricTriangulationNet_CPM(cfg, is_train=True)
    opt = train_vol.build_optimizer(cfg, model)
    assert [g['name'] for g in opt.param_groups] == ['backbone', 'process_features', 'volume_net']
    assert [g['lr'] for g in opt.param_groups] == [1e-4, 1e-3, 1e-3]
    want = [p for n in ('Mconv3_stage6', 'Mconv4_stage6', 'Mconv5_stage6') for p in getattr(model.backbone, n).parameters()]
    assert len(opt.param_groups[0]['params']) == 6
    assert all(a is b for a, b in zip(opt.param_groups[0]['params'], want))


@pytest.mark.parametrize('case,hm', [('b', (10, 18)), ('c', (4, 4))])
def test_the_commuted_feature_path_is_the_reference_order(case, hm):
    """conv then up-sample equals up-sample then conv in float64: the four bilinear weights sum to 1, so the bias passes.
    tests/golden/make_golden_vol_cpm.py holds the restated backbone to the reference's module at these cases"""
    z = np.load(KEYS)
    assert float(z[case + '/agree']) <= 1e-10 and float(z[case + '/commuted']) <= 1e-12
    state = R.to_torch(R.fill_state_dict(), torch.float64)
    img, cm = (torch.tensor(a) for a in R.inputs(case))
    w, b = (torch.tensor(a) for a in VC.process_weights())
    with torch.no_grad():
        low, heat, feat = VC.backbone(state, img, cm, hm)
        want = R.forward(state, img, cm)
        a, r = VC.features_commuted(feat, w, b, hm), VC.features_reference(feat, w, b, hm)
    assert len(low) == 5 and all(torch.equal(x, y) for x, y in zip(low, want[:5]))
    assert torch.equal(heat, VC.upsample(want[5], hm)) and tuple(heat.shape[2:]) == hm
    assert tuple(feat.shape[1:]) == (128,) + tuple(want[5].shape[2:]) and tuple(a.shape) == (img.shape[0], 32) + hm
    assert R.rel(a.numpy(), r.numpy()) <= 1e-12
    # without the bias passing through (weights that do not sum to 1) the orders would differ: nearest-exact does not
    # blend, bicubic's weights sum to 1 as well - so the check is that a NON-affine map in between breaks it
    assert R.rel(VC.upsample(torch.relu(torch.nn.functional.conv2d(feat, w, b)), hm).numpy(),
                 torch.relu(r).numpy()) > 1e-6
