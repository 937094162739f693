"""Host side of the volumetric model (MODEL.NAME vol): the new C ABI entries; the state_dict keys and shapes of
pose_hrnet_volumetric and of VolumetricTriangulationNet against the reference's (tests/golden/vol_state_keys.npz,
written by tests/golden/make_golden_vol.py); the frozen set; every refusal of the model and of tools/train_vol.py and
tools/evaluate_vol.py on a fake MHP tree (tests/mhp_tree.py); the shipped yaml; the old tools still refuse `vol`; the
projection rule of core/function_vol.py against the reader's own heat-map joints; the coordinate volume of
tests/vol_ref.py against utils.volumetric.build_coord_volumes. No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import mhp_tree
import vol_ref as VOL

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = os.path.join(HERE, 'golden', 'vol_state_keys.npz')
YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_VolTriangulation_w32_v1.yaml')
NEW = ('hrnet_pointwise_nchw_supported', 'hrnet_pointwise_nchw', 'hrnet_pointwise_nchw_parts', 'hrnet_pointwise_nchw_bwd')


def _tools():
    tools = os.path.join(mhp_tree.PKG, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import evaluate_3D
    import evaluate_vol
    import train3D
    import train_vol
    return train_vol, evaluate_vol, train3D, evaluate_3D


def _cfg(opts=(), data='.'):
    return mhp_tree.config(data, list(opts), YAML)


def _table(z, name):
    keys = [str(k) for k in z[name + '_keys']]
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(z[name + '_shapes'], z[name + '_ndims'])]
    return keys, shapes


def test_abi_entries_and_queries():
    from hipnet import _capi as C
    assert C.ABI_VERSION == 2 and C.call('hrnet_abi_version') == 2
    for name in NEW:
        assert name in C.EXPORTED and hasattr(C.lib(), name), name
    assert C.call('hrnet_pointwise_nchw_supported', C.HR_F32, 480, 32) == 1
    assert C.call('hrnet_pointwise_nchw_supported', C.HR_F32, 3, 1) == 1
    assert C.call('hrnet_pointwise_nchw_supported', C.HR_BF16, 480, 32) == 0
    assert C.call('hrnet_pointwise_nchw_supported', C.HR_F32, 480, 65) == 0
    assert C.call('hrnet_pointwise_nchw_supported', C.HR_F32, 0, 32) == 0
    assert C.call('hrnet_pointwise_nchw_parts', 1, 1) == 1 and C.call('hrnet_pointwise_nchw_parts', 2, 4096) == 16
    assert C.call('hrnet_pointwise_nchw_parts', 12, 4096) == 96 and C.call('hrnet_pointwise_nchw_parts', 0, 16) == 0
    # refused before any launch: no device is needed to be told so
    with pytest.raises(RuntimeError, match='null pointer'):
        C.call('hrnet_pointwise_nchw', C.HR_F32, None, None, None, None, 1, 4, 4, 16, None)
    with pytest.raises(RuntimeError, match='only f32'):
        C.call('hrnet_pointwise_nchw_bwd', C.HR_BF16, None, None, None, None, None, None, None, 0, 1, 4, 4, 16, None)


@pytest.mark.parametrize('conf', [False, True])
def test_backbone_state_dict_is_the_reference(conf):
    from models import pose_hrnet_volumetric
    z = np.load(KEYS)
    keys, shapes = _table(z, 'backbone_conf' if conf else 'backbone')
    model = pose_hrnet_volumetric.get_pose_net(_cfg(['MODEL.VOL_CONFIDENCES', str(conf)]), is_train=False)
    sd = model.state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert any(k.startswith('vol_confidences.') for k in keys) == conf
    if conf:
        assert sd['vol_confidences.features.0.weight'].shape == (512, 480, 3, 3)
        assert sd['vol_confidences.head.4.weight'].shape == (32, 256)
        first = keys.index('vol_confidences.features.0.weight')
        assert keys[first - 1].startswith('stage4.') and keys[first + 20] == 'last_layer.0.weight'
    with pytest.raises(NotImplementedError, match='ALG_CONFIDENCES'):
        pose_hrnet_volumetric.get_pose_net(_cfg(['MODEL.ALG_CONFIDENCES', 'True']), is_train=False)


def test_model_state_dict_and_frozen_set():
    from models.triangulation import VolumetricTriangulationNet
    z = np.load(KEYS)
    keys, shapes = _table(z, 'model')
    model = VolumetricTriangulationNet(_cfg(), is_train=True)
    sd = model.state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    # the reference's freeze (triangulation.py:330-343): stage4 and the head train, the temperature does not
    for k, p in model.named_parameters():
        want = k.startswith(('backbone.stage4.', 'backbone.last_layer.', 'process_features.', 'volume_net.'))
        assert p.requires_grad == want, k
    assert not model.backbone.trainable_temp.requires_grad
    assert model.volume_net.trainable
    # a reference-shaped checkpoint loads strictly, and without is_train nothing is frozen or trainable-only
    other = VolumetricTriangulationNet(_cfg(), is_train=False)
    other.load_state_dict({k: torch.zeros(s, dtype=sd[k].dtype) for k, s in zip(keys, shapes)}, strict=True)
    assert not other.volume_net.trainable


def test_backbone_checkpoint_is_loaded_non_strictly(tmp_path):
    from models import pose_hrnet_softmax
    from models.triangulation import VolumetricTriangulationNet
    torch.manual_seed(3)
    two_d = pose_hrnet_softmax.get_pose_net(_cfg(), is_train=False)
    path = str(tmp_path / 'backbone.pth.tar')
    sd = {'module.' + k: v for k, v in two_d.state_dict().items()}
    sd['module.not_a_key'] = torch.zeros(1)
    torch.save({'state_dict': sd, 'epoch': 4}, path)
    model = VolumetricTriangulationNet(_cfg(['MODEL.BACKBONE_MODEL_PATH', path]), is_train=True)
    for k, v in two_d.state_dict().items():
        assert torch.equal(model.backbone.state_dict()[k], v), k


def test_model_refusals():
    from models.triangulation import VolumetricTriangulationNet
    for opts, exc, match in ((['MODEL.VOLUME_AGGREGATION_METHOD', 'conf'], NotImplementedError, 'conf'),
                             (['MODEL.VOLUME_AGGREGATION_METHOD', 'conf_norm'], NotImplementedError, 'conf_norm'),
                             (['MODEL.VOLUME_SIZE', '48'], ValueError, 'multiple of 32'),
                             (['MODEL.VOLUME_SIZE', '16'], ValueError, 'multiple of 32'),
                             (['MODEL.BACKBONE_NAME', 'pose_resnet'], ValueError, 'BACKBONE_NAME'),
                             (['MODEL.ALG_CONFIDENCES', 'True'], NotImplementedError, 'ALG_CONFIDENCES')):
        with pytest.raises(exc, match=match):
            VolumetricTriangulationNet(_cfg(opts), is_train=False)
    model = VolumetricTriangulationNet(_cfg(['MODEL.VOLUME_SIZE', '32']), is_train=False).eval()
    with pytest.raises(ValueError, match='HIP-device'):
        model(torch.zeros(1, 2, 3, 64, 64), torch.zeros(1, 2, 3, 4))
    with pytest.raises(ValueError, match='HIP-device'):
        model.lift(torch.zeros(2, 21, 16, 16), torch.zeros(2, 480, 16, 16), torch.zeros(1, 2, 3, 4))


def test_tools_refuse_what_they_cannot_run(tmp_path):
    train_vol, evaluate_vol, train3D, evaluate_3D = _tools()
    mhp_tree.write_tree(tmp_path, {'data_1': 1})
    good = _cfg([], tmp_path)
    train_vol.check_config(good)                           # the shipped yaml on an existing tree passes
    evaluate_vol.check_config(good)
    assert good.MODEL.NAME == 'vol' and good.MODEL.BACKBONE_NAME == 'pose_hrnet_volumetric'
    assert good.MODEL.VOLUME_AGGREGATION_METHOD == 'softmax' and not good.MODEL.VOL_CONFIDENCES
    assert good.MODEL.VOLUME_SIZE == 64 and good.MODEL.CUBOID_SIZE == 500.0
    assert good.LOSS.WITH_POSE3D_LOSS and good.LOSS.WITH_VOLUMETRIC_CE_LOSS and good.LOSS.VOLUMETRIC_LOSS_FACTOR == 0.01
    assert good.TRAIN.IMAGES_PER_GPU == 3 and good.TRAIN.LR == 1e-4
    assert good.TRAIN.PROCESS_FEATURE_LR == 1e-3 and good.TRAIN.VOLUME_NET_LR == 1e-3
    for opts, exc, match in ((['MODEL.NAME', 'pose_hrnet_softmax'], ValueError, "MODEL.NAME 'pose_hrnet_softmax'"),
                             (['MODEL.NAME', 'alg'], ValueError, "MODEL.NAME 'alg'"),
                             (['MODEL.VOLUME_AGGREGATION_METHOD', 'conf_norm'], NotImplementedError, 'conf_norm'),
                             (['MODEL.VOLUME_SIZE', '40'], ValueError, 'multiple of 32'),
                             (['MODEL.BACKBONE_NAME', 'pose_hrnet'], ValueError, 'BACKBONE_NAME'),
                             (['DATASET.DATASET', "['MHP_kpt']"], ValueError, 'DATASET.DATASET'),
                             (['DATASET.TEST_DATASET', "['MHP']"], ValueError, 'DATASET.TEST_DATASET'),
                             (['LOSS.WITH_POSE3D_LOSS', 'False'], ValueError, 'WITH_POSE3D_LOSS'),
                             (['LOSS.WITH_BONE_LOSS', 'True'], ValueError, 'WITH_BONE_LOSS'),
                             (['LOSS.WITH_KCS_LOSS', 'True'], ValueError, 'WITH_KCS_LOSS')):
        with pytest.raises(exc, match=match):
            train_vol.check_config(_cfg(opts, tmp_path))
    with pytest.raises(ValueError, match='WORLD_SIZE 2'):
        train_vol.check_config(good, world=2)
    with pytest.raises(ValueError, match='annotated_frames'):
        train_vol.check_config(_cfg([], tmp_path / 'nowhere'))
    for opts, exc, match in ((['MODEL.NAME', 'pose_hrnet'], ValueError, "MODEL.NAME 'pose_hrnet'"),
                             (['MODEL.VOLUME_AGGREGATION_METHOD', 'conf'], NotImplementedError, 'conf'),
                             (['MODEL.VOLUME_SIZE', '40'], ValueError, 'multiple of 32')):
        with pytest.raises(exc, match=match):
            evaluate_vol.check_config(_cfg(opts, tmp_path))
    # the command line: the refusal comes before any device work (this machine may have no device at all)
    with pytest.raises(ValueError, match='annotated_frames'):
        train_vol.main(['--cfg', YAML, 'DATA_DIR', str(tmp_path / 'nowhere')])
    with pytest.raises(ValueError, match='--views'):
        train_vol.main(['--cfg', YAML, '--views', '[1]', 'DATA_DIR', str(tmp_path)])
    # evaluate_vol never evaluates random weights: no --model_path, or a missing one, is refused before any device work
    with pytest.raises(ValueError, match='--model_path'):
        evaluate_vol.main(['--cfg', YAML, 'DATA_DIR', str(tmp_path)])
    with pytest.raises(ValueError, match='no such file'):
        evaluate_vol.main(['--cfg', YAML, '--model_path', str(tmp_path / 'none.pth.tar'), 'DATA_DIR', str(tmp_path)])
    # the triangulating tools still refuse the model
    with pytest.raises(ValueError, match="MODEL.NAME 'vol'"):
        train3D.check_config(_cfg([], tmp_path))
    with pytest.raises(ValueError, match="MODEL.NAME 'vol' is not built"):
        evaluate_3D.build_model('vol')


def test_optimizer_groups_and_schedule():
    train_vol = _tools()[0]
    from models.triangulation import VolumetricTriangulationNet
    cfg = _cfg(['TRAIN.LR_STEP', '[2, 4]', 'TRAIN.LR_FACTOR', '0.1'])
    model = VolumetricTriangulationNet(cfg, is_train=True)
    opt = train_vol.build_optimizer(cfg, model)
    assert [g['name'] for g in opt.param_groups] == ['backbone', 'process_features', 'volume_net']
    assert [g['initial_lr'] for g in opt.param_groups] == [1e-4, 1e-3, 1e-3]
    assert all(g['weight_decay'] == 0 for g in opt.param_groups)
    held = {id(p) for g in opt.param_groups for p in g['params']}
    assert held == {id(p) for p in model.parameters() if p.requires_grad}
    assert [train_vol.lr_factor(cfg, e) for e in range(5)] == pytest.approx([1, 1, 0.1, 0.1, 0.01])
    crit = train_vol.build_criterion(cfg)
    assert sorted(crit) == ['pose3d_loss', 'volumetric_ce_loss']


def test_projection_rule_lands_on_the_readers_heatmap_joints(tmp_path):
    """world joints through A K [R|t] of core/function_vol.py are the reader's `pose2d` heat-map coordinates (the
    tolerance of tests/test_mhp_mv_cpu.py for the same reader's geometry, 1e-6, relative to the 64-pixel map)"""
    from core.function_vol import heatmap_projections
    from dataset.mhp import MHP_mv, collate_rgb
    mhp_tree.write_tree(tmp_path, {'data_17': 3})
    ds = MHP_mv(mhp_tree.config(tmp_path, ['WORKERS', '0'], mhp_tree.SOFTMAX_YAML), 'eval')
    b = collate_rgb([ds[0], ds[2]])
    proj = heatmap_projections(b['intrinsic_matrix'], b['extrinsic_matrices'], b['hm_inverse'])
    assert proj.shape == (2, 4, 3, 4) and proj.dtype == torch.float64
    X = torch.cat([b['pose3d'].double(), torch.ones(2, 21, 1, dtype=torch.float64)], dim=2)      # (B, K, 4)
    uvw = torch.einsum('bvij,bkj->bvki', proj, X)
    uv = (uvw[..., :2] / uvw[..., 2:]).reshape(8, 21, 2).numpy()
    # pose2d is stored as float32: one rounding of a coordinate below 2^10 on top of the reader's 1e-6
    assert np.allclose(uv, b['pose2d'].double().numpy(), rtol=0, atol=1e-6 * 64 + 2.0 ** -14)


def test_restated_coordinate_volume_is_build_coord_volumes():
    from utils.volumetric import build_coord_volumes
    base = np.array([[10.0, -5.0, 20.0], [-94.0, 9.0, 600.0]])
    for thetas in ([0.0, 0.0], [0.0, 1.0], [2.5, 6.0]):
        ours = build_coord_volumes(torch.from_numpy(base).float(), 100.0, 32, thetas).double().numpy()
        ref = VOL.coord_volumes(base, 100.0, 32, thetas)
        # float32 arithmetic on coordinates up to 650: a few roundings of 2^-24 * 650 each
        assert ours.shape == ref.shape == (2, 32, 32, 32, 3)
        assert np.abs(ours - ref).max() <= 8 * 2.0 ** -24 * 650.0
    assert np.array_equal(build_coord_volumes(torch.from_numpy(base).float(), 100.0, 32, 0.0).numpy(),
                          build_coord_volumes(torch.from_numpy(base).float(), 100.0, 32, [0.0, 0.0]).numpy())
