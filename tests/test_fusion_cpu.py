"""Host side of the cross-view fusion model (MODEL.NAME multiview_pose_hrnet): the pair index n(i, j) against hand-written
tables, tests/fusion_ref.py against explicit loops, the model's state-dict keys, every refusal of
tools/train_fusion.check_config, CPU tensors refused, the new C entry points. No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import fusion_ref as R
import mhp_tree

YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_HRNet_w32_fusion_v1.yaml')
SMALL = ['MODEL.IMAGE_SIZE', '[32, 32]', 'MODEL.HEATMAP_SIZE', '[8, 8]']

# n(i, j) written out by hand: row i, column j; None on the diagonal
TABLES = {2: [[None, 0], [1, None]],
          3: [[None, 0, 1], [2, None, 3], [4, 5, None]],
          4: [[None, 0, 1, 2], [3, None, 4, 5], [6, 7, None, 8], [9, 10, 11, None]]}


def _cfg(opts=(), data_dir=None):
    from config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list((['DATA_DIR', str(data_dir)] if data_dir is not None else []) + list(opts))
    return cfg


@pytest.fixture(scope='module')
def train_fusion():
    tools = os.path.join(mhp_tree.PKG, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import train_fusion as T
    return T


@pytest.mark.parametrize('V', [2, 3, 4])
def test_pair_index_tables(V):
    from models.multiview_pose_hrnet import pair_index
    seen = []
    for i in range(V):
        for j in range(V):
            if i == j:
                with pytest.raises(ValueError):
                    pair_index(i, j, V)
                continue
            assert pair_index(i, j, V) == TABLES[V][i][j] == R.pair_index(i, j, V)
            seen.append(pair_index(i, j, V))
    assert seen == list(range(V * (V - 1)))          # the reference's running index: target-major, sources ascending


def test_fusion_ref_against_loops():
    H, Ws, _ = R.inputs(2, 3, 2, 4, seed=5)
    got = R.fusion_ref(H, Ws, 0.4, 0.2).numpy()
    want = R.fusion_loops(H.numpy(), [w.numpy() for w in Ws], 0.4, 0.2)
    assert got.shape == (2, 3, 2, 4)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    # the formula is not symmetric in the pair index: swapping two matrices changes the result
    swapped = R.fusion_ref(H, [Ws[1], Ws[0]] + Ws[2:]).numpy()
    assert np.abs(swapped - want).max() > 1e-3


def test_state_dict_keys_shapes_and_order():
    from models.multiview_pose_hrnet import Aggregation, ChannelWiseFC, MultiViewPoseNet, get_pose_net
    torch.manual_seed(0)
    model = get_pose_net(_cfg(SMALL))
    assert isinstance(model, MultiViewPoseNet) and isinstance(model.aggre_layer, Aggregation)
    assert all(isinstance(m, ChannelWiseFC) for m in model.aggre_layer.aggre)
    keys = list(model.state_dict())
    fusion = [k for k in keys if not k.startswith('backbone.')]
    assert fusion == ['aggre_layer.aggre.{}.weight.weight'.format(n) for n in range(12)]
    assert keys[-12:] == fusion and keys[0].startswith('backbone.')          # backbone first, as the reference
    P = 64
    for k in fusion:
        w = model.state_dict()[k]
        assert tuple(w.shape) == (P, P) and w.dtype == torch.float32
        assert float(w.abs().max()) <= 1.0 / np.sqrt(P) + 1e-7 and float(w.std()) > 0.03     # nn.Linear's default draw
    assert model.aggre_layer.weights == [0.4, 0.2, 0.2, 0.2]
    # frozen as the reference: stage4 and last_layer train, the rest of the backbone does not
    for name, p in model.backbone.named_parameters():
        assert p.requires_grad == name.startswith(('stage4.', 'last_layer.')), name
    assert all(p.requires_grad for p in model.aggre_layer.parameters())
    # a state dict with the reference's keys loads strictly
    model.load_state_dict({k: v.clone() for k, v in model.state_dict().items()}, strict=True)


def test_cpu_tensors_refused():
    from models.multiview_pose_hrnet import get_pose_net, view_fusion
    model = get_pose_net(_cfg(SMALL))
    with pytest.raises(ValueError, match='no CPU path'):
        model(torch.zeros(1, 4, 3, 32, 32))
    with pytest.raises(ValueError, match='no CPU path'):
        view_fusion(torch.zeros(1, 2, 3, 4, 4), [torch.zeros(16, 16)] * 2)
    with pytest.raises(ValueError, match='no CPU path'):
        model.aggre_layer(torch.zeros(1, 4, 21, 8, 8))


def test_aggregation_refuses_unequal_other_weights():
    from models.multiview_pose_hrnet import Aggregation
    with pytest.raises(ValueError, match='ONE for every other view'):
        Aggregation(_cfg(SMALL), weights=[0.4, 0.3, 0.2, 0.1])


def test_check_config_accepts_the_yaml(train_fusion, tmp_path):
    mhp_tree.write_tree(tmp_path, {'data_1': 1})
    train_fusion.check_config(_cfg(data_dir=tmp_path))
    train_fusion.check_config(_cfg(SMALL, data_dir=tmp_path))


@pytest.mark.parametrize('opts, world, message', [
    (['MODEL.NAME', 'vol'], 1, 'MODEL.NAME'),
    (['MODEL.NAME', 'pose_hrnet_softmax'], 1, 'MODEL.NAME'),
    (['DATASET.DATASET', "['MHP_kpt']"], 1, 'DATASET.DATASET'),
    (['DATASET.TEST_DATASET', "['MHP']"], 1, 'DATASET.TEST_DATASET'),
    (['MODEL.HEATMAP_SIZE', '[64, 48]'], 1, 'square'),
    (['MODEL.HEATMAP_SIZE', '[32, 32]'], 1, 'IMAGE_SIZE'),
    (['MODEL.BACKBONE_NAME', 'resnet'], 1, 'BACKBONE_NAME'),
    (['MODEL.AGGRE', 'False'], 1, 'AGGRE'),
    (['LOSS.WITH_POSE2D_LOSS', 'False'], 1, 'both false'),
    ([], 2, 'WORLD_SIZE'),
])
def test_check_config_refusals(train_fusion, tmp_path, opts, world, message):
    mhp_tree.write_tree(tmp_path, {'data_1': 1})
    with pytest.raises(ValueError, match=message):
        train_fusion.check_config(_cfg(opts, data_dir=tmp_path), world)


def test_check_config_refuses_a_missing_tree(train_fusion, tmp_path):
    with pytest.raises(ValueError, match='not found'):
        train_fusion.check_config(_cfg(data_dir=tmp_path / 'nowhere'))


def test_new_symbols_exported():
    from hipnet import _capi as C
    assert C.ABI_VERSION == 2
    for name in ('hrnet_view_fusion_supported', 'hrnet_view_fusion', 'hrnet_view_fusion_bwd'):
        assert name in C.EXPORTED and hasattr(C.lib(), name)
    assert C.lib().hrnet_abi_version() == 2
    assert C.call('hrnet_view_fusion_supported', C.HR_F32, 4, 4096) == 1
    assert C.call('hrnet_view_fusion_supported', C.HR_F32, 2, 1) == 1
    assert C.call('hrnet_view_fusion_supported', C.HR_F32, 5, 4096) == 0
    assert C.call('hrnet_view_fusion_supported', C.HR_F32, 1, 4096) == 0
    assert C.call('hrnet_view_fusion_supported', C.HR_BF16, 4, 4096) == 0
    assert C.call('hrnet_view_fusion_supported', C.HR_F32, 4, 0) == 0


def test_traffic_model_counts():
    """the byte / FLOP function next to the timing script, at the workload's size: 12 matrices of 64 MiB"""
    tools = os.path.join(mhp_tree.PKG, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import bench_fusion as BF
    t = BF.traffic(B=1, V=4, K=21, P=4096)
    wbytes = 12 * 4096 * 4096 * 4
    act = 1 * 4 * 21 * 4096 * 4
    assert t['forward']['bytes'] == wbytes + 2 * act and t['dH']['bytes'] == wbytes + 2 * act
    assert t['dW']['bytes'] == wbytes + 2 * act
    assert t['forward']['flops'] == t['dH']['flops'] == t['dW']['flops'] == 2 * 21 * 4096 * 4096 * 12
    assert t['forward']['bound'] == 'bandwidth' and BF.traffic(8, 4, 21, 4096)['forward']['bound'] == 'compute'
