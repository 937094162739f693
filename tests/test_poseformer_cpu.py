"""Host side of pose_hrnet_transformer (the PoseFormer head): tests/poseformer_ref.py against the fixture of the
reference's own run, the model's state dict, freezing, checkpoint loading, every refusal, the C entry points, the yaml,
the MHP_seq branch of core.function and the bench tool's cost model. No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mhp_tree
import poseformer_ref as R

YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_HRNet_w32_trainable_softmax_pose2dloss_PoseFormer_v1.yaml')
SMALL = ['MODEL.IMAGE_SIZE', '[64, 64]', 'MODEL.HEATMAP_SIZE', '[16, 16]']
TF_NAMES = ['hrnet_tf_supported', 'hrnet_tf_layernorm_scratch', 'hrnet_tf_layernorm', 'hrnet_tf_layernorm_bwd',
            'hrnet_tf_linear', 'hrnet_tf_linear_bwd', 'hrnet_tf_attention', 'hrnet_tf_attention_bwd',
            'hrnet_tf_frame_mean', 'hrnet_tf_frame_mean_bwd', 'hrnet_tf_add_rows']


def _cfg(opts=()):
    from config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(list(opts))
    return cfg


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'poseformer.npz'))


@pytest.fixture(scope='module')
def model():
    from models import pose_hrnet_transformer
    torch.manual_seed(0)
    return pose_hrnet_transformer.get_pose_net(_cfg(SMALL), is_train=True)


@pytest.mark.parametrize('S,F,J', R.SHAPES)
def test_restatement_against_the_fixture(golden, S, F, J):
    """float64: 1e-10 of max|.| against the reference's float64 run; float32: the recorded e32 figures reproduce (they are
    what the GPU bounds are built from) and stay of the order of float32 rounding"""
    t = R.tag(S, F, J)
    p, g = golden[t + '/p'], golden[t + '/g']
    p2, g2 = R.inputs(S, F, J, int(golden['seed']))
    assert np.array_equal(p, p2) and np.array_equal(g, g2)
    state = R.fill_state_dict(R.head_keys(F, J), int(golden['seed']))
    y, dp, grads = R.run(p, g, state, torch.float64)
    assert R.rel(y, golden[t + '/y64']) <= 1e-10 and R.rel(dp, golden[t + '/dp64']) <= 1e-10
    wmax = float(golden[t + '/gmax/weighted_mean.weight'])
    for k in R.STORED:
        denom = wmax if k == 'weighted_mean.bias' else float(golden[t + '/gmax/' + k])
        assert R.rel(R.sample(grads[k]), golden[t + '/grad/' + k], denom) <= 1e-9, k
        assert np.isclose(np.abs(grads[k]).max(), float(golden[t + '/gmax/' + k]), rtol=1e-9, atol=1e-12 * wmax), k
    # exactly zero in exact arithmetic: weighted_mean.bias, and the k third of every qkv.bias
    assert np.abs(grads['weighted_mean.bias']).max() <= 1e-12 * wmax
    for k in ('Spatial_blocks.1.attn.qkv.bias', 'blocks.2.attn.qkv.bias'):
        third = grads[k].size // 3
        assert np.abs(grads[k][third:2 * third]).max() <= 1e-12 * np.abs(grads[k]).max(), k
    y32, dp32, _ = R.run(p, g, state, torch.float32)
    e32 = golden[t + '/e32']
    assert R.rel(y32, golden[t + '/y64']) <= 5e-6 and R.rel(dp32, golden[t + '/dp64']) <= 5e-6
    assert e32[0] <= 5e-6 and e32[1] <= 5e-6
    assert R.rel(golden[t + '/y32'], golden[t + '/y64']) <= 5e-6           # the reference's own float32 run


def test_state_dict_keys_shapes_and_order(golden, model):
    t = R.tag(4, 9, 21)
    want = [(str(k), tuple(int(v) for v in s[:max(1, int(np.count_nonzero(s)))]))
            for k, s in zip(golden[t + '/keys'], golden[t + '/shapes'])]
    assert want == R.head_keys(9, 21) and len(want) == 110
    sd = model.state_dict()
    keys = list(sd)
    assert [(k, tuple(sd[k].shape)) for k in keys if not k.startswith('backbone.')] == want
    assert keys[:2] == ['Spatial_pos_embed', 'Temporal_pos_embed'] and keys[2].startswith('backbone.')
    first_head = keys.index('Spatial_patch_to_embedding.weight')
    assert all(k.startswith('backbone.') for k in keys[2:first_head])
    assert not any(k.startswith('backbone.') for k in keys[first_head:])
    assert sum(int(np.prod(s)) for _, s in want) == 14552276
    assert float(model.Spatial_pos_embed.detach().abs().max()) == 0 and float(model.Temporal_pos_embed.detach().abs().max()) == 0
    assert model.head[0].eps == 1e-5 and model.Spatial_norm.eps == model.blocks[0].norm1.eps == 1e-6
    assert [round(b.drop_path, 6) for b in model.blocks] == [round(r, 6) for r in R.drop_rates()]
    assert [b.drop_path for b in model.Spatial_blocks] == [b.drop_path for b in model.blocks]
    for holder in (model.blocks[0], model.blocks[0].attn, model.blocks[0].mlp):
        with pytest.raises(NotImplementedError):
            holder(torch.zeros(1, 9, 672))


def test_reference_shaped_checkpoint_loads_strictly(model):
    from models import pose_hrnet_softmax, pose_hrnet_transformer
    cfg = _cfg(SMALL)
    backbone = pose_hrnet_softmax.get_pose_net(cfg, is_train=False).state_dict()
    head = R.to_torch(R.fill_state_dict(R.head_keys(9, 21)), torch.float32)
    ckpt = {'Spatial_pos_embed': head['Spatial_pos_embed'], 'Temporal_pos_embed': head['Temporal_pos_embed']}
    ckpt.update({'backbone.' + k: v for k, v in backbone.items()})
    ckpt.update({k: head[k] for k, _ in R.head_keys(9, 21) if not k.endswith('pos_embed')})      # the reference's order
    fresh = pose_hrnet_transformer.get_pose_net(cfg, is_train=False)
    assert list(ckpt) == list(fresh.state_dict())
    fresh.load_state_dict(ckpt, strict=True)
    assert torch.equal(fresh.head[1].weight, head['head.1.weight'])
    assert all(p.requires_grad for k, p in fresh.named_parameters() if k != 'backbone.trainable_temp')   # is_train False


def test_frozen_set(model):
    trains = {k for k, p in model.named_parameters() if p.requires_grad}
    want = {k for k, _ in model.named_parameters()
            if not k.startswith('backbone.') or k.startswith(('backbone.stage4.', 'backbone.last_layer.'))}
    assert trains == want and 'backbone.trainable_temp' not in trains
    assert any(k.startswith('backbone.stage4.') for k in trains) and any(k.startswith('backbone.last_layer.') for k in trains)
    from utils.utils import get_optimizer
    opt = get_optimizer(_cfg(SMALL), model)
    assert isinstance(opt, torch.optim.Adam)
    assert {id(p) for g in opt.param_groups for p in g['params']} == {id(p) for p in model.parameters() if p.requires_grad}


def test_backbone_checkpoint_is_loaded_non_strictly(tmp_path):
    from models import pose_hrnet_softmax, pose_hrnet_transformer
    cfg = _cfg(SMALL)
    torch.manual_seed(1)
    src = pose_hrnet_softmax.get_pose_net(cfg, is_train=False)
    state = {'module.' + k: v + 0.25 for k, v in src.state_dict().items() if k.startswith(('conv1.', 'stage4.'))}
    state['module.not_a_key'] = torch.zeros(1)
    path = str(tmp_path / 'backbone.pth.tar')
    torch.save({'state_dict': state, 'epoch': 3}, path)
    m = pose_hrnet_transformer.get_pose_net(_cfg(SMALL + ['MODEL.BACKBONE_MODEL_PATH', path]), is_train=True)
    assert torch.equal(m.backbone.conv1.weight, src.conv1.weight + 0.25)
    torch.save(state, path)                                       # a bare state dict loads as well
    m = pose_hrnet_transformer.get_pose_net(_cfg(SMALL + ['MODEL.BACKBONE_MODEL_PATH', path]), is_train=True)
    assert torch.equal(m.backbone.conv1.weight, src.conv1.weight + 0.25)
    # is_train False: the path is not read (reference :126)
    pose_hrnet_transformer.get_pose_net(_cfg(SMALL + ['MODEL.BACKBONE_MODEL_PATH', str(tmp_path / 'missing')]),
                                        is_train=False)


def test_refusals(model):
    from hipnet import transformer as T
    from models import pose_hrnet_transformer as M
    with pytest.raises(ValueError, match='HIP-device'):
        model(torch.zeros(1, 9, 3, 64, 64))
    with pytest.raises(ValueError, match='HIP-device'):
        model.head_forward(torch.zeros(1, 9, 21, 2))
    with pytest.raises(ValueError, match='INIT_WEIGHTS'):
        M.get_pose_net(_cfg(SMALL + ['MODEL.INIT_WEIGHTS', 'True']), is_train=True)
    with pytest.raises(ValueError, match='frames'):
        M.get_pose_net(_cfg(SMALL + ['DATASET.SEQ_IDX', str(list(range(65)))]), is_train=True)
    with pytest.raises(ValueError, match='NUM_JOINTS'):
        M.get_pose_net(_cfg(SMALL + ['DATASET.NUM_JOINTS', '33', 'MODEL.NUM_JOINTS', '33']), is_train=True)
    with pytest.raises(ValueError, match='BACKBONE_NAME'):
        M.get_pose_net(_cfg(SMALL + ['MODEL.BACKBONE_NAME', 'pose_resnet']), is_train=True)
    c = torch.zeros(4, 32)
    for call in (lambda: T.layer_norm(c, c[0], c[0], 1e-6), lambda: T.linear(c, torch.zeros(8, 32)),
                 lambda: T.attention(torch.zeros(1, 4, 96), 8, 1.0), lambda: T.frame_mean(torch.zeros(2, 4, 8), c[0, :4]),
                 lambda: T.add_rows(c, c[:2])):
        with pytest.raises(ValueError, match='HIP-device'):
            call()
    # eval mode with a gradient required: the message the other models give, before any device work
    src = open(os.path.join(mhp_tree.PKG, 'lib', 'models', 'pose_hrnet_transformer.py')).read()
    assert 'eval mode with a gradient required is refused' in src


def test_abi_names_are_exported_and_resolve():
    from hipnet import _capi as C
    lib = C.lib()
    for name in TF_NAMES:
        assert name in C.EXPORTED and hasattr(lib, name), name
    assert C.ABI_VERSION == 2 and C.call('hrnet_abi_version') == 2
    assert C.call('hrnet_tf_supported', 2, 21, 4) == 1 and C.call('hrnet_tf_supported', 2, 9, 84) == 1
    assert C.call('hrnet_tf_supported', 2, 65, 4) == 0 and C.call('hrnet_tf_supported', 2, 9, 129) == 0
    assert C.call('hrnet_tf_layernorm_scratch', 36, 672) == 72 + 1344
    assert C.call('hrnet_tf_layernorm_scratch', 1 << 22, 65536) == (2 << 22) + 65536 * 2 * 65536      # a 64-bit return
    with pytest.raises(RuntimeError, match='N = 65'):
        C.call('hrnet_tf_attention', 1, 1, 1, 65, 8, 4, 1.0, None)
    build = open(os.path.join(mhp_tree.PKG, 'build.py')).read()
    assert "'transformer.hip'" in build


def test_yaml_values():
    cfg = _cfg()
    assert cfg.MODEL.NAME == 'pose_hrnet_transformer' and cfg.MODEL.BACKBONE_NAME == 'pose_hrnet_softmax'
    assert cfg.MODEL.BACKBONE_MODEL_PATH == '' and cfg.MODEL.INIT_WEIGHTS is False
    assert cfg.MODEL.HEATMAP_SOFTMAX is True and cfg.MODEL.TRAINABLE_SOFTMAX is True
    assert list(cfg.DATASET.DATASET) == ['MHP_seq'] and list(cfg.DATASET.TEST_DATASET) == ['MHP_seq']
    assert list(cfg.DATASET.SEQ_IDX) == list(range(-4, 5)) and cfg.DATASET.STRIDE == 2
    L = cfg.LOSS
    assert L.WITH_POSE2D_LOSS and L.POSE2D_LOSS_FACTOR == 1.0
    assert not (L.WITH_HEATMAP_LOSS or L.WITH_BONE_LOSS or L.WITH_JOINTANGLE_LOSS or L.WITH_TIME_CONSISTENCY_LOSS or
                L.WITH_POSE3D_LOSS)
    T = cfg.TRAIN
    assert T.IMAGES_PER_GPU == 1 and T.LR == 1e-3 and T.LR_FACTOR == 0.5 and list(T.LR_STEP) == [16, 32, 48]
    assert T.END_EPOCH == 6 and T.WD == 1e-4
    for tool in ('train.py', 'evaluate_2D.py'):
        src = open(os.path.join(mhp_tree.PKG, 'tools', tool)).read()
        line = next(l for l in src.splitlines() if l.startswith('from models import'))
        assert 'pose_hrnet_transformer' in [t.strip() for t in line.split('import', 1)[1].split('#')[0].split(',')]


def test_function_branch_picks_the_centre_frame(monkeypatch):
    """a fake MHP_seq batch of B = 2 windows of F = 3 frames: the model stub sees the frame-major images with frames=3,
    the loss gets the refined poses against the batch's labels in the order s = b * 4 + view, and with the heat-map loss
    on the CENTRE frame's predicted maps"""
    from core import function
    B, F, V, J = 2, 3, 4, 21
    S = B * V
    cfg = _cfg(SMALL + ['DATASET.SEQ_IDX', '[-1, 0, 1]', 'LOSS.WITH_HEATMAP_LOSS', 'True'])
    monkeypatch.setattr(function, '_to_device', lambda t, device: t)
    imgs = torch.arange(F * S, dtype=torch.float32).reshape(F * S, 1, 1, 1).expand(F * S, 3, 4, 4)
    maps = torch.arange(F * S, dtype=torch.float32).reshape(F * S, 1, 1, 1).expand(F * S, J, 2, 2) + 0.5
    poses = torch.arange(S, dtype=torch.float32).reshape(S, 1, 1).expand(S, J, 2) + 100
    seen = {}

    def model(x, frames=None):
        seen['x'], seen['frames'] = x, frames
        return poses, maps, torch.tensor(1.0)

    class Recorder(object):
        def computeLosses(self, heatmaps_pred, heatmaps_gt, pose2d_pred, pose2d_gt, visibility=None):
            seen.update(hm=heatmaps_pred, hm_gt=heatmaps_gt, pred=pose2d_pred, gt=pose2d_gt, vis=visibility)
            return {'total_loss': torch.tensor(0.)}

    ret = {'imgs': imgs, 'heatmaps': torch.full((S, J, 2, 2), 7.0),
           'pose2d': torch.arange(S, dtype=torch.float32).reshape(S, 1, 1).expand(S, J, 2) + 200,
           'visibility': torch.ones(S, J, 1, dtype=torch.bool)}
    out_imgs, losses = function._forward_and_losses(cfg, ret, model, Recorder(), None)
    assert out_imgs is imgs and 'total_loss' in losses
    assert seen['frames'] == F and seen['x'] is imgs
    assert seen['pred'] is poses and torch.equal(seen['gt'][:, 0, 0], torch.arange(S) + 200.0)
    assert tuple(seen['vis'].shape) == (S, J)
    # slot f * S + s: the centre frame (f = 1) is rows S .. 2 S - 1, in the order s = b * 4 + view
    assert torch.equal(seen['hm'][:, 0, 0, 0], torch.arange(S, 2 * S) + 0.5) and tuple(seen['hm_gt'].shape) == (S, J, 2, 2)
    # every other model keeps its path: a model called without `frames`
    cfg2 = _cfg(SMALL + ['MODEL.NAME', 'pose_hrnet_softmax'])
    with pytest.raises(TypeError):
        function._forward_and_losses(cfg2, ret, lambda x: (_ for _ in ()).throw(TypeError('generic path')), Recorder(),
                                     None)


def test_bench_counts_only():
    r = subprocess.run([sys.executable, os.path.join('tools', 'bench_poseformer.py'), '--counts-only'], cwd=mhp_tree.PKG,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    row = json.loads(r.stdout.strip().splitlines()[-1])
    assert (row['S'], row['F'], row['J']) == (4, 9, 21) and 'times' not in row
    c = row['counts']
    assert c['launches_per_block_forward'] == 7 and c['launches_forward'] == 8 * 7 + 8
    assert c['launches_backward'] == 34 * 2 + 19 * 3 + 8 + 1 + 2
    assert c['weight_bytes'] == 14552276 * 4
    assert 5 < c['forward_floor_us'] < 20 and 20 < c['forward_backward_floor_us'] < 60
