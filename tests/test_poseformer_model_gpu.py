"""pose_hrnet_transformer end to end on the GPU: one training step of the whole model through core.function.train_helper
with utils.get_optimizer on a fake MHP_seq batch (launch counts, which parameters move, frame-major against (S, F, ...)
input), eval mode, and tools/train.py + tools/evaluate_2D.py as subprocesses on a tiny written MHP tree
(tests/mhp_tree.py). The model tests run in spawned children (tests/spawned.py); every subprocess has a timeout."""
import collections
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mhp_tree
from spawned import spawned

pytestmark = pytest.mark.gpu
YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_HRNet_w32_trainable_softmax_pose2dloss_PoseFormer_v1.yaml')
SMALL = ['MODEL.IMAGE_SIZE', '[64, 64]', 'MODEL.HEATMAP_SIZE', '[16, 16]', 'DATASET.SEQ_IDX', '[-1, 0, 1]']
F, S, J, HM = 3, 4, 21, 16


def _cfg(opts=()):
    from config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(SMALL + ['PRINT_FREQ', '1'] + list(opts))
    return cfg


def _model(cfg, seed=3):
    from hipnet import synth
    from models import pose_hrnet_transformer
    torch.manual_seed(seed)
    model = pose_hrnet_transformer.get_pose_net(cfg, is_train=True)
    sd = synth.fill_state_dict(model.backbone.state_dict(), 5)
    model.backbone.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    with torch.no_grad():                     # the position embeddings start as zeros: give them values
        model.Spatial_pos_embed.normal_(0, 0.5)
        model.Temporal_pos_embed.normal_(0, 0.5)
    return model.cuda()


def _fake_batch(seed=11):
    """an MHP_seq batch of B = 1: 12 images frame-major (slot f * S + s, s = view), the centre frame's labels"""
    from hipnet import synth
    rng = np.random.default_rng(seed)
    imgs = torch.from_numpy(synth.rhd_batch(F * S, seed=seed, img_h=64, img_w=64)['imgs'])
    return {'imgs': imgs, 'heatmaps': torch.zeros(S, J, HM, HM),
            'pose2d': torch.from_numpy(rng.uniform(2, 14, (S, J, 2)).astype(np.float32)),
            'visibility': torch.ones(S, J, 1, dtype=torch.bool)}


@spawned
def test_one_training_step_of_the_whole_model(tmp_path):
    from core import function
    from core.loss import JointsMSELoss
    from hipnet import _capi
    from utils.utils import get_optimizer
    cfg = _cfg()
    model = _model(cfg).train()
    optimizer = get_optimizer(cfg, model)
    assert isinstance(optimizer, torch.optim.Adam)
    assert sum(len(g['params']) for g in optimizer.param_groups) == sum(p.requires_grad for p in model.parameters())
    recorder = function.AverageMeter(cfg, {'pose2d_loss': JointsMSELoss()})
    ret = _fake_batch()
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    calls = collections.Counter()
    real = _capi.call

    def counting(name, *args):
        calls[name] += 1
        return real(name, *args)

    _capi.call = counting
    try:
        writer_dict = {'writer': None, 'train_global_steps': 0, 'valid_global_steps': 0}
        function.train_helper(0, 0, None, cfg, True, ret, model, optimizer, 'MHP_seq', [ret], writer_dict,
                              logging.getLogger('poseformer-test'), str(tmp_path), str(tmp_path), recorder=recorder)
        torch.cuda.synchronize()
    finally:
        _capi.call = real
    assert calls['hrnet_decode_expectation'] == 1 and calls['hrnet_decode_expectation_bwd'] == 1, dict(calls)
    assert calls['hrnet_tf_attention'] == 8 and calls['hrnet_tf_attention_bwd'] == 8, dict(calls)
    assert calls['hrnet_tf_linear'] == 8 * 4 + 2 and calls['hrnet_tf_linear_bwd'] == 8 * 4 + 2, dict(calls)
    assert calls['hrnet_tf_layernorm'] == 8 * 2 + 3 and calls['hrnet_tf_layernorm_bwd'] == 8 * 2 + 3, dict(calls)
    assert set(calls) <= set(_capi.EXPORTED), set(calls) - set(_capi.EXPORTED)
    assert np.isfinite(recorder.total_loss) and recorder.n == 1
    moved = {k: not torch.equal(v.detach(), before[k]) for k, v in model.named_parameters()}
    for k, m in moved.items():
        if not k.startswith('backbone.') or k.startswith(('backbone.stage4.', 'backbone.last_layer.')):
            assert m, k + ' did not move'
        else:
            assert not m, k + ' is frozen and moved'
    assert not moved['backbone.trainable_temp']


@spawned
def test_frame_major_and_sequence_major_inputs_agree_and_eval_mode():
    cfg = _cfg()
    model = _model(cfg).train()
    imgs = _fake_batch()['imgs'].cuda()                                   # (F * S, 3, 64, 64), slot f * S + s
    seq = imgs.reshape(F, S, 3, 64, 64).permute(1, 0, 2, 3, 4).contiguous()         # (S, F, 3, 64, 64)
    flags = model.draw_drop_flags(S, 'cuda')
    with torch.no_grad():
        # the backbone runs in training mode on the same 12 images in two orders: its batch statistics agree up to the
        # rounding of their sums, so the heat MAPS are compared with a tolerance; the head on identical poses gives the
        # same bits, which is what the second comparison pins (eval mode below gives the same bits end to end)
        a, hm_a, temp = model(imgs, frames=F, drop_flags=flags)
        b, hm_b, _ = model(seq, drop_flags=flags)
        assert tuple(a.shape) == tuple(b.shape) == (S, J, 2) and tuple(hm_a.shape) == (F * S, J, HM, HM)
        assert temp is model.backbone.trainable_temp
        assert float((hm_a.reshape(F, S, J, HM, HM).permute(1, 0, 2, 3, 4) - hm_b.reshape(S, F, J, HM, HM)).abs().max()) \
            <= 1e-3 * float(hm_b.abs().max())
        from utils.heatmap_decoding import get_final_preds
        p = get_final_preds(hm_a, use_softmax=True)
        from_fm = model.head_forward(p.reshape(F, S, J, 2).permute(1, 0, 2, 3).contiguous(), flags)
        assert torch.equal(from_fm, a)                                    # only the poses were reordered
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    model.eval()
    with pytest.raises(NotImplementedError, match='eval mode'):
        model(seq)
    with torch.no_grad():
        pose, hm, temp = model(seq)
        again, _, _ = model(imgs, frames=F)
    assert tuple(pose.shape) == (S, J, 2) and tuple(hm.shape) == (S * F, J, HM, HM) and temp.numel() == 1
    assert torch.equal(pose, again)           # eval mode: running statistics, per-image maps, so the same bits
    with pytest.raises(ValueError, match='HIP-device'):
        model(seq.cpu())
    with torch.no_grad(), pytest.raises(ValueError, match='frames'):
        model(imgs)


def _run(tool, args, timeout):
    return subprocess.run([sys.executable, os.path.join('tools', tool), '--cfg', YAML] + args, cwd=mhp_tree.PKG,
                          capture_output=True, text=True, timeout=timeout)


def test_train_then_evaluate_2d(tmp_path):
    data, out = tmp_path / 'data', str(tmp_path / 'out')
    mhp_tree.write_tree(data, {'data_1': 4, 'data_17': 2})
    common = ['DATA_DIR', str(data), 'OUTPUT_DIR', out, 'LOG_DIR', str(tmp_path / 'log'), 'WORKERS', '0'] + SMALL
    r = _run('train.py', ['--batches-per-epoch', '2'] + common +
             ['TRAIN.BEGIN_EPOCH', '0', 'TRAIN.END_EPOCH', '1', 'PRINT_FREQ', '1'], 600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert 'Pose2DLoss' in log and 'TotalLoss' in log, log[-3000:]
    run = os.path.join(out, 'MHP_seq', 'MHP_HRNet_w32_trainable_softmax_pose2dloss_PoseFormer_v1')
    found = [os.path.join(d, 'final_state.pth.tar') for d, _, fs in os.walk(out) if 'final_state.pth.tar' in fs]
    assert found, (run, log[-2000:])
    final = found[0]
    assert os.path.isfile(os.path.join(os.path.dirname(final), 'checkpoint.pth.tar'))
    state = torch.load(final, map_location='cpu')
    assert tuple(state['Temporal_pos_embed'].shape) == (1, F, 32 * J) and tuple(state['head.1.weight'].shape) == (2 * J, 32 * J)

    r = _run('evaluate_2D.py', ['--model_path', final, '--batch_size', '1', '--num_batches', '2', '--gpu', '0'] + common, 600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert 'fps:' in log and 'mean EPE' in log, log[-2000:]
    res = os.path.join(out, 'eval2D_results_MHP_HRNet_w32_trainable_softmax_pose2dloss_PoseFormer_v1')
    assert np.loadtxt(os.path.join(res, 'PCK2d.txt')).shape == (2, 49)
    assert np.loadtxt(os.path.join(res, 'mse2d_each_joint.txt')).shape == (J,)

    r = subprocess.run([sys.executable, os.path.join('tools', 'train.py'), '--cfg', YAML] + common, cwd=mhp_tree.PKG,
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, WORLD_SIZE='2', RANK='0'))
    assert r.returncode != 0 and 'data-parallel training of pose_hrnet_transformer is not built' in r.stderr
