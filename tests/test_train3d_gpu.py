"""The 3-D training path end to end on the device: the gradient of the chain heat maps -> expectation decode ->
triangulation -> Joints3DMSELoss against the checked kernels; one forward and one backward triangulation launch per
step of core/function3D.py; tools/train3D.py on a fake MHP tree (tests/mhp_tree.py) - logs, checkpoints, moved
parameters, tools/evaluate_3D.py on its final state, bit-identical repeats under HRNET_DETERMINISTIC=1."""
import collections
import logging
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mhp_tree
from spawned import spawned

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'triangulation.npz')
YAML3D = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_HRNet_w32_trainable_softmax_pose3dloss_v1.yaml')
EXP = 'MHP_HRNet_w32_trainable_softmax_pose3dloss_v1'


@spawned
def test_heat_map_gradient_of_the_whole_chain():
    from core.loss import Joints3DMSELoss
    from utils.heatmap_decoding import get_final_preds
    from utils.multiview import triangulate_batch_of_points
    z = np.load(GOLD)
    B, V, K, H, W = 3, 4, 21, 16, 16
    gen = torch.Generator().manual_seed(2)
    hm = torch.rand(B * V, K, H, W, generator=gen)
    hm = (hm / hm.sum((2, 3), keepdim=True)).cuda().requires_grad_(True)
    proj = torch.from_numpy(np.broadcast_to(z['rig_wide'], (B, V, 3, 4)).copy()).cuda()
    to_frame = torch.tensor([[30.0, 0.0, 90.0], [0.0, 25.0, 40.0]], dtype=torch.float64).repeat(B * V, 1, 1).cuda()
    gt = (torch.randn(B, K, 3, generator=gen) * 60).cuda()

    def loss_of(points):
        X = triangulate_batch_of_points(proj, points.view(B, V, K, 2), to_frame=to_frame)
        return Joints3DMSELoss()(X, gt) * 0.5

    # the gradient with respect to the decoded points, from the kernels tests/test_triangulate_grad_gpu.py checks
    pts = get_final_preds(hm.detach(), True).requires_grad_(True)
    loss_of(pts).backward()
    dpts = pts.grad
    assert torch.isfinite(dpts).all() and dpts.abs().max() > 0
    # the whole chain: the expectation decode is linear in the map, d pred / d hm[y, x] = (x, y)
    loss = loss_of(get_final_preds(hm, True))
    loss.backward()
    torch.cuda.synchronize()
    xs = torch.arange(W, dtype=torch.float32, device='cuda').view(1, 1, 1, W)
    ys = torch.arange(H, dtype=torch.float32, device='cuda').view(1, 1, H, 1)
    expect = dpts[..., 0, None, None] * xs + dpts[..., 1, None, None] * ys
    err = ((hm.grad - expect).abs().max() / expect.abs().max()).item()
    print('chain', err)
    assert hm.grad.shape == hm.shape and err <= 1e-6


def _fake_batch(B, V, size, K=21):
    """an MHP_mv-shaped device batch on the calibration of tests/mhp_tree.py, without a dataset"""
    from dataset.mhp import INTRINSIC, rodrigues
    gen = torch.Generator().manual_seed(4)
    ext = np.stack([np.c_[rodrigues(r), t] for r, t in (mhp_tree.calibration(1, c) for c in range(1, V + 1))])
    hm = size // 4
    inv = np.array([[640.0 / hm, 0.0, 0.0], [0.0, 480.0 / hm, 0.0]])
    return {'imgs': torch.randn(B * V, 3, size, size, generator=gen).cuda(),
            'extrinsic_matrices': torch.from_numpy(np.broadcast_to(ext, (B, V, 3, 4)).copy()),
            'intrinsic_matrix': torch.from_numpy(np.broadcast_to(INTRINSIC, (B, 3, 3)).copy()),
            'hm_inverse': torch.from_numpy(np.broadcast_to(inv, (B * V, 2, 3)).copy()),
            'pose3d': torch.from_numpy(np.stack([mhp_tree.joints(1, f) for f in range(B)])),
            'pose2d': torch.zeros(B * V, K, 2), 'visibility': torch.ones(B * V, K, 1, dtype=torch.bool)}


@spawned
def test_one_triangulation_launch_each_way_per_step(tmp_path):
    from core import function3D
    from core.loss import Joints3DMSELoss
    from hipnet import _capi
    from models import pose_hrnet_softmax
    from utils.utils import get_optimizer
    cfg = mhp_tree.config(tmp_path, ['MODEL.IMAGE_SIZE', '[64, 64]', 'MODEL.HEATMAP_SIZE', '[16, 16]',
                                     'PRINT_FREQ', '1'], YAML3D)
    torch.manual_seed(0)
    model = pose_hrnet_softmax.get_pose_net(cfg, is_train=True).cuda().train()
    optimizer = get_optimizer(cfg, model)
    recorder = function3D.AverageMeter3D(cfg, {'pose3d_loss': Joints3DMSELoss()})
    ret = _fake_batch(2, 4, 64)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    calls = collections.Counter()
    real = _capi.call

    def counting(name, *args):
        calls[name] += 1
        return real(name, *args)

    _capi.call = counting
    try:
        writer_dict = {'writer': None, 'train_global_steps': 0, 'valid_global_steps': 0}
        function3D.train_helper(0, 0, None, cfg, True, ret, model, optimizer, 'MHP_mv', [ret], writer_dict,
                                logging.getLogger('train3d-test'), str(tmp_path), str(tmp_path), recorder=recorder)
        torch.cuda.synchronize()
    finally:
        _capi.call = real
    assert calls['hrnet_triangulate'] == 1 and calls['hrnet_triangulate_bwd'] == 1, dict(calls)
    assert calls['hrnet_joints3d_loss_fwd'] == 1 and calls['hrnet_joints3d_loss_bwd'] == 1
    assert calls['hrnet_decode_expectation'] == 1 and calls['hrnet_decode_expectation_bwd'] == 1
    assert calls['hrnet_triangulate_ransac'] == 0
    avg = recorder.computeAvgLosses()
    assert set(avg) == {'total_loss', 'pose3d_loss', 'epe3d'} and all(np.isfinite(v) for v in avg.values())
    assert writer_dict['train_global_steps'] == 1
    after = model.state_dict()
    assert not torch.equal(before['conv1.weight'], after['conv1.weight'])          # the gradient reached the stem
    assert not torch.equal(before['last_layer.3.weight'], after['last_layer.3.weight'])
    # validate: no graph, the same lifting, the end-point error reported
    val = function3D.validate(cfg, None, True, {'MHP_mv': _Loader([ret])}, model, {'pose3d_loss': Joints3DMSELoss()},
                              str(tmp_path), str(tmp_path), writer_dict, logging.getLogger('train3d-test'))
    assert np.isfinite(val.avg_epe3d) and val.avg_epe3d > 0 and writer_dict['valid_global_steps'] == 1


class _Loader(list):
    batch_size = 2


def _run(cmd, cwd, env=None):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


def test_train3d_tool_and_evaluate_3d_on_its_state(tmp_path):
    from models import pose_hrnet_softmax
    mhp_tree.write_tree(tmp_path / 'data')
    cfg = mhp_tree.config(tmp_path / 'data', [], YAML3D)
    torch.manual_seed(0)
    sd0 = pose_hrnet_softmax.get_pose_net(cfg, is_train=False).state_dict()
    start = str(tmp_path / 'start.pth.tar')
    torch.save({'state_dict': {'module.' + k: v for k, v in sd0.items()}, 'epoch': 0}, start)
    env = dict(os.environ, HRNET_DETERMINISTIC='1')
    finals = []
    for run in ('a', 'b'):
        out = str(tmp_path / ('out_' + run))
        log = _run([sys.executable, 'tools/train3D.py', '--cfg', YAML3D, '--batches-per-epoch', '3', '--views',
                    '[1,2,3,4]', '--model_path', start, 'TRAIN.BEGIN_EPOCH', '0', 'TRAIN.END_EPOCH', '2',
                    'TRAIN.IMAGES_PER_GPU', '2', 'TEST.IMAGES_PER_GPU', '2', 'DATA_DIR', str(tmp_path / 'data'),
                    'OUTPUT_DIR', out, 'LOG_DIR', str(tmp_path / ('log_' + run)), 'PRINT_FREQ', '1', 'WORKERS', '2'],
                   mhp_tree.PKG, env)
        exp = os.path.join(out, 'MHP', EXP)
        assert 'Dataset: MHP_mv Epoch: [0][0/3]' in log and 'Dataset: MHP_mv Epoch: [1][2/3]' in log, log[-3000:]
        assert 'Validating on MHP_mv dataset' in log and 'Dataset: MHP_mv Test: [2/3]' in log
        assert 'mean 3-D end-point error' in log and 'backbone weights from' in log and 'synthetic' not in log
        pairs = re.findall(r'(?:TotalLoss|Pose3DLoss|EPE3D) ([-+0-9.eEnaif]+) \(([-+0-9.eEnaif]+)\)', log)
        vals = [float(x) for pair in pairs for x in pair]
        # 6 training lines of two terms, 6 validation lines of three, each with its running average
        assert len(vals) == 2 * (6 * 2 + 6 * 3) and np.isfinite(vals).all(), log[-3000:]
        assert len(re.findall(r'Pose3DLoss ', log)) == 2 * (3 + 3)
        for name in ('checkpoint.pth.tar', 'model_best.pth.tar', 'final_state.pth.tar'):
            assert os.path.isfile(os.path.join(exp, name)), name
        ckpt = torch.load(os.path.join(exp, 'checkpoint.pth.tar'), map_location='cpu')
        assert ckpt['epoch'] == 2 and ckpt['train_global_steps'] == 6 and ckpt['model'] == 'pose_hrnet_softmax'
        finals.append(torch.load(os.path.join(exp, 'final_state.pth.tar'), map_location='cpu'))
    final = finals[0]
    assert list(final) == list(sd0)                        # the backbone's own keys, no prefix
    for key in ('conv1.weight', 'stage4.2.fuse_layers.0.1.0.weight', 'last_layer.3.weight'):
        assert not torch.equal(final[key], sd0[key]), key
    assert all(torch.isfinite(v).all() for v in final.values() if v.is_floating_point())
    for key in final:                                      # HRNET_DETERMINISTIC=1: the two runs are the same bits
        assert torch.equal(final[key], finals[1][key]), key
    out = str(tmp_path / 'out_a')
    log = _run([sys.executable, 'tools/evaluate_3D.py', '--cfg', YAML3D, '--model_path',
                os.path.join(out, 'MHP', EXP, 'final_state.pth.tar'), '--views', '[1,2,3,4]', '--batch_size', '2',
                '--gpu', '0', 'DATA_DIR', str(tmp_path / 'data'), 'OUTPUT_DIR', out, 'WORKERS', '0'], mhp_tree.PKG)
    assert '3D pose EPE:' in log and '3D PCKAUC:' in log, log[-2000:]
    res = os.path.join(out, 'eval3D_results_' + EXP)
    for name, shape in (('mse2d_each_joint.txt', (21,)), ('mse3d_each_joint.txt', (21,)), ('PCK2d.txt', (2, 49)),
                        ('PCK3d.txt', (2, 50))):
        assert np.loadtxt(os.path.join(res, name)).shape == shape, name
    # a refusal reaches the command line as the clear error, before any device work
    r = subprocess.run([sys.executable, 'tools/train3D.py', '--cfg', YAML3D, 'MODEL.HEATMAP_SOFTMAX', 'False',
                        'DATA_DIR', str(tmp_path / 'data')], cwd=mhp_tree.PKG, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and 'arg-max decode has no gradient' in r.stderr, r.stderr[-2000:]
