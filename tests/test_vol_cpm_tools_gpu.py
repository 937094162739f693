"""tools/train_vol.py and tools/evaluate_vol.py end to end with MODEL.NAME vol_CPM on a fake MHP tree (tests/mhp_tree.py):
two training iterations and one validation pass with the shipped yaml at reduced sizes (64 x 64 images, 16 x 16 heat maps,
VOLUME_SIZE 32), then the evaluation of the final_state.pth.tar it wrote and its four result files. Every subprocess has a
timeout."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mhp_tree

pytestmark = pytest.mark.gpu

YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_VolTriangulation_CPM_v1.yaml')


def _run(tool, args, timeout):
    return subprocess.run([sys.executable, os.path.join('tools', tool), '--cfg', YAML] + args, cwd=mhp_tree.PKG,
                          capture_output=True, text=True, timeout=timeout)


def test_train_vol_then_evaluate_vol_on_the_cpm_backbone(tmp_path):
    data, out = tmp_path / 'data', str(tmp_path / 'out')
    mhp_tree.write_tree(data, {'data_1': 4, 'data_17': 2})
    common = ['DATA_DIR', str(data), 'OUTPUT_DIR', out, 'LOG_DIR', str(tmp_path / 'log'), 'WORKERS', '0',
              'MODEL.VOLUME_SIZE', '32', 'MODEL.IMAGE_SIZE', '[64, 64]', 'MODEL.HEATMAP_SIZE', '[16, 16]']
    r = _run('train_vol.py', ['--batches-per-epoch', '2'] + common +
             ['TRAIN.BEGIN_EPOCH', '0', 'TRAIN.END_EPOCH', '1', 'TRAIN.IMAGES_PER_GPU', '2', 'TEST.IMAGES_PER_GPU', '2',
              'PRINT_FREQ', '1'], 600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert 'Pose3DLoss' in log and 'VolumetricCELoss' in log and 'HeatmapLoss' in log and 'EPE3D' in log, log[-3000:]
    assert log.count('Epoch: [0]') >= 2, log[-3000:]
    final = os.path.join(out, 'MHP', 'MHP_VolTriangulation_CPM_v1', 'final_state.pth.tar')
    assert os.path.isfile(final), log[-2000:]
    sd = torch.load(final, map_location='cpu')
    assert 'backbone.Mconv5_stage6.weight' in sd and 'backbone.vol_confidences.head.4.weight' in sd
    assert tuple(sd['process_features.0.weight'].shape) == (32, 128, 1, 1)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.dtype.is_floating_point)

    r = _run('evaluate_vol.py', ['--model_path', final, '--views', '[1,2,3,4]', '--batch_size', '2', '--num_batches', '1',
                                 '--gpu', '0'] + common, 600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert '3D pose EPE:' in log and '2D pose EPE:' in log and 'fps:' in log, log[-2000:]
    res = os.path.join(out, 'eval3D_results_MHP_VolTriangulation_CPM_v1')
    pck3d = np.loadtxt(os.path.join(res, 'PCK3d.txt'))
    pck2d = np.loadtxt(os.path.join(res, 'PCK2d.txt'))
    assert pck3d.shape == (2, 50) and np.array_equal(pck3d[0], np.arange(1, 51))
    assert pck2d.shape == (2, 49) and np.array_equal(pck2d[0], np.arange(1, 50))
    assert np.loadtxt(os.path.join(res, 'mse2d_each_joint.txt')).shape == (21,)
    assert np.loadtxt(os.path.join(res, 'mse3d_each_joint.txt')).shape == (21,)
