"""tools/train_vol.py and tools/evaluate_vol.py end to end on a fake MHP tree (tests/mhp_tree.py): two training batches
and one validation pass of the volumetric model at VOLUME_SIZE 32, then the evaluation of the checkpoint it wrote.
tools/evaluate_3D.py keeps refusing MODEL.NAME vol. Every subprocess has a timeout."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mhp_tree

pytestmark = pytest.mark.gpu

YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_VolTriangulation_w32_v1.yaml')


def _run(tool, args, timeout):
    return subprocess.run([sys.executable, os.path.join('tools', tool), '--cfg', YAML] + args, cwd=mhp_tree.PKG,
                          capture_output=True, text=True, timeout=timeout)


def test_train_vol_then_evaluate_vol(tmp_path):
    data, out = tmp_path / 'data', str(tmp_path / 'out')
    mhp_tree.write_tree(data, {'data_1': 4, 'data_17': 2})
    common = ['DATA_DIR', str(data), 'OUTPUT_DIR', out, 'LOG_DIR', str(tmp_path / 'log'), 'WORKERS', '0',
              'MODEL.VOLUME_SIZE', '32']
    r = _run('train_vol.py', ['--batches-per-epoch', '2'] + common +
             ['TRAIN.END_EPOCH', '1', 'TRAIN.IMAGES_PER_GPU', '2', 'TEST.IMAGES_PER_GPU', '2', 'PRINT_FREQ', '1'], 600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert 'Pose3DLoss' in log and 'VolumetricCELoss' in log and 'EPE3D' in log, log[-3000:]
    final = os.path.join(out, 'MHP', 'MHP_VolTriangulation_w32_v1', 'final_state.pth.tar')
    assert os.path.isfile(final), log[-2000:]

    r = _run('evaluate_vol.py', ['--model_path', final, '--views', '[1,2,3,4]', '--batch_size', '2', '--num_batches', '1',
                                 '--gpu', '0'] + common, 600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert '3D pose EPE:' in log and '2D pose EPE:' in log and 'fps:' in log, log[-2000:]
    res = os.path.join(out, 'eval3D_results_MHP_VolTriangulation_w32_v1')
    pck3d = np.loadtxt(os.path.join(res, 'PCK3d.txt'))
    pck2d = np.loadtxt(os.path.join(res, 'PCK2d.txt'))
    assert pck3d.shape == (2, 50) and np.array_equal(pck3d[0], np.arange(1, 51))
    assert pck2d.shape == (2, 49) and np.array_equal(pck2d[0], np.arange(1, 50))
    assert np.loadtxt(os.path.join(res, 'mse2d_each_joint.txt')).shape == (21,)
    assert np.loadtxt(os.path.join(res, 'mse3d_each_joint.txt')).shape == (21,)

    # the triangulating tool still refuses the model, before any device work
    r = subprocess.run([sys.executable, 'tools/evaluate_3D.py', '--cfg', mhp_tree.SOFTMAX_YAML, 'MODEL.NAME', 'vol',
                        'DATA_DIR', str(data)], cwd=mhp_tree.PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "MODEL.NAME 'vol' is not built" in r.stderr, r.stderr[-2000:]
