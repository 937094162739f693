"""The 3-D evaluation end to end on the device, on a fake MHP tree (tests/mhp_tree.py): the MHP_mv reader's
ground-truth heat-map points through its hm_inverse into hrnet_triangulate give back its world joints (zero distortion,
so this pins the reader's geometry and the kernel together); tools/evaluate_3D.py on random pose_hrnet_softmax
weights writes the reference's four result files and prints fps and both EPEs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mhp_tree
from spawned import spawned

pytestmark = pytest.mark.gpu


@spawned
def test_ground_truth_through_the_reader_and_the_kernel(tmp_path):
    from dataset.mhp import make_loader
    from utils.multiview import triangulate_batch_of_points
    mhp_tree.write_tree(tmp_path, {'data_17': 5})
    cfg = mhp_tree.config(tmp_path, ['WORKERS', '0', 'TEST.IMAGES_PER_GPU', '2'], mhp_tree.SOFTMAX_YAML)
    for views in ((1, 2, 3, 4), (1, 3)):
        V = len(views)
        loader = make_loader(cfg, 'MHP_mv', 'eval', False, views=views)
        n = 0
        for b in loader:
            B = b['pose3d'].shape[0]
            assert b['imgs'].shape == (B * V, 3, 256, 256) and b['imgs'].is_cuda
            assert torch.isfinite(b['imgs']).all()
            proj = (b['intrinsic_matrix'][:, None] @ b['extrinsic_matrices']).cuda()
            X, frame = triangulate_batch_of_points(proj, b['pose2d'].view(B, V, 21, 2).cuda(),
                                                   to_frame=b['hm_inverse'].cuda(), return_frame_points=True)
            err = (X.cpu().double() - b['pose3d']).abs().max().item()
            assert err <= 1e-2, (views, err)
            # the mapped ground truth is the frame projection the visibility rule was decided on
            vis = b['visibility'].view(B, V, 21).numpy()
            f = frame.cpu().numpy()
            inside = (f[..., 0] > -1e-2) & (f[..., 1] > -1e-2) & (f[..., 0] < 640.01) & (f[..., 1] < 480.01)
            assert not (vis & ~inside).any()
            n += B
        assert n == 5


def test_evaluate_3d_cli(tmp_path):
    from models import pose_hrnet_softmax
    mhp_tree.write_tree(tmp_path / 'data', {'data_17': 5})
    cfg = mhp_tree.config(tmp_path / 'data', [], mhp_tree.SOFTMAX_YAML)
    torch.manual_seed(0)
    model = pose_hrnet_softmax.get_pose_net(cfg, is_train=False)
    ckpt = str(tmp_path / 'random.pth.tar')
    torch.save({'state_dict': model.state_dict(), 'epoch': 0}, ckpt)
    out = str(tmp_path / 'out')
    r = subprocess.run([sys.executable, 'tools/evaluate_3D.py', '--cfg', mhp_tree.SOFTMAX_YAML, '--model_path', ckpt,
                        '--views', '[1,2,3,4]', '--batch_size', '2', '--num_batches', '2', '--gpu', '0',
                        'DATA_DIR', str(tmp_path / 'data'), 'OUTPUT_DIR', out, 'WORKERS', '0'],
                       cwd=mhp_tree.PKG, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert 'fps:' in log and '2D pose EPE:' in log and '3D pose EPE:' in log and '3D PCKAUC:' in log, log[-2000:]
    res = os.path.join(out, 'eval3D_results_' + cfg.EXP_NAME)
    pck3d = np.loadtxt(os.path.join(res, 'PCK3d.txt'))
    pck2d = np.loadtxt(os.path.join(res, 'PCK2d.txt'))
    assert pck3d.shape == (2, 50) and np.array_equal(pck3d[0], np.arange(1, 51))
    assert pck2d.shape == (2, 49) and np.array_equal(pck2d[0], np.arange(1, 50))
    assert np.loadtxt(os.path.join(res, 'mse2d_each_joint.txt')).shape == (21,)
    assert np.loadtxt(os.path.join(res, 'mse3d_each_joint.txt')).shape == (21,)
    # a refused model fails before any device work, with the clear error
    r = subprocess.run([sys.executable, 'tools/evaluate_3D.py', '--cfg', mhp_tree.SOFTMAX_YAML, 'MODEL.NAME', 'vol',
                        'DATA_DIR', str(tmp_path / 'data')], cwd=mhp_tree.PKG, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "MODEL.NAME 'vol' is not built" in r.stderr, r.stderr[-2000:]
