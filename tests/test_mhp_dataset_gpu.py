"""The MHP readers on the device (lib/dataset/mhp.py) on a fake MHP tree (tests/mhp_tree.py): a loader batch against
the same samples packed in this process and against the float64 warp oracle of tests/test_rhd_dataset_gpu.py, at its
tolerance; tools/train.py training pose_hrnet_PoseAggr on MHP_seq and pose_hrnet_softmax on MHP_kpt;
tools/evaluate_2D.py on MHP_seq."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mhp_tree
from spawned import spawned
from test_rhd_dataset_gpu import _check, _kfd_children, _oracle

pytestmark = pytest.mark.gpu


@spawned
def test_seq_loader_batch_equals_the_cpu_path(tmp_path):
    from dataset.build import make_dataloader
    from dataset.mhp import collate, decode
    from dataset.preprocess import affine_warp_normalize
    from dataset.rhd import RHDLoader
    from dataset.target_generators import HeatmapGenerator
    mhp_tree.write_tree(tmp_path)
    cfg = mhp_tree.config(tmp_path, ['WITH_DATA_AUG', 'True', 'WORKERS', '2', 'TRAIN.IMAGES_PER_GPU', '2'])
    loader = make_dataloader(cfg, True)['MHP_seq']
    assert isinstance(loader, RHDLoader)
    loader.sampler.set_epoch(2)
    keys = [list(b) for b in loader.loader.batch_sampler]
    batches = list(loader)
    assert [b['imgs'].shape[0] for b in batches] == [40, 40, 20]
    assert not _kfd_children(), 'a DataLoader worker opened the GPU'
    ds = loader.dataset
    n_out = 0
    for bi, (b, ks) in enumerate(zip(batches, keys)):
        samples = [ds[k] for k in ks]
        ref = collate(samples)
        assert torch.equal(b['pose2d'], ref['pose2d']) and torch.equal(b['visibility'], ref['visibility'])
        assert torch.equal(b['hm_inverse'], ref['hm_inverse'])
        assert b['pose2d'].shape == (4 * len(ks), 21, 2)
        joints = torch.cat((ref['pose2d'], ref['visibility'].float()), 2)
        assert torch.equal(b['heatmaps'], HeatmapGenerator(64, 21, 2)(joints))
        imgs = affine_warp_normalize(ref['buffer'].cuda(), ref['table'], ref['inverse'], (256, 256))
        assert torch.equal(b['imgs'], imgs)
        if bi:
            continue
        # every slot of the first batch against the float64 oracle on its decoded frame
        B = len(ks)
        for s, sample in enumerate(samples):
            for j in range(5):
                for c in range(4):
                    slot = (j * B + s) * 4 + c
                    frame = decode(sample['paths'][j * 4 + c], False)
                    v, outside = _oracle(frame, 0, 0, 480, 640, ref['inverse'][slot].numpy(), 256)
                    _check(b['imgs'][slot], v, outside)
                    n_out += int(outside.sum())
    assert n_out > 0                                   # the augmentation moved some output pixels off the frame


def _run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


def _losses(log):
    vals = [float(v) for v in re.findall(r'TotalLoss ([-+0-9.eEnaif]+) ', log)]
    assert vals, log[-3000:]
    return vals


def test_train_poseaggr_on_seq_and_evaluate(tmp_path):
    mhp_tree.write_tree(tmp_path / 'data')
    out = str(tmp_path / 'out')
    common = ['DATA_DIR', str(tmp_path / 'data'), 'OUTPUT_DIR', out, 'LOG_DIR', str(tmp_path / 'log'),
              'PRINT_FREQ', '1', 'WORKERS', '2']
    exp = os.path.join(out, 'MHP', 'MHP_HRNet_w32_trainable_softmax_pose2dloss_PoseAggr_v1')
    # no epoch: the initial weights, then one epoch of two steps resumed from them
    _run([sys.executable, 'tools/train.py', '--cfg', mhp_tree.AGGR_YAML, 'TRAIN.BEGIN_EPOCH', '0',
          'TRAIN.END_EPOCH', '0'] + common, mhp_tree.PKG)
    sd0 = torch.load(os.path.join(exp, 'final_state.pth.tar'), map_location='cpu')
    torch.save({'epoch': 0, 'state_dict': sd0}, os.path.join(exp, 'checkpoint.pth.tar'))
    log = _run([sys.executable, 'tools/train.py', '--cfg', mhp_tree.AGGR_YAML, '--batches-per-epoch', '2',
                'TRAIN.BEGIN_EPOCH', '0', 'TRAIN.END_EPOCH', '1'] + common, mhp_tree.PKG)
    assert 'Dataset: MHP_seq Epoch: [0][1/2]' in log and 'Validating on MHP_seq dataset' in log
    assert 'Dataset: MHP_seq Test: [1/2]' in log and 'synthetic' not in log
    assert np.isfinite(_losses(log)).all()
    sd1 = torch.load(os.path.join(exp, 'final_state.pth.tar'), map_location='cpu')
    assert not torch.equal(sd0['offsets1.weight'], sd1['offsets1.weight'])
    assert not torch.equal(sd0['deform_conv3.weight'], sd1['deform_conv3.weight'])
    assert torch.equal(sd0['conv1.weight'], sd1['conv1.weight'])          # the backbone gets no gradient
    log = _run([sys.executable, 'tools/evaluate_2D.py', '--cfg', mhp_tree.AGGR_YAML, '--model_path',
                os.path.join(exp, 'final_state.pth.tar'), '--batch_size', '2', '--gpu', '0'] + common, mhp_tree.PKG)
    res = os.path.join(out, 'eval2D_results_MHP_HRNet_w32_trainable_softmax_pose2dloss_PoseAggr_v1')
    mse = np.loadtxt(os.path.join(res, 'mse2d_each_joint.txt'))
    pck = np.loadtxt(os.path.join(res, 'PCK2d.txt'))
    assert mse.shape == (21,) and np.isfinite(mse[1:]).all() and pck.shape == (2, 49) and np.isfinite(pck).all()
    assert 'mean EPE' in log


def test_train_softmax_on_mhp_kpt(tmp_path):
    mhp_tree.write_tree(tmp_path / 'data')
    log = _run([sys.executable, 'tools/train.py', '--cfg', mhp_tree.SOFTMAX_YAML, '--batches-per-epoch', '1',
                'TRAIN.BEGIN_EPOCH', '0', 'TRAIN.END_EPOCH', '1', 'TRAIN.IMAGES_PER_GPU', '4',
                'TEST.IMAGES_PER_GPU', '4', 'DATA_DIR', str(tmp_path / 'data'), 'OUTPUT_DIR', str(tmp_path / 'out'),
                'LOG_DIR', str(tmp_path / 'log'), 'PRINT_FREQ', '1', 'WORKERS', '2'] + mhp_tree.KPT_OPTS,
               mhp_tree.PKG)
    assert 'Dataset: MHP_kpt Epoch: [0][0/1]' in log and 'Validating on MHP dataset' in log
    assert 'Dataset: MHP Test: [2/3]' in log and 'synthetic' not in log
    assert np.isfinite(_losses(log)).all()
