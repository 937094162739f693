"""MultiViewPoseNet (lib/models/multiview_pose_hrnet.py) on the device at 64 x 64 images (16 x 16 heat maps, P = 256), the
smallest input the volumetric model's GPU tests run the backbone at: output shapes and slot order, one Adam step with the
optimiser tools/train_fusion.py builds; then tools/train_fusion.py and tools/evaluate_3D.py end to end on a fake MHP tree
(tests/mhp_tree.py). The model test runs in a spawned child (tests/spawned.py); every subprocess has a timeout."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fusion_ref as R
import mhp_tree
from spawned import spawned

pytestmark = pytest.mark.gpu

YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_HRNet_w32_fusion_v1.yaml')
SMALL = ['MODEL.IMAGE_SIZE', '[64, 64]', 'MODEL.HEATMAP_SIZE', '[16, 16]']
V, K, HM = 4, 21, 16


def _cfg(opts=()):
    from config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(SMALL + list(opts))
    return cfg


def _images(B, seed):
    from hipnet import synth
    return torch.from_numpy(synth.rhd_batch(B * V, seed=seed, img_h=64, img_w=64)['imgs']).reshape(B, V, 3, 64, 64)


@spawned
def test_model_slot_order_and_one_adam_step():
    from core.loss import JointsMSELoss
    from models.multiview_pose_hrnet import MultiViewPoseNet
    from utils.heatmap_decoding import get_final_preds
    sys.path.insert(0, os.path.join(mhp_tree.PKG, 'tools'))
    import train_fusion
    from hipnet import synth
    cfg = _cfg()
    torch.manual_seed(3)
    model = MultiViewPoseNet(cfg)
    # hipnet.synth's seeded weights give heat maps that differ from view to view; they need batch statistics (their
    # running statistics are not calibrated), so the forward checks run in training mode under no_grad
    sd = synth.fill_state_dict(model.backbone.state_dict(), 5)
    model.backbone.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.cuda().train()
    B = 2
    img = _images(B, 11).cuda()
    with torch.no_grad():
        fused, single = model(img)
        assert tuple(fused.shape) == tuple(single.shape) == (B * V, K, HM, HM)
        assert bool(torch.isfinite(fused).all()) and bool(torch.isfinite(single).all())
        # the fused maps are the formula applied to the single-view maps, rows in slot order b * V + v
        Ws = [model.aggre_layer.aggre[n].weight.weight.detach().double().cpu() for n in range(12)]
        H = single.double().cpu().reshape(B, V, K, HM * HM)
        ref = R.fusion_ref(H, Ws)
        err = (fused.double().cpu().reshape(ref.shape) - ref).abs() / R.forward_bound(H, Ws)
        assert float(err.max()) <= 1.0
        # swap views 1 and 3 of the input: single swaps those rows (the batch statistics see the same images, in another
        # order: equal up to the rounding of their sums, held to 1e-3 of the largest value, while the two views' maps
        # differ by more than a hundred times that); fused is the formula on the maps the same call returned
        perm = [0, 3, 2, 1]
        fused_p, single_p = model(img[:, perm].contiguous())
        s, sp = single.view(B, V, K, HM, HM), single_p.view(B, V, K, HM, HM)
        tol = 1e-3 * float(s.abs().max())
        assert float((s[:, 1] - s[:, 3]).abs().max()) > 100 * tol, 'the views do not differ enough to tell a swap'
        assert float((sp - s[:, perm]).abs().max()) <= tol
        Hp = single_p.double().cpu().reshape(B, V, K, HM * HM)
        ref_p = R.fusion_ref(Hp, Ws)
        err = (fused_p.double().cpu().reshape(ref_p.shape) - ref_p).abs() / R.forward_bound(Hp, Ws)
        assert float(err.max()) <= 1.0
        # a (V, 3, H, W) input is a batch of one
        f1, s1 = model(img[0])
        assert tuple(f1.shape) == tuple(s1.shape) == (V, K, HM, HM)
    model.eval()
    with pytest.raises(NotImplementedError, match='eval mode'):
        model(img)
    # MODEL.AGGRE false returns the single-view maps alone
    plain = MultiViewPoseNet(_cfg(['MODEL.AGGRE', 'False']))
    plain.load_state_dict(model.state_dict(), strict=True)
    plain = plain.cuda().train()
    with torch.no_grad():
        only = plain(img)
    assert isinstance(only, torch.Tensor) and tuple(only.shape) == (B * V, K, HM, HM)
    assert float((only - single).abs().max()) <= tol

    model.train()
    opt = train_fusion.build_optimizer(cfg, model)
    assert [g['name'] for g in opt.param_groups] == ['backbone', 'aggre_layer']
    assert [g['lr'] for g in opt.param_groups] == [cfg.TRAIN.LR, cfg.TRAIN.LR]
    assert all(g['weight_decay'] == 0 for g in opt.param_groups) and isinstance(opt, torch.optim.Adam)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    gt2d = torch.linspace(3.0, 12.0, 2 * B * V * K * 2, device='cuda').reshape(2 * B * V, K, 2)
    fused, single = model(img)
    pred = torch.cat((get_final_preds(single, use_softmax=True), get_final_preds(fused, use_softmax=True)), 0)
    loss = JointsMSELoss()(pred, gt2d)
    opt.zero_grad()
    loss.backward()
    assert bool(torch.isfinite(loss))
    for n in range(12):
        g = model.aggre_layer.aggre[n].weight.weight.grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    opt.step()
    torch.cuda.synchronize()
    moved = {k: not torch.equal(v.detach(), before[k]) for k, v in model.named_parameters()}
    for k, m in moved.items():
        if k.startswith('aggre_layer.'):
            assert m, k + ' did not move'
        elif not k.startswith(('backbone.stage4.', 'backbone.last_layer.')):
            assert not m, k + ' is frozen and moved'
    assert any(m for k, m in moved.items() if k.startswith('backbone.stage4.'))
    assert any(m for k, m in moved.items() if k.startswith('backbone.last_layer.'))


def _run(tool, args, timeout):
    return subprocess.run([sys.executable, os.path.join('tools', tool), '--cfg', YAML] + args, cwd=mhp_tree.PKG,
                          capture_output=True, text=True, timeout=timeout)


def test_train_fusion_then_evaluate_3d(tmp_path):
    data, out = tmp_path / 'data', str(tmp_path / 'out')
    mhp_tree.write_tree(data, {'data_1': 4, 'data_17': 2})
    common = ['DATA_DIR', str(data), 'OUTPUT_DIR', out, 'LOG_DIR', str(tmp_path / 'log'), 'WORKERS', '0'] + SMALL
    r = _run('train_fusion.py', ['--batches-per-epoch', '2'] + common +
             ['TRAIN.END_EPOCH', '1', 'TRAIN.IMAGES_PER_GPU', '2', 'TEST.IMAGES_PER_GPU', '2', 'PRINT_FREQ', '1'], 600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert 'Pose2DLoss' in log and 'TotalLoss' in log, log[-3000:]
    assert 'EPE2D single' in log and 'EPE2D fused' in log and 'mean 2-D end-point error: single' in log, log[-3000:]
    run = os.path.join(out, 'MHP', 'MHP_HRNet_w32_fusion_v1')
    final = os.path.join(run, 'final_state.pth.tar')
    assert os.path.isfile(final), log[-2000:]
    assert os.path.isfile(os.path.join(run, 'checkpoint.pth.tar'))
    state = torch.load(final, map_location='cpu')
    assert tuple(state['aggre_layer.aggre.11.weight.weight'].shape) == (HM * HM, HM * HM)

    r = _run('evaluate_3D.py', ['--model_path', final, '--views', '[1,2,3,4]', '--batch_size', '2', '--num_batches', '1',
                                '--gpu', '0'] + common, 600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert '3D pose EPE:' in log and '2D pose EPE:' in log and 'fps:' in log, log[-2000:]
    res = os.path.join(out, 'eval3D_results_MHP_HRNet_w32_fusion_v1')
    pck3d = np.loadtxt(os.path.join(res, 'PCK3d.txt'))
    pck2d = np.loadtxt(os.path.join(res, 'PCK2d.txt'))
    assert pck3d.shape == (2, 50) and pck2d.shape == (2, 49)
    assert np.loadtxt(os.path.join(res, 'mse2d_each_joint.txt')).shape == (21,)
    assert np.loadtxt(os.path.join(res, 'mse3d_each_joint.txt')).shape == (21,)
