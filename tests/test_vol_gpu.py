"""VolumetricTriangulationNet (lib/models/triangulation.py) on the device against tests/vol_ref.py, the float64
restatement of its `lift`. The rig: V = 2 views of tests/volumetric_ref.ring_cameras on a 600 mm ring, principal point
at the centre of 16 x 16 heat maps (64 x 64 images), VOLUME_SIZE 32, CUBOID_SIZE 100, seeded weights (the reference's
init_weights for the backbone, tests/v2v_ref.fill_state_dict for V2V, a seeded draw for process_features), theta given
explicitly.
Criterion: per tensor, max-abs error over max|float64| is held to 4 x the largest such error of the same graph run in
float32 on the CPU over the tensors of the case - the project's whole-network rule (tests/v2v_train_ref.compare).
Each test runs in a spawned child (tests/spawned.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import mhp_tree
import v2v_ref as R
import v2v_train_ref as TR
import vol_ref as VOL
import volumetric_ref as VR
from spawned import spawned

pytestmark = pytest.mark.gpu

YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_VolTriangulation_w32_v1.yaml')
V, HM, S, SIDE, FEAT, K = 2, 16, 32, 100.0, 480, 21
OPTS = ['MODEL.VOLUME_SIZE', str(S), 'MODEL.CUBOID_SIZE', str(SIDE), 'MODEL.IMAGE_SIZE', '[64, 64]',
        'MODEL.HEATMAP_SIZE', '[16, 16]']


def _cfg(opts=()):
    from config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(OPTS + list(opts))
    return cfg


def _proj(B):
    p = VR.ring_cameras(V, 600.0, 80.0, (HM / 2.0, HM / 2.0))
    return np.repeat(p[None], B, 0).astype(np.float32).astype(np.float64)


def _fill(model, seed):
    """seeded weights for the whole model; -> (V2V state as float64 numpy, w, b of process_features as float64).
    The backbone gets the reference's own initialisation (init_weights: conv N(0, 0.001), BatchNorm (1, 0) over running
    statistics (0, 1)), which stays finite in eval mode; hipnet.synth's weights need calibrated running statistics
    there (tests/golden/make_golden.py calibrate_bn) and overflow without them."""
    torch.manual_seed(seed)
    model.backbone.init_weights('')
    sd0 = model.volume_net.state_dict()
    fill = R.fill_state_dict([(k, tuple(v.shape)) for k, v in sd0.items()], seed + 1)
    fill = {k: (np.asarray(v, dtype=np.float32).astype(np.float64) if np.asarray(v).dtype.kind == 'f' else v)
            for k, v in fill.items()}
    model.volume_net.load_state_dict({k: torch.from_numpy(np.asarray(fill[k])).to(sd0[k].dtype) for k in sd0}, strict=True)
    rng = np.random.default_rng(seed + 2)
    w = rng.normal(0.0, 1.4 / np.sqrt(FEAT), (32, FEAT, 1, 1)).astype(np.float32).astype(np.float64)
    b = rng.uniform(-0.1, 0.1, 32).astype(np.float32).astype(np.float64)
    with torch.no_grad():
        model.process_features[0].weight.copy_(torch.from_numpy(w).float())
        model.process_features[0].bias.copy_(torch.from_numpy(b).float())
    return fill, w, b


def _leaves(rng, B):
    z = rng.normal(0.0, 1.0, (B * V, K, HM * HM))
    e = np.exp(z - z.max(-1, keepdims=True))
    hm = (e / e.sum(-1, keepdims=True)).reshape(B * V, K, HM, HM).astype(np.float32)
    feat = rng.normal(0.0, 1.0, (B * V, FEAT, HM, HM)).astype(np.float32)
    return hm, feat


def _compare(what, dev, r64, r32, factor=4.0, losses_apart=False):
    """every tensor's max-abs error over max|float64| against `factor` x the largest such error of the float32 CPU run
    over the tensors of the case (the whole-network rule of tests/v2v_train_ref.compare). An all-zero tensor scores 1
    and a sign error 2, so the rule bites where factor x e_ref stays below 1. losses_apart: the scalars named loss* are
    held to factor x the largest float32 error among THEMSELVES instead - never looser, and not spoilt by
    ill-conditioned gradients in the same case. (Not each to its own float32 error: one scalar's can be small by
    chance - 5.7e-4 on one machine and 1.4e-2 on another for the same loss, the CPU's summation order differing.)"""
    own = {k: TR.rel_err(r32[k], r64[k]) for k in r64}
    e_ref = max(own.values())
    e_loss = max([own[k] for k in own if k.startswith('loss')] or [e_ref])
    worst = {}
    for k in r64:
        worst[k] = TR.rel_err(dev[k], r64[k])
        print('{}: {} device {:.3e} (float32 on the CPU {:.3e})'.format(what, k, worst[k], own[k]))
    print('{}: e_ref {:.3e}, bound {:.3e}{}'.format(what, e_ref, factor * e_ref, ', losses {:.3e}'.format(
        factor * e_loss) if losses_apart else ''))
    for k, e in worst.items():
        lim = factor * (e_loss if losses_apart and k.startswith('loss') else e_ref)
        assert e <= lim, (what, k, e, lim)
    return e_ref


@spawned
def test_lift_eval_against_float64():
    """B = 1, leaf heat maps (a softmax of normals: the decode lies well inside the map) and features (2, 480, 16, 16):
    vol_keypoints_3d, volumes, coord_volumes and base_points against the restatement.
    First run on an MI355X: vol_keypoints_3d 8.3e-8, volumes 5.1e-6, coord_volumes 1.1e-7, base_points 2.5e-8 of the
    largest float64 value; the float32 CPU run 5.7e-6 (key points), so the bound was 2.3e-5."""
    from models.triangulation import VolumetricTriangulationNet
    rng = np.random.default_rng(301)
    model = VolumetricTriangulationNet(_cfg(), is_train=False)
    fill, w, b = _fill(model, 31)
    hm, feat = _leaves(rng, 1)
    proj, theta = _proj(1), 0.4

    def ref(dtype):
        with torch.no_grad():
            kp, p, coord, base = VOL.lift(R.Net(fill, dtype), torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype),
                                          torch.from_numpy(hm).to(dtype), torch.from_numpy(feat).to(dtype), proj, SIDE, S,
                                          [theta], dtype=dtype)
        return {'vol_keypoints_3d': kp.double().numpy(), 'volumes': p.double().numpy(), 'coord_volumes': coord.numpy(),
                'base_points': base.numpy()}
    r64, r32 = ref(torch.float64), ref(torch.float32)
    model = model.cuda().eval()
    with torch.no_grad():
        out = model.lift(torch.from_numpy(hm).cuda(), torch.from_numpy(feat).cuda(),
                         torch.from_numpy(proj).float().cuda(), theta=theta)
    torch.cuda.synchronize()
    assert out[4] is None and tuple(out[1].shape) == (1, V, K, 2) and tuple(out[2].shape) == (1, V, K, HM, HM)
    dev = {'vol_keypoints_3d': out[0], 'volumes': out[3], 'coord_volumes': out[5], 'base_points': out[6]}
    dev = {k: v.cpu().double().numpy() for k, v in dev.items()}
    _compare('lift, eval', dev, r64, r32)
    # eval mode with a gradient required is refused, and so are CPU tensors
    with pytest.raises(NotImplementedError, match='eval mode'):
        model.lift(torch.from_numpy(hm).cuda(), torch.from_numpy(feat).cuda(), torch.from_numpy(proj).float().cuda(), theta=theta)
    with pytest.raises(ValueError, match='HIP-device'):
        model.lift(torch.from_numpy(hm), torch.from_numpy(feat), torch.from_numpy(proj).float(), theta=theta)


def _ground_truth(rng, coord):
    """(B, K, 3): 0.3 of the voxel pitch from a voxel centre towards its neighbour along the first grid axis, so the
    nearest-voxel choice is not a tie (as tests/golden/make_golden_volumetric.py displaces its ground truth)"""
    B = coord.shape[0]
    ijk = rng.integers(8, 24, (B, K, 3))
    bi = np.arange(B)[:, None]
    here = coord[bi, ijk[..., 0], ijk[..., 1], ijk[..., 2]]
    there = coord[bi, ijk[..., 0] + 1, ijk[..., 1], ijk[..., 2]]
    return (0.7 * here + 0.3 * there).astype(np.float32).astype(np.float64)


def _training_case(what, B, thetas, steps, seed, losses_apart):
    """loss Joints3DMSELoss + 0.01 VolumetricCELoss through `lift` on fixed leaves: the gradients of the first step
    (leaf features, process_features, V2V's first and last convolution) and the loss of each of `steps`
    Adam(lr = 1e-3) steps on process_features and volume_net, on the device and in the restatement -> e_ref"""
    from core.loss import Joints3DMSELoss, VolumetricCELoss
    from models.triangulation import VolumetricTriangulationNet
    rng = np.random.default_rng(seed)
    model = VolumetricTriangulationNet(_cfg(), is_train=True)
    fill, w, b = _fill(model, 33)
    hm, feat = _leaves(rng, B)
    proj = _proj(B)
    _pred, base = VOL.base_points(torch.from_numpy(hm), proj)
    gt = _ground_truth(rng, VOL.coord_volumes(base, SIDE, S, thetas))
    names = {'front_layers.0.block.0.weight', 'output_layer.weight'}

    def ref(dtype):
        net = TR.TrainNet(fill, dtype)
        wt = torch.from_numpy(w).to(dtype).requires_grad_(True)
        bt = torch.from_numpy(b).to(dtype).requires_grad_(True)
        params = [wt, bt] + [v for k, v in net.sd.items() if net.is_param(k)]
        opt = torch.optim.Adam(params, lr=1e-3)
        out = {}
        for s in range(steps):
            ft = torch.from_numpy(feat).to(dtype).requires_grad_(True)
            kp, p, coord, _base = VOL.lift(net, wt, bt, torch.from_numpy(hm).to(dtype), ft, proj, SIDE, S, thetas, dtype=dtype)
            total = VOL.loss(kp, p, coord, gt)
            opt.zero_grad()
            total.backward()
            if s == 0:
                out.update({'grad:features': ft.grad, 'grad:process_features.0.weight': wt.grad.clone(),
                            'grad:process_features.0.bias': bt.grad.clone()})
                out.update({'grad:volume_net.' + k: net.sd[k].grad.clone() for k in names})
            out['loss{}'.format(s)] = total.detach().reshape(1)
            if s + 1 < steps:
                opt.step()
        return {k: v.double().numpy() for k, v in out.items()}
    r64, r32 = ref(torch.float64), ref(torch.float32)

    model = model.cuda().train()
    params = list(model.process_features.parameters()) + list(model.volume_net.parameters())
    opt = torch.optim.Adam(params, lr=1e-3)
    j3d, ce = Joints3DMSELoss(), VolumetricCELoss()
    gtd = torch.from_numpy(gt).float().cuda()
    ones = torch.ones(B, K, 1, device='cuda')
    dev = {}
    for s in range(steps):
        ft = torch.from_numpy(feat).cuda().requires_grad_(True)
        out = model.lift(torch.from_numpy(hm).cuda(), ft, torch.from_numpy(proj).float().cuda(), theta=thetas)
        total = j3d(out[0], gtd) + 0.01 * ce(out[5], out[3], gtd, ones)
        opt.zero_grad()
        total.backward()
        if s == 0:
            dev['grad:features'] = ft.grad
            dev['grad:process_features.0.weight'] = model.process_features[0].weight.grad.clone()
            dev['grad:process_features.0.bias'] = model.process_features[0].bias.grad.clone()
            got = dict(model.volume_net.named_parameters())
            dev.update({'grad:volume_net.' + k: got[k].grad.clone() for k in names})
        dev['loss{}'.format(s)] = total.detach().reshape(1)
        if s + 1 < steps:
            opt.step()
    torch.cuda.synchronize()
    dev = {k: v.cpu().double().numpy() for k, v in dev.items()}
    print('losses: device {}, float64 {}'.format([float(dev['loss{}'.format(s)]) for s in range(steps)],
                                                 [float(r64['loss{}'.format(s)]) for s in range(steps)]))
    assert set(dev) == set(r64)
    return _compare(what, dev, r64, r32, losses_apart=losses_apart)


@spawned
def test_lift_training_gradients_and_adam_steps():
    """B = 2, theta = (0, 1.0): the gradients of the first step and the losses of three Adam steps by the
    whole-network rule, the three losses held apart to 4 x the largest float32 CPU error among the losses.
    What this rig can and cannot show, from the runs on an MI355X: the losses were 51.4631, 50.3289, 48.1072 against
    51.4635, 50.5122, 48.2775 in float64 (8.2e-6, 3.6e-3, 3.5e-3; float32 on the CPU 3.2e-3, 1.7e-2, 5.7e-4 on one
    machine and 2.4e-3, 2.5e-2, 1.4e-2 on another, so their bound was 6.6e-2 and 0.1): the trajectory of three
    optimiser steps is held. Every gradient was at 0.49 to 0.55 (output_layer.weight 1.9e-3) where the float32 CPU run
    is at 0.84 to 1.25: with two samples the bottom level of V2V normalises two values per channel, the backward is
    that sensitive in float32 on any machine, and a bound of 4 x such an error (5.0) passes a zero or a sign-flipped
    gradient. This case therefore says NOTHING about the gradients; the well-conditioned case below holds them.
    The float64 restatement takes about 30 s on 16 CPU threads, the float32 one 8 s."""
    _training_case('lift, training, B = 2', 2, [0.0, 1.0], 3, 303, losses_apart=True)


@spawned
def test_lift_training_gradients_where_float32_is_accurate():
    """B = 4, theta = (0, 1, 2, 3), one forward and backward: with four values per channel at V2V's bottom level the
    float32 CPU run of the same graph is within 2.7e-3 of float64 in every gradient (features 1.3e-3,
    process_features 2.0e-3 and 2.6e-3, V2V's first convolution 1.6e-3, its last 6e-6; loss 1e-6), so the
    whole-network rule, 4 x the largest of them = 1.1e-2, is a real bound on the gradient path _PointwiseFn ->
    unprojection -> V2V -> soft-argmax -> both losses: a missing term, a zero or a wrong sign scores 1 or more. The
    test asserts that the bound it derives stays below 0.1, so it cannot turn vacuous unnoticed. On an MI355X:
    features 6.0e-3, process_features 5.3e-3 and 7.9e-3, V2V's first convolution 4.8e-3, its last 6.6e-6, loss
    4.3e-7. About 21 s of float64 and 4 s of float32 restatement on 16 CPU threads."""
    e_ref = _training_case('lift, training, B = 4', 4, [0.0, 1.0, 2.0, 3.0], 1, 305, losses_apart=False)
    assert 4.0 * e_ref < 0.1, e_ref


def _images(B, seed):
    from hipnet import synth
    return torch.from_numpy(synth.rhd_batch(B * V, seed=seed, img_h=64, img_w=64)['imgs']).reshape(B, V, 3, 64, 64)


@spawned
def test_whole_model_forward_is_lift_and_one_training_step():
    """Eval mode: forward(images, proj) is lift(*backbone(images)[:2], proj) bit for bit, and theta=None is theta=0.
    Then one training step at B = 2 with the optimiser tools/train_vol.py builds. The loss is Joints3DMSELoss + 0.01
    VolumetricCELoss + JointsMSELoss on the decoded heat maps (LOSS.WITH_POSE2D_LOSS): base points and coordinate
    volumes are constants here, so without a 2-D term nothing reaches last_layer, whose output feeds the heat maps only
    (the features branch off before it). Finite non-zero gradients in stage4, last_layer, process_features and
    volume_net; the frozen parameters keep their bits through optimizer.step(), the three groups move; a second
    forward and backward reuses the plans."""
    from core.loss import Joints3DMSELoss, JointsMSELoss, VolumetricCELoss
    from models.triangulation import VolumetricTriangulationNet
    sys.path.insert(0, os.path.join(mhp_tree.PKG, 'tools'))
    import train_vol
    cfg = _cfg()
    model = VolumetricTriangulationNet(cfg, is_train=True)
    _fill(model, 35)
    model = model.cuda().eval()
    img1, proj1 = _images(1, 5).cuda(), torch.from_numpy(_proj(1)).float().cuda()
    with torch.no_grad():
        full = model(img1, proj1, theta=0.25)
        hm, feat = model.backbone(img1.reshape(-1, 3, 64, 64))[:2]
        parts = model.lift(hm, feat, proj1, theta=0.25)
        none = model(img1, proj1)
        zero = model(img1, proj1, theta=0.0)
    for i in (0, 1, 2, 3, 5, 6):
        assert bool(torch.isfinite(full[i]).all()), 'output {} is not finite'.format(i)
        assert torch.equal(full[i], parts[i]), 'forward differs from backbone + lift in output {}'.format(i)
        assert torch.equal(none[i], zero[i]), 'theta=None in eval mode is not theta=0 (output {})'.format(i)
    assert full[4] is None and tuple(full[0].shape) == (1, K, 3) and tuple(full[3].shape) == (1, K, S, S, S)
    assert bool(torch.isfinite(full[0]).all())

    model.train()
    B = 2
    img, proj = _images(B, 7).cuda(), torch.from_numpy(_proj(B)).float().cuda()
    opt = train_vol.build_optimizer(cfg, model)
    assert [g['name'] for g in opt.param_groups] == ['backbone', 'process_features', 'volume_net']
    assert [g['lr'] for g in opt.param_groups] == [cfg.TRAIN.LR, cfg.TRAIN.PROCESS_FEATURE_LR, cfg.TRAIN.VOLUME_NET_LR]
    assert all(g['weight_decay'] == 0 for g in opt.param_groups)
    j3d, ce, j2d = Joints3DMSELoss(), VolumetricCELoss(), JointsMSELoss()
    ones = torch.ones(B, K, 1, device='cuda')
    gt2d = torch.linspace(3.0, 12.0, B * V * K * 2, device='cuda').reshape(B * V, K, 2)

    def step():
        out = model(img, proj, theta=[0.0, 1.0])
        gt = (out[6][:, None, :] + torch.linspace(-20.0, 20.0, K * 3, device='cuda').reshape(1, K, 3)).detach()
        total = j3d(out[0], gt) + 0.01 * ce(out[5], out[3], gt, ones) + \
            j2d(out[1].reshape(B * V, K, 2), gt2d, visibility=torch.ones(B * V, K, device='cuda'))
        opt.zero_grad()
        total.backward()
        return total
    step()
    torch.cuda.synchronize()
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    for k, p in model.named_parameters():
        trains = k.startswith(('backbone.stage4.', 'backbone.last_layer.', 'process_features.', 'volume_net.'))
        assert p.requires_grad == trains, k
    for prefix in ('backbone.stage4.', 'backbone.last_layer.', 'process_features.', 'volume_net.'):
        grads = [p.grad for k, p in model.named_parameters() if k.startswith(prefix)]
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads), prefix
        assert max(float(g.abs().max()) for g in grads) > 0, prefix
    opt.step()
    torch.cuda.synchronize()
    changed = {'backbone.': 0, 'process_features.': 0, 'volume_net.': 0}
    for k, p in model.named_parameters():
        same = torch.equal(p.detach().view(torch.int32) if p.dtype == torch.float32 else p.detach(),
                           before[k].view(torch.int32) if p.dtype == torch.float32 else before[k])
        if not p.requires_grad:
            assert same, 'the frozen parameter {} moved'.format(k)
        elif not same:
            changed[[g for g in changed if k.startswith(g)][0]] += 1
    assert all(n > 0 for n in changed.values()), changed
    # a second forward and backward: the plans are reused, the updated weights are read
    total = step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(total))


@spawned
def test_backbone_with_the_confidence_head_runs_and_leaves_it_alone():
    """pose_hrnet_volumetric with MODEL.VOL_CONFIDENCES true on the device: hipnet.net.HipNet must walk past the
    head's children (its 480 -> 512 3 x 3 convolution exceeds the weight packer's staging, its BatchNorms would enter
    the engine's tables). With the weights of a VOL_CONFIDENCES false backbone: eval-mode heat maps and features are the
    same bits; one training forward and backward (ordered batch statistics, HRNET_DETERMINISTIC=1) gives the same
    gradients; every vol_confidences.* parameter and buffer keeps its bits and receives no gradient."""
    os.environ['HRNET_DETERMINISTIC'] = '1'
    from models import pose_hrnet_volumetric
    torch.manual_seed(41)
    plain = pose_hrnet_volumetric.get_pose_net(_cfg(['MODEL.VOL_CONFIDENCES', 'False']), is_train=False)
    plain.init_weights('')
    conf = pose_hrnet_volumetric.get_pose_net(_cfg(['MODEL.VOL_CONFIDENCES', 'True']), is_train=False)
    res = conf.load_state_dict(plain.state_dict(), strict=False)
    assert not res.unexpected_keys and len(res.missing_keys) == 18      # num_batches_tracked is never reported
    assert all(k.startswith('vol_confidences.') for k in res.missing_keys)
    head = {k: v.clone() for k, v in conf.state_dict().items() if k.startswith('vol_confidences.')}
    assert len(head) == 20
    x = _images(2, 11).reshape(-1, 3, 64, 64).cuda()
    plain, conf = plain.cuda().eval(), conf.cuda().eval()
    with torch.no_grad():
        a, b = plain(x), conf(x)
    assert len(b) == 4 and b[3] is None and a[3] is None
    for i, name in ((0, 'heat maps'), (1, 'features')):
        assert bool(torch.isfinite(b[i]).all()), name
        assert torch.equal(a[i], b[i]), '{} differ with the confidence head present'.format(name)
    assert tuple(b[1].shape) == (4, FEAT, HM, HM)

    g_hm = torch.linspace(-1.0, 1.0, 4 * K * HM * HM, device='cuda').reshape(4, K, HM, HM)
    g_ft = torch.linspace(1.0, -1.0, 4 * FEAT * HM * HM, device='cuda').reshape(4, FEAT, HM, HM)
    grads = []
    for model in (plain, conf):
        model.train()
        hm, feat = model(x)[:2]
        ((hm * g_hm).sum() + 1e-3 * (feat * g_ft).sum()).backward()
        torch.cuda.synchronize()
        grads.append({k: p.grad.clone() for k, p in model.named_parameters()
                      if not k.startswith('vol_confidences.') and p.grad is not None})
    assert set(grads[0]) == set(grads[1]) and len(grads[0]) > 300
    worst = 0.0
    for k, g in grads[0].items():
        top = float(g.abs().max())
        worst = max(worst, float((g - grads[1][k]).abs().max()) / max(top, 1e-30))
    print('confidence head present: largest gradient difference over max|gradient| = {:.3e}'.format(worst))
    assert worst == 0.0, worst            # the same launches on the same values in a fixed order
    assert float(grads[1]['last_layer.3.weight'].abs().max()) > 0 and float(grads[1]['conv1.weight'].abs().max()) > 0
    # the default mode (atomic batch sums, BatchNorm coefficients built by the consumers) on a plan of its own: the
    # engine's decision must not see the head's 512-wide BatchNorm, which is wider than the tables of hrnet_sum_terms
    os.environ['HRNET_DETERMINISTIC'] = '0'
    for model in (plain, conf):
        hm, feat = model(x[:2])[:2]
        ((hm * g_hm[:2]).sum() + 1e-3 * (feat * g_ft[:2]).sum()).backward()
        torch.cuda.synchronize()
        plans = [p for p in model.hip().all_plans() if p.training and p.N == 2]
        assert len(plans) == 1 and plans[0].bn_sums, 'the consumer-side BatchNorm path was not taken'
        assert not any(n.startswith('vol_confidences') for n in list(plans[0].bns) + list(model.hip().convs))
        assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    for k, p in conf.named_parameters():
        if k.startswith('vol_confidences.'):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    after = conf.state_dict()
    for k, v in head.items():
        assert torch.equal(after[k].cpu(), v), '{} changed'.format(k)


@spawned
def test_checkpoint_round_trip(tmp_path):
    from models.triangulation import VolumetricTriangulationNet
    cfg = _cfg()
    model = VolumetricTriangulationNet(cfg, is_train=False)
    _fill(model, 37)
    path = str(tmp_path / 'vol.pth.tar')
    torch.save(model.state_dict(), path)
    img, proj = _images(1, 9).cuda(), torch.from_numpy(_proj(1)).float().cuda()
    model = model.cuda().eval()
    with torch.no_grad():
        a = model(img, proj)
    other = VolumetricTriangulationNet(cfg, is_train=False)
    other.load_state_dict(torch.load(path, map_location='cpu'), strict=True)
    other = other.cuda().eval()
    with torch.no_grad():
        b = other(img, proj)
    for i in (0, 1, 2, 3, 5, 6):
        assert bool(torch.isfinite(a[i]).all()), 'output {} is not finite'.format(i)
        assert torch.equal(a[i], b[i]), 'output {} differs after the round trip'.format(i)
