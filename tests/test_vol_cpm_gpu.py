"""CPM_volumetric and VolumetricTriangulationNet_CPM on the GPU against tests/vol_cpm_ref.py, with the seeded weights of
cpm_ref.fill_state_dict (none stored).

Backbone, cases c (8 x 16 -> 1 x 2 maps, HEATMAP_SIZE [4, 4]) and b (40 x 72 -> 5 x 9 maps, HEATMAP_SIZE [18, 10]): the seven
outputs against the float64 restatement under cpm_ref.bound(e_ref), e_ref the float32 CPU run (the convention of
tests/test_cpm_model_gpu.py). Short backward: the loss and the gradients of Mconv3/4/5_stage6 and of process_features
against float64 autograd of the restatement with the device's ReLU decisions of Mconv3/4_stage6 handed in (the convention of
tests/test_cpm_train_model_gpu.py: err = max|dev - ref64| / max|ref64| per tensor within cpm_ref.bound(e_ref)). Frozen
layers keep their bits through an optimiser step and get no gradient; the training forward has the inference forward's
bits. Whole model at B = 1, V = 2, 64 x 64 images, 16 x 16 heat maps, VOLUME_SIZE 32: the eval forward against
vol_cpm_ref.lift (tests/vol_ref.py's pieces) on the restated backbone by the whole-network rule of tests/test_vol_gpu.py, one
training step, a checkpoint round trip. Gradients through trained-mode V2V are not compared at this size (DESIGN: its
bottom level normalises two values per channel)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import cpm_ref as R
import mhp_tree
import v2v_ref as V2V
import v2v_train_ref as TR
import vol_cpm_ref as VC
import volumetric_ref as VR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_VolTriangulation_CPM_v1.yaml')
HM = {'c': (4, 4), 'b': (18, 10)}                    # MODEL.HEATMAP_SIZE (width, height)
V, S, SIDE, K = 2, 32, 100.0, 21


def _cfg(opts=()):
    return mhp_tree.config('.', list(opts), YAML)


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def _state():
    return R.fill_state_dict(R.K_JOINTS, R.SEED)


def _backbone(case, trainable=False):
    from models import CPM_volumetric
    model = CPM_volumetric.get_pose_net(_cfg(['MODEL.HEATMAP_SIZE', str(list(HM[case]))]), is_train=trainable,
                                        trainable=trainable)
    res = model.load_state_dict(R.to_torch(_state(), torch.float32), strict=False)
    assert not res.unexpected_keys and all(k.startswith('vol_confidences.') for k in res.missing_keys)
    if trainable:
        for k, p in model.named_parameters():
            p.requires_grad = k.split('.')[0] in VC.TRAINED
    return model.to(DEV)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _reference(case, dtype):
    hw = HM[case][::-1]
    img, cm = R.inputs(case)
    with torch.no_grad():
        low, heat, feat = VC.backbone(R.to_torch(_state(), dtype), torch.tensor(img, dtype=dtype), torch.tensor(cm, dtype=dtype), hw)
    return [t.double().numpy() for t in list(low) + [heat, feat]]


@functools.lru_cache(maxsize=None)
def _inference(case):
    img, cm = R.inputs(case)
    model = _backbone(case).eval()
    with torch.no_grad():
        out = model(_dev(img), _dev(cm))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('case', sorted(HM))
def test_backbone_outputs_against_float64(case):
    from models import CPM_volumetric
    out = _inference(case)
    B, H, W = R.CASES[case]
    assert len(out) == 8 and out[7] is None
    assert tuple(out[5].shape) == (B, K + 1) + HM[case][::-1] and tuple(out[6].shape) == (B, H // 8, W // 8, 128)
    assert CPM_volumetric.CPM.inter_feat(out) is out[6]
    dev = [o.cpu().double().numpy() for o in out[:6]] + [_nchw(out[6]).cpu().double().numpy()]
    r64, r32 = _reference(case, torch.float64), _reference(case, torch.float32)
    names = ['stage%d' % s for s in range(1, 6)] + ['stage6 lifted', 'inter_feat']
    for name, d, a, b in zip(names, dev, r64, r32):
        err, e_ref = R.rel(d, a), R.rel(b, a)
        print('{} {}: err {:.3g} e_ref {:.3g} bound {:.3g}'.format(case, name, err, e_ref, R.bound(e_ref)))
        assert err <= R.bound(e_ref), (name, err, e_ref)


@functools.lru_cache(maxsize=None)
def _short_run(case):
    """one training forward, backward and Adam step of the backbone with process_features behind it ->
    (loss, gradients, the seven outputs, the decisions, parameters before, parameters after, gradient presence)"""
    from hipnet import upsample_slice as S_
    from models.triangulation import process_features_nhwc
    hw = HM[case][::-1]
    img, cm = R.inputs(case)
    tgt, wts = VC.short_targets(case, hw)
    w, b = VC.process_weights()
    model = _backbone(case, trainable=True).train()
    conv = torch.nn.Conv2d(VC.INTER, 32, 1).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(_dev(w))
        conv.bias.copy_(_dev(b))
    out = model(_dev(img), _dev(cm))
    tape = model.tape
    dec = {'Mconv3_stage6': _nchw(tape['m3']).cpu() > 0, 'Mconv4_stage6': _nchw(tape['m4']).cpu() > 0}
    feats = S_.upsample_slice(process_features_nhwc(model.inter_feat(out), conv), 0, 32, hw)
    loss = ((out[5] - _dev(tgt)) ** 2).sum((2, 3)).mean() + (feats * _dev(wts)).sum() / feats.shape[0]
    trained = [p for p in model.parameters() if p.requires_grad] + list(conv.parameters())
    opt = torch.optim.Adam(trained, lr=1e-3)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    loss.backward()
    torch.cuda.synchronize()
    assert model.tape is None
    grads = {'backbone.' + k: p.grad.double().cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}
    grads.update({'process_features.0.' + k: p.grad.double().cpu().numpy() for k, p in conv.named_parameters()})
    present = {k: p.grad is not None for k, p in model.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    after = {k: p.detach().clone() for k, p in model.named_parameters()}
    return float(loss.detach()), grads, [o.detach() for o in out[:7]], dec, before, after, present


@pytest.mark.parametrize('case', sorted(HM))
def test_short_backward_against_float64_autograd(case):
    hw = HM[case][::-1]
    loss, grads, _, dec, _, _, _ = _short_run(case)
    l64, g64 = VC.short_loss_and_grads(_state(), case, hw, torch.float64, dec)
    l32, g32 = VC.short_loss_and_grads(_state(), case, hw, torch.float32, dec)
    assert set(grads) == set(g64) and len(g64) == 8
    e_ref = abs(l32 - l64) / abs(l64)
    print('{} loss {:.9g} ref {:.9g}: err {:.3g} e_ref {:.3g}'.format(case, loss, l64, abs(loss - l64) / abs(l64), e_ref))
    assert abs(loss - l64) / abs(l64) <= R.bound(e_ref)
    worst = []
    for name in sorted(g64):
        denom = float(np.abs(g64[name]).max())
        assert denom > 0, name
        err, e_ref = R.rel(grads[name], g64[name], denom), R.rel(g32[name], g64[name], denom)
        print('{} {}: err {:.3g} e_ref {:.3g} bound {:.3g}'.format(case, name, err, e_ref, R.bound(e_ref)))
        if err > R.bound(e_ref):
            worst.append((name, err, e_ref, R.bound(e_ref)))
    assert not worst, worst


@pytest.mark.parametrize('case', sorted(HM))
def test_frozen_layers_keep_their_bits_and_the_training_forward_has_the_inference_bits(case):
    _, _, outs, _, before, after, present = _short_run(case)
    moved = 0
    for k in before:
        trains = k.split('.')[0] in VC.TRAINED
        assert present[k] == trains, k
        same = torch.equal(before[k].view(torch.int32), after[k].view(torch.int32))
        assert same != trains, k
        moved += int(not same)
    assert moved == 6 and len(before) == 80 + 14         # the CPM's tensors and the confidence head's parameters
    want = _inference(case)
    for i in range(7):
        assert torch.equal(outs[i], want[i]), i


# ---------------------------------------------------------------------------------------------------- the whole model
OPTS = ['MODEL.VOLUME_SIZE', str(S), 'MODEL.CUBOID_SIZE', str(SIDE), 'MODEL.IMAGE_SIZE', '[64, 64]',
        'MODEL.HEATMAP_SIZE', '[16, 16]']


@functools.lru_cache(maxsize=None)
def _proj(B):
    """the ring rig of tests/test_vol_gpu.py with each view's principal point moved onto the pixel the float64 restatement
    decodes for the base joint: the two rays then meet at the ring's centre, so the cuboid lies where the maps see it
    (the seeded CPM's maps know nothing of any rig; an inconsistent pair of pixels triangulates metres away)"""
    from oracle import hrnet_cpu as O
    img, cm = R.inputs('a')
    with torch.no_grad():
        heat = VC.backbone(R.to_torch(_state(), torch.float64), torch.tensor(img), torch.tensor(cm), (16, 16))[1]
    pred = O.get_final_preds(heat[:, 1:], False).double().numpy()
    p = VR.ring_cameras(V, 600.0, 80.0, (8.0, 8.0))
    for v in range(V):
        shift = np.eye(3)
        shift[:2, 2] = pred[v, VC.BASE_JOINT] - 8.0
        p[v] = shift @ p[v]
    return np.repeat(p[None], B, 0).astype(np.float32).astype(np.float64)


def _model(is_train):
    from models.triangulation import VolumetricTriangulationNet_CPM
    model = VolumetricTriangulationNet_CPM(_cfg(OPTS), is_train=is_train)
    model.backbone.load_state_dict(R.to_torch(_state(), torch.float32), strict=False)
    sd0 = model.volume_net.state_dict()
    fill = V2V.fill_state_dict([(k, tuple(v.shape)) for k, v in sd0.items()], 71)
    fill = {k: (np.asarray(v, dtype=np.float32).astype(np.float64) if np.asarray(v).dtype.kind == 'f' else v)
            for k, v in fill.items()}
    model.volume_net.load_state_dict({k: torch.from_numpy(np.asarray(fill[k])).to(sd0[k].dtype) for k in sd0}, strict=True)
    w, b = VC.process_weights()
    with torch.no_grad():
        model.process_features[0].weight.copy_(torch.from_numpy(w).float())
        model.process_features[0].bias.copy_(torch.from_numpy(b).float())
    return model, fill, w, b


def _inputs(B=1):
    """(image, centre map) of cpm_ref's case a, (2, 3, 64, 64): B = 1, V = 2; B = 2 adds the two views swapped"""
    img, cm = R.inputs('a')
    if B == 2:
        img, cm = np.concatenate([img, img[::-1]]), np.concatenate([cm, cm[::-1]])
    return img, cm, _dev(img).view(B, V, 3, 64, 64), _dev(cm).view(B, V, 1, 64, 64)


def test_whole_model_eval_against_the_restatement():
    model, fill, w, b = _model(False)
    img, cm, dimg, dcm = _inputs()
    proj, theta = _proj(1), 0.4

    def ref(dtype):
        t = lambda a: torch.tensor(a, dtype=dtype)
        with torch.no_grad():
            _low, heat, feat = VC.backbone(R.to_torch(_state(), dtype), t(img), t(cm), (16, 16))
            kp, p, coord, base, pred = VC.lift(V2V.Net(fill, dtype), t(w), t(b), heat, feat, proj, SIDE, S, [theta], dtype=dtype)
        return {'vol_keypoints_3d': kp.double().numpy(), 'volumes': p.double().numpy(), 'coord_volumes': coord.numpy(),
                'base_points': base.numpy(), 'heatmaps': heat.double().numpy()[None]}, pred
    (r64, p64), (r32, p32) = ref(torch.float64), ref(torch.float32)
    assert np.array_equal(p64, p32)                 # the arg-max decode is not within rounding of a tie
    model = model.to(DEV).eval()
    with torch.no_grad():
        out = model(dimg, dcm, _dev(proj), theta=theta)
        none, zero = model(dimg, dcm, _dev(proj)), model(dimg, dcm, _dev(proj), theta=0.0)
    torch.cuda.synchronize()
    assert out[4] is None and tuple(out[1].shape) == (1, V, K, 2) and tuple(out[2].shape) == (1, V, K + 1, 16, 16)
    assert np.array_equal(out[1].cpu().double().numpy(), p64)
    dev = {'vol_keypoints_3d': out[0], 'volumes': out[3], 'coord_volumes': out[5], 'base_points': out[6], 'heatmaps': out[2]}
    dev = {k: v.cpu().double().numpy() for k, v in dev.items()}
    own = {k: TR.rel_err(r32[k], r64[k]) for k in r64}
    e_ref = max(own.values())
    for k in r64:
        err = TR.rel_err(dev[k], r64[k])
        print('{}: device {:.3e} (float32 on the CPU {:.3e}), bound {:.3e}'.format(k, err, own[k], 4 * e_ref))
        assert err <= 4.0 * e_ref, (k, err, e_ref)
    assert 4.0 * e_ref < 0.1
    for i in (0, 1, 2, 3, 5, 6):
        assert torch.equal(none[i], zero[i]), i
    with pytest.raises(NotImplementedError, match='eval mode'):
        model(dimg, dcm, _dev(proj), theta=theta)


def test_whole_model_training_step_and_checkpoint_round_trip(tmp_path):
    """one training step at B = 2 (at B = 1 and VOLUME_SIZE 32 the bottom level of V2V holds ONE value per channel, and
    V2VModel refuses batch statistics over it, as torch's BatchNorm does), then the checkpoint round trip at B = 1"""
    from core.loss import HeatmapLoss, Joints3DMSELoss, VolumetricCELoss
    from models.triangulation import VolumetricTriangulationNet_CPM
    sys.path.insert(0, os.path.join(mhp_tree.PKG, 'tools'))
    import train_vol
    cfg = _cfg(OPTS)
    model, _fill, _w, _b = _model(True)
    model = model.to(DEV).train()
    B = 2
    _img, _cm, dimg, dcm = _inputs(B)
    proj = _dev(_proj(B))
    opt = train_vol.build_optimizer(cfg, model)
    assert [len(g['params']) for g in opt.param_groups][:2] == [6, 2]
    tgt = _dev(np.random.RandomState(3).uniform(0, 1, (B * V, K + 1, 16, 16)))
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    out = model(dimg, dcm, proj, theta=[0.3, 1.0])
    gt = (out[6][:, None, :] + torch.linspace(-20.0, 20.0, K * 3, device=DEV).reshape(1, K, 3)).detach()
    total = Joints3DMSELoss()(out[0], gt) + 0.01 * VolumetricCELoss()(out[5], out[3], gt, torch.ones(B, K, 1, device=DEV)) + \
        0.1 * HeatmapLoss()(out[2].reshape(B * V, K + 1, 16, 16), tgt)
    opt.zero_grad()
    total.backward()
    opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(total)), float(total)
    changed = {'backbone.': 0, 'process_features.': 0, 'volume_net.': 0}
    for k, p in model.named_parameters():
        same = torch.equal(p.detach().view(torch.int32), before[k].view(torch.int32))
        if not p.requires_grad:
            assert same and p.grad is None, k
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
            changed[[g for g in changed if k.startswith(g)][0]] += int(not same)
    assert changed['backbone.'] == 6 and changed['process_features.'] == 2 and changed['volume_net.'] > 0, changed
    # the updated weights are read by the next forward (the packed copies follow the parameters)
    model.eval()
    dimg, dcm, proj = dimg[:1].contiguous(), dcm[:1].contiguous(), proj[:1].contiguous()
    path = str(tmp_path / 'vol_cpm.pth.tar')
    torch.save(model.state_dict(), path)
    with torch.no_grad():
        a = model(dimg, dcm, proj)
    other = VolumetricTriangulationNet_CPM(cfg, is_train=False)
    other.load_state_dict(torch.load(path, map_location='cpu'), strict=True)
    other = other.to(DEV).eval()
    with torch.no_grad():
        c = other(dimg, dcm, proj)
    for i in (0, 1, 2, 3, 5, 6):
        assert bool(torch.isfinite(a[i]).all()), i
        assert torch.equal(a[i], c[i]), 'output {} differs after the round trip'.format(i)
