"""A trainable models.FTL_encoder_decoder on the device against tests/ftl_train_ref.py: the loss, the heat maps and the
gradient of every head parameter of one training step in float64, within bound(e_ref) = 4 e_ref + 2 * 2^-24 with e_ref the
same measure of the float32 CPU run - which itself must stay within 1e-3, so that a vacuous bound fails loudly. The biases
whose true gradient is zero are measured on the scale of their layer's pre-BatchNorm gradient (ftl_train_ref.run's
'scale/...'). Then: equal bits of two backward passes, the running statistics after a step, the inference path of a
trainable model, the 3-D-phase loss, and a short training run through tools/train_ftl.py's step and checkpoint."""
import os
import sys

import numpy as np
import pytest
import torch

import ftl_ref as R
import ftl_train_ref as TR
import mhp_tree

pytestmark = pytest.mark.gpu

YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_HRNet_w32_softmax_pose2dloss_FTL_v1.yaml')
_MODELS = {}


def _cfg(channels, V):
    return mhp_tree.config('', ['MODEL.EXTRA.STAGE4.NUM_CHANNELS', str(list(channels)), 'DATASET.NUM_VIEWS', str(V)], YAML)


def _model(channels, V, trainable=True):
    from models.FTL_encoder_decoder import FTLMultiviewNet
    key = (channels, V, trainable)
    if key not in _MODELS:
        torch.manual_seed(0)
        _MODELS[key] = FTLMultiviewNet(_cfg(channels, V), trainable=trainable).cuda()
    return _MODELS[key]


def _load_head(model, state):
    full = dict(model.state_dict())
    full.update({k: v.to('cuda') for k, v in R.to_torch(state, torch.float32).items()})
    model.load_state_dict(full, strict=True)


def _case_inputs(case):
    channels, V, B, (h, w), kind = R.CASES[case]
    feat, ext, K = R.inputs(case)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32, device='cuda')
    return f32(feat), f32(ext), torch.tensor(K, dtype=torch.float32), f32(TR.targets(case))


def _step(case, model=None):
    """one training forward + backward of a case from the fixture's parameters: (model, loss, heat maps)"""
    channels, V, B, (h, w), kind = R.CASES[case]
    model = _model(channels, V) if model is None else model
    _load_head(model, R.fill_state_dict(channels, V, kind=kind))
    model.train()
    feat, ext, K, gt = _case_inputs(case)
    hm, pose2d, pose3d = model.head_forward(feat, ext, K)
    loss = ((pose2d - gt) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    return model, loss.detach(), hm.detach()


def _head_named_parameters(model):
    from hipnet import ftl_train
    return [(n, p) for m in ftl_train.HEAD_MODULES for n, p in getattr(model, m).named_parameters(prefix=m)]


@pytest.mark.parametrize('case', sorted(R.CASES))
def test_gradient_parity(case):
    ref64, ref32 = TR.run(case, torch.float64), TR.run(case, torch.float32)
    model, loss, hm = _step(case)
    worst = 0.0

    def hold(what, got, key, denom=None):
        nonlocal worst
        e_ref = R.rel(ref32[key], ref64[key], denom)
        err = R.rel(got, ref64[key], denom)
        print('case {} {}: err {:.2e}, e_ref {:.2e}, bound {:.2e}'.format(case, what, err, e_ref, R.bound(e_ref)))
        assert e_ref <= 1e-3, '{}: the float32 reference itself is off by {:.2e}: the bound would be vacuous'.format(what, e_ref)
        assert np.isfinite(err) and err <= R.bound(e_ref), what
        worst = max(worst, e_ref)

    hold('loss', loss.cpu().numpy(), 'loss')
    hold('heatmaps', hm.cpu().numpy(), 'heatmaps')
    names = [n for n, _ in _head_named_parameters(model)]
    assert sorted(names) == sorted(k[5:] for k in ref64 if k.startswith('grad/'))
    for name, p in _head_named_parameters(model):
        assert p.grad is not None and p.grad.shape == p.shape, name
        got = p.grad.cpu().numpy()
        if name in TR.ZERO_GRAD_BIASES:
            # true gradient zero: measured on the scale of the sums that cancel
            assert np.abs(ref64['grad/' + name]).max() <= 1e-9 * ref64['scale/' + name], name
            hold(name, got, 'grad/' + name, denom=ref64['scale/' + name])
        else:
            hold(name, got, 'grad/' + name)
    print('case {}: worst e_ref {:.2e}'.format(case, worst))


def test_two_backward_passes_give_equal_bits():
    model, loss1, hm1 = _step('c')
    g1 = [p.grad.clone() for _, p in _head_named_parameters(model)]
    model, loss2, hm2 = _step('c')
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(hm1), bits(hm2)) and torch.equal(bits(loss1.reshape(1)), bits(loss2.reshape(1)))
    for (name, p), a in zip(_head_named_parameters(model), g1):
        assert torch.equal(bits(p.grad), bits(a)), name


@pytest.mark.parametrize('case', ['b', 'd'])
def test_running_statistics_after_a_step(case):
    ref64, ref32 = TR.run(case, torch.float64), TR.run(case, torch.float32)
    model, _, _ = _step(case)
    state = model.state_dict()
    seen = 0
    for key in ref64:
        if not key.startswith('stat/'):
            continue
        name, got = key[5:], state[key[5:]].cpu().double().numpy()
        if name.endswith('num_batches_tracked'):
            assert int(got) == int(ref64[key]) + 1, name            # the functional reference does not count; a module does
            continue
        e_ref, err = R.rel(ref32[key], ref64[key]), R.rel(got, ref64[key])
        print('case {} {}: err {:.2e}, e_ref {:.2e}'.format(case, name, err, e_ref))
        assert err <= R.bound(e_ref), name
        seen += 1
    assert seen == 14


def test_inference_path_of_a_trainable_model():
    channels, V, B, (h, w), kind = R.CASES['b']
    plain, model = _model(channels, V, trainable=False).eval(), _model(channels, V)
    state = R.fill_state_dict(channels, V, kind=kind)
    _load_head(plain, state)
    _load_head(model, state)
    feat, ext, K, _ = _case_inputs('b')
    with torch.no_grad():
        want = plain.head_forward(feat, ext, K)
    model.hip()                                   # the flat buffers exist: the parameters are views of them
    before = {k: v.clone() for k, v in model.state_dict().items()}
    model.train()
    with torch.no_grad():
        got_train = model.head_forward(feat, ext, K)
    model.eval()
    got_eval = model.head_forward(feat, ext, K)
    with torch.no_grad():
        got_eval_ng = model.head_forward(feat, ext, K)
    torch.cuda.synchronize()
    for got in (got_train, got_eval, got_eval_ng):
        for a, b in zip(got, want):
            assert not a.requires_grad and torch.equal(a, b)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k        # no running statistic moved
    # and the refusals of a model built without trainable=True are as they were
    plain.train()
    with pytest.raises(NotImplementedError, match='training of FTL is not built'):
        plain.head_forward(feat, ext, K)
    plain.eval()
    with pytest.raises(NotImplementedError, match='build the model with trainable=True'):
        plain.hip()


def test_phase_two_loss_is_the_sum_of_its_terms():
    """the 3-D-phase loss, 0.1 pose2d + pose3d, on a unit case: finite gradients that equal the sum of the gradients of
    its two terms taken in separate backward passes, to a relative 1e-5 of their largest entry"""
    from core.loss import Joints3DMSELoss, JointsMSELoss
    case = 'a'
    channels, V, B, (h, w), kind = R.CASES[case]
    model = _model(channels, V)
    feat, ext, K, gt = _case_inputs(case)
    rng = np.random.RandomState(9)
    gt3d = torch.tensor(rng.standard_normal((B, R.K_JOINTS, 3)), dtype=torch.float32, device='cuda')
    c2d, c3d = JointsMSELoss(), Joints3DMSELoss()

    def grads(w2d, w3d):
        _load_head(model, R.fill_state_dict(channels, V, kind=kind))
        model.train()
        hm, pose2d, pose3d = model.head_forward(feat, ext, K)
        assert tuple(pose3d.shape) == (B, R.K_JOINTS, 3)
        loss = 0
        if w2d:
            loss = loss + w2d * c2d(pose2d.reshape(B * V, -1, 2), gt.reshape(B * V, -1, 2))
        if w3d:
            loss = loss + w3d * c3d(pose3d, gt3d)
        loss.backward()
        torch.cuda.synchronize()
        return [p.grad.clone().double() for _, p in _head_named_parameters(model)]

    both, two, three = grads(0.1, 1.0), grads(0.1, 0), grads(0, 1.0)
    largest = max(float(g.abs().max()) for g in both)
    for (name, _), g, a, b in zip(_head_named_parameters(model), both, two, three):
        assert torch.isfinite(g).all(), name
        # a bias whose true gradient is zero holds the float residue of sums that cancel: it has no scale of its own and
        # is held to the largest entry of all the gradients
        scale = largest if name in TR.ZERO_GRAD_BIASES else max(float(g.abs().max()), float((a + b).abs().max()))
        diff = float((g - (a + b)).abs().max())
        print('phase 2 {}: |both - (2-D + 3-D)| {:.2e} on a scale of {:.2e}'.format(name, diff, scale))
        assert scale > 0 and diff <= 1e-5 * scale, name
    assert any(float(t.abs().max()) > 0 for t in three)


def test_a_short_training_run_and_its_checkpoint(tmp_path):
    sys.path.insert(0, os.path.join(mhp_tree.PKG, 'tools'))
    import train_ftl
    from hipnet.optim import FlatAdam
    from models.FTL_encoder_decoder import FTLMultiviewNet
    case = 'b'
    channels, V, B, (h, w), kind = R.CASES[case]
    model = _model(channels, V)
    _load_head(model, R.fill_state_dict(channels, V, kind=kind))
    model.train()
    feat, ext, K, gt = _case_inputs(case)
    opt = FlatAdam(model, lr=1e-3)
    losses = []
    for _ in range(6):
        hm, pose2d, _ = model.head_forward(feat, ext, K)
        loss = ((pose2d - gt) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print('2-D loss over six steps:', ' '.join('{:.4f}'.format(v) for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    path = train_ftl.save_final_state(model, str(tmp_path))
    assert os.path.basename(path) == 'final_state.pth.tar'
    plain = FTLMultiviewNet(_cfg(channels, V)).cuda().eval()
    saved = torch.load(path, map_location='cpu')
    saved = saved['state_dict'] if 'state_dict' in saved else saved
    plain.load_state_dict({k.replace('module.', ''): v for k, v in saved.items()}, strict=True)
    with torch.no_grad():
        hm, pose2d, pose3d = plain.head_forward(feat, ext, K)
    torch.cuda.synchronize()
    assert torch.isfinite(hm).all() and tuple(pose2d.shape) == (B, V, R.K_JOINTS, 2) and torch.isfinite(pose3d).all()
