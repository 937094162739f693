"""Training of pose_hrnet_hamburger on the GPU: the trainable head (HamNet(trainable=True).head_forward in training mode) at
cases A, B and C of tests/hamburger_ref with the fixture's bases and keep mask against tests/hamburger_train_ref
differentiated in float64 on the CPU, the running statistics, equal bits on two runs, eval on the trained state, one
whole-model SGD step with the backbone, and tools/train_hamburger.py as a subprocess.

err = max|dev - ref64| / max|ref64| must stay within bound(e_ref) = 4 * e_ref + 2 * 2^-24, e_ref being the same measure of
the restatement run and differentiated in float32 on the CPU, and e_ref itself within 1e-4. fc.1.bias is left out of the
rule: its gradient is zero by the softmax's shift invariance (1e-16 in float64); it must stay below 16 times the float32
restatement's own magnitude of it, or below 2^-20 of max|d fc.1.weight|, whichever is larger."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hamburger_ref as R
import hamburger_train_ref as T

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hrnet-hand-pose-estimation_amd')
YAML = os.path.join(PKG, 'experiments', 'RHD', 'RHD_HRNet_w32_Hamburger_v2.yaml')
SMALL = ['MODEL.IMAGE_SIZE', '[64, 64]', 'MODEL.HEATMAP_SIZE', '[16, 16]', 'MODEL.EMB_DIM', '[32]', 'MODEL.R', '16']
_CACHE = {}


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'hamburger_train.npz'))


def _cfg(opts):
    from config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(list(opts))
    return cfg


def _case_opts(case):
    h, w = case['size']
    return ['MODEL.IMAGE_SIZE', '[{}, {}]'.format(4 * w, 4 * h), 'MODEL.HEATMAP_SIZE', '[{}, {}]'.format(w, h),
            'MODEL.EMB_DIM', '[{}]'.format(case['emb']), 'MODEL.R', str(case['R']), 'MODEL.S', str(case['S']),
            'MODEL.DUAL_HAM', str(case['dual']), 'MODEL.SPATIAL', str(case['spatial']),
            'MODEL.CHEESE_FACTOR', str(case['cheese']), 'MODEL.EVAL_STEPS', str(case['steps']), 'MODEL.TRAIN_STEPS',
            str(T.TRAIN_STEPS)]


def _head(case, trainable=True):
    """the head alone with the case's seeded state: the features are given"""
    from models import pose_hrnet_hamburger
    model = pose_hrnet_hamburger.get_pose_net(_cfg(_case_opts(case)), is_train=False, trainable=trainable)
    del model.backbone
    model.load_state_dict(R.to_torch(R.fill_state_dict(R.head_keys(case), T.SEED), torch.float32), strict=True)
    return model.cuda()


def _refs(golden, tag):
    """the restatement's step in float64 and float32, once per case"""
    if tag not in _CACHE:
        case = R.CASES[tag]
        bases = [golden['{}/bases{}'.format(tag, i)] for i in range(len(R.ham_list(case)))]
        keep, targets = golden[tag + '/keep'], golden[tag + '/targets']
        _CACHE[tag] = (case, bases, keep, targets, T.run_train(case, torch.float64, bases, keep, targets),
                       T.run_train(case, torch.float32, bases, keep, targets))
    return _CACHE[tag]


def _step(model, case, bases, keep, targets):
    x = torch.tensor(R.inputs(case, T.SEED), dtype=torch.float32).cuda().requires_grad_(True)
    for p in model.parameters():
        p.grad = None
    hm = model.head_forward(x, [torch.from_numpy(b) for b in bases], torch.from_numpy(keep).cuda())
    loss = _loss(hm, targets)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    grads['features'] = x.grad.detach().clone()
    return hm.detach(), loss.detach(), grads


def _loss(hm, targets):
    """hamburger_train_ref.loss on the device: the same ops on float32 tensors"""
    B, J, h, w = hm.shape
    ys, xs = torch.arange(h, dtype=hm.dtype, device=hm.device), torch.arange(w, dtype=hm.dtype, device=hm.device)
    px, py = (hm.sum(dim=2) * xs).sum(dim=2), (hm.sum(dim=3) * ys).sum(dim=2)
    t = torch.tensor(targets, dtype=hm.dtype, device=hm.device)
    return (torch.stack([px, py], dim=2) - t).norm(dim=2).mean()


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_head_training_step_against_the_restatement(golden, tag):
    case, bases, keep, targets, r64, r32 = _refs(golden, tag)
    model = _head(case).train()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    hm, loss, grads = _step(model, case, bases, keep, targets)
    failures = []

    def hold(label, dev, a, b):
        err, e_ref = R.rel(dev.double().cpu().numpy(), a), R.rel(b, a)
        print('{} {}: err {:.3g}, e_ref {:.3g}, bound {:.3g}'.format(tag, label, err, e_ref, R.bound(e_ref)))
        if not (e_ref <= 1e-4 and err <= R.bound(e_ref)):
            failures.append((label, err, e_ref))

    hold('loss', loss.reshape(1), np.array([r64['loss']]), np.array([r32['loss']]))
    hold('heat maps', hm, r64['hm'], r32['hm'])
    assert set(grads) == set(r64['grads'])
    for k in ['features'] + T.param_keys(case):
        if k == 'fc.1.bias':
            continue
        hold('d ' + k, grads[k].reshape(r64['grads'][k].shape), r64['grads'][k], r32['grads'][k])
    got = float(grads['fc.1.bias'].abs().max())
    allowed = max(16 * np.abs(r32['grads']['fc.1.bias']).max(), 2.0 ** -20 * np.abs(r64['grads']['fc.1.weight']).max())
    print('{} d fc.1.bias: max {:.3g}, allowed {:.3g}'.format(tag, got, allowed))
    if got > allowed:
        failures.append(('d fc.1.bias', got, allowed))
    # the running buffers: (1 - m) * old + m * (batch statistic), the statistic itself under the rule
    after = model.state_dict()
    m = T.MOMENTUM
    for prefix in T.BN_PREFIXES:
        for i, leaf in enumerate(('running_mean', 'running_var')):
            a, b = r64['batch'][prefix][i], r32['batch'][prefix][i]
            want = (1 - m) * before[prefix + leaf].double().cpu().numpy() + m * a
            tol = 2.0 ** -23 * np.abs(want).max() + m * R.bound(R.rel(b, a)) * np.abs(a).max()
            diff = np.abs(after[prefix + leaf].double().cpu().numpy() - want).max()
            print('{} {}: diff {:.3g}, tolerance {:.3g}'.format(tag, prefix + leaf, diff, tol))
            if diff > tol:
                failures.append((prefix + leaf, diff, tol))
            assert not torch.equal(after[prefix + leaf], before[prefix + leaf])
        assert int(after[prefix + 'num_batches_tracked']) == 0
    assert not failures, failures


def test_two_runs_are_bit_identical_and_eval_follows_the_trained_state(golden):
    case, bases, keep, targets, _, _ = _refs(golden, 'c')
    runs = []
    for _ in range(2):
        model = _head(case).train()
        hm, loss, grads = _step(model, case, bases, keep, targets)
        runs.append((hm, loss, grads, {k: v.clone() for k, v in model.state_dict().items()}))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    for k in runs[0][3]:
        assert torch.equal(runs[0][3][k], runs[1][3][k]), k
    # eval under no_grad afterwards is the inference path on the statistics training left: a fresh inference model
    # loaded from the trained state dict gives the same bits
    x = torch.tensor(R.inputs(case, T.SEED), dtype=torch.float32).cuda()
    host = [torch.from_numpy(b) for b in bases]
    model.eval()
    with torch.no_grad():
        stale = model.head_forward(x, host)          # packs the plan on the trained statistics
        model.train()
    _step(model, case, bases, keep, targets)         # a second step moves the statistics again
    model.eval()
    fresh = _head(case, trainable=False).eval()
    fresh.load_state_dict(model.state_dict(), strict=True)
    with torch.no_grad():
        got, want = model.head_forward(x, host), fresh.head_forward(x, host)
    assert torch.equal(got, want) and not torch.equal(got, stale)
    with pytest.raises(NotImplementedError, match='eval mode with a gradient required'):
        model.head_forward(x, host)
    with pytest.raises(ValueError, match='drop_keep'):
        with torch.no_grad():
            model.head_forward(x, host, torch.from_numpy(keep).cuda())


def test_whole_model_sgd_step():
    from models import pose_hrnet_hamburger
    torch.manual_seed(0)
    model = pose_hrnet_hamburger.get_pose_net(_cfg(SMALL), is_train=True, trainable=True)
    with torch.no_grad():
        model.hamburger.coef_ham.fill_(0.7)          # ZERO_HAM starts it at 0, which would stop every gradient in the ham
    model = model.cuda().train()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1.0)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    torch.manual_seed(5)
    hm, temp = model(x)
    assert tuple(hm.shape) == (2, 21, 16, 16) and temp is model.trainable_temp and hm.requires_grad
    weight = torch.randn(hm.shape, generator=torch.Generator().manual_seed(2)).cuda()
    (hm * weight).sum().backward()
    opt.step()
    torch.cuda.synchronize()
    after = model.state_dict()
    for k, p in model.named_parameters():
        if k.startswith('backbone.'):
            assert not p.requires_grad and p.grad is None and torch.equal(after[k], before[k]), k
        elif k != 'fc.1.bias':
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and not torch.equal(after[k], before[k]), k
    for prefix in T.BN_PREFIXES:
        assert not torch.equal(after[prefix + 'running_var'], before[prefix + 'running_var'])


def test_train_hamburger_tool_and_its_checkpoint(tmp_path):
    out = str(tmp_path / 'out')
    small = SMALL + ['MODEL.EMB_DIM', '[16]', 'MODEL.R', '8']
    common = ['DATA_DIR', str(tmp_path / 'no_data'), 'OUTPUT_DIR', out, 'LOG_DIR', str(tmp_path / 'log')] + small
    r = subprocess.run([sys.executable, os.path.join('tools', 'train_hamburger.py'), '--cfg', YAML,
                        '--batches-per-epoch', '2', 'TRAIN.END_EPOCH', '1', 'TRAIN.IMAGES_PER_GPU', '2',
                        'TEST.IMAGES_PER_GPU', '2', 'WORKERS', '0'] + common,
                       cwd=PKG, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    finals = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs if f == 'final_state.pth.tar']
    assert len(finals) == 1, log[-2000:]
    from models import pose_hrnet_hamburger
    model = pose_hrnet_hamburger.get_pose_net(_cfg(small), is_train=False)
    state = torch.load(finals[0], map_location='cpu')
    model.load_state_dict(state, strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in state.values())
    assert int(state['squeeze.bn.num_batches_tracked']) == 0 and float(state['squeeze.bn.running_mean'].abs().max()) > 0
