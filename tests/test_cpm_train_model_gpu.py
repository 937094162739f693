"""models.CPM(k, trainable=True) on the GPU: the loss and all 80 gradients against the float64 restatement of
tests/cpm_train_ref.py, which takes its ReLU and arg-max decisions from the device's saved activations (its docstring says
why). err = max|dev - ref64| / max|ref64| per tensor within cpm_ref.bound(e_ref), e_ref the same restatement in float32 on
the CPU; nothing is excluded. Cases: B = 2 at 24 x 40 (3 x 5 maps) and B = 1 at 8 x 16 (1 x 2 maps), last-stage loss and
all six stages."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cpm_ref as R
import cpm_train_ref as TR
import mhp_tree

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'hrnet-hand-pose-estimation_amd')
YAML = os.path.join(PKG, 'experiments', 'MHP', 'MHP_CPM_v1.yaml')


@functools.lru_cache(maxsize=None)
def _state():
    return R.fill_state_dict(R.K_JOINTS, R.SEED)


def _model(trainable=True):
    from models import CPM
    model = CPM.CPM(R.K_JOINTS, trainable=trainable)
    model.load_state_dict(R.to_torch(_state(), torch.float32), strict=True)
    return model.to(DEV)


def _dev(a):
    return torch.tensor(a, dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def _device_run(case, weights):
    """one training forward + backward: (loss, name -> gradient numpy, the six maps, the decisions, flat gradient)"""
    from models import CPM
    img, cm, tgt = TR.inputs(case)
    model = _model().train()
    maps = model(_dev(img), _dev(cm))
    dec = TR.decisions_of(model)
    loss = CPM.cpm_loss(maps, _dev(tgt), weights)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.double().cpu().numpy() for k, p in model.named_parameters()}
    return float(loss.detach()), grads, [m.detach().cpu() for m in maps], dec, model.hip().flat_g.clone()


@pytest.mark.parametrize('weights', (TR.LAST_STAGE, TR.ALL_STAGES), ids=('last', 'all'))
@pytest.mark.parametrize('case', sorted(TR.CASES))
def test_loss_and_all_gradients(case, weights):
    img, cm, tgt = TR.inputs(case)
    loss, grads, _, dec, _ = _device_run(case, weights)
    l64, g64 = TR.loss_and_grads(_state(), img, cm, tgt, weights, torch.float64, dec)
    l32, g32 = TR.loss_and_grads(_state(), img, cm, tgt, weights, torch.float32, dec)
    assert len(grads) == 80 and set(grads) == set(g64)
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


@pytest.mark.parametrize('case', sorted(TR.CASES))
def test_training_forward_has_the_inference_bits_and_backward_repeats(case):
    img, cm, tgt = TR.inputs(case)
    _, _, maps, _, flat_g = _device_run(case, TR.ALL_STAGES)
    infer = _model(trainable=False).eval()
    trainable_eval = _model().eval()
    with torch.no_grad():
        want = infer(_dev(img), _dev(cm))
        same = trainable_eval(_dev(img), _dev(cm))
    for s in range(6):
        assert torch.equal(maps[s], want[s].cpu()) and torch.equal(same[s], want[s]), s
    from models import CPM
    model = _model().train()
    CPM.cpm_loss(model(_dev(img), _dev(cm)), _dev(tgt), TR.ALL_STAGES).backward()
    torch.cuda.synchronize()
    assert torch.equal(model.hip().flat_g, flat_g)
    with pytest.raises(NotImplementedError, match='training of CPM is not built'):
        _model(trainable=False).train()(_dev(img), _dev(cm))


def test_five_adam_steps_lower_the_loss():
    """one fixed batch, FlatAdam at the fixture's lr (the yaml's 1e-4), last-stage loss: the loss after five steps lies below
    the first. tests/golden/make_golden_cpm_train.py asserts that the reference in float64 ends below 0.8 of its first loss
    with this lr; its trajectory is printed beside the device's"""
    from hipnet.optim import FlatAdam
    from models import CPM
    G = np.load(os.path.join(REPO, 'tests', 'golden', 'cpm_train.npz'))
    img, cm, tgt = TR.inputs('p')
    model = _model().train()
    opt = FlatAdam(model, lr=float(G['lr']))
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = CPM.cpm_loss(model(_dev(img), _dev(cm)), _dev(tgt))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print('losses', losses, 'float64 reference', G['p/trajectory'].tolist())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_train_tool_writes_a_checkpoint_that_evaluates(tmp_path):
    mhp_tree.write_tree(tmp_path)
    out = tmp_path / 'out'
    opts = ['DATA_DIR', str(tmp_path), 'OUTPUT_DIR', str(out), 'LOG_DIR', str(tmp_path / 'log'), 'MODEL.IMAGE_SIZE', '[64, 64]',
            'MODEL.HEATMAP_SIZE', '[8, 8]', 'TRAIN.IMAGES_PER_GPU', '2', 'WORKERS', '0', 'PRINT_FREQ', '1']
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, os.environ.get('PYTHONPATH', '')]))
    r = subprocess.run([sys.executable, os.path.join('tools', 'train_cpm.py'), '--cfg', YAML, '--iterations', '2'] + opts,
                       cwd=PKG, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    final = [os.path.join(d, f) for d, _, fs in os.walk(str(out)) for f in fs if f == 'final_state.pth.tar']
    assert len(final) == 1, final
    sd = torch.load(final[0], map_location='cpu')
    from models import CPM
    CPM.CPM(R.K_JOINTS).load_state_dict(sd, strict=True)
    assert (r.stdout + r.stderr).count('loss') >= 2
    r = subprocess.run([sys.executable, os.path.join('tools', 'evaluate_2D.py'), '--cfg', YAML, '--model_path', final[0],
                        '--batch_size', '2', '--num_batches', '2', '--gpu', '0'] + opts, cwd=PKG, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    r = subprocess.run([sys.executable, os.path.join('tools', 'train.py'), '--cfg', YAML], cwd=PKG, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and 'training of CPM is not built' in r.stderr
