"""models.predrnn on the device: the RNN and the ResNet tail against the fixture recorded from the reference's own modules
(tests/golden/predrnn.npz, cases a and b), the whole model against tests/predrnn_ref.py applied to the device backbone's own
outputs, the frame map's layout, the strict load of a reference-shaped state dict, run-to-run equality and the refusals."""
import os

import numpy as np
import pytest
import torch

import mhp_tree
import predrnn_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(REPO, 'hrnet-hand-pose-estimation_amd', 'experiments', 'Pred_RNN',
                    'PredRNN_8frames_256x256_adam_lr1e-3.yaml')
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(REPO, 'tests', 'golden', 'predrnn.npz'))


def _cfg(nh, ks, size):
    return mhp_tree.config('', ['MODEL.N_HIDDEN', list(nh), 'MODEL.FILTER_SIZE', ks, 'MODEL.HEATMAP_SIZE', [size, size],
                                'MODEL.IMAGE_SIZE', [4 * size, 4 * size]], YAML)


def _model(case, seed, backbone_seed=None):
    """the model of a case with the head's state drawn by predrnn_ref (loaded strict, the backbone's own entries kept or
    drawn by hipnet.synth), on the device in eval mode; and the head's state"""
    from hipnet import synth
    from models import predrnn
    model = predrnn.get_pose_net(_cfg(case['nh'], case['ks'], case['size']), is_train=False)
    state = R.fill_state_dict(case, seed)
    full = {k: v for k, v in model.state_dict().items() if k.startswith('HRNet.')}
    if backbone_seed is not None:
        drawn = synth.fill_state_dict(model.HRNet.state_dict(), backbone_seed)
        full = {'HRNet.' + k: torch.from_numpy(np.asarray(v)) for k, v in drawn.items()}
    full.update(R.to_torch(state, torch.float32))
    model.load_state_dict(full, strict=True)
    return model.to(DEV).eval(), state


@pytest.fixture(scope='module', params=sorted(R.CASES))
def fixture_case(request, golden):
    name = request.param
    model, _ = _model(R.CASES[name], int(golden['seed']))
    return name, model


def test_rnn_and_tail_against_the_fixture(fixture_case, golden):
    name, model = fixture_case
    x = torch.tensor(golden[name + '/frames'].astype(np.float32), device=DEV)
    last = torch.tensor(golden[name + '/last'].astype(np.float32), device=DEV)
    with torch.no_grad():
        y = model.rnn_forward(x)
        pose = model.pose_forward(last)
        again = model.rnn_forward(x)
    torch.cuda.synchronize()
    assert tuple(y.shape) == golden[name + '/rnn64'].shape and tuple(pose.shape) == golden[name + '/pose64'].shape
    assert torch.equal(y, again)
    for what, got, key in (('rnn', y, 'rnn'), ('pose', pose, 'pose')):
        e32 = float(golden[name + '/' + key + '_e32'])
        err = R.rel(got.cpu().double().numpy(), golden[name + '/' + key + '64'])
        print('case {} {}: err {:.2e} e32 {:.2e} bound {:.2e}'.format(name, what, err, e32, R.bound(e32)))
        assert err <= R.bound(e32), what


WHOLE = dict(nh=[8, 8], ks=3, size=16, B=1, L=2)             # 64 x 64 images: the smallest the backbone's tests use


@pytest.fixture(scope='module')
def whole():
    model, state = _model(WHOLE, R.SEED + 1, backbone_seed=5)
    rng = np.random.RandomState(R.SEED + 2)
    frames = torch.tensor(rng.standard_normal((WHOLE['B'], WHOLE['L'], 3, 64, 64)) * 0.5, dtype=torch.float32, device=DEV)
    return model, state, frames


def test_whole_model_against_the_restatement_on_the_device_backbones_outputs(whole):
    model, state, frames = whole
    B, L, s = WHOLE['B'], WHOLE['L'], WHOLE['size']
    with torch.no_grad():
        fm = model.frame_map(frames)
        heat, feat = model.HRNet(frames.transpose(0, 1).reshape(L * B, 3, 64, 64).contiguous())
        pose = model(frames)
        again = model(frames)
    torch.cuda.synchronize()
    # the frame map: time-major, 21 heat maps, then the 32 features, then zeros
    assert tuple(fm.shape) == (L, B, s, s, 56) and tuple(pose.shape) == (B, 21, 3) and torch.equal(pose, again)
    flat = fm.view(L * B, s, s, 56)
    assert torch.equal(flat[..., :21], heat.permute(0, 2, 3, 1)) and torch.equal(flat[..., 21:53], feat.permute(0, 2, 3, 1))
    assert float(flat[..., 53:].abs().max()) == 0.0 and float(flat[..., :53].abs().max()) > 0.0
    # the head alone: the restatement on the device backbone's own outputs, so the backbone's error is not counted
    x = torch.cat((heat, feat), 1).view(L, B, 53, s, s).transpose(0, 1).cpu()
    outs = {}
    for dtype in (torch.float64, torch.float32):
        P = R.to_torch(state, dtype)
        with torch.no_grad():
            outs[dtype] = R.pose_forward(P, R.rnn_forward(P, x.to(dtype), WHOLE['nh'])[:, -1]).double().numpy()
    ref64 = outs[torch.float64]
    e_ref, err = R.rel(outs[torch.float32], ref64), R.rel(pose.reshape(B, 63).cpu().double().numpy(), ref64)
    print('whole model: err {:.2e} e_ref {:.2e} bound {:.2e}; {} of 63 outputs positive'.format(
        err, e_ref, R.bound(e_ref), int((ref64 > 0).sum())))
    assert (ref64 > 0).sum() >= 10 and err <= R.bound(e_ref)


def test_refusals_on_the_device(whole):
    model, _, frames = whole
    with pytest.raises(NotImplementedError, match='training of PredRNN is not built'):
        model(frames)                                        # eval mode, gradients enabled, parameters that require one
    with torch.no_grad():
        with pytest.raises(ValueError, match='HIP-device'):
            model(frames.cpu())
        with pytest.raises(ValueError, match='expected'):
            model(frames[0])
        with pytest.raises(ValueError, match='float32 only'):
            model(frames.double())
        with pytest.raises(ValueError, match='expected'):
            model.rnn_forward(torch.zeros((1, 2, 53, 8, 8), device=DEV))
        model.train()
        try:
            with pytest.raises(NotImplementedError, match='training of PredRNN is not built'):
                model(frames)
        finally:
            model.eval()


def test_strict_load_of_a_reference_shaped_state_dict(golden):
    from models import predrnn
    model = predrnn.get_pose_net(mhp_tree.config('', [], YAML), is_train=False)
    state = {str(k): torch.empty([int(d) for d in s[:n]], dtype=torch.int64 if str(k).endswith('num_batches_tracked')
                                 else torch.float32)
             for k, s, n in zip(golden['keys'], golden['shapes'], _ranks(golden))}
    model.load_state_dict(state, strict=True)


def _ranks(golden):
    """the number of axes of every entry: the shapes are padded with zeros to four"""
    return [int((s != 0).sum()) for s in golden['shapes']]
