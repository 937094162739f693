"""models.CPM on the GPU against tests/golden/cpm.npz (the reference's own float64 run; tests/golden/make_golden_cpm.py) and,
at 256 x 256, against the torch-ops model of tools/bench_cpm.py on the same device.

err = max|dev - ref64| / max|ref64| per stage must stay within cpm_ref.bound(e_ref) = 4 * e_ref + 2 * 2^-24, e_ref being the
same measure of the reference's float32 CPU run (the fixture's y32)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cpm_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'hrnet-hand-pose-estimation_amd')
YAML = os.path.join(PKG, 'experiments', 'MHP', 'MHP_CPM_v1.yaml')


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(REPO, 'tests', 'golden', 'cpm.npz'))


@functools.lru_cache(maxsize=None)
def _model(seed):
    """one model per seed for the whole file: 127 MB of weights are drawn and packed once"""
    from models import CPM
    model = CPM.CPM(R.K_JOINTS)
    model.load_state_dict(R.to_torch(R.fill_state_dict(R.K_JOINTS, seed), torch.float32), strict=True)
    return model.cuda().eval()


def _run(model, case):
    z = _golden()
    img = torch.tensor(z[case + '/img'].astype(np.float32)).cuda()
    cm = torch.tensor(z[case + '/center'].astype(np.float32)).cuda()
    with torch.no_grad():
        outs = model(img, cm)
    torch.cuda.synchronize()
    return img, cm, outs


@pytest.mark.parametrize('case', sorted(R.CASES))
def test_six_stages_against_the_fixture(case):
    """cases a (B 2, 8x8 maps), b (5x9 maps under an 11x11 kernel) and c (1x2 maps): all six outputs within bound(e_ref), and
    the argmax key points of the last map equal the fixture's on all 21 joints (the recorder made sure that the gap between
    a joint's two largest values is at least ten bounds).
    MI355X, worst stage of each case: a err 8.7e-07 (e_ref 1.45e-06, bound 5.9e-06); b err 6.3e-07 (e_ref 1.27e-06, bound
    5.2e-06); c err 2.6e-07 (e_ref 2.4e-07, bound 1.07e-06)."""
    z = _golden()
    B, H, W = R.CASES[case]
    _, _, outs = _run(_model(int(z['seed'])), case)
    assert len(outs) == 6
    y64, y32 = z[case + '/y64'], z[case + '/y32']
    for s, o in enumerate(outs):
        assert tuple(o.shape) == (B, R.K_JOINTS + 1, H // 8, W // 8) and o.dtype == torch.float32 and o.is_contiguous()
        dev = o.double().cpu().numpy()
        assert np.isfinite(dev).all()
        err, e_ref = R.rel(dev, y64[s]), R.rel(y32[s], y64[s])
        print('case {} stage {}: err {:.3g} e_ref {:.3g} bound {:.3g}'.format(case, s + 1, err, e_ref, R.bound(e_ref)))
        assert err <= R.bound(e_ref), (case, s, err, R.bound(e_ref))
    assert np.array_equal(R.keypoints(outs[5].cpu().numpy()), z[case + '/kpts'])


def test_batch_slices_and_repeats_give_equal_bits():
    z = _golden()
    model = _model(int(z['seed']))
    img, cm, outs = _run(model, 'a')
    with torch.no_grad():
        again = model(img, cm)
        first = model(img[:1].contiguous(), cm[:1].contiguous())
    torch.cuda.synchronize()
    for o, a, f in zip(outs, again, first):
        assert torch.equal(o, a)
        assert torch.equal(o[:1], f)


def test_packed_weights_follow_load_state_dict():
    """a second forward after load_state_dict of other weights differs, and loading the first ones again restores the
    first result bit for bit: the packed copies were rebuilt both times"""
    from models import CPM
    z = _golden()
    seed = int(z['seed'])
    model = CPM.CPM(R.K_JOINTS).cuda().eval()
    model.load_state_dict(R.to_torch(R.fill_state_dict(R.K_JOINTS, seed), torch.float32), strict=True)
    _, _, first = _run(model, 'c')
    model.load_state_dict(R.to_torch(R.fill_state_dict(R.K_JOINTS, seed + 1), torch.float32), strict=True)
    _, _, second = _run(model, 'c')
    assert not torch.equal(first[5], second[5]) and not torch.equal(first[0], second[0])
    model.load_state_dict(R.to_torch(R.fill_state_dict(R.K_JOINTS, seed), torch.float32), strict=True)
    _, _, third = _run(model, 'c')
    assert all(torch.equal(a, b) for a, b in zip(first, third))


def test_refusals_on_the_device():
    z = _golden()
    model = _model(int(z['seed']))
    img = torch.zeros(1, 3, 16, 16, device='cuda')
    cm = torch.zeros(1, 1, 16, 16, device='cuda')
    with torch.no_grad():
        for bad_img, bad_cm in ((img[:, :, :12], cm[:, :, :12]), (img, cm[:, :, :8]), (img.cpu(), cm), (img, cm.cpu()),
                                (img[:, :2], cm), (img.double(), cm.double())):
            with pytest.raises(ValueError):
                model(bad_img, bad_cm)
    with pytest.raises(NotImplementedError, match='not built'):
        model(img, cm)                                   # parameters require a gradient and no_grad is off
    model.train()
    try:
        with torch.no_grad(), pytest.raises(NotImplementedError, match='training of CPM is not built'):
            model(img, cm)
    finally:
        model.eval()


def test_full_size_forward_against_the_torch_ops_model():
    """one 256 x 256 B = 1 forward: shapes, finiteness, and agreement with the same model built from F.conv2d / F.max_pool2d
    / F.avg_pool2d on the device (tools/bench_cpm.torch_forward) in the bound convention with that model as the reference:
    err = max|hip - torch| / max|torch| per stage within bound(e_ref), e_ref the same measure of the float32 CPU run of
    cpm_ref. MI355X: err 2.3e-06 .. 3.1e-06 per stage, e_ref 2.0e-06 .. 4.5e-06 (bounds 8.0e-06 .. 1.8e-05)."""
    sys.path.insert(0, os.path.join(PKG, 'tools'))
    import bench_cpm
    seed = 11
    state = R.fill_state_dict(R.K_JOINTS, seed)
    rng = np.random.RandomState(seed)
    img = (rng.standard_normal((1, 3, 256, 256)) * 0.5).astype(np.float32)
    yy, xx = np.mgrid[0:256, 0:256]
    cm = np.exp(-((xx - 140.0) ** 2 + (yy - 101.0) ** 2) / 18.0).astype(np.float32)[None, None]
    cm[cm < 0.0099] = 0
    with torch.no_grad():
        cpu32 = R.forward(R.to_torch(state, torch.float32), torch.tensor(img), torch.tensor(cm))
    model = _model(seed)
    P = {k: v.cuda() for k, v in R.to_torch(state, torch.float32).items()}
    xd, cd = torch.tensor(img).cuda(), torch.tensor(cm).cuda()
    with torch.no_grad():
        outs = model(xd, cd)
        ref = bench_cpm.torch_forward(P, xd, cd)
    torch.cuda.synchronize()
    for s in range(6):
        assert tuple(outs[s].shape) == (1, 22, 32, 32) and bool(torch.isfinite(outs[s]).all())
        torch_dev = ref[s].double().cpu().numpy()
        e_ref = R.rel(cpu32[s].double().numpy(), torch_dev)
        err = R.rel(outs[s].double().cpu().numpy(), torch_dev)
        print('256x256 stage {}: err {:.3g} e_ref {:.3g} bound {:.3g}'.format(s + 1, err, e_ref, R.bound(e_ref)))
        assert err <= R.bound(e_ref), (s, err, R.bound(e_ref))


def test_evaluate_2d_runs_and_train_refuses(tmp_path):
    """tools/evaluate_2D.py on the synthetic MHP tree with a seeded checkpoint, two batches of two frames: writes
    mse2d_each_joint.txt and PCK2d.txt; tools/train.py with the same yaml exits with CPM's refusal"""
    import mhp_tree
    from models import CPM
    root = str(tmp_path / 'data')
    mhp_tree.write_tree(root, {'data_1': 3})         # 12 images: the evaluation split is the last 3
    ckpt = str(tmp_path / 'cpm.pth.tar')
    torch.save(R.to_torch(R.fill_state_dict(R.K_JOINTS, 3), torch.float32), ckpt)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, os.environ.get('PYTHONPATH', '')]))
    opts = ['DATA_DIR', root, 'OUTPUT_DIR', str(tmp_path / 'out'), 'LOG_DIR', str(tmp_path / 'log'), 'WORKERS', '0']
    r = subprocess.run([sys.executable, os.path.join(PKG, 'tools', 'evaluate_2D.py'), '--cfg', YAML, '--model_path', ckpt,
                        '--batch_size', '2', '--num_batches', '2', '--gpu', '0'] + opts, env=env, cwd=PKG,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / 'out' / 'eval2D_results_MHP_CPM_v1'
    mse = np.loadtxt(str(out / 'mse2d_each_joint.txt'))
    pck = np.loadtxt(str(out / 'PCK2d.txt'))
    # the tree's wrist (joint 0) lies outside every frame: no visible sample, its mean is NaN as in the reference's tool
    assert mse.size == 21 and np.isfinite(mse[1:]).all() and pck.shape == (2, 49)
    r = subprocess.run([sys.executable, os.path.join(PKG, 'tools', 'train.py'), '--cfg', YAML] + opts, env=env, cwd=PKG,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and CPM.NOT_BUILT in r.stderr, r.stderr[-2000:]
