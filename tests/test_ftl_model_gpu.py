"""models.FTL_encoder_decoder on the device: head_forward against the fixture recorded from the reference's own forward
(tests/golden/ftl.npz) and against the float64 restatement at full width, forward end to end on synthetic images (shapes,
slot order, the DLT), a strict load of a checkpoint, and tools/evaluate_ftl.py on the synthetic MHP tree.

Measured on an MI355X: the heat maps of the six fixture cases at 0.08 to 0.23 of bound(e32), every recorded stage at most
0.41 of its bound, the full-width heat maps at 2.7e-6 against a bound of 1.45e-5 ("FTL inference")."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ftl_ref as R
import mhp_tree

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_HRNet_w32_softmax_pose2dloss_FTL_v1.yaml')
FULL = (32, 64, 128, 256)
_MODELS = {}


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(REPO, 'tests', 'golden', 'ftl.npz'))


def _model(channels, V):
    """one model per (width, views), on the device in eval mode; the tests load the head's state they need"""
    from models.FTL_encoder_decoder import FTLMultiviewNet
    if (channels, V) not in _MODELS:
        cfg = mhp_tree.config('', ['MODEL.EXTRA.STAGE4.NUM_CHANNELS', str(list(channels)), 'DATASET.NUM_VIEWS', str(V)], YAML)
        torch.manual_seed(0)
        _MODELS[(channels, V)] = FTLMultiviewNet(cfg).cuda().eval()
    return _MODELS[(channels, V)]


def _load_head(model, state):
    full = dict(model.state_dict())
    full.update({k: v.to('cuda') for k, v in R.to_torch(state, torch.float32).items()})
    model.load_state_dict(full, strict=True)


def _nchw(y):
    return y.permute(0, 3, 1, 2).cpu().double().numpy()


@pytest.mark.parametrize('case', sorted(R.CASES))
def test_head_against_the_fixture(golden, case):
    channels, V, B, (h, w), kind = R.CASES[case]
    model = _model(channels, V)
    _load_head(model, R.fill_state_dict(channels, V, kind=kind))
    feat = torch.tensor(golden[case + '/feat'].astype(np.float32), device='cuda')
    ext = torch.tensor(golden[case + '/ext'], dtype=torch.float32, device='cuda')
    K = torch.tensor(golden[case + '/K'], dtype=torch.float32)
    e32 = dict(zip(R.STAGES, golden[case + '/e32']))
    with torch.no_grad():
        st = model.head_stages(feat, ext, K)
        hm, pose2d, pose3d = model.head_forward(feat, ext, K.expand(B, 3, 3))
    torch.cuda.synchronize()
    assert torch.equal(hm, st['heatmaps'])
    for s in R.STAGES[:3]:
        err = R.rel(R.kept(s, _nchw(st[s])), golden[case + '/' + s])
        print('case {} {}: err {:.2e}, e32 {:.2e}, bound {:.2e}'.format(case, s, err, e32[s], R.bound(e32[s])))
        assert err <= R.bound(e32[s]), s
    err = R.rel(hm.cpu().numpy(), golden[case + '/heatmaps'])
    print('case {} heatmaps: err {:.2e}, e32 {:.2e}, bound {:.2e}'.format(case, err, e32['heatmaps'], R.bound(e32['heatmaps'])))
    assert tuple(hm.shape) == (B * V, R.K_JOINTS, h, w)
    assert err <= R.bound(e32['heatmaps'])
    pix32 = np.abs(golden[case + '/pose2d32'] - golden[case + '/pose2d']).max()
    pix = np.abs(pose2d.cpu().double().numpy() - golden[case + '/pose2d']).max()
    print('case {} pose2d: off by {:.2e} px, the float32 run by {:.2e} px'.format(case, pix, pix32))
    assert tuple(pose2d.shape) == (B, V, R.K_JOINTS, 2) and tuple(pose3d.shape) == (B, R.K_JOINTS, 3)
    assert pix <= 4 * pix32 + 1e-4


def test_head_at_full_width():
    """C = 480, 64 x 64 features, B x V = 1 x 4, unit-scale cameras: 33 and 18 on the way and the real channel tiling"""
    V = 4
    model = _model(FULL, V)
    state = R.fill_state_dict(FULL, V, seed=R.SEED + 1)
    _load_head(model, state)
    rng = np.random.RandomState(5)
    feat = np.abs(rng.standard_normal((V, 480, 64, 64))).astype(np.float16).astype(np.float64)
    ext, K = R.cameras('unit', 1, V, rng)
    with torch.no_grad():
        y64 = R.forward(R.to_torch(state, torch.float64), torch.tensor(feat), torch.tensor(ext), torch.tensor(K))
        y32 = R.forward(R.to_torch(state, torch.float32), torch.tensor(feat, dtype=torch.float32),
                        torch.tensor(ext, dtype=torch.float32), torch.tensor(K, dtype=torch.float32))
        st = model.head_stages(torch.tensor(feat, dtype=torch.float32, device='cuda'),
                               torch.tensor(ext, dtype=torch.float32, device='cuda'), torch.tensor(K, dtype=torch.float32))
    torch.cuda.synchronize()
    assert tuple(st['encoder_head'].shape) == (4, 18, 18, 240) and tuple(st['heatmaps'].shape) == (4, 21, 64, 64)
    for s in ('encoder_head', 'fuse_after_FTL', 'channel_expansion', 'heatmaps'):
        e_ref = R.rel(y32[s].double().numpy(), y64[s].numpy())
        got = st[s].cpu().numpy() if s == 'heatmaps' else _nchw(st[s])
        err = R.rel(got, y64[s].numpy())
        print('full width {}: err {:.2e}, e_ref {:.2e}, bound {:.2e}'.format(s, err, e_ref, R.bound(e_ref)))
        assert 5e-8 < e_ref < 1e-4 and err <= R.bound(e_ref), s


def test_forward_end_to_end_slot_order_and_dlt():
    from utils.multiview import triangulate_batch_of_points
    B, V = 2, 4
    model = _model(FULL, V)
    _load_head(model, R.fill_state_dict(FULL, V, seed=R.SEED + 2))
    g = torch.Generator().manual_seed(3)
    images = torch.randn(B, V, 3, 256, 256, generator=g).cuda()
    rng = np.random.RandomState(9)
    ext, K = R.cameras('unit', B, V, rng)
    ext, K = torch.tensor(ext, dtype=torch.float32, device='cuda'), torch.tensor(K, dtype=torch.float32, device='cuda')
    with torch.no_grad():
        hm, pose2d, pose3d = model(images, ext, K)
        assert tuple(hm.shape) == (B * V, 21, 64, 64) and tuple(pose2d.shape) == (B, V, 21, 2)
        assert tuple(pose3d.shape) == (B, 21, 3) and bool(torch.isfinite(pose3d).all())
        assert float((hm.sum((2, 3)) - 1).abs().max()) < 1e-4
        # forward is the backbone's features (slot 1 of its output), view-images in slot order, through head_forward
        feats = model.backbone(images.reshape(B * V, 3, 256, 256))[1]
        assert tuple(feats.shape) == (B * V, 480, 64, 64)
        hm0, pose2d0, pose3d0 = model.head_forward(feats, ext, K)
        assert R.rel(hm0.cpu().numpy(), hm.cpu().numpy()) < 1e-6
        # the frames swapped: every output row moves with its frame, bit for bit (slot b V + v, not v B + b)
        hm2, p2, p3 = model.head_forward(feats.view(B, V, 480, 64, 64).flip(0).reshape(B * V, 480, 64, 64), ext.flip(0), K)
        assert torch.equal(hm2.view(B, V, 21, 64, 64).flip(0), hm0.view(B, V, 21, 64, 64))
        assert torch.equal(p2.flip(0), pose2d0) and torch.equal(p3.flip(0), pose3d0)
        # one frame alone gives the rows of that frame
        hm1 = model.head_forward(feats[V:], ext[1:], K.expand(1, 3, 3))[0]
        assert torch.equal(hm1, hm0[V:])
        # pose3d is the DLT of the returned pose2d: heat-map pixels to the 640 x 480 frame, P = K [R | t]
        to_frame = torch.tensor([[10., 0., 0.], [0., 7.5, 0.]], dtype=torch.float64, device='cuda').expand(B * V, 2, 3)
        want = triangulate_batch_of_points(K.double() @ ext.double(), pose2d, to_frame=to_frame.contiguous())
        assert torch.equal(want, pose3d)
        inv = torch.tensor([[4., 0., 1.], [0., 4., 2.]], dtype=torch.float64, device='cuda').expand(B * V, 2, 3).contiguous()
        hm3, p2b, p3b = model(images, ext, K, to_frame=inv)
        assert torch.equal(p2b, pose2d) and torch.equal(p3b, triangulate_batch_of_points(K.double() @ ext.double(), pose2d,
                                                                                         to_frame=inv))
        # the views permuted, with a fuse_after_FTL.0 that treats every view alike: the fused map is the same (up to the
        # order of its sum), so every view's output moves with the view
        w = model.fuse_after_FTL.layer_lst[0][0].weight
        w.copy_(w[:, :240].repeat(1, V, 1, 1) / V)
        perm = [2, 0, 3, 1]
        f5 = feats.view(B, V, 480, 64, 64)
        a = model.head_forward(feats, ext, K)[0].view(B, V, 21, 64, 64)
        b = model.head_forward(f5[:, perm].reshape(B * V, 480, 64, 64), ext[:, perm], K)[0].view(B, V, 21, 64, 64)
        assert R.rel(b.cpu().numpy(), a[:, perm].cpu().numpy()) < 1e-3
        assert R.rel(b.cpu().numpy(), a.cpu().numpy()) > 1e-2          # and the views do differ
        with pytest.raises(ValueError, match='DATASET.NUM_VIEWS'):
            model(images[:, :3], ext[:, :3], K)
        with pytest.raises(ValueError, match='DATASET.NUM_VIEWS = 4'):
            model.head_forward(torch.zeros(3, 480, 64, 64, device='cuda'), ext[:1, :3], K)
        with pytest.raises(ValueError, match='triplets'):
            model.head_forward(torch.zeros(4, 480, 8, 8, device='cuda'), ext[:1], K)      # 8 -> 5 -> 4: 16 pixels
        with pytest.raises(ValueError, match='differ'):
            model(images, ext, torch.stack([K, 2 * K]))
    del _MODELS[(FULL, V)]                                  # its fuse weight was overwritten


def test_strict_load_of_a_checkpoint(golden, tmp_path):
    from core.evaluate2d import load_checkpoint_state
    channels, V = R.NARROW, 3
    model = _model(channels, V)
    state = {k: v.cpu() for k, v in model.state_dict().items()}
    head = R.to_torch(R.fill_state_dict(channels, V, seed=4), torch.float32)
    assert list(head) and sorted(head) == sorted(golden['40_3/keys'])
    state.update(head)
    path = str(tmp_path / 'ftl.pth.tar')
    torch.save({'state_dict': {'module.' + k: v for k, v in state.items()}}, path)
    load_checkpoint_state(model, path)
    got = model.state_dict()
    assert all(torch.equal(got[k].cpu(), v) for k, v in head.items())
    with pytest.raises(RuntimeError, match='final_layer.bias'):
        model.load_state_dict({k: v for k, v in state.items() if k != 'final_layer.bias'}, strict=True)
    # the plan follows the parameters: the same input, new weights, other maps
    case = 'b'
    feat = torch.tensor(golden[case + '/feat'].astype(np.float32), device='cuda')
    ext = torch.tensor(golden[case + '/ext'], dtype=torch.float32, device='cuda')
    K = torch.tensor(golden[case + '/K'], dtype=torch.float32)
    with torch.no_grad():
        a = model.head_forward(feat, ext, K)[0]
        _load_head(model, R.fill_state_dict(channels, V))
        b = model.head_forward(feat, ext, K)[0]
    assert not torch.equal(a, b)
    assert R.rel(b.cpu().numpy(), golden[case + '/heatmaps']) <= R.bound(float(golden[case + '/e32'][4]))


def test_evaluate_ftl_tool(tmp_path):
    from models.FTL_encoder_decoder import FTLMultiviewNet
    data, out = tmp_path / 'data', str(tmp_path / 'out')
    mhp_tree.write_tree(data, {'data_1': 2, 'data_17': 2})
    torch.manual_seed(1)
    model = FTLMultiviewNet(mhp_tree.config('', [], YAML))
    ckpt = str(tmp_path / 'ftl_model.pth.tar')
    torch.save({'state_dict': {'module.' + k: v for k, v in model.state_dict().items()}}, ckpt)
    r = subprocess.run([sys.executable, os.path.join('tools', 'evaluate_ftl.py'), '--cfg', YAML, '--model_path', ckpt, '--views',
                        '[1,2,3,4]', '--batch_size', '2', '--num_batches', '1', '--gpu', '0', 'DATA_DIR', str(data),
                        'OUTPUT_DIR', out, 'LOG_DIR', str(tmp_path / 'log'), 'WORKERS', '0'], cwd=mhp_tree.PKG,
                       capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert '3D pose EPE:' in log and '2D pose EPE:' in log and 'fps:' in log, log[-2000:]
    res = os.path.join(out, 'eval3D_results_MHP_HRNet_w32_softmax_pose2dloss_FTL_v1')
    pck3d, pck2d = np.loadtxt(os.path.join(res, 'PCK3d.txt')), np.loadtxt(os.path.join(res, 'PCK2d.txt'))
    assert pck3d.shape == (2, 50) and np.array_equal(pck3d[0], np.arange(1, 51)) and np.isfinite(pck3d).all()
    assert pck2d.shape == (2, 49) and np.array_equal(pck2d[0], np.arange(1, 50)) and np.isfinite(pck2d).all()
    for name in ('mse2d_each_joint.txt', 'mse3d_each_joint.txt'):
        v = np.loadtxt(os.path.join(res, name))
        # the synthetic tree's wrist lies outside every frame: it is never visible and its 2-D error is a mean of nothing
        assert v.shape == (21,) and np.isfinite(v[1:]).all() and (name[3] == '2' or np.isfinite(v[0])), (name, v)
