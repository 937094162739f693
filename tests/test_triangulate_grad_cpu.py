"""Host side of the 3-D training path: the float64 numpy restatement of the triangulation backward
(tests/triangulate_grad_ref.py) against the reference's own float64 autograd gradients in
tests/golden/triangulation_grad.npz (tests/golden/make_golden_triangulation_grad.py); the three new C ABI entries; what
tools/train3D.py refuses; the recorder of core/function3D.py; the CPU-tensor errors of the new Python surface."""
import os
import sys

import numpy as np
import pytest

import mhp_tree
import triangulate_grad_ref as G

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'triangulation.npz')
GRAD = os.path.join(HERE, 'golden', 'triangulation_grad.npz')
YAML3D = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_HRNet_w32_trainable_softmax_pose3dloss_v1.yaml')
# the reference's SVD autograd and the formula agree to 8e-13 of a case's largest gradient through numpy's SVD and to
# 4e-9 through eigh of A^T A (the near-parallel rig, relative gap (s3^2 - s4^2) / s1^2 down to 3e-8); both are held to
FORMULA_TOL = 1e-8


def _cases(z):
    return sorted(k[:-2] for k in z.files if k.endswith('_X'))


def _inputs(z, g, name):
    conf = z[name + '_conf'] if name + '_conf' in z.files else None
    return z[name + '_proj'], z[name + '_pts'], conf, g[name + '_gX']


def test_fixture_covers_every_case_of_the_forward_fixture():
    z, g = np.load(GOLD), np.load(GRAD)
    names = _cases(z)
    assert len(names) == 14
    for name in names:
        B, V, K = z[name + '_pts'].shape[:3]
        assert g[name + '_gX'].shape == (B, K, 3) and g[name + '_dpts'].shape == (B, V, K, 2)
        assert np.isfinite(g[name + '_dpts']).all() and np.abs(g[name + '_dpts']).max() > 1.0
        # dconf on the noisy cases with confidences only: on noiseless points it is rounding noise
        assert (name + '_dconf' in g.files) == (name + '_conf' in z.files and '_noisy_' in name)
    assert sorted(k[:-6] for k in g.files if k.endswith('_dconf')) == ['near_noisy_v4_conf', 'wide_noisy_v4_conf']
    assert min(np.abs(g[k]).max() for k in g.files if k.endswith('_dconf')) > 1.0


@pytest.mark.parametrize('route', ['svd', 'eigh'])
def test_formula_reproduces_the_reference_autograd(route):
    z, g = np.load(GOLD), np.load(GRAD)
    fn = G.grad_point if route == 'svd' else G.grad_point_eigh
    for name in _cases(z):
        dpts, dconf = G.grad_batch(*_inputs(z, g, name), point_fn=fn)
        ref = g[name + '_dpts']
        err = np.abs(dpts - ref).max() / np.abs(ref).max()
        print(route, name, 'dpts', err)
        assert err <= FORMULA_TOL, (name, err)
        if name + '_dconf' in g.files:
            ref = g[name + '_dconf']
            err = np.abs(dconf - ref).max() / np.abs(ref).max()
            print(route, name, 'dconf', err)
            assert err <= FORMULA_TOL, (name, err)


def test_near_parallel_rig_has_the_small_gap():
    z = np.load(GOLD)
    name = 'near_clean_v2'
    gaps = [G.relative_gap(z[name + '_proj'][b], z[name + '_pts'][b, :, k]) for b in range(4) for k in range(21)]
    assert 0.0 < min(gaps) < 1e-6


def test_zero_weight_view_has_exactly_zero_gradients():
    z, g = np.load(GOLD), np.load(GRAD)
    name = 'wide_noisy_v4_conf'
    proj, pts, conf, gX = _inputs(z, g, name)
    assert (conf[:, 1, ::3] == 0).all()
    dpts, dconf = G.grad_batch(proj, pts, conf, gX)
    assert (dpts[:, 1, ::3] == 0).all() and (dconf[:, 1, ::3] == 0).all()
    assert (dpts[:, 0] != 0).all()


def test_c_abi_entry_points():
    from hipnet import _capi
    header = open(os.path.join(os.path.dirname(_capi.LIB_PATH), '..', '..', 'include', 'hrnet_hip.h')).read()
    assert 'int hrnet_triangulate_bwd(const float* pts, const double* to_frame, const double* proj, ' \
           'const float* conf,\n                          const float* gX, float* dpts, float* dconf, int B, int V, ' \
           'int K, hr_stream_t stream);' in header
    assert 'int hrnet_joints3d_loss_fwd(const float* pred, const float* gt, float* loss, int B, int K, ' \
           'hr_stream_t stream);' in header
    assert 'int hrnet_joints3d_loss_bwd(const float* pred, const float* gt, const float* gout, float* dpred, int B, ' \
           'int K,' in header
    sigs = {'hrnet_triangulate_bwd': (7, 3), 'hrnet_joints3d_loss_fwd': (3, 2), 'hrnet_joints3d_loss_bwd': (4, 2)}
    import ctypes
    for name, (n_ptr, n_int) in sigs.items():
        assert name in _capi.EXPORTED
        assert _capi._SIGS[name] == [ctypes.c_void_p] * n_ptr + [ctypes.c_int] * n_int + [ctypes.c_void_p], name
        assert hasattr(_capi.lib(), name)                 # loads without a GPU; nothing is launched
    assert _capi.ABI_VERSION == 2                         # entries were added, nothing existing changed


def _train3d():
    tools = os.path.join(mhp_tree.PKG, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import train3D
    return train3D


def test_train3d_refuses_what_it_cannot_train(tmp_path):
    train3D = _train3d()
    mhp_tree.write_tree(tmp_path, {'data_1': 1})
    good = mhp_tree.config(tmp_path, [], YAML3D)
    train3D.check_config(good)                             # the shipped yaml on an existing tree passes
    assert list(good.DATASET.DATASET) == ['MHP_mv'] and list(good.DATASET.TEST_DATASET) == ['MHP_mv']
    assert good.LOSS.WITH_POSE3D_LOSS and not good.LOSS.WITH_HEATMAP_LOSS and not good.LOSS.WITH_POSE2D_LOSS
    for opts, match in ((['MODEL.NAME', 'pose_hrnet'], "MODEL.NAME 'pose_hrnet'"),
                        (['MODEL.NAME', 'vol'], "MODEL.NAME 'vol'"),
                        (['MODEL.HEATMAP_SOFTMAX', 'False'], 'arg-max decode has no gradient'),
                        (['MODEL.ALG_CONFIDENCES', 'True'], 'confidence head'),
                        (['DATASET.DATASET', "['MHP_kpt']"], 'DATASET.DATASET'),
                        (['DATASET.TEST_DATASET', "['MHP']"], 'DATASET.TEST_DATASET'),
                        (['DATASET.DATASET', "['RHD_kpt']"], 'MHP_mv'),
                        (['LOSS.WITH_POSE3D_LOSS', 'False'], 'WITH_POSE3D_LOSS'),
                        (['LOSS.WITH_BONE_LOSS', 'True'], 'WITH_BONE_LOSS')):
        with pytest.raises(ValueError, match=match):
            train3D.check_config(mhp_tree.config(tmp_path, opts, YAML3D))
    with pytest.raises(ValueError, match='annotated_frames'):
        train3D.check_config(mhp_tree.config(tmp_path / 'nowhere', [], YAML3D))
    # the command line: the refusal comes before any device work (this machine may have no device at all)
    with pytest.raises(ValueError, match='annotated_frames'):
        train3D.main(['--cfg', YAML3D, 'DATA_DIR', str(tmp_path / 'nowhere')])
    with pytest.raises(ValueError, match='--views'):
        train3D.main(['--cfg', YAML3D, '--views', '[1]', 'DATA_DIR', str(tmp_path)])
    args = train3D.parse_args(['--cfg', YAML3D, '--views', '[1,3]', '--model_path', 'a.pth', '--batches-per-epoch',
                               '3', 'WORKERS', '0'])
    assert args.views == '[1,3]' and args.model_path == 'a.pth' and args.batches_per_epoch == 3
    assert args.opts == ['WORKERS', '0']


def test_function3d_recorder_keys_and_averages(tmp_path):
    import torch
    from core.function3D import AverageMeter3D
    cfg = mhp_tree.config(tmp_path, ['LOSS.POSE3D_LOSS_FACTOR', '2.0', 'LOSS.WITH_POSE2D_LOSS', 'True',
                                     'LOSS.POSE2D_LOSS_FACTOR', '0.5'], YAML3D)
    seen = []

    def pose3d(pred, gt):
        return (gt - pred).norm(dim=2).sum() / pred.shape[1]

    def pose2d(pred, gt, visibility=None):
        seen.append(visibility)
        return ((pred - gt).norm(dim=2) * visibility).sum()

    with pytest.raises(ValueError, match='pose3d_loss'):
        AverageMeter3D(cfg, {'pose2d_loss': pose2d})
    rec = AverageMeter3D(cfg, {'pose3d_loss': pose3d, 'pose2d_loss': pose2d})
    gt3 = torch.zeros(2, 21, 3)
    p3a = torch.zeros(2, 21, 3)
    p3a[..., 0] = 3.0                                      # every joint 3 away: loss 2 * 21 * 3 / 21 = 6, EPE 3
    p3b = torch.zeros(2, 21, 3, requires_grad=True)        # loss 0, EPE 0
    gt2, p2 = torch.zeros(8, 21, 2), torch.ones(8, 21, 2)
    vis = torch.zeros(8, 21)
    vis[0, :4] = 1.0                                       # 4 visible joints sqrt(2) away
    a = rec.computeLosses(p3a, gt3, pose2d_pred=p2, pose2d_gt=gt2, visibility=vis)
    assert set(a) == {'pose3d_loss', 'heatmap_loss', 'pose2d_loss', 'total_loss', 'epe3d'}
    assert a['heatmap_loss'] is None and seen[0] is vis
    assert a['pose3d_loss'].item() == pytest.approx(6.0) and a['epe3d'].item() == pytest.approx(3.0)
    assert a['pose2d_loss'].item() == pytest.approx(4 * 2 ** 0.5)
    assert a['total_loss'].item() == pytest.approx(2.0 * 6.0 + 0.5 * 4 * 2 ** 0.5)
    b = rec.computeLosses(p3b, gt3, pose2d_pred=gt2, pose2d_gt=gt2, visibility=vis)
    assert b['total_loss'].requires_grad and b['total_loss'].item() == 0.0
    avg = rec.computeAvgLosses()
    assert set(avg) == {'total_loss', 'pose3d_loss', 'pose2d_loss', 'epe3d'} and rec.n == 2
    assert avg['pose3d_loss'] == pytest.approx(3.0) and avg['epe3d'] == pytest.approx(1.5)
    assert avg['pose2d_loss'] == pytest.approx(2 * 2 ** 0.5)
    assert avg['total_loss'] == pytest.approx(6.0 + 2 ** 0.5)
    assert rec.avg_total_loss == avg['total_loss'] and rec.avg_pose3d_loss == avg['pose3d_loss']
    assert rec.avg_epe3d == avg['epe3d'] and rec.pose3d_loss == pytest.approx(6.0)
    # the sums are detached: reading them keeps no graph alive
    assert not torch.as_tensor(rec._sums['total_loss']).requires_grad


def test_new_python_surface_has_no_cpu_path():
    import torch
    from core.loss import Joints3DMSELoss
    from utils.multiview import triangulate_batch_of_points
    with pytest.raises(RuntimeError, match='HIP-device'):
        Joints3DMSELoss()(torch.zeros(2, 21, 3, requires_grad=True), torch.zeros(2, 21, 3))
    proj = torch.zeros(2, 4, 3, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='HIP-device'):
        triangulate_batch_of_points(proj, torch.zeros(2, 4, 21, 2, requires_grad=True))
    with pytest.raises(RuntimeError, match='HIP-device'):
        triangulate_batch_of_points(proj, torch.zeros(2, 4, 21, 2), torch.ones(2, 4, 21, requires_grad=True))
