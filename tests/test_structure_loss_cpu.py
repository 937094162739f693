"""Host side of the hand-structure losses (csrc/loss.hip hrnet_structure_loss, core.loss BoneLengthLoss /
JointAngleLoss / structure_losses): a float64 numpy restatement of the semantics against the reference's own results
in tests/golden/structure_loss.npz (tests/golden/make_golden_structure_loss.py), the C ABI entry, the criterion that
tools/train.py builds from the LOSS.WITH_* flags, the AverageMeter keys, and the argument checks of the modules."""
import importlib.util
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'hrnet-hand-pose-estimation_amd')
GOLD = os.path.join(REPO, 'tests', 'golden', 'structure_loss.npz')
CASES = ('b6', 'b1', 'b70', 'b6_vis', 'zero_bone', 'zero_scale', 'raw')
QUANTITIES = ('bone', 'angle', 'dbone', 'dangle')


def _unit(d, n):
    """d / n with torch.norm's backward convention: 0 where n == 0"""
    with np.errstate(all='ignore'):
        return np.where(n[..., None] == 0, 0.0, d / n[..., None])


def _scale(p):
    """scale_pose2d: relative to the wrist, divided by |r9 - r0| per sample, no epsilon -> (x, s)"""
    r = p - p[:, 0:1]
    s = np.sqrt(((r[:, 9] - r[:, 0]) ** 2).sum(-1))
    with np.errstate(all='ignore'):
        return r / s[:, None, None], s


def _through_scale(g, x, s):
    """d loss / d x -> d loss / d p for x = (p - p0) / |p9 - p0|"""
    with np.errstate(all='ignore'):
        gr = g / s[:, None, None]
        gs = -(g * x).sum((1, 2)) / s
        u = np.where(s[:, None] == 0, 0.0, x[:, 9] - x[:, 0])         # (r9 - r0) / s; 0 at s == 0 (torch.norm backward)
        gr[:, 9] += gs[:, None] * u
        gr[:, 0] -= gs[:, None] * u
        gr[:, 0] -= gr.sum(1)
    return gr


def restatement(pred, gt, normalize):
    """float64 (bone, angle, dbone, dangle): what the kernel computes, vectorised over the batch"""
    p, g = pred.astype(np.float64), gt[:, :, 0:2].astype(np.float64)
    with np.errstate(all='ignore'):
        (x, s), y = (_scale(p), _scale(g)[0]) if normalize else ((p, None), g)
        # bone j = x[j] - x[j-1] for every j = 1..20; sum over batch and bones of (len_gt - len_pred)^2, over 20
        d = x[:, 1:] - x[:, :-1]
        lp = np.sqrt((d ** 2).sum(-1))
        lg = np.sqrt(((y[:, 1:] - y[:, :-1]) ** 2).sum(-1))
        e = lg - lp
        bone = (e ** 2).sum(1).sum() / 20
        gb = (-2 * e / 20)[..., None] * _unit(d, lp)
        g_bone = np.zeros_like(x)
        g_bone[:, 1:] += gb
        g_bone[:, :-1] -= gb
        # finger f = joints 4f..4f+4, bones b1..b4; z components of b4 x b3, b3 x b2, b2 x b1
        f = x[:, :20].reshape(-1, 5, 4, 2)
        b = x[:, 1:21].reshape(-1, 5, 4, 2) - f                 # [:, f, i-1] = x[4f+i] - x[4f+i-1]
        cross = lambda u, v: u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]  # noqa: E731
        c43, c32, c21 = cross(b[:, :, 3], b[:, :, 2]), cross(b[:, :, 2], b[:, :, 1]), cross(b[:, :, 1], b[:, :, 0])
        d1, d2 = c43 * c32, c21 * c32
        n1, n2 = d1 < 0, d2 < 0
        # Rule 1 (coplanarity) on z = 0: exactly 0 for finite poses; the reference still evaluates it, so
        # non-finite poses (zero scale) turn it - and the loss - into NaN
        rule1 = lambda u, v, w: ((u[..., 1] * 0 - 0 * v[..., 1]) * w[..., 0] + (0 * v[..., 0] - u[..., 0] * 0) * w[..., 1]  # noqa: E731
                                 + cross(u, v) * 0)
        coplanar = rule1(b[:, :, 1], b[:, :, 0], b[:, :, 3]) + rule1(b[:, :, 2], b[:, :, 1], b[:, :, 3])
        angle = (coplanar + np.where(n1, d1 ** 2, 0.0) + np.where(n2, d2 ** 2, 0.0)).sum(1).sum()
        g43 = np.where(n1, 2 * d1 * c32, 0.0)
        g21 = np.where(n2, 2 * d2 * c32, 0.0)
        g32 = np.where(n1, 2 * d1 * c43, 0.0) + np.where(n2, 2 * d2 * c21, 0.0)
        du = lambda gc, v: gc[..., None] * np.stack([v[..., 1], -v[..., 0]], -1)    # noqa: E731  d(u x v)/du
        dv = lambda gc, u: gc[..., None] * np.stack([-u[..., 1], u[..., 0]], -1)    # noqa: E731  d(u x v)/dv
        gbone = np.zeros_like(b)
        gbone[:, :, 3] = du(g43, b[:, :, 2])
        gbone[:, :, 2] = dv(g43, b[:, :, 3]) + du(g32, b[:, :, 1])
        gbone[:, :, 1] = dv(g32, b[:, :, 2]) + du(g21, b[:, :, 0])
        gbone[:, :, 0] = dv(g21, b[:, :, 1])
        g_angle = np.zeros_like(x)
        g_angle[:, 1:21] += gbone.reshape(-1, 20, 2)
        g_angle[:, 0:20] -= gbone.reshape(-1, 20, 2)
        if normalize:
            g_bone, g_angle = _through_scale(g_bone, x, s), _through_scale(g_angle, x, s)
    return bone, angle, g_bone, g_angle


def test_fixture_covers_the_cases():
    z = np.load(GOLD)
    for c in CASES:
        for q in QUANTITIES:
            for suffix in ('', '_f32', '_dev', '_nonfinite'):
                assert '{}_{}{}'.format(c, q, suffix) in z.files
    assert z['b6_pred'].shape == (6, 21, 2) and z['b1_pred'].shape[0] == 1 and z['b70_pred'].shape[0] == 70
    assert z['b6_vis_gt'].shape == (6, 21, 3) and z['b6_pred'].dtype == np.float32
    assert not z['raw_normalize'] and z['b6_normalize']
    # every sample of case 1 takes a d < 0 branch: its angle gradient is not zero
    assert (np.abs(z['b6_dangle']).reshape(6, -1).max(1) > 0).all()
    assert np.array_equal(z['zero_bone_pred'][0, 3], z['zero_bone_pred'][0, 2])
    assert np.array_equal(z['zero_scale_pred'][1, 9], z['zero_scale_pred'][1, 0])
    assert z['zero_scale_bone_nonfinite'] and z['zero_scale_angle_nonfinite']
    for q in ('dbone', 'dangle'):
        m = z['zero_scale_{}_nonfinite'.format(q)]
        assert m[1].all() and not np.delete(m, 1, axis=0).any()
        assert np.array_equal(z['b6_vis_' + q], z['b6_' + q])
        assert not z['zero_bone_{}_nonfinite'.format(q)].any()


@pytest.mark.parametrize('case', CASES)
def test_restatement_matches_the_reference(case):
    z = np.load(GOLD)
    ours = restatement(z[case + '_pred'], z[case + '_gt'], bool(z[case + '_normalize']))
    for q, v in zip(QUANTITIES, ours):
        ref, v = z['{}_{}'.format(case, q)], np.asarray(v)
        fin = np.isfinite(ref)
        assert np.array_equal(~np.isfinite(v), ~fin), (case, q)
        assert np.array_equal(~fin, z['{}_{}_nonfinite'.format(case, q)])
        if fin.any():
            scale = np.abs(ref[fin]).max()
            assert np.abs(v[fin] - ref[fin]).max() <= 1e-10 * scale, (case, q)


def test_c_abi_entry_points():
    from hipnet import _capi
    header = open(os.path.join(REPO, 'include', 'hrnet_hip.h')).read()
    for name in ('hrnet_structure_loss', 'hrnet_structure_loss_bwd'):
        assert 'int {}('.format(name) in header
        assert name in _capi.EXPORTED
        assert hasattr(_capi.lib(), name)          # loads without a GPU; nothing is launched
    assert _capi.ABI_VERSION == 2


def _train_tool():
    import sys
    tools = os.path.join(PKG, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    spec = importlib.util.spec_from_file_location('hrnet_train_tool', os.path.join(tools, 'train.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cfg(bone, angle):
    from config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(PKG, 'experiments', 'RHD', 'RHD_HRNet_w32_trainable_softmax_pose2dloss_v1.yaml'))
    cfg.LOSS.WITH_BONE_LOSS, cfg.LOSS.WITH_JOINTANGLE_LOSS = bone, angle
    return cfg


@pytest.mark.parametrize('bone,angle', [(False, False), (True, False), (False, True), (True, True)])
def test_train_tool_builds_the_criterion_the_flags_ask_for(bone, angle):
    from core.function import AverageMeter
    from core.loss import BoneLengthLoss, JointAngleLoss
    cfg = _cfg(bone, angle)
    criterion = _train_tool().build_criterion(cfg)
    assert ('bone_loss' in criterion) == bone and ('jointangle_loss' in criterion) == angle
    assert ('heatmap_loss' in criterion) == bool(cfg.LOSS.WITH_HEATMAP_LOSS)
    assert ('pose2d_loss' in criterion) == bool(cfg.LOSS.WITH_POSE2D_LOSS)
    if bone:
        assert isinstance(criterion['bone_loss'], BoneLengthLoss)
    if angle:
        assert isinstance(criterion['jointangle_loss'], JointAngleLoss)
    meter = AverageMeter(cfg, criterion)
    avg = meter.computeAvgLosses()
    assert ('bone_loss' in avg) == bone and ('jointangle_loss' in avg) == angle
    assert (meter.bone_loss is not None) == bone and (meter.jointangle_loss is not None) == angle
    if bone:
        assert avg['bone_loss'] == meter.avg_bone_loss == 0.0
    if angle:
        assert avg['jointangle_loss'] == meter.avg_jointangle_loss == 0.0


def test_loss_names_drive_the_messages():
    from core import function as F
    labels = {key: label for key, _flag, label, _attr in F._LOSS_NAMES}
    assert labels['bone_loss'] == 'BoneLoss' and labels['jointangle_loss'] == 'JointAngleLoss'
    assert [k for k, *_ in F._LOSS_NAMES][:2] == ['heatmap_loss', 'pose2d_loss']


def test_pose3d_loss_is_still_refused():
    """a guard, not a feature test (it passes without the feature): the refusal was rewritten with the loop"""
    from core.function import AverageMeter
    meter = AverageMeter(_cfg(False, False), {'pose3d_loss': object()})
    with pytest.raises(NotImplementedError, match='pose3d_loss'):
        meter.computeLosses(pose2d_pred=torch.zeros(1, 21, 2), pose2d_gt=torch.zeros(1, 21, 2))


def test_modules_check_their_arguments():
    from core.loss import BoneLengthLoss, JointAngleLoss, structure_losses
    p = torch.zeros(2, 21, 2)
    with pytest.raises(RuntimeError, match='HIP-device'):
        BoneLengthLoss()(p, p)
    with pytest.raises(RuntimeError, match='HIP-device'):
        JointAngleLoss()(p)
    with pytest.raises(RuntimeError, match='HIP-device'):
        structure_losses(p, torch.zeros(2, 21, 3))
    for bad in (torch.zeros(2, 20, 2), torch.zeros(2, 22, 2)):
        with pytest.raises(ValueError, match='21'):
            BoneLengthLoss()(bad, bad)
        with pytest.raises(ValueError, match='21'):
            JointAngleLoss()(bad)
        with pytest.raises(ValueError, match='21'):
            structure_losses(bad, bad)
    p3 = torch.zeros(2, 21, 3)
    with pytest.raises(ValueError, match='3-D poses'):
        BoneLengthLoss()(p3, p3)
    with pytest.raises(ValueError, match='3-D poses'):
        BoneLengthLoss()(p, p3)
    with pytest.raises(ValueError, match='3-D poses'):
        JointAngleLoss()(p3)
    with pytest.raises(ValueError, match='3-D poses'):
        structure_losses(p3, p)
    with pytest.raises(ValueError, match='pose2d_gt'):
        structure_losses(p, None)
    with pytest.raises(ValueError, match='terms'):
        structure_losses(p, p, terms=0)
