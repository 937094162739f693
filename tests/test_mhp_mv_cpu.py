"""Host side of the 3-D evaluation: the MHP_mv reader (lib/dataset/mhp.py) on a fake MHP tree (tests/mhp_tree.py) -
sample order, world joints, extrinsics, the reference's occlusion (centres against tests/golden/triangulation.npz,
the painted disc, the visibility rule), a view subset, make_dataloader; the 3-D accumulator (core/evaluate3d.py)
against a hand count and the reference's result-file formats; tools/evaluate_3D.py's refusals. No GPU: loaders are
built, not iterated, and collate runs in this process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mhp_tree

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('mhp_mv')
    mhp_tree.write_tree(root)
    return root


def _cfg(root, opts=()):
    return mhp_tree.config(root, ['WORKERS', '0'] + list(opts), mhp_tree.SOFTMAX_YAML)


def _frame2d(d, f, c):
    from dataset.mhp import IDX_MHP, INTRINSIC, project_points
    rvec, tvec = mhp_tree.calibration(d, c)
    return project_points(mhp_tree.joints(d, f)[list(IDX_MHP)], rvec, tvec, INTRINSIC, np.zeros(5))


def test_sample_count_and_order(tree):
    from dataset.mhp import MHP_mv
    ev = MHP_mv(_cfg(tree), 'eval')
    assert len(ev) == 5 and ev.index == [('data_17', f) for f in range(5)]
    tr = MHP_mv(_cfg(tree), 'train')
    assert tr.index == [('data_1', f) for f in range(6)] + [('data_2', f) for f in range(3)]
    s = tr[7]
    assert [os.path.basename(p) for p in s['paths']] == ['1_webcam_{}.jpg'.format(c) for c in (1, 2, 3, 4)]
    assert all(os.path.basename(os.path.dirname(p)) == 'data_2' for p in s['paths'])
    assert s['frames'] == 1 and s['views'] == 4


def test_pose3d_and_extrinsics(tree):
    from dataset.mhp import IDX_MHP, INTRINSIC, MHP_mv, collate_rgb, rodrigues
    ds = MHP_mv(_cfg(tree), 'eval')
    b = collate_rgb([ds[2], ds[3]])
    assert b['pose3d'].dtype == torch.float64 and b['pose3d'].shape == (2, 21, 3)
    for i, f in enumerate((2, 3)):
        assert np.allclose(b['pose3d'][i].numpy(), mhp_tree.joints(17, f)[list(IDX_MHP)], atol=1e-6)
    assert b['extrinsic_matrices'].shape == (2, 4, 3, 4) and b['intrinsic_matrix'].shape == (2, 3, 3)
    for c in range(1, 5):
        rvec, tvec = mhp_tree.calibration(17, c)
        E = b['extrinsic_matrices'][1, c - 1].numpy()
        assert np.array_equal(E[:, :3], rodrigues(rvec)) and np.array_equal(E[:, 3], tvec.reshape(3))
    assert np.array_equal(b['intrinsic_matrix'][0].numpy(), INTRINSIC)
    assert b['pose2d'].shape == (8, 21, 2) and b['visibility'].shape == (8, 21, 1)
    assert b['hm_inverse'].shape == (8, 2, 3) and b['hm_inverse'].dtype == torch.float64


def test_occlusion_centres_match_the_reference_draw(tree):
    from dataset.mhp import MHP_mv, occlusion_centre
    joint = np.load(os.path.join(GOLD, 'triangulation.npz'))['occlusion_joint']
    ds = MHP_mv(_cfg(tree), 'eval')
    for i in range(len(ds)):
        s = ds[i]
        for c in range(1, 5):
            p = _frame2d(17, i, c)[joint[i, c - 1]]
            assert s['occlusion'][c - 1] == (int(p[0]), int(p[1]))
    frame2d = np.zeros((21, 2))
    frame2d[:, 0] = np.arange(21)
    for i in range(64):
        for c in range(1, 5):
            assert occlusion_centre(frame2d, i, c) == (joint[i, c - 1], 0)


def test_painted_disc_and_visibility(tree):
    from dataset.mhp import MHP_mv, collate_rgb, decode, paint_disc
    ds = MHP_mv(_cfg(tree), 'eval')
    s = ds[1]
    b = collate_rgb([s])
    for c in range(1, 5):
        off, h, w, pitch = b['table'][c - 1].tolist()
        img = b['buffer'].numpy()[off:off + h * pitch].reshape(h, w, 3)
        ref = decode(s['paths'][c - 1], False)
        cx, cy = s['occlusion'][c - 1]
        yy, xx = np.mgrid[0:480, 0:640]
        inside = (xx - cx) ** 2 + (yy - cy) ** 2 <= 2500
        assert inside.sum() > 0
        assert (img[inside] == 0).all() and np.array_equal(img[~inside], ref[~inside])
        assert np.array_equal(img, paint_disc(ref, (cx, cy)))
        p = _frame2d(17, 1, c)
        vis = (p[:, 0] >= 0) & (p[:, 1] >= 0) & (p[:, 0] < 640) & (p[:, 1] < 480) & \
              (np.linalg.norm(p - np.array([cx, cy]), axis=1) > 50)
        assert np.array_equal(b['visibility'][c - 1, :, 0].numpy(), vis)
        assert not vis[0]                           # the wrist lies outside every frame (tests/mhp_tree.joints)
    assert (~b['visibility']).sum() > 4             # the discs hide joints beyond the wrists
    # a disc at the frame's corner is clipped, not wrapped
    corner = paint_disc(np.full((480, 640, 3), 7, np.uint8), (0, 479))
    assert corner[479, 0].sum() == 0 and corner[479, 51].sum() == 21 and corner[0, 0].sum() == 21


def test_view_subset(tree):
    from dataset.mhp import MHP_mv, collate_rgb, rodrigues
    ds = MHP_mv(_cfg(tree), 'eval', views=(2, 4))
    s = ds[3]
    assert [os.path.basename(p) for p in s['paths']] == ['3_webcam_2.jpg', '3_webcam_4.jpg']
    full = MHP_mv(_cfg(tree), 'eval')[3]
    assert s['occlusion'] == [full['occlusion'][1], full['occlusion'][3]]
    b = collate_rgb([s, ds[4]])
    assert b['pose2d'].shape == (4, 21, 2) and b['extrinsic_matrices'].shape == (2, 2, 3, 4)
    assert np.array_equal(b['extrinsic_matrices'][0, 1, :, :3].numpy(), rodrigues(mhp_tree.calibration(17, 4)[0]))
    for bad in ((1,), (1, 1), (0, 2), (2, 5)):
        with pytest.raises(ValueError, match='views'):
            MHP_mv(_cfg(tree), 'eval', views=bad)


def test_make_dataloader_builds_mhp_mv(tree):
    from dataset.build import make_dataloader
    from dataset.mhp import MHP_mv, collate_rgb, make_loader
    from dataset.rhd import RHDLoader
    cfg = _cfg(tree, ['DATASET.TEST_DATASET', "['MHP_mv']", 'TEST.IMAGES_PER_GPU', '2'])
    loader = make_dataloader(cfg, False)['MHP_mv']
    assert isinstance(loader, RHDLoader) and isinstance(loader.dataset, MHP_mv)
    assert loader.loader.collate_fn is collate_rgb and not loader.heatmaps and len(loader) == 3
    sub = make_loader(cfg, 'MHP_mv', 'eval', False, views=(1, 3))
    assert sub.dataset.views == (1, 3)


def test_accumulator_hand_count(tmp_path):
    from core.evaluate3d import Eval3DAccumulator, auc
    acc = Eval3DAccumulator(21, 64)
    B, V, K = 3, 2, 21
    gt3 = np.zeros((B, K, 3))
    pred3 = np.zeros((B, K, 3))
    pred3[:, :, 0] = np.arange(K) * 2.5             # joint k off by 2.5 k mm
    pred3[1] += 1000.0                              # sample 1 is invalid below: its error must not count
    vis = np.ones((B * V, K, 1))
    vis[2:4, :15] = 0                               # sample 1: 12 of 42 visible < 0.65
    vis[4, :14] = 0                                 # sample 2: 28 of 42 visible = 0.667 >= 0.65
    gt2 = np.full((B * V, K, 2), 10.0)
    inv = np.tile(np.array([[10.0, 0, 0], [0, 7.5, 0]]), (B * V, 1, 1))
    acc.add(gt2 + [0.3, 0.4], gt2, vis, inv, pred3, gt3)
    assert acc.n_valid == 2
    assert np.allclose(acc.mse, 2 * 2.5 * np.arange(K))
    err = 2.5 * np.arange(K)
    assert np.array_equal(acc.pck, [2 * (err < t).sum() for t in range(1, 51)])     # strict <
    mse2d, pck2d, mse3d, pck3d = acc.save(str(tmp_path))
    assert np.allclose(mse3d, err) and np.allclose(pck3d[1], [(err < t).mean() for t in range(1, 51)])
    assert np.allclose(mse2d, np.sqrt(18.0))         # (0.3, 0.4) heat-map px through diag(10, 7.5): (3, 3) px
    assert np.allclose(auc(np.arange(1, 4), [0.0, 0.5, 1.0]), 0.5)


def test_saved_files_have_the_reference_formats(tmp_path):
    from core.evaluate3d import Eval3DAccumulator
    acc = Eval3DAccumulator(21, 64)
    rng = np.random.default_rng(3)
    gt2 = rng.uniform(0, 64, (8, 21, 2))
    acc.add(gt2 + rng.normal(0, 1, gt2.shape), gt2, np.ones((8, 21, 1)),
            np.tile(np.array([[10.0, 0, 0], [0, 10.0, 0]]), (8, 1, 1)), rng.normal(0, 10, (2, 21, 3)), np.zeros((2, 21, 3)))
    acc.save(str(tmp_path))
    ref_dir = os.path.join(GOLD, 'ref_eval3D_Volumetric_triangulation_MHP_v1')
    for name in ('mse2d_each_joint.txt', 'mse3d_each_joint.txt'):
        ours, ref = np.loadtxt(os.path.join(str(tmp_path), name)), np.loadtxt(os.path.join(ref_dir, name))
        assert ours.shape == ref.shape == (21,)
        line = open(os.path.join(str(tmp_path), name)).readline().strip()
        assert len(line.split('.')[1]) == 4          # '%.4f', as the reference's
    pck2d, ref2d = np.loadtxt(os.path.join(str(tmp_path), 'PCK2d.txt')), np.loadtxt(os.path.join(ref_dir, 'PCK2d.txt'))
    assert pck2d.shape == ref2d.shape == (2, 49) and np.array_equal(pck2d[0], ref2d[0])
    pck3d, ref3d = np.loadtxt(os.path.join(str(tmp_path), 'PCK3d.txt')), np.loadtxt(os.path.join(ref_dir, 'PCK3d.txt'))
    # the reference's committed file keeps thresholds 20..50 of the 1..50 it computes (evaluate_3D.py:251)
    assert pck3d.shape == (2, 50) and ref3d.shape[0] == 2 and np.array_equal(pck3d[0], np.arange(1, 51))
    assert np.array_equal(pck3d[0, -ref3d.shape[1]:], ref3d[0])


def _tool(args, tree, cwd):
    pkg = os.path.dirname(mhp_tree.PKG + os.sep)
    return subprocess.run([sys.executable, os.path.join(pkg, 'tools', 'evaluate_3D.py'), '--cfg', mhp_tree.SOFTMAX_YAML]
                          + args + ['DATA_DIR', str(tree)], cwd=cwd, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize('name', ['alg', 'ransac', 'vol', 'vol_CPM', 'FTL'])
def test_tool_refuses_models_that_are_not_built(tree, tmp_path, name):
    r = _tool(['MODEL.NAME', name], tree, str(tmp_path))
    assert r.returncode != 0 and 'ValueError' in r.stderr and 'is not built' in r.stderr, r.stderr[-2000:]


def test_tool_refuses_bad_views_and_a_missing_tree(tree, tmp_path):
    r = _tool(['--views', '[1]'], tree, str(tmp_path))
    assert r.returncode != 0 and 'two or more distinct views' in r.stderr, r.stderr[-2000:]
    missing = tmp_path / 'nowhere'
    r = _tool([], missing, str(tmp_path))
    assert r.returncode != 0 and os.path.join(str(missing), 'MHP', 'annotated_frames') in r.stderr, r.stderr[-2000:]
