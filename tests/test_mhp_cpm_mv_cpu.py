"""The reader MHP_CPM_mv (lib/dataset/mhp.py; reference MHP_CPMMultiViewDataset.py:36-274) on the fake MHP tree of
tests/mhp_tree.py: slot order, the heat-map channel layout and the int() truncation, the background channel and the centre
map, hm_inverse and core.function_vol.heatmap_projections equal to update_after_resize(K) [R|t], the frames undisturbed (no
occlusion disc), a training loader. No GPU: loaders are built, not iterated, and collate runs in this process."""
import os

import numpy as np
import pytest
import torch

import mhp_tree

YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_VolTriangulation_CPM_v1.yaml')
IMG, HM = (96, 64), (24, 8)          # (width, height): x and y scale differently, and so do their heat-map factors (4, 8)


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('mhp_cpm_mv')
    mhp_tree.write_tree(root)
    return root


def _cfg(root, opts=()):
    return mhp_tree.config(root, ['WORKERS', '0', 'MODEL.IMAGE_SIZE', str(list(IMG)), 'MODEL.HEATMAP_SIZE', str(list(HM))]
                           + list(opts), YAML)


def _image2d(d, f, c):
    """the joints of frame f in the pixels of the resized image, projected without distortion"""
    from dataset.mhp import IDX_MHP, INTRINSIC, project_points
    rvec, tvec = mhp_tree.calibration(d, c)
    p = project_points(mhp_tree.joints(d, f)[list(IDX_MHP)], rvec, tvec, INTRINSIC, np.zeros(5))
    return p * np.array([IMG[0] / 640.0, IMG[1] / 480.0])


def test_registered_indexed_like_mhp_mv_and_slot_order(tree):
    from dataset.mhp import MHP_CPM_mv, MHP_mv, READERS, collate_bgr
    assert READERS['MHP_CPM_mv'] is MHP_CPM_mv and issubclass(MHP_CPM_mv, MHP_mv) and MHP_CPM_mv.bgr and MHP_CPM_mv.resize
    ds = MHP_CPM_mv(_cfg(tree), 'training')
    assert ds.index == MHP_mv(_cfg(tree), 'training').index and len(ds) == 9
    assert (ds.width, ds.height, ds.hm_w, ds.hm_h) == IMG + HM
    s = ds[7]
    assert [os.path.basename(p) for p in s['paths']] == ['1_webcam_{}.jpg'.format(c) for c in (1, 2, 3, 4)]
    assert s['frames'] == 1 and s['views'] == 4 and 'occlusion' not in s
    b = collate_bgr([ds[2], ds[7]])
    assert b['heatmaps'].shape == (8, 22, HM[1], HM[0]) and b['heatmaps'].dtype == torch.float32
    assert b['centermaps'].shape == (8, 1, IMG[1], IMG[0]) and b['pose2d'].shape == (8, 21, 2)
    assert b['pose3d'].shape == (2, 21, 3) and b['extrinsic_matrices'].shape == (2, 4, 3, 4)
    for i, (d, f) in enumerate(((1, 2), (2, 1))):                         # slot b * V + v
        for v in range(4):
            want = _image2d(d, f, v + 1) / np.array([IMG[0] / HM[0], IMG[1] / HM[1]])
            assert np.allclose(b['pose2d'][i * 4 + v].numpy(), want, atol=1e-4)
    sub = MHP_CPM_mv(_cfg(tree), 'evaluation', views=(2, 4))
    assert sub[0]['views'] == 2 and sub[0]['heatmaps'].shape[0] == 2
    with pytest.raises(ValueError, match='multiples of 8'):
        MHP_CPM_mv(_cfg(tree, ['MODEL.IMAGE_SIZE', '[100, 64]']), 'training')


def test_heat_map_channels_truncation_background_and_centre_map(tree):
    from dataset.mhp import MHP_CPM_mv, cpm_center, gaussian_map
    ds = MHP_CPM_mv(_cfg(tree), 'evaluation')
    s = ds[3]
    fx, fy = IMG[0] / HM[0], IMG[1] / HM[1]
    truncated = 0
    for v, c in enumerate((1, 2, 3, 4)):
        p = _image2d(17, 3, c)
        heat = s['heatmaps'][v]
        for j in range(21):
            # joint j in channel j + 1, centred at int(coordinate) / factor: the coordinate is truncated BEFORE the division
            want = gaussian_map(HM[1], HM[0], int(p[j, 0]) / fx, int(p[j, 1]) / fy, 2).astype(np.float32)
            assert np.array_equal(heat[j + 1], want), (c, j)
            plain = gaussian_map(HM[1], HM[0], p[j, 0] / fx, p[j, 1] / fy, 2).astype(np.float32)
            truncated += int(not np.array_equal(plain, want))
        assert np.array_equal(heat[0], 1.0 - heat[1:].max(axis=0))
        assert float(heat[1:].max()) <= 1.0 and float(heat[1:][heat[1:] > 0].min()) >= 0.0099
        centre, exception = cpm_center(p, IMG[0], IMG[1])
        # (the reader projects the joints as the annotation files print them: a last-digit difference from mhp_tree.joints)
        assert np.allclose(s['centermaps'][v, 0], gaussian_map(IMG[1], IMG[0], centre[0], centre[1], 3), atol=1e-5)
        assert s['centermaps'].dtype == np.float32 and float(s['centermaps'][v].max()) > 0.5
        assert bool(s['exception'][v]) == exception
        vis = (p[:, 0] >= 0) & (p[:, 1] >= 0) & (p[:, 0] < IMG[0]) & (p[:, 1] < IMG[1])
        assert np.array_equal(s['visibility'][v][:, 0], vis)
    assert truncated > 0                         # the truncation is seen: some maps differ from the untruncated ones


def test_hm_inverse_and_projections_are_update_after_resize(tree):
    from core.function_vol import heatmap_projections
    from dataset.mhp import INTRINSIC, MHP_CPM_mv, collate_bgr
    ds = MHP_CPM_mv(_cfg(tree), 'evaluation')
    b = collate_bgr([ds[0], ds[4]])
    want = np.array([[640.0 / HM[0], 0, 0], [0, 480.0 / HM[1], 0]])
    assert all(np.array_equal(m, want) for m in b['hm_inverse'].numpy())
    proj = heatmap_projections(b['intrinsic_matrix'], b['extrinsic_matrices'], b['hm_inverse']).numpy()
    # the reference (lib/core/function3D.py:89-93, lib/utils/misc.py:16-27): fx, cx scaled by new_width / width, fy, cy by
    # new_height / height, then K [R|t]
    K = INTRINSIC.copy()
    K[0, 0], K[0, 2] = K[0, 0] * (HM[0] / 640.0), K[0, 2] * (HM[0] / 640.0)
    K[1, 1], K[1, 2] = K[1, 1] * (HM[1] / 480.0), K[1, 2] * (HM[1] / 480.0)
    ref = K[None, None] @ b['extrinsic_matrices'].numpy()
    assert np.allclose(proj, ref, rtol=1e-14, atol=1e-12)
    # and it projects the world joints onto the reader's own heat-map joints
    world = np.concatenate([b['pose3d'].numpy(), np.ones((2, 21, 1))], axis=2)
    uvw = np.einsum('bvij,bkj->bvki', proj, world)
    assert np.allclose(uvw[..., :2] / uvw[..., 2:], b['pose2d'].numpy().reshape(2, 4, 21, 2), atol=1e-4)


def test_frames_are_left_whole_and_a_training_loader_is_allowed(tree):
    from dataset.mhp import MHP_CPM_mv, collate_bgr, decode, make_loader
    ds = MHP_CPM_mv(_cfg(tree), 'training', is_train=True)          # the reference applies no random transform here
    s = ds[1]
    again = MHP_CPM_mv(_cfg(tree), 'training', is_train=True, seed=5)[(1, 3)]
    assert all(np.array_equal(s[k], again[k]) for k in ('heatmaps', 'centermaps', 'pose2d'))
    b = collate_bgr([s])
    for v in range(4):
        off, h, w, pitch = b['table'][v].tolist()
        img = b['buffer'].numpy()[off:off + h * pitch].reshape(h, w, 3)
        assert np.array_equal(img, decode(s['paths'][v], True))         # BGR, no occlusion disc
    loader = make_loader(_cfg(tree, ['TRAIN.IMAGES_PER_GPU', '2']), 'MHP_CPM_mv', 'training', True, heatmaps=False,
                         views=(1, 3))
    assert loader.batch_size == 2 and len(loader) == 5 and loader.dataset.views == (1, 3) and not loader.heatmaps
