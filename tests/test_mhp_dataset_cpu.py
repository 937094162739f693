"""The MHP readers' host side (lib/dataset/mhp.py, dataset/build.py) on a fake MHP tree (tests/mhp_tree.py): file
order and split, MHP_seq sample counts and windows, the idx_MHP reorder, the projection against hand-worked cases,
visibility, channel order, slot order and frame sharing of a packed batch, seeded augmentation, the heat-map inverse
and make_dataloader's choice of loader. No GPU: the loaders are built, not iterated."""
import logging
import os

import numpy as np
import pytest
import torch

import mhp_tree

FX, FY, CX, CY = 614.878, 615.479, 313.219, 231.288


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('mhp')
    mhp_tree.write_tree(root)
    return root


def _kpt_cfg(root, opts=()):
    return mhp_tree.config(root, mhp_tree.KPT_OPTS + list(opts), mhp_tree.SOFTMAX_YAML)


def test_natural_sort_and_split(tree):
    from dataset.mhp import MHP, MHP_kpt, natural_sort, split_range
    names = ['a/data_17/0_webcam_1.jpg', 'a/data_2/10_webcam_1.jpg', 'a/data_2/9_webcam_2.jpg',
             'a/data_2/9_webcam_1.jpg', 'a/data_1/1_webcam_4.jpg']
    assert natural_sort(names) == ['a/data_1/1_webcam_4.jpg', 'a/data_2/9_webcam_1.jpg', 'a/data_2/9_webcam_2.jpg',
                                   'a/data_2/10_webcam_1.jpg', 'a/data_17/0_webcam_1.jpg']
    assert split_range(56, 'training') == (0, 44) and split_range(56, 'evaluation') == (44, 56)
    assert split_range(7, 'train') == (0, 5) and split_range(7, 'valid') == (5, 7)
    cfg = _kpt_cfg(tree)
    tr, ev = MHP_kpt(cfg, 'training'), MHP(cfg, 'evaluation')
    rel = [os.path.relpath(p, os.path.join(str(tree), 'MHP', 'annotated_frames')) for p in tr.images + ev.images]
    want = [os.path.join(d, '{}_webcam_{}.jpg'.format(f, c)) for d in ('data_1', 'data_2', 'data_17')
            for f in range(mhp_tree.DIRS[d]) for c in range(1, 5)]
    assert rel == want and len(tr) == 44 and len(ev) == 12


def test_seq_counts_and_windows(tree):
    from dataset.mhp import MHP_seq, seq_windows
    c, w = seq_windows(6, 2, [-2, -1, 0, 1, 2])
    assert c.tolist() == [0, 2, 4]
    assert w.tolist() == [[0, 0, 0, 1, 2], [0, 1, 2, 3, 4], [2, 3, 4, 5, 5]]       # clamped at both ends
    c, w = seq_windows(3, 1, [-2, -1, 0, 1, 2])
    assert c.tolist() == [0, 1, 2] and w.tolist() == [[0, 0, 0, 1, 2], [0, 0, 1, 2, 2], [0, 1, 2, 2, 2]]
    for n in range(1, 12):
        for s in (1, 2, 3):
            assert len(seq_windows(n, s, [0])[0]) == (n - 1) // s + 1
    tr = MHP_seq(mhp_tree.config(tree), 'training')
    assert len(tr) == 3 + 2
    assert [tr.window(i)[:2] for i in range(5)] == [('data_1', 0), ('data_1', 2), ('data_1', 4), ('data_2', 0),
                                                    ('data_2', 2)]
    assert tr.window(4)[2] == [0, 1, 2, 2, 2]
    assert len(MHP_seq(mhp_tree.config(tree, ['DATASET.STRIDE', '1']), 'training')) == 6 + 3
    ev = MHP_seq(mhp_tree.config(tree), 'evaluation')
    assert len(ev) == 3 and [ev.window(i)[0] for i in range(3)] == ['data_17'] * 3
    s = ev[1]
    frames = [int(os.path.basename(p).split('_')[0]) for p in s['paths']]
    views = [int(os.path.splitext(p)[0][-1]) for p in s['paths']]
    assert frames == [f for f in (0, 1, 2, 3, 4) for _ in range(4)] and views == [1, 2, 3, 4] * 5


def test_projection_hand_cases():
    from dataset.mhp import DISTORTION, INTRINSIC, project_points, rodrigues
    zero = np.zeros(3)
    # zero rotation, a translation: (2, -1, 4) + (0, 0, 1) -> x' = 0.4, y' = -0.2
    p = project_points([[2, -1, 4]], zero, [0, 0, 1], INTRINSIC, np.zeros(5))
    np.testing.assert_allclose(p, [[FX * 0.4 + CX, -FY * 0.2 + CY]], rtol=0, atol=1e-9)
    # a 90 degree turn about z takes x to y: (1, 0, 5) -> (0, 1, 5)
    R = rodrigues([0, 0, np.pi / 2])
    np.testing.assert_allclose(R @ [1, 0, 0], [0, 1, 0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(rodrigues([np.pi / 2, 0, 0]) @ [0, 1, 0], [0, 0, 1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(rodrigues(zero), np.eye(3), rtol=0, atol=0)
    p = project_points([[1, 0, 5]], [0, 0, np.pi / 2], zero, INTRINSIC, np.zeros(5))
    np.testing.assert_allclose(p, [[CX, FY * 0.2 + CY]], rtol=0, atol=1e-9)
    # a point on the optical axis lands on the principal point whatever the distortion
    np.testing.assert_allclose(project_points([[0, 0, 3]], zero, zero, INTRINSIC, DISTORTION), [[CX, CY]], rtol=0,
                               atol=1e-12)
    # one distorted point worked by hand: x' = 0.1, y' = 0.2, r2 = 0.05
    # radial = 1 + 0.092701 * 0.05 - 0.175877 * 0.0025 = 1.0041953575
    # x'' = 0.1 * radial + 2 * (-0.0035687) * 0.02 + (-0.00302299) * (0.05 + 0.02) = 0.10006517845
    # y'' = 0.2 * radial + (-0.0035687) * (0.05 + 0.08) + 2 * (-0.00302299) * 0.02 = 0.2002542209
    p = project_points([[0.1, 0.2, 1]], zero, zero, INTRINSIC, DISTORTION)
    np.testing.assert_allclose(p, [[FX * 0.10006517845 + CX, FY * 0.2002542209 + CY]], rtol=0, atol=1e-8)
    np.testing.assert_allclose(p, [[374.746877, 354.540268]], rtol=0, atol=1e-5)


def test_visibility_at_the_frame_border():
    from dataset.mhp import visibility
    p = np.array([[0, 0], [639.999, 479.999], [640, 10], [10, 480], [-0.001, 5], [5, -0.001], [320, 240]])
    assert visibility(p).ravel().tolist() == [True, True, False, False, False, False, True]
    assert visibility(p).shape == (7, 1)


def test_reorder_projection_and_heatmap_inverse(tree):
    from dataset.mhp import (DISTORTION, IDX_MHP, INTRINSIC, MHP, MHP_seq, project_points, read_calibration,
                             read_joints)
    assert sorted(IDX_MHP) == list(range(21)) and IDX_MHP[0] == 20
    ev = MHP(_kpt_cfg(tree), 'evaluation')
    for i in (0, 5, 11):
        s = ev[i]
        path = s['paths'][0]
        f, _, c = os.path.splitext(os.path.basename(path))[0].split('_')
        world = read_joints(os.path.join(str(tree), 'MHP', 'annotations', 'data_17', f + '_joints.txt'))
        np.testing.assert_allclose(world, mhp_tree.joints(17, int(f)), rtol=0, atol=1e-6)
        uv = project_points(world[list(IDX_MHP)], *read_calibration(str(tree), 'data_17', c), INTRINSIC, DISTORTION)
        m = s['hm_inverse'][0]
        back = s['pose2d'][0] @ m[:, :2].T + m[:, 2]
        np.testing.assert_allclose(back, uv, rtol=0, atol=1e-6)
        assert not s['visibility'][0, 0, 0] and s['visibility'][0, 1:].sum() >= 15   # file joint 20 is the wrist
    # MHP_seq: the centre frame's labels, no distortion
    ev = MHP_seq(mhp_tree.config(tree), 'evaluation')
    s = ev[2]                                                               # centre 4 of data_17
    world = mhp_tree.joints(17, 4)[list(IDX_MHP)]
    for v in range(4):
        uv = project_points(world, *read_calibration(str(tree), 'data_17', v + 1), INTRINSIC, np.zeros(5))
        m = s['hm_inverse'][v]
        np.testing.assert_allclose(s['pose2d'][v] @ m[:, :2].T + m[:, 2], uv, rtol=0, atol=1e-6)


def test_plain_geometry_is_the_short_side_scale(tree):
    from dataset.mhp import MHP
    s = MHP(_kpt_cfg(tree), 'evaluation')[0]
    inv = s['inverse'][0]
    # 'short': the central 480 x 480 square of the frame onto 256 x 256
    np.testing.assert_allclose(inv @ [0, 0, 1], [80, 0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(inv @ [256, 256, 1], [560, 480], rtol=0, atol=1e-9)
    np.testing.assert_allclose(s['hm_inverse'][0] @ [64, 64, 1], [560, 480], rtol=0, atol=1e-9)


def _frame(tree, d, f, c):
    from dataset.preprocess import read_image_rgb
    return read_image_rgb(os.path.join(str(tree), 'MHP', 'annotated_frames', d, '{}_webcam_{}.jpg'.format(f, c)))


def _slot(b, k):
    off, h, w, pitch = b['table'][k].tolist()
    return b['buffer'].numpy()[off:off + h * pitch].reshape(h, w, 3)


def test_channel_order(tree):
    from dataset.build import make_dataloader
    cfg = _kpt_cfg(tree, ['WORKERS', '0', 'TRAIN.IMAGES_PER_GPU', '2', 'TEST.IMAGES_PER_GPU', '2'])
    for loader in (make_dataloader(cfg, True)['MHP_kpt'], make_dataloader(cfg, False)['MHP']):
        ds = loader.dataset
        b = loader.loader.collate_fn([ds[0], ds[1]])
        f, _, c = os.path.splitext(os.path.basename(ds.images[1]))[0].split('_')
        d = os.path.basename(os.path.dirname(ds.images[1]))
        assert np.array_equal(_slot(b, 1), _frame(tree, d, f, c)[:, :, ::-1])          # BGR, as cv2.imread
    seq = make_dataloader(mhp_tree.config(tree, ['WORKERS', '0']), False)['MHP_seq']
    b = seq.loader.collate_fn([seq.dataset[0]])
    assert np.array_equal(_slot(b, 0), _frame(tree, 'data_17', 0, 1))                   # RGB


def test_seq_slot_order_and_frame_sharing(tree):
    from dataset.mhp import MHP_seq, collate, slot_order
    assert slot_order(2, 5, 4)[1].tolist() == [(j * 2 + 1) * 4 + c for j in range(5) for c in range(4)]
    ev = MHP_seq(mhp_tree.config(tree), 'evaluation')
    samples = [ev[0], ev[1]]                                # centres 0 and 2 of data_17 (5 frames)
    b = collate(samples)
    assert b['table'].shape == (40, 4) and b['inverse'].shape == (40, 6)
    assert b['pose2d'].shape == (8, 21, 2) and b['visibility'].shape == (8, 21, 1) and b['hm_inverse'].shape == (8, 2, 3)
    # frames 0..4 of each view are decoded once: 20 distinct frames for 40 slots
    assert b['table'][:, 0].unique().numel() == 20
    assert b['buffer'].numel() == 20 * 480 * 640 * 3
    B = 2
    for s, sample in enumerate(samples):
        _, _, window = ev.window(s)
        for j, f in enumerate(window):
            for c in range(4):
                k = (j * B + s) * 4 + c
                assert np.array_equal(_slot(b, k), _frame(tree, 'data_17', f, c + 1))
                np.testing.assert_array_equal(b['inverse'][k].numpy(),
                                              sample['inverse'][j * 4 + c].astype(np.float32).reshape(6))
    for s, sample in enumerate(samples):
        assert torch.equal(b['pose2d'][4 * s:4 * s + 4], torch.from_numpy(sample['pose2d'].astype(np.float32)))
        assert torch.equal(b['visibility'][4 * s:4 * s + 4], torch.from_numpy(sample['visibility']))


def test_seeded_augmentation(tree):
    from dataset.mhp import MHP_kpt, MHP_seq
    cfg = _kpt_cfg(tree, ['WITH_DATA_AUG', 'True'])
    ds = MHP_kpt(cfg, 'training', is_train=True)
    a, b, c = ds[(3, 1)], ds[(3, 1)], ds[(3, 2)]
    assert np.array_equal(a['inverse'], b['inverse']) and np.array_equal(a['pose2d'], b['pose2d'])
    assert not np.array_equal(a['inverse'], c['inverse'])
    plain = MHP_kpt(cfg, 'training', is_train=False)
    assert np.array_equal(plain[(3, 1)]['inverse'], plain[(3, 2)]['inverse'])
    seq = MHP_seq(mhp_tree.config(tree, ['WITH_DATA_AUG', 'True']), 'training', is_train=True)
    a, b, c = seq[(1, 0)], seq[(1, 0)], seq[(1, 1)]
    assert np.array_equal(a['inverse'], b['inverse']) and not np.array_equal(a['inverse'], c['inverse'])
    assert len({m.tobytes() for m in a['inverse']}) == 20                  # one draw per image
    with pytest.raises(ValueError, match='SCALE_AWARE_SIGMA'):
        MHP_seq(mhp_tree.config(tree, ['DATASET.SCALE_AWARE_SIGMA', 'True']), 'training', is_train=True)


def test_errors(tree, tmp_path):
    from dataset.mhp import MHP_seq, collate
    with pytest.raises(ValueError, match='no data_N'):
        MHP_seq(mhp_tree.config(tmp_path), 'training')
    mhp_tree.write_tree(tmp_path, {'data_18': 2})
    from PIL import Image
    small = os.path.join(str(tmp_path), 'MHP', 'annotated_frames', 'data_18', '1_webcam_3.jpg')
    Image.fromarray(np.zeros((240, 320, 3), np.uint8)).save(small)
    ev = MHP_seq(mhp_tree.config(tmp_path), 'evaluation')
    with pytest.raises(ValueError, match='1_webcam_3.jpg'):
        collate([ev[0]])


def test_eval_accumulator_maps_through_the_inverse():
    from core.evaluate2d import Eval2DAccumulator
    acc = Eval2DAccumulator(2, 64)
    inv = np.array([[[7.5, 0, 80], [0, 7.5, 0]]])
    pred = np.array([[[10.0, 10.0], [0.0, 0.0]]])
    gt = np.array([[[10.0, 10.4], [0.0, 0.0]]])
    acc.add(pred, gt, np.ones((1, 2, 1)), inverse=inv)
    mse, pck = acc.result()
    np.testing.assert_allclose(mse, [3.0, 0.0], rtol=0, atol=1e-9)
    assert pck[1, 2] == 0.5 and pck[1, 3] == 1.0                           # 3 px is not < 3


def test_make_dataloader_picks_mhp_or_synthetic(tree, tmp_path, caplog):
    from dataset.build import SyntheticLoader, make_dataloader
    from dataset.mhp import MHP, MHP_kpt, MHP_seq
    from dataset.rhd import RHDLoader, _InOrder
    cfg = mhp_tree.config(tree, ['WORKERS', '0'])
    tr = make_dataloader(cfg, True)
    assert list(tr) == ['MHP_seq'] and isinstance(tr['MHP_seq'], RHDLoader)
    assert type(tr['MHP_seq'].dataset) is MHP_seq and tr['MHP_seq'].heatmaps and len(tr['MHP_seq']) == 3
    va = make_dataloader(cfg, False)['MHP_seq']
    assert len(va) == 2 and isinstance(va.sampler, _InOrder)
    kcfg = _kpt_cfg(tree, ['WORKERS', '0', 'TRAIN.IMAGES_PER_GPU', '8', 'TEST.IMAGES_PER_GPU', '8'])
    k = make_dataloader(kcfg, True)['MHP_kpt']
    assert type(k.dataset) is MHP_kpt and k.heatmaps and len(k) == 6
    v = make_dataloader(kcfg, False)['MHP']
    assert type(v.dataset) is MHP and not v.heatmaps and len(v) == 2
    assert make_dataloader(kcfg, False, heatmaps=True)['MHP'].heatmaps
    with caplog.at_level(logging.WARNING):
        syn = make_dataloader(mhp_tree.config(tmp_path / 'absent'), True, num_batches=5)
    assert list(syn) == ['synthetic_kpt'] and isinstance(syn['synthetic_kpt'], SyntheticLoader)
    missing = os.path.join(str(tmp_path / 'absent'), 'MHP', 'annotated_frames')
    assert [r for r in caplog.records if missing in r.getMessage()]
