"""The RHD reader's host side (lib/dataset/rhd.py, dataset/build.py) on a fake RHD tree, against the reference's own
geometry code as pinned in tests/golden/rhd_geometry.npz (tests/golden/make_golden_rhd.py): hand choice, crop,
reorder and visibility exactly, the float64 matrices and transformed joints to 1e-9; then the augmentation draws,
the errors, the samplers and make_dataloader's choice of loader. No GPU: the loaders are built, not iterated."""
import logging
import os
import re

import numpy as np
import pytest
import torch

import rhd_tree
from rhd_tree import golden

SCALE_TYPES = ('short', 'long')


def _aug(case):
    from dataset.rhd import Augment
    max_rot, min_s, max_s, max_t, st, prob = case
    return Augment(max_rot, min_s, max_s, max_t, SCALE_TYPES[int(st)], bool(prob))


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('rhd')
    rhd_tree.write_tree(root)
    return root


def test_hand_choice_crop_reorder_visibility_equal_reference(tree):
    from dataset.rhd import IDX_RHD, RHD, choose_hand, crop_box
    g = golden()
    ds = RHD(rhd_tree.config(tree), 'evaluation')
    assert len(ds) == len(g['uv_vis'])
    for i, uv_vis in enumerate(g['uv_vis']):
        pose2d, vis = choose_hand(uv_vis)
        corner, crop = crop_box(pose2d, 320, 320)
        assert corner == tuple(g['corner'][i]) and crop == g['crop_size'][i]
        assert np.array_equal((pose2d - np.array(corner))[list(IDX_RHD)], g['pose2d'][i])
        assert np.array_equal(vis, g['visibility'][i])
        s = ds[i]
        assert np.array_equal(s['corner'], g['corner'][i]) and s['crop_size'] == g['crop_size'][i]
        assert s['visibility'].dtype == np.bool_ and np.array_equal(s['visibility'], g['visibility'][i])
        assert s['crop'].shape == (crop, crop, 3)
    # the fixture covers both hands, a tie (left), and crops clamped at the image edges
    n_vis = g['uv_vis'][:, :, 2].reshape(-1, 2, 21).sum(2)
    assert (n_vis[:, 0] > n_vis[:, 1]).any() and (n_vis[:, 0] < n_vis[:, 1]).any() and (n_vis[:, 0] == n_vis[:, 1]).any()
    assert (g['corner'] == 0).any() and (g['corner'] + g['crop_size'][:, None] == 320).any()


def test_matrices_and_joints_match_reference():
    from dataset.rhd import geometry, transform_joints
    g = golden()
    inp, hm = (int(v) for v in g['sizes'])
    for i in range(len(g['uv_vis'])):
        crop = int(g['crop_size'][i])
        for c, case in enumerate(g['cases']):
            aug = _aug(case)
            params = {'u_scale': g['u'][i, c, 0], 'u_rot': g['u'][i, c, 1], 'dx': int(g['dxy'][i, c, 0]),
                      'dy': int(g['dxy'][i, c, 1]), 'flip': bool(g['flip'][i, c])}
            geo = geometry(crop, crop, params, aug, inp, hm)
            np.testing.assert_allclose(geo['mat_input'], g['mat_input'][i, c], rtol=0, atol=1e-9)
            np.testing.assert_allclose(geo['mat_output'], g['mat_output'][i, c], rtol=0, atol=1e-9)
            joints = transform_joints(g['pose2d'][i], geo['mat_output'], params['flip'], hm)
            np.testing.assert_allclose(joints, g['joints'][i, c], rtol=0, atol=1e-9)
            # the inverse maps an output pixel (after the flip) back to the crop pixel the forward matrix sends there
            fwd = np.vstack([geo['mat_input'], [0, 0, 1]])
            p = np.array([[3.0, 7.0], [200.5, 100.25], [255.0, 0.0]])
            q = np.c_[p, np.ones(3)] @ fwd.T
            if params['flip']:
                q[:, 0] = inp - 1 - q[:, 0]
            back = np.c_[q[:, :2], np.ones(3)] @ geo['inverse'].T
            np.testing.assert_allclose(back, p, rtol=0, atol=1e-9)


def test_translation_bounds_and_draws():
    from dataset.rhd import Augment, _base_scale, draw_params
    g = golden()
    for i in range(len(g['uv_vis'])):
        crop = int(g['crop_size'][i])
        for c, case in enumerate(g['cases']):
            aug = _aug(case)
            if aug.max_translate == 0:
                continue
            scale = _base_scale(crop, crop, aug.scale_type) * (g['u'][i, c, 0] * (aug.max_scale - aug.min_scale)
                                                                + aug.min_scale)
            lo, hi = g['translate_bounds'][i, c]
            assert (int(-aug.max_translate * scale), int(aug.max_translate * scale)) == (int(lo), int(hi))
    aug = Augment(30, 0.75, 1.25, 40, 'short', True)
    a = draw_params(np.random.default_rng((0, 1, 5)), 150, 150, aug)
    assert a == draw_params(np.random.default_rng((0, 1, 5)), 150, 150, aug)
    assert a != draw_params(np.random.default_rng((0, 2, 5)), 150, 150, aug)
    flips = [draw_params(np.random.default_rng((0, 0, k)), 150, 150, aug)['flip'] for k in range(50)]
    assert all(flips)                                           # FLIP: true -> random() < True always
    aug_no = aug._replace(flip=False)
    assert not any(draw_params(np.random.default_rng((0, 0, k)), 150, 150, aug_no)['flip'] for k in range(50))
    # MAX_TRANSLATE * scale < 1: the reference's randint(0, 0) raises; here no translation
    tiny = Augment(30, 0.75, 1.25, 0.5, 'short', False)
    for k in range(20):
        p = draw_params(np.random.default_rng((0, 0, k)), 100, 100, tiny)
        assert p['dx'] == 0 and p['dy'] == 0


def test_augmented_sample_is_seeded_by_epoch_and_index(tree):
    from dataset.rhd import RHD_kpt
    cfg = rhd_tree.config(tree, ['WITH_DATA_AUG', 'True'])
    ds = RHD_kpt(cfg, 'training', is_train=True)
    a, b, c = ds[(3, 1)], ds[(3, 1)], ds[(3, 2)]
    assert np.array_equal(a['inverse'], b['inverse']) and np.array_equal(a['pose2d'], b['pose2d'])
    assert not np.array_equal(a['inverse'], c['inverse'])
    assert np.array_equal(a['corner'], c['corner']) and a['crop_size'] == c['crop_size']
    plain = RHD_kpt(cfg, 'training', is_train=False)[(3, 1)]
    g = golden()
    np.testing.assert_allclose(plain['pose2d'], g['joints'][3, 0], rtol=0, atol=1e-9)


def test_errors(tree, tmp_path):
    from dataset.rhd import RHD, augment_from_cfg
    with pytest.raises(ValueError, match='SCALE_AWARE_SIGMA'):
        augment_from_cfg(rhd_tree.config(tree, ['DATASET.SCALE_AWARE_SIGMA', 'True']), True)
    uv = golden()['uv_vis'][:2].copy()
    uv[1, :21, :2] = 40.25                                     # every key point of the chosen hand on one spot
    uv[1, :21, 2] = 1
    rhd_tree.write_tree(tmp_path, ('evaluation',), uv_vis=uv)
    ds = RHD(rhd_tree.config(tmp_path), 'evaluation')
    ds[0]
    with pytest.raises(ValueError, match=re.escape(os.path.join('color', '00001.png'))):
        ds[1]


def test_collate_packs_crops():
    from dataset.rhd import collate
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    samples = [{'crop': img[y:y + s, x:x + s], 'inverse': np.eye(3)[:2] * (k + 1), 'corner': np.array((x, y)),
                'crop_size': s, 'pose2d': np.full((21, 2), k, dtype=np.float64), 'visibility': np.ones((21, 1), bool)}
               for k, (x, y, s) in enumerate(((0, 0, 10), (30, 12, 20), (5, 39, 1)))]
    b = collate(samples)
    buf = b['buffer'].numpy()
    assert not b['buffer'].is_pinned()
    for s, (off, h, w, pitch) in zip(samples, b['table'].tolist()):
        assert (h, w, pitch) == (s['crop_size'], s['crop_size'], 3 * s['crop_size'])
        assert np.array_equal(buf[off:off + h * pitch].reshape(h, w, 3), s['crop'])
    assert b['inverse'].dtype == torch.float32 and b['inverse'].shape == (3, 6)
    assert b['pose2d'].shape == (3, 21, 2) and b['visibility'].shape == (3, 21, 1)
    assert b['corner'].tolist() == [[0, 0], [30, 12], [5, 39]] and b['crop_size'].tolist() == [10, 20, 1]


def test_make_dataloader_picks_rhd_or_synthetic(tree, tmp_path, caplog):
    from dataset.build import SyntheticLoader, make_dataloader
    from dataset.rhd import RHD, RHD_kpt, RHDLoader
    cfg = rhd_tree.config(tree, ['WORKERS', '0', 'TRAIN.IMAGES_PER_GPU', '3', 'TEST.IMAGES_PER_GPU', '3'])
    tr = make_dataloader(cfg, True)
    assert list(tr) == ['RHD_kpt'] and isinstance(tr['RHD_kpt'], RHDLoader)
    assert type(tr['RHD_kpt'].dataset) is RHD_kpt and tr['RHD_kpt'].heatmaps and len(tr['RHD_kpt']) == 3
    va = make_dataloader(cfg, False)
    assert list(va) == ['RHD'] and type(va['RHD'].dataset) is RHD and not va['RHD'].heatmaps
    assert make_dataloader(cfg, False, heatmaps=True)['RHD'].heatmaps
    assert len(make_dataloader(cfg, True, max_batches=2)['RHD_kpt']) == 2
    with caplog.at_level(logging.WARNING):
        syn = make_dataloader(rhd_tree.config(tmp_path / 'absent'), True, num_batches=5)
    assert list(syn) == ['synthetic_kpt'] and isinstance(syn['synthetic_kpt'], SyntheticLoader)
    assert len(syn['synthetic_kpt']) == 5
    missing = os.path.join(str(tmp_path / 'absent'), 'RHD', 'training', 'anno_training.pickle')
    assert [r for r in caplog.records if missing in r.getMessage()]


def test_samplers(tree):
    from dataset.rhd import RHD_kpt, RHDLoader, RHD
    cfg = rhd_tree.config(tree, ['WORKERS', '0'])
    ds = RHD_kpt(cfg, 'training', is_train=True)
    n = len(ds)
    shares = []
    for rank in range(2):
        ld = RHDLoader(cfg, ds, 2, True, rank=rank, world=2)
        ld.sampler.set_epoch(3)
        keys = [k for b in ld.loader.batch_sampler for k in b]
        assert all(e == 3 for _, e in keys)
        shares.append([i for i, _ in keys])
    assert sorted(shares[0] + shares[1]) == list(range(n)) and len(shares[0]) == n // 2
    one = RHDLoader(cfg, ds, 3, True)
    one.sampler.set_epoch(0)
    e0 = [i for b in one.loader.batch_sampler for i, _ in b]
    one.sampler.set_epoch(1)
    e1 = [i for b in one.loader.batch_sampler for i, _ in b]
    assert sorted(e0) == sorted(e1) == list(range(n)) and e0 != e1
    ev = RHDLoader(cfg, RHD(cfg, 'evaluation'), 3, False)
    assert [[i for i, _ in b] for b in ev.loader.batch_sampler] == [[0, 1, 2], [3, 4, 5], [6, 7]]
    capped = RHDLoader(cfg, RHD(cfg, 'evaluation'), 3, False, max_batches=2)
    assert len(capped) == 2 and len(list(capped.loader.batch_sampler)) == 2


def test_header_declares_the_new_entry_point():
    from hipnet import _capi
    header = open(os.path.join(rhd_tree.PKG, '..', 'include', 'hrnet_hip.h')).read()
    m = re.search(r'int hrnet_affine_warp_normalize_u8\(([^)]*)\)', header)
    assert m is not None and 'hrnet_affine_warp_normalize_u8' in _capi.EXPORTED
    assert len(m.group(1).split(',')) == len(_capi._SIGS['hrnet_affine_warp_normalize_u8'])
