"""The RHD reader on the device: hrnet_affine_warp_normalize_u8 (csrc/preprocess.hip) against a float64 restatement
of cv2.warpAffine (INTER_LINEAR, BORDER_CONSTANT 0: inverse map, bilinear blend, 0 outside the crop slot) followed by
ToTensor + Normalize; the loader end to end on a fake RHD tree (tests/rhd_tree.py); tools/train.py and
tools/evaluate_2D.py on that tree. The kernel's u8 code is recovered exactly from its output as
round((out*std + mean)*255); it must equal the oracle's code except within 1e-3 of a .5 boundary (f32 blend against
f64), and never differ by more than 1."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rhd_tree
from spawned import spawned

pytestmark = pytest.mark.gpu

MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])


def _oracle(img, x0, y0, h, w, inv, size):
    """(3, size, size) float64 blend of the crop img[y0:y0+h, x0:x0+w] at the inverse-mapped output pixels, and a
    mask of the pixels whose four neighbours all lie outside the crop"""
    crop = img[y0:y0 + h, x0:x0 + w].astype(np.float64)
    m = np.asarray(inv, dtype=np.float32).astype(np.float64).reshape(2, 3)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    sx = m[0, 0] * xx + m[0, 1] * yy + m[0, 2]
    sy = m[1, 0] * xx + m[1, 1] * yy + m[1, 2]
    fx0, fy0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - fx0, sy - fy0
    out = np.zeros((size, size, 3))
    inside_any = np.zeros((size, size), bool)
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xi, yi = fx0 + dx, fy0 + dy
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            inside_any |= ok
            v = crop[np.where(ok, yi, 0).astype(int), np.where(ok, xi, 0).astype(int)]
            out += (wy * wx * ok)[..., None] * v
    return out.transpose(2, 0, 1), ~inside_any


def _codes(out):
    return np.round((out.double().cpu().numpy() * STD[:, None, None] + MEAN[:, None, None]) * 255.0)


def _check(out, v, outside):
    want = np.clip(np.round(v), 0, 255)
    got = _codes(out)
    assert np.isfinite(got).all()
    diff = np.abs(got - want)
    near_half = np.abs((v - np.floor(v)) - 0.5) < 1e-3
    assert diff.max() <= 1.0
    bad = (diff > 0) & ~near_half
    assert not bad.any(), 'codes differ away from a .5 boundary at {} pixels'.format(int(bad.sum()))
    zero = ((np.float32(0) / np.float32(255) - MEAN.astype(np.float32)) / STD.astype(np.float32)).astype(np.float32)
    o = out.cpu().numpy()
    for c in range(3):
        assert (o[c][outside] == zero[c]).all()
    return int((diff > 0).sum())


@spawned
def test_warp_matches_the_f64_oracle():
    from dataset.preprocess import affine_warp_normalize, pack_images
    from dataset.rhd import Augment, geometry
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (320, 320, 3), dtype=np.uint8) for _ in range(2)]
    p = pack_images(imgs)
    aug = Augment(30, 0.75, 1.25, 40, 'short', True)
    # crops at the four image edges and inside; rotation 0 / +-30, scale 0.75 / 1.25, translation, flip
    crops = [(0, 0, 0, 150), (1, 320 - 120, 0, 120), (0, 0, 320 - 170, 170), (1, 320 - 90, 320 - 90, 90),
             (0, 60, 80, 200), (1, 0, 0, 320), (0, 150, 40, 14)]
    params = [(0.5, 0.5, 0, 0, False), (0.0, 0.0, 10, -7, False), (1.0, 1.0, -25, 30, True), (0.25, 0.8, 3, 3, True),
              (0.9, 0.1, 0, 0, True), (0.5, 0.5, 40, 0, False), (0.0, 1.0, -1, 0, True)]
    table, inv, cases = [], [], []
    for (i, x0, y0, s), (us, ur, dx, dy, flip) in zip(crops, params):
        table.append([p.offsets[i] + y0 * 960 + 3 * x0, s, s, 960])   # a slot inside the image: image pitch
        g = geometry(s, s, {'u_scale': us, 'u_rot': ur, 'dx': dx, 'dy': dy, 'flip': flip}, aug, 256, 64)
        inv.append(g['inverse'])
        cases.append((imgs[i], x0, y0, s))
    out = affine_warp_normalize(p.buffer.cuda(), torch.tensor(table), torch.tensor(np.stack(inv)), (256, 256))
    assert out.shape == (len(crops), 3, 256, 256)
    n_out = 0
    for k, (img, x0, y0, s) in enumerate(cases):
        v, outside = _oracle(img, x0, y0, s, s, np.float32(inv[k]), 256)
        n = _check(out[k], v, outside)
        n_out += int(outside.sum())
        print('case {}: {} codes one off at a .5 boundary, {} pixels outside the crop'.format(k, n, outside.sum()))
    assert n_out > 0


@spawned
def test_identity_is_bit_identical_to_normalize_u8():
    from dataset.preprocess import affine_warp_normalize, pack_images
    from dataset.rhd import augment_from_cfg, geometry
    from dataset.target_generators import normalize_u8
    img = np.random.default_rng(2).integers(0, 256, (320, 320, 3), dtype=np.uint8)
    crop = np.ascontiguousarray(img[30:286, 50:306])
    aug = augment_from_cfg(rhd_tree.config('.'), is_train=False)
    g = geometry(256, 256, {'u_scale': 0.3, 'u_rot': 0.7, 'dx': 5, 'dy': 5, 'flip': False}, aug, 256, 64)
    assert np.array_equal(g['inverse'], np.eye(3)[:2])
    p = pack_images([img])
    out = affine_warp_normalize(p.buffer.cuda(), torch.tensor([[30 * 960 + 150, 256, 256, 960]]),
                                torch.tensor(g['inverse'][None]), (256, 256))
    assert torch.equal(out, normalize_u8(torch.from_numpy(crop)[None].cuda()))


@spawned
def test_corrupt_row_gives_nan_and_no_read():
    from dataset.preprocess import affine_warp_normalize
    buf = torch.full((3 * 20 * 20,), 100, dtype=torch.uint8, device='cuda')
    table = torch.tensor([[0, 20, 20, 60], [60, 20, 20, 60], [-3, 5, 5, 15]])
    inv = torch.tensor(np.tile(np.eye(3)[:2].reshape(1, 6), (3, 1)))
    out = affine_warp_normalize(buf, table, inv, (16, 16), validate=False)
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    assert torch.isnan(out[1]).all() and torch.isnan(out[2]).all()
    with pytest.raises(ValueError):
        affine_warp_normalize(buf, table, inv, (16, 16))


def _kfd_children():
    """this process's children that hold a GPU device file open"""
    found = []
    for pid in os.listdir('/proc'):
        if not pid.isdigit():
            continue
        try:
            with open('/proc/{}/stat'.format(pid)) as f:
                ppid = int(f.read().rsplit(')', 1)[1].split()[1])
            if ppid != os.getpid():
                continue
            for fd in os.listdir('/proc/{}/fd'.format(pid)):
                t = os.readlink('/proc/{}/fd/{}'.format(pid, fd))
                if t == '/dev/kfd' or t.startswith('/dev/dri/'):
                    found.append(pid)
        except OSError:
            continue
    return found


@spawned
def test_loader_batch_equals_the_cpu_path(tmp_path):
    from dataset.build import make_dataloader
    from dataset.preprocess import affine_warp_normalize, pack_images
    from dataset.rhd import RHDLoader
    from dataset.target_generators import HeatmapGenerator
    rhd_tree.write_tree(tmp_path)
    g = rhd_tree.golden()
    cfg = rhd_tree.config(tmp_path, ['WITH_DATA_AUG', 'True', 'WORKERS', '2', 'TRAIN.IMAGES_PER_GPU', '3',
                                     'TEST.IMAGES_PER_GPU', '3'])
    loader = make_dataloader(cfg, True)['RHD_kpt']
    assert isinstance(loader, RHDLoader)
    loader.sampler.set_epoch(4)
    keys = [list(b) for b in loader.loader.batch_sampler]
    batches = list(loader)
    assert len(batches) == 3 and [b['imgs'].shape[0] for b in batches] == [3, 3, 2]
    assert not _kfd_children(), 'a DataLoader worker opened the GPU'
    ds = loader.dataset
    for b, ks in zip(batches, keys):
        ref = [ds[k] for k in ks]
        pose = np.stack([r['pose2d'] for r in ref]).astype(np.float32)
        vis = np.stack([r['visibility'] for r in ref])
        assert torch.equal(b['pose2d'], torch.from_numpy(pose)) and torch.equal(b['visibility'], torch.from_numpy(vis))
        assert b['corner'].tolist() == [r['corner'].tolist() for r in ref]
        assert b['crop_size'].tolist() == [r['crop_size'] for r in ref]
        joints = np.concatenate([pose, vis.astype(np.float32)], 2)
        assert torch.equal(b['heatmaps'], HeatmapGenerator(64, 21, 2)(torch.from_numpy(joints)))
        pk = pack_images([r['crop'] for r in ref], pin=False)
        imgs = affine_warp_normalize(pk.buffer.cuda(), pk.table, torch.tensor(np.stack([r['inverse'] for r in ref])),
                                     (256, 256))
        assert torch.equal(b['imgs'], imgs)
    # evaluation: every sample in order, no augmentation; crop_size / corner take the joints back to image pixels
    ev = make_dataloader(cfg, False)['RHD']
    got = [b for b in ev]
    assert 'heatmaps' not in got[0]
    pose = torch.cat([b['pose2d'] for b in got]).double().numpy()
    crop = torch.cat([b['crop_size'] for b in got]).double().numpy()
    corner = torch.cat([b['corner'] for b in got]).double().numpy()
    assert np.array_equal(corner, g['corner']) and np.array_equal(crop, g['crop_size'])
    back = pose * crop[:, None, None] / 64 + corner[:, None]
    np.testing.assert_allclose(back, g['pose2d'] + g['corner'][:, None], rtol=0, atol=1e-3)
    assert torch.isfinite(torch.cat([b['imgs'] for b in got])).all()


def _run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


def test_train_and_evaluate_on_the_fake_tree(tmp_path):
    rhd_tree.write_tree(tmp_path / 'data')
    out = str(tmp_path / 'out')
    common = ['DATA_DIR', str(tmp_path / 'data'), 'OUTPUT_DIR', out, 'LOG_DIR', str(tmp_path / 'log'),
              'TRAIN.IMAGES_PER_GPU', '4', 'TEST.IMAGES_PER_GPU', '3', 'PRINT_FREQ', '1', 'WORKERS', '2']
    log = _run([sys.executable, 'tools/train.py', '--cfg', rhd_tree.YAML, 'TRAIN.BEGIN_EPOCH', '0',
                'TRAIN.END_EPOCH', '2', 'WITH_DATA_AUG', 'True'] + common, rhd_tree.PKG)
    assert 'Dataset: RHD_kpt Epoch: [1][1/2]' in log and 'Validating on RHD dataset' in log
    assert 'Dataset: RHD Test: [2/3]' in log and 'synthetic' not in log
    exp = os.path.join(out, 'RHD', 'RHD_HRNet_w32_max_hmloss_v1')
    state = os.path.join(exp, 'final_state.pth.tar')
    assert os.path.exists(state)
    log = _run([sys.executable, 'tools/evaluate_2D.py', '--cfg', rhd_tree.YAML, '--model_path', state,
                '--batch_size', '3', '--gpu', '0'] + common, rhd_tree.PKG)
    res = os.path.join(out, 'eval2D_results_RHD_HRNet_w32_max_hmloss_v1')
    mse = np.loadtxt(os.path.join(res, 'mse2d_each_joint.txt'))
    pck = np.loadtxt(os.path.join(res, 'PCK2d.txt'))
    assert mse.shape == (21,) and np.isfinite(mse).all() and pck.shape == (2, 49) and np.isfinite(pck).all()
    assert 'mean EPE' in log
