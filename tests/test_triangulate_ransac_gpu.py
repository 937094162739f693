"""hrnet_triangulate_ransac (csrc/triangulate.hip) through utils/multiview.py on the device: the reference's own
triangulate_ransac results in tests/golden/triangulation_ransac.npz (tests/golden/make_golden_triangulation_ransac.py)
- the inlier mask exactly and X to 1e-6 relative on every case; the bit-for-bit ties to hrnet_triangulate (the same
device functions in the same order); table forms, batch sizes that do not fill a lane group or a workgroup, eight
views, the frame mapping, degenerate tables; what the feature is for (a displaced view is dropped and the result is
nearer the world point than the all-view DLT); tools/evaluate_3D.py --triangulation ransac end to end. Each device
test runs in a spawned child (tests/spawned.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mhp_tree
from spawned import spawned

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'triangulation_ransac.npz')
RTOL = 1e-6                 # RTOL of tests/test_triangulate_gpu.py
CASES = ['{}_v{}_{}'.format(rig, v, tag) for rig in ('wide', 'near')
         for v, tag in ((4, 'one'), (4, 'none'), (4, 'two'), (3, 'one'), (3, 'none'))]
ALL4 = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def _dev(a):
    return a.cuda() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ransac(proj, pts, pairs=None, epsilon=25, to_frame=None, frame_points=False):
    """-> device tensors (X float32 (B, K, 3), inliers bool (B, K, V)[, frame points])"""
    from utils.multiview import triangulate_ransac_batch
    if pairs is not None:
        pairs = torch.from_numpy(np.array(pairs, np.int32))
    out = triangulate_ransac_batch(_dev(proj), _dev(pts), pairs, epsilon,
                                   to_frame=None if to_frame is None else _dev(to_frame),
                                   return_frame_points=frame_points)
    torch.cuda.synchronize()
    return out


def _dlt(proj, pts):
    from utils.multiview import triangulate_batch_of_points
    X = triangulate_batch_of_points(_dev(proj), _dev(pts))
    torch.cuda.synchronize()
    return X


def _rel(X, ref):
    X = X.cpu().numpy() if torch.is_tensor(X) else X
    return np.linalg.norm(X.astype(np.float64) - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


@spawned
def test_matches_the_reference_on_every_case():
    z = np.load(GOLD)
    assert sorted(k[:-2] for k in z.files if k.endswith('_X')) == sorted(CASES)
    for name in CASES:
        X, mask = _ransac(z[name + '_proj'], z[name + '_pts'], z[name + '_pairs'], float(z['epsilon']))
        assert tuple(X.shape) == (4, 21, 3) and X.dtype == torch.float32
        assert mask.dtype == torch.bool and tuple(mask.shape) == z[name + '_mask'].shape
        wrong = int((mask.cpu().numpy() != z[name + '_mask']).any(-1).sum())
        rel = _rel(X, z[name + '_X'])
        print(name, 'points with another mask', wrong, 'largest relative error', rel.max())
        assert wrong == 0, name
        assert rel.max() <= RTOL, (name, rel.max())


@spawned
def test_bit_equal_to_the_plain_kernel_where_the_sets_coincide():
    z = np.load(GOLD)
    for name in CASES:
        proj, pts = z[name + '_proj'], z[name + '_pts']
        V = pts.shape[1]
        # epsilon = inf: every view is an inlier of the first hypothesis
        X, mask = _ransac(proj, pts, None, float('inf'))
        assert mask.all() and torch.equal(X, _dlt(proj, pts)), name
        X, mask = _ransac(proj, pts, z[name + '_pairs'], float('inf'))
        assert mask.all() and torch.equal(X, _dlt(proj, pts)), name
        # V = 2: the one pair is the whole set, whatever epsilon
        for eps in (25, 0.0):
            X, mask = _ransac(proj[:, :2], pts[:, :2], None, eps)
            assert mask.all() and torch.equal(X, _dlt(proj[:, :2], pts[:, :2])), name
        # epsilon = 0 with a single pair: those two views alone
        for i in range(V):
            for j in range(i + 1, V):
                X, mask = _ransac(proj, pts, [[i, j]], 0.0)
                want = np.zeros(V, bool)
                want[[i, j]] = True
                assert (mask.cpu().numpy() == want).all(), (name, i, j)
                assert torch.equal(X, _dlt(proj[:, [i, j]], pts[:, [i, j]])), (name, i, j)


@spawned
def test_shared_and_per_point_tables_agree():
    z = np.load(GOLD)
    for name in ('wide_v4_one', 'near_v4_two', 'near_v3_one'):
        proj, pts = z[name + '_proj'], z[name + '_pts']
        V = pts.shape[1]
        shared = np.array([(i, j) for i in range(V) for j in range(i + 1, V)], np.int32)
        for table in (shared, shared[::-1].copy(), shared[[2, 0]]):
            Xs, ms = _ransac(proj, pts, table)
            Xp, mp = _ransac(proj, pts, np.broadcast_to(table, (84,) + table.shape).copy())
            assert torch.equal(Xs, Xp) and torch.equal(ms, mp), name
        Xn, mn = _ransac(proj, pts, None)                   # None is every pair in lexicographic order
        Xs, ms = _ransac(proj, pts, shared)
        assert torch.equal(Xn, Xs) and torch.equal(mn, ms), name


@spawned
def test_batches_that_do_not_fill_a_group_or_a_workgroup():
    z = np.load(GOLD)
    for name in ('near_v4_one', 'wide_v3_one'):
        proj, pts, pairs = z[name + '_proj'], z[name + '_pts'], z[name + '_pairs'].reshape(4, 21, 10, 2)
        big = np.arange(37) % 4                                       # B * K = 777
        Xb, mb = _ransac(proj[big], pts[big], pairs[big].reshape(-1, 10, 2))
        ref, ref_mask = z[name + '_X'], z[name + '_mask']
        assert (mb.cpu().numpy() == ref_mask[big]).all() and _rel(Xb, ref[big]).max() <= RTOL
        for B in (1, 3, 5, 32):                                       # B * K = 21, 63, 105, 672
            idx = big[:B]
            X, m = _ransac(proj[idx], pts[idx], pairs[idx].reshape(-1, 10, 2))
            assert torch.equal(X, Xb[:B]) and torch.equal(m, mb[:B]), (name, B)
        for K in (1, 5, 21):
            X, m = _ransac(proj[big], pts[big][:, :, :K], pairs[big][:, :K].reshape(-1, 10, 2))
            assert torch.equal(X, Xb[:, :K]) and torch.equal(m, mb[:, :K]), (name, K)
        # a table longer than a lane group (repeats change nothing: only a strictly larger set replaces)
        long_pairs = np.concatenate([pairs, pairs, pairs], 2)[big].reshape(-1, 30, 2)
        X, m = _ransac(proj[big], pts[big], long_pairs)
        assert torch.equal(X, Xb) and torch.equal(m, mb), name


@spawned
def test_eight_views_with_all_28_pairs():
    """the four wide and the four near cameras as one rig of eight; one view of every point displaced by 80-110 px per
    axis. Held to the float64 restatement (tests/triangulate_ransac_ref.py): the same mask, X to 1e-6 relative. The
    inputs are asserted to be off the threshold, as the fixture's are."""
    import triangulate_ransac_ref as RR
    import triangulate_ref as T
    z = np.load(GOLD)
    rig = np.concatenate([z['wide_v4_none_proj'][0], z['near_v4_none_proj'][0]])        # (8, 3, 4)
    world = z['wide_v4_none_world']                                                      # (4, 21, 3)
    rng = np.random.default_rng(8)
    h = np.einsum('vij,bkj->bvki', rig, np.concatenate([world, np.ones((4, 21, 1))], -1))
    pts = h[..., :2] / h[..., 2:] + rng.normal(0, 1.0, (4, 8, 21, 2))
    bad = rng.integers(0, 8, (4, 21))
    for b in range(4):
        for k in range(21):
            pts[b, bad[b, k], k] += rng.uniform(80, 110, 2) * rng.choice([-1.0, 1.0], 2)
    pts = pts.astype(np.float32)
    proj = np.broadcast_to(rig, (4, 8, 3, 4)).copy()
    pairs = [(i, j) for i in range(8) for j in range(i + 1, 8)]
    assert len(pairs) == 28
    gap = np.inf
    for b in range(4):
        for k in range(21):
            p2 = pts[b, :, k].astype(np.float64)
            for i, j in pairs:
                err = RR.reprojection_errors(rig, p2, T.triangulate(rig[[i, j]], p2[[i, j]])[0])
                gap = min(gap, np.abs(np.delete(err, [i, j]) - 25.0).min())
    assert gap >= 1e-3, gap
    ref, ref_mask = RR.triangulate_ransac_batch(proj, pts, pairs, 25.0)
    X, mask = _ransac(proj, pts, None, 25)
    assert (mask.cpu().numpy() == ref_mask).all()
    assert _rel(X, ref).max() <= RTOL
    dropped = ~ref_mask[np.arange(4)[:, None], np.arange(21)[None], bad]
    assert dropped.mean() >= 0.9 and (ref_mask.sum(-1) >= 7).mean() >= 0.9      # the rule does its work at V = 8


@spawned
def test_a_displaced_view_is_dropped_and_the_point_is_nearer():
    z = np.load(GOLD)
    for rig in ('wide', 'near'):
        name = rig + '_v4_one'
        proj, pts, bad, world = z[name + '_proj'], z[name + '_pts'], z[name + '_bad'], z[name + '_world']
        ref_mask = z[name + '_mask']
        assert (bad.sum(-1) == 1).all()
        clean = (ref_mask == ~bad).all(-1)                  # the reference kept exactly the three clean views
        print(name, 'points whose reference mask is the three clean views:', int(clean.sum()), 'of', clean.size)
        assert clean.sum() * 2 >= clean.size
        X, mask = _ransac(proj, pts, z[name + '_pairs'], float(z['epsilon']))
        X = X.cpu().numpy().astype(np.float64)
        assert (mask.cpu().numpy()[clean] == ~bad[clean]).all()
        # the plain kernel over those three views, per dropped view
        three = np.empty_like(X)
        for v in range(4):
            keep = [u for u in range(4) if u != v]
            Xv = _dlt(proj[:, keep], pts[:, keep]).cpu().numpy()
            sel = bad[..., v]
            three[sel] = Xv[sel]
        rel = _rel(X[clean], three[clean])
        print(name, 'against the three-view DLT, largest relative difference', rel.max())
        assert rel.max() <= RTOL
        every = _dlt(proj, pts).cpu().numpy().astype(np.float64)
        d_ransac = np.linalg.norm(X - world, axis=-1)[clean]
        d_all = np.linalg.norm(every - world, axis=-1)[clean]
        print(name, 'distance to the world point, mean: RANSAC', d_ransac.mean(), 'all-view DLT', d_all.mean())
        assert (d_all > d_ransac).all(), (name, int((d_all <= d_ransac).sum()))


@spawned
def test_to_frame_and_frame_points():
    z = np.load(GOLD)
    name = 'wide_v4_one'
    proj, pts, pairs = z[name + '_proj'], z[name + '_pts'].astype(np.float64), z[name + '_pairs']
    B, V, K = pts.shape[:3]
    rng = np.random.default_rng(11)
    # per-slot affine frame -> heat map and its inverse for the kernel, as tests/test_triangulate_gpu.py
    fwd = np.zeros((B * V, 3, 3))
    fwd[:, 0, 0], fwd[:, 1, 1] = rng.uniform(0.12, 0.15, B * V), rng.uniform(0.12, 0.15, B * V)
    fwd[:, 0, 1], fwd[:, 1, 0] = rng.uniform(-0.01, 0.01, B * V), rng.uniform(-0.01, 0.01, B * V)
    fwd[:, :2, 2] = rng.uniform(-20, 5, (B * V, 2))
    fwd[:, 2, 2] = 1.0
    inv = np.linalg.inv(fwd)[:, :2]
    flat = pts.reshape(B * V, K, 2)
    hm = (np.einsum('sij,skj->ski', fwd[:, :2, :2], flat) + fwd[:, None, :2, 2]).astype(np.float32)
    X, mask, frame = _ransac(proj, hm.reshape(B, V, K, 2), pairs, 25, to_frame=inv, frame_points=True)
    mapped = np.einsum('sij,skj->ski', inv[:, :, :2], hm.astype(np.float64)) + inv[:, None, :, 2]
    assert tuple(frame.shape) == (B, V, K, 2) and frame.dtype == torch.float32
    assert np.abs(frame.cpu().numpy().reshape(B * V, K, 2) - mapped).max() <= 1e-3     # f32 output of ~600 px values
    Xm, mm = _ransac(proj, mapped.reshape(B, V, K, 2).astype(np.float32), pairs, 25)
    assert torch.equal(mask, mm) and (mask.cpu().numpy() == z[name + '_mask']).all()
    assert _rel(X, Xm.cpu().numpy().astype(np.float64)).max() <= 1e-5
    # the frame points are those of the plain kernel, bit for bit
    from utils.multiview import triangulate_batch_of_points
    _, plain = triangulate_batch_of_points(_dev(proj), _dev(hm.reshape(B, V, K, 2)), to_frame=_dev(inv),
                                           return_frame_points=True)
    assert torch.equal(frame, plain)
    # null to_frame: the frame points come back as given, and asking for them changes nothing else
    X2, m2, same = _ransac(proj, pts.astype(np.float32), pairs, 25, frame_points=True)
    X1, m1 = _ransac(proj, pts.astype(np.float32), pairs, 25)
    assert np.array_equal(same.cpu().numpy(), pts.astype(np.float32))
    assert torch.equal(X1, X2) and torch.equal(m1, m2)


@spawned
def test_degenerate_tables_and_non_finite_points():
    z = np.load(GOLD)
    name = 'near_v4_one'
    proj, pts = z[name + '_proj'], z[name + '_pts']
    every = _dlt(proj, pts)
    for table in ([[1, 1]], [[0, 4]], [[-1, 2]], [[7, 9], [3, 3]], np.zeros((0, 2), np.int32),
                  np.full((84, 3, 2), 2, np.int32)):
        X, mask = _ransac(proj, pts, table, 25)
        assert mask.all() and torch.equal(X, every)
    # unusable pairs among usable ones are passed over
    Xa, ma = _ransac(proj, pts, [[2, 2], [0, 9], [1, 3], [-4, 0], [0, 2]], 25)
    Xb, mb = _ransac(proj, pts, [[1, 3], [0, 2]], 25)
    assert torch.equal(Xa, Xb) and torch.equal(ma, mb) and not ma.all()
    # more hypotheses than the entry point takes: refused on the host and by the library, nothing is launched
    from hipnet import _capi as C
    with pytest.raises(ValueError, match='hypotheses'):
        _ransac(proj, pts, np.zeros((65, 2), np.int32))
    d = [_dev(a) for a in (pts, proj, np.zeros((65, 2), np.int32))]
    out, m = torch.empty(4, 21, 3, device='cuda'), torch.empty(4, 21, dtype=torch.int32, device='cuda')
    with pytest.raises(RuntimeError, match='n_hyp'):
        C.call('hrnet_triangulate_ransac', d[0].data_ptr(), None, d[1].data_ptr(), d[2].data_ptr(), 65, 0, 25.0,
               out.data_ptr(), m.data_ptr(), None, 4, 4, 21, C.stream_ptr())
    # a non-finite point gives a non-finite result for that point only, and the launch ends
    bad = pts.copy()
    bad[3, 0, 0] = np.nan
    X, mask = _ransac(proj, bad, None, 25)
    Xg, mg = _ransac(proj, pts, None, 25)
    X, Xg = X.cpu().numpy().reshape(-1, 3), Xg.cpu().numpy().reshape(-1, 3)
    assert not np.isfinite(X[3 * 21]).any()
    assert np.array_equal(np.delete(X, 3 * 21, 0), np.delete(Xg, 3 * 21, 0))


def _tool(args, data, out):
    return subprocess.run([sys.executable, 'tools/evaluate_3D.py', '--cfg', mhp_tree.SOFTMAX_YAML, '--views',
                           '[1,2,3,4]', '--batch_size', '2', '--num_batches', '2', '--gpu', '0'] + args +
                          ['DATA_DIR', str(data), 'OUTPUT_DIR', out, 'WORKERS', '0'],
                          cwd=mhp_tree.PKG, capture_output=True, text=True, timeout=600)


def test_evaluate_3d_cli_with_ransac(tmp_path):
    from models import pose_hrnet_softmax
    mhp_tree.write_tree(tmp_path / 'data', {'data_17': 5})
    cfg = mhp_tree.config(tmp_path / 'data', [], mhp_tree.SOFTMAX_YAML)
    torch.manual_seed(0)
    model = pose_hrnet_softmax.get_pose_net(cfg, is_train=False)
    ckpt = str(tmp_path / 'random.pth.tar')
    torch.save({'state_dict': model.state_dict(), 'epoch': 0}, ckpt)
    for extra, sub in ((['--triangulation', 'ransac'], 'all_pairs'),
                       (['--triangulation', 'ransac', '--ransac_iters', '10', '--seed', '3', '--ransac_epsilon', '10'],
                        'sampled')):
        out = str(tmp_path / sub)
        r = _tool(['--model_path', ckpt] + extra, tmp_path / 'data', out)
        log = r.stdout + r.stderr
        assert r.returncode == 0, log[-4000:]
        assert 'fps:' in log and '3D pose EPE:' in log and '3D PCKAUC:' in log, log[-2000:]
        assert 'RANSAC inlier views per joint:' in log and 'dropped per camera: cam1' in log, log[-2000:]
        res = os.path.join(out, 'eval3D_results_' + cfg.EXP_NAME)
        pck3d = np.loadtxt(os.path.join(res, 'PCK3d.txt'))
        pck2d = np.loadtxt(os.path.join(res, 'PCK2d.txt'))
        assert pck3d.shape == (2, 50) and np.array_equal(pck3d[0], np.arange(1, 51))
        assert pck2d.shape == (2, 49) and np.array_equal(pck2d[0], np.arange(1, 50))
        assert np.loadtxt(os.path.join(res, 'mse2d_each_joint.txt')).shape == (21,)
        assert np.loadtxt(os.path.join(res, 'mse3d_each_joint.txt')).shape == (21,)
        share = np.loadtxt(os.path.join(res, 'ransac_inliers.txt'))
        assert share.shape == (4, 21) and (share >= 0).all() and (share <= 1).all()
        assert (share.sum(0) >= 2 - 1e-9).all()             # a final set has two views or more
    # the default lifting is the DLT of before: no inlier line, no inlier file
    out = str(tmp_path / 'dlt')
    r = _tool(['--model_path', ckpt], tmp_path / 'data', out)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert 'fps:' in log and 'RANSAC' not in log
    res = os.path.join(out, 'eval3D_results_' + cfg.EXP_NAME)
    assert os.path.exists(os.path.join(res, 'PCK3d.txt'))
    assert not os.path.exists(os.path.join(res, 'ransac_inliers.txt'))
    # the refinement is refused before any device work
    r = _tool(['--triangulation', 'ransac', 'MODEL.DIRECT_OPTIMIZATION', 'True'], tmp_path / 'data', out)
    assert r.returncode != 0 and 'DIRECT_OPTIMIZATION true is not built' in r.stderr, r.stderr[-2000:]
