"""Host side of the RANSAC triangulation (hrnet_triangulate_ransac in csrc/triangulate.hip, utils/multiview.py,
tools/evaluate_3D.py --triangulation ransac): the float64 numpy restatement of the kernel's rule
(tests/triangulate_ransac_ref.py) against the reference's own triangulate_ransac results in
tests/golden/triangulation_ransac.npz (tests/golden/make_golden_triangulation_ransac.py) - the inlier mask exactly, X to
the 1e-6 relative of the GPU tests; the C ABI entry; sample_view_pairs against the draws the reference made; the
argument checks of the Python surface and of the tool."""
import os
import sys

import numpy as np
import pytest

import triangulate_ransac_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'triangulation_ransac.npz')
PKG = os.path.join(os.path.dirname(HERE), 'hrnet-hand-pose-estimation_amd')
RTOL = 1e-6                 # RTOL of tests/test_triangulate_gpu.py
CASES = ['{}_v{}_{}'.format(rig, v, tag) for rig in ('wide', 'near')
         for v, tag in ((4, 'one'), (4, 'none'), (4, 'two'), (3, 'one'), (3, 'none'))]


def _rel(X, ref):
    return np.linalg.norm(X - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


def test_fixture_covers_the_cases():
    z = np.load(GOLD)
    assert sorted(k[:-2] for k in z.files if k.endswith('_X')) == sorted(CASES)
    assert float(z['epsilon']) == 25 and int(z['n_iters']) == 10
    for name in CASES:
        V, n_bad = int(name.split('_v')[1][0]), {'one': 1, 'none': 0, 'two': 2}[name.rsplit('_', 1)[1]]
        assert z[name + '_pts'].shape == (4, V, 21, 2) and z[name + '_pts'].dtype == np.float32
        assert z[name + '_pairs'].shape == (84, 10, 2) and z[name + '_mask'].shape == (4, 21, V)
        assert (z[name + '_bad'].sum(-1) == n_bad).all()
        assert (z[name + '_mask'].sum(-1) >= 2).all()
        pairs = z[name + '_pairs']
        assert (pairs[..., 0] < pairs[..., 1]).all() and pairs.min() >= 0 and pairs.max() < V
    assert os.path.getsize(GOLD) < 200 * 1024


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_the_reference(name):
    z = np.load(GOLD)
    X, mask = RR.triangulate_ransac_batch(z[name + '_proj'], z[name + '_pts'], z[name + '_pairs'], float(z['epsilon']))
    assert np.array_equal(mask, z[name + '_mask'])
    rel = _rel(X, z[name + '_X'])
    print(name, 'largest relative error', rel.max())
    assert rel.max() <= RTOL


def test_restatement_rule_details():
    z = np.load(GOLD)
    name = 'wide_v4_one'
    proj, pts = z[name + '_proj'][0], z[name + '_pts'][0, :, 0].astype(np.float64)
    import triangulate_ref as T
    # no usable pair: every view; epsilon = inf: every view; epsilon = 0 with one pair: that pair
    for table in (np.zeros((0, 2), int), [[1, 1]], [[0, 4]], [[-1, 2]]):
        X, m = RR.triangulate_ransac(proj, pts, table, 25.0)
        assert m.all() and np.array_equal(X, T.triangulate(proj, pts)[0])
    X, m = RR.triangulate_ransac(proj, pts, [[0, 1], [2, 3]], np.inf)
    assert m.all()
    X, m = RR.triangulate_ransac(proj, pts, [[1, 3]], 0.0)
    assert m.tolist() == [False, True, False, True] and np.array_equal(X, T.triangulate(proj[[1, 3]], pts[[1, 3]])[0])
    # a non-finite point is not hidden by dropping its view
    bad = pts.copy()
    bad[0, 0] = np.nan
    X, m = RR.triangulate_ransac(proj, bad, [[0, 1], [1, 2], [2, 3]], 25.0)
    assert np.isnan(X).all() and not m[0]
    # the first largest set wins: two disjoint pairs at epsilon 0 keep the first
    X, m = RR.triangulate_ransac(proj, pts, [[2, 3], [0, 1]], 0.0)
    assert m.tolist() == [False, False, True, True]


def test_c_abi_entry_point():
    from hipnet import _capi
    header = open(os.path.join(os.path.dirname(_capi.LIB_PATH), '..', '..', 'include', 'hrnet_hip.h')).read()
    assert 'int hrnet_triangulate_ransac(const float* pts, const double* to_frame, const double* proj, ' \
           'const int* pairs, int n_hyp,' in header
    assert 'hrnet_triangulate_ransac' in _capi.EXPORTED and 'hrnet_triangulate' in _capi.EXPORTED
    assert _capi.ABI_VERSION == 2
    assert hasattr(_capi.lib(), 'hrnet_triangulate_ransac')      # loads without a GPU; nothing is launched


@pytest.mark.parametrize('name', CASES)
def test_sample_view_pairs_reproduces_the_recorded_draws(name):
    from utils.multiview import sample_view_pairs
    z = np.load(GOLD)
    rec = z[name + '_pairs']
    V = z[name + '_pts'].shape[1]
    got = sample_view_pairs(rec.shape[0], V, rec.shape[1], int(z[name + '_seed']))
    assert tuple(got.shape) == rec.shape and np.array_equal(got.numpy(), rec)


def test_view_pair_helpers():
    import random

    import torch
    from utils.multiview import all_view_pairs, sample_view_pairs
    assert all_view_pairs(4).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert all_view_pairs(4).dtype == torch.int32 and tuple(all_view_pairs(8).shape) == (28, 2)
    whole = sample_view_pairs(6, 4, 10, 5)
    rng = random.Random(5)
    parts = torch.cat([sample_view_pairs(2, 4, 10, rng) for _ in range(3)])
    assert torch.equal(whole, parts)                  # a generator continues its stream, batch after batch
    with pytest.raises(ValueError, match='n_views'):
        sample_view_pairs(1, 1, 10, 0)


def test_python_surface_checks_its_arguments():
    import torch
    from utils.multiview import triangulate_ransac_batch
    proj, pts = torch.zeros(2, 4, 3, 4), torch.zeros(2, 4, 21, 2)
    with pytest.raises(RuntimeError, match='HIP-device'):
        triangulate_ransac_batch(proj, pts)
    with pytest.raises(ValueError, match='points_batch'):
        triangulate_ransac_batch(proj, pts[..., :1])
    with pytest.raises(ValueError, match='proj_matricies_batch'):
        triangulate_ransac_batch(proj[:, :3], pts)
    with pytest.raises(ValueError, match='to_frame'):
        triangulate_ransac_batch(proj, pts, to_frame=torch.zeros(2, 2, 3))
    with pytest.raises(ValueError, match='pairs'):
        triangulate_ransac_batch(proj, pts, pairs=torch.zeros(6, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match='pairs'):
        triangulate_ransac_batch(proj, pts, pairs=torch.zeros(41, 6, 2, dtype=torch.int32))    # B * K is 42
    with pytest.raises(ValueError, match='pairs'):
        triangulate_ransac_batch(proj, pts, pairs=torch.zeros(6, 2))                           # float indices
    with pytest.raises(ValueError, match='hypotheses'):
        triangulate_ransac_batch(proj, pts, pairs=torch.zeros(65, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match='NaN'):
        triangulate_ransac_batch(proj, pts, reprojection_error_epsilon=float('nan'))


@pytest.fixture()
def tool():
    sys.path.insert(0, os.path.join(PKG, 'tools'))
    try:
        import evaluate_3D
        yield evaluate_3D
    finally:
        sys.path.remove(os.path.join(PKG, 'tools'))


def test_tool_parser_takes_the_ransac_flags(tool, capsys):
    a = tool.parse_args(['--cfg', 'x.yaml'])
    assert (a.triangulation, a.ransac_epsilon, a.ransac_iters, a.seed) == ('dlt', 25.0, 0, 0)
    a = tool.parse_args(['--cfg', 'x.yaml', '--triangulation', 'ransac', '--ransac_epsilon', '12.5', '--ransac_iters',
                         '10', '--seed', '7', 'WORKERS', '0'])
    assert (a.triangulation, a.ransac_epsilon, a.ransac_iters, a.seed) == ('ransac', 12.5, 10, 7)
    assert a.opts == ['WORKERS', '0']
    for bad in (['--triangulation', 'lmeds'], ['--ransac_iters', '-1'], ['--ransac_iters', '65'],
                ['--ransac_epsilon', 'nan']):
        with pytest.raises(SystemExit):
            tool.parse_args(['--cfg', 'x.yaml'] + bad)
    assert 'invalid choice' in capsys.readouterr().err


def test_tool_refuses_direct_optimization_with_ransac(tool):
    import mhp_tree
    cfg = mhp_tree.config('/nonexistent', ['MODEL.DIRECT_OPTIMIZATION', 'True'], mhp_tree.SOFTMAX_YAML)
    with pytest.raises(ValueError, match='DIRECT_OPTIMIZATION'):
        tool.check_lifting(tool.parse_args(['--cfg', 'x.yaml', '--triangulation', 'ransac']), cfg)
    tool.check_lifting(tool.parse_args(['--cfg', 'x.yaml']), cfg)            # dlt never reads it, as today
    off = mhp_tree.config('/nonexistent', [], mhp_tree.SOFTMAX_YAML)
    tool.check_lifting(tool.parse_args(['--cfg', 'x.yaml', '--triangulation', 'ransac']), off)
    # the refused model keeps its error and names the flag
    with pytest.raises(ValueError, match='is not built.*--triangulation ransac'):
        tool.build_model('ransac')
