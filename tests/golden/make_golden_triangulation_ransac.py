"""Writes tests/golden/triangulation_ransac.npz: the reference's own RANSAC triangulation on fixed inputs, for
tests/test_triangulate_ransac_cpu.py and tests/test_triangulate_ransac_gpu.py.

    python tests/golden/make_golden_triangulation_ransac.py <reference checkout>

Runs the reference's lib/utils/misc.py triangulate_ransac (n_iters 10, reprojection_error_epsilon 25, the value
RANSACTriangulationNet.forward passes, direct_optimization False) point by point. misc.py imports matplotlib and
models.triangulation_model_utils.multiview: stub modules stand in for matplotlib and the `models` packages, and both
reference files are loaded by path. random.sample is wrapped while the reference runs, so that the pairs it actually
drew are recorded: random.seed(SEED of the case) once per case, then the points in (b, k) order.

Cases, for the wide and the near-parallel rig and the point generator of make_golden_triangulation.py, B = 4, K = 21,
1 px noise on every 2-D point:
- <rig>_v4_one:  V = 4, one view of every point displaced by 60-120 px per axis (either sign);
- <rig>_v4_none: V = 4, no outlier;
- <rig>_v4_two:  V = 4, two views of every point displaced;
- <rig>_v3_one, <rig>_v3_none: the first three cameras.
Stored per case: _proj (B, V, 3, 4), _pts (B, V, K, 2) float32 (triangulated from exactly those values), _world,
_bad (B, K, V) the displaced views, _pairs (B * K, 10, 2) the recorded draws, _seed, _X (B, K, 3) float64 and
_mask (B, K, V) the reference's inlier list. epsilon and n_iters are stored once.

No case may sit on the threshold: for every recorded draw of every point, the reprojection error of every view outside
the drawn pair (the reference's own two-view DLT and calc_reprojection_error_matrix) is at least GAP away from epsilon,
asserted below. If a seed gives a closer case, change SEED0; do not drop the case."""
import importlib.util
import os
import random
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_triangulation import near_rig, project, wide_rig, world_points  # noqa: E402

B, K = 4, 21
N_ITERS, EPSILON = 10, 25
GAP = 1e-3
SEED0 = 20261016


def load_reference(ref_root):
    """the reference's multiview.py and misc.py by path, with stubs for what misc.py imports and does not need here"""
    def by_path(name, *parts):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, *parts))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    for name in ('matplotlib', 'matplotlib.pyplot', 'models', 'models.triangulation_model_utils'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['matplotlib'].pyplot = sys.modules['matplotlib.pyplot']
    mv = by_path('models.triangulation_model_utils.multiview', 'lib', 'models', 'triangulation_model_utils',
                 'multiview.py')
    sys.modules['models'].triangulation_model_utils = sys.modules['models.triangulation_model_utils']
    sys.modules['models.triangulation_model_utils'].multiview = mv
    return mv, by_path('ref_misc', 'lib', 'utils', 'misc.py')


def displace(rng, pts, n_bad):
    """pts (B, V, K, 2): n_bad views of every point moved by 60-120 px per axis -> (pts, bad (B, K, V))"""
    Bn, V, Kn = pts.shape[:3]
    bad = np.zeros((Bn, Kn, V), bool)
    for b in range(Bn):
        for k in range(Kn):
            for v in rng.choice(V, n_bad, replace=False):
                bad[b, k, v] = True
                pts[b, v, k] += rng.uniform(60, 120, 2) * rng.choice([-1.0, 1.0], 2)
    return pts, bad


def main(ref_root):
    mv, misc = load_reference(ref_root)
    rng = np.random.default_rng(SEED0)
    out = {'epsilon': np.float64(EPSILON), 'n_iters': np.int64(N_ITERS)}
    drawn = []
    real_sample = random.sample

    def recording_sample(population, k):
        got = real_sample(population, k)
        drawn.append(sorted(got))
        return got

    smallest_gap = {}
    case_no = 0
    for rig_name, rig in (('wide', wide_rig()), ('near', near_rig())):
        for V, n_bad, tag in ((4, 1, 'one'), (4, 0, 'none'), (4, 2, 'two'), (3, 1, 'one'), (3, 0, 'none')):
            name = '{}_v{}_{}'.format(rig_name, V, tag)
            seed = SEED0 + case_no
            case_no += 1
            world = world_points(rng, B * K).reshape(B, K, 3)
            proj = np.broadcast_to(rig[:V], (B, V, 3, 4)).copy()
            pts = np.stack([project(proj[b], world[b]) for b in range(B)])                     # B V K 2
            pts = pts + rng.normal(0, 1.0, pts.shape)
            pts, bad = displace(rng, pts, n_bad)
            pts = pts.astype(np.float32)
            X = np.empty((B, K, 3))
            mask = np.zeros((B, K, V), bool)
            del drawn[:]
            random.seed(seed)
            random.sample = recording_sample
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore', DeprecationWarning)     # random.sample of a set (the reference's)
                    for b in range(B):
                        for k in range(K):
                            X[b, k], inl = misc.triangulate_ransac(proj[b], pts[b, :, k].astype(np.float64),
                                                                   n_iters=N_ITERS,
                                                                   reprojection_error_epsilon=EPSILON,
                                                                   direct_optimization=False)
                            mask[b, k, inl] = True
            finally:
                random.sample = real_sample
            pairs = np.array(drawn, np.int8).reshape(B * K, N_ITERS, 2)
            # the condition on the inputs: nothing sits on the threshold
            gap = np.inf
            for b in range(B):
                for k in range(K):
                    p2 = pts[b, :, k].astype(np.float64)
                    for i, j in pairs[b * K + k]:
                        x2 = misc.DLT(p2[[i, j], np.newaxis], proj[b][[i, j]])
                        err = mv.calc_reprojection_error_matrix(x2, p2, proj[b])[0]
                        others = [v for v in range(V) if v not in (i, j)]
                        gap = min(gap, np.abs(err[others] - EPSILON).min())
            assert gap >= GAP, '{}: a view is {} from the threshold; change SEED0'.format(name, gap)
            smallest_gap[name] = gap
            out[name + '_proj'] = proj
            out[name + '_pts'] = pts
            out[name + '_world'] = world
            out[name + '_bad'] = bad
            out[name + '_pairs'] = pairs
            out[name + '_seed'] = np.int64(seed)
            out[name + '_X'] = X
            out[name + '_mask'] = mask
            print('{}: smallest gap to epsilon {:.4f}; inlier views {:.3f}; exact clean set on {} of {}'.format(
                name, gap, mask.sum(-1).mean(), int((mask == ~bad).all(-1).sum()), B * K))
    path = os.path.join(HERE, 'triangulation_ransac.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '/path/to/reference')
