"""3-D evaluation on the output side of tools/evaluate_3D.py (reference tools/evaluate_3D.py:251-257 accumulators,
:377-407 metrics and result files, :121,134 AUC): per-joint 3-D end-point error and PCK at 1..50 mm over the valid
samples, next to the 2-D metrics of core/evaluate2d.py, written in the reference's formats so that its committed
tools/eval3D_results_*/ files are format targets."""
import os

import numpy as np

from core.evaluate2d import Eval2DAccumulator

VALID_SHARE = 0.65          # a sample counts when at least this share of its V * K joints is visible (:391)


def auc(th, pck):
    """the reference's trapezoid area under a PCK curve, normalised by the threshold range (:121,134)"""
    th, pck = np.asarray(th, dtype=np.float64), np.asarray(pck, dtype=np.float64)
    return (pck[0] + 2 * pck[1:-1].sum() + pck[-1]) * (th[1] - th[0]) / 2 / (th[-1] - th[0])


class Eval3DAccumulator(object):
    """running sums of tools/evaluate_3D.py:251-257,377-407: the 2-D part is an Eval2DAccumulator fed through each
    image's heat-map inverse; the 3-D part sums, over valid samples, the per-joint error ||X - X_gt|| and the count of
    joints with an error strictly below each threshold 1..50"""

    def __init__(self, n_joints, hm_size):
        self.K = n_joints
        self.acc2d = Eval2DAccumulator(n_joints, hm_size)
        self.th = np.arange(1, 51)
        self.pck = np.zeros(len(self.th))
        self.mse = np.zeros(n_joints)
        self.n_valid = 0

    def add(self, pred2d, gt2d, visibility, inverse, pred3d, gt3d):
        """pred2d / gt2d (B*V, K, 2) heat-map pixels, slot b * V + v; visibility (B*V, K[, 1]); inverse (B*V, 2, 3)
        heat-map pixel -> frame pixel; pred3d / gt3d (B, K, 3)"""
        self.acc2d.add(pred2d, gt2d, visibility, inverse=inverse)
        pred3d = np.asarray(pred3d, dtype=np.float64)
        gt3d = np.asarray(gt3d, dtype=np.float64)
        B = pred3d.shape[0]
        vis = np.asarray(visibility, dtype=np.float64).reshape(B, -1)
        valid = vis.sum(1) >= vis.shape[1] * VALID_SHARE
        each = np.linalg.norm(pred3d[valid] - gt3d[valid], axis=2)          # n_valid x K
        self.n_valid += int(valid.sum())
        self.mse += each.sum(0)
        self.pck += (each[None] < self.th[:, None, None]).sum((1, 2))

    def result(self):
        """(mse2d (K,), PCK2d (2, 49), mse3d (K,), PCK3d (2, 50)); no valid sample gives nan, as the reference"""
        mse2d, pck2d = self.acc2d.result()
        with np.errstate(invalid='ignore', divide='ignore'):
            mse3d = self.mse / self.n_valid
            pck3d = self.pck / (self.n_valid * self.K)
        return mse2d, pck2d, mse3d, np.stack((self.th, pck3d))

    def save(self, out_dir):
        os.makedirs(out_dir, exist_ok=True)
        mse2d, pck2d, mse3d, pck3d = self.result()
        np.savetxt(os.path.join(out_dir, 'mse2d_each_joint.txt'), mse2d, fmt='%.4f')
        np.savetxt(os.path.join(out_dir, 'mse3d_each_joint.txt'), mse3d, fmt='%.4f')
        np.savetxt(os.path.join(out_dir, 'PCK2d.txt'), pck2d)
        np.savetxt(os.path.join(out_dir, 'PCK3d.txt'), pck3d)
        return mse2d, pck2d, mse3d, pck3d
