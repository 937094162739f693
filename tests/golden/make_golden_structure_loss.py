"""Reference pins for the hand-structure losses (build container only).

    python tests/golden/make_golden_structure_loss.py      # writes tests/golden/structure_loss.npz

BoneLengthLoss and JointAngleLoss (lib/core/loss.py:150-223) and scale_pose2d (lib/utils/transforms.py:146-175) are
executed FROM the reference's own files on the CPU. Neither module can be imported as a whole (utils.transforms pulls
in cv2, which this image does not have), so the three definitions are compiled out of the files with ast, as
tests/golden/make_golden_inference.py does, into a namespace that holds torch and torch.nn.

The losses are called as the reference's AverageMeter.computeLosses calls them (lib/core/function.py:1352-1373):
both poses through scale_pose2d, the bone loss on columns 0:2, the angle loss on the scaled prediction padded with
z = 0. The `raw` case calls the two modules on the poses as given (no scale_pose2d).

Stored per case <c>: <c>_pred, <c>_gt (float32 inputs), <c>_normalize, and for q in bone, angle (scalars) and dbone,
dangle (autograd gradients with respect to the UNSCALED pred, B x 21 x 2):
    <c>_<q>        the reference in float64 on the float32 inputs
    <c>_<q>_f32    the reference in float32 (only sizes the tolerance)
    <c>_<q>_dev    max |f32 - f64| over the elements finite in both, relative to the max-abs of the finite f64 ones
    <c>_<q>_nonfinite   element by element: the float64 value is NaN or +-inf
Only data is stored.
"""
import ast
import os

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('HRNET_REFERENCE', '/root/reference')


def load_definitions(path, names, ns):
    tree = ast.parse(open(path).read())
    defs = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert len(defs) == len(names), (path, names)
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, 'exec'), ns)
    return ns


def poses(b):
    """hand-like poses at heat-map scale: wrist uniform in [22, 42)^2, every joint = wrist + N(0, 6^2)"""
    wrist = 22.0 + 20.0 * torch.rand(b, 1, 2)
    return (wrist + 6.0 * torch.randn(b, 21, 2)).float()


def reference(ns, pred32, gt32, normalize, dtype):
    """(bone, angle, dbone, dangle) of the reference code in `dtype`"""
    pred = torch.from_numpy(pred32).to(dtype).requires_grad_(True)
    gt = torch.from_numpy(gt32).to(dtype)
    if normalize:
        p, g = ns['scale_pose2d'](pred), ns['scale_pose2d'](gt)
    else:
        p, g = pred, gt
    bone = ns['BoneLengthLoss']()(p[:, :, 0:2], g[:, :, 0:2])
    zeros = torch.zeros((p.shape[0], p.shape[1], 1), dtype=dtype)
    angle = ns['JointAngleLoss']()(torch.cat((p[:, :, 0:2], zeros), dim=2))
    out = []
    for l in (bone, angle):
        if isinstance(l, torch.Tensor) and l.requires_grad:
            out.append(torch.autograd.grad(l, pred, retain_graph=True)[0].numpy().astype(np.float64))
        else:                                   # no branch of the angle loss was taken: a Python float
            out.append(np.zeros(pred32.shape[:2] + (2,)))
    return float(bone), float(angle), out[0], out[1]


def main():
    ns = load_definitions(os.path.join(REF, 'lib/utils/transforms.py'), ('scale_pose2d',), {'torch': torch, 'nn': nn})
    load_definitions(os.path.join(REF, 'lib/core/loss.py'), ('BoneLengthLoss', 'JointAngleLoss'), ns)

    torch.manual_seed(0)
    cases = {}
    pred6, gt6 = poses(6).numpy(), poses(6).numpy()
    cases['b6'] = (pred6, gt6, True)
    cases['b1'] = (poses(1).numpy(), poses(1).numpy(), True)
    cases['b70'] = (poses(70).numpy(), poses(70).numpy(), True)
    vis = (torch.rand(6, 21, 1) > 0.3).float().numpy()
    cases['b6_vis'] = (pred6, np.concatenate([gt6, vis], axis=2), True)
    p = pred6.copy()
    p[0, 3] = p[0, 2]
    cases['zero_bone'] = (p, gt6, True)
    p = pred6.copy()
    p[1, 9] = p[1, 0]
    cases['zero_scale'] = (p, gt6, True)
    cases['raw'] = (pred6, gt6, False)

    out = {}
    for name, (pred, gt, normalize) in cases.items():
        r64 = reference(ns, pred, gt, normalize, torch.float64)
        r32 = reference(ns, pred, gt, normalize, torch.float32)
        out[name + '_pred'], out[name + '_gt'], out[name + '_normalize'] = pred, gt, np.array(normalize)
        for q, a, b in zip(('bone', 'angle', 'dbone', 'dangle'), r64, r32):
            a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
            fin = np.isfinite(a)
            both = fin & np.isfinite(b)
            scale = np.abs(a[fin]).max() if fin.any() else 1.0
            dev = np.abs(a[both] - b[both]).max() / scale if both.any() and scale > 0 else 0.0
            out['{}_{}'.format(name, q)], out['{}_{}_f32'.format(name, q)] = a, b
            out['{}_{}_dev'.format(name, q)] = np.array(dev)
            out['{}_{}_nonfinite'.format(name, q)] = ~fin
        print('{:10s} bone {:.6g} angle {:.6g} dev {}'.format(name, r64[0], r64[1], ' '.join(
            '{:.1e}'.format(float(out['{}_{}_dev'.format(name, q)])) for q in ('bone', 'angle', 'dbone', 'dangle'))))
    # what the cases are there for
    b6 = cases['b6']
    per_sample = [reference(ns, b6[0][i:i + 1], b6[1][i:i + 1], True, torch.float64)[1] for i in range(6)]
    print('b6 angle loss per sample', ['{:.3g}'.format(v) for v in per_sample])
    assert all(v > 0 for v in per_sample), 'every sample of b6 takes a d < 0 branch'
    for q in ('bone', 'angle', 'dbone', 'dangle'):
        assert np.array_equal(out['b6_vis_' + q], out['b6_' + q]), 'the visibility column changes nothing'
        assert not out['zero_bone_{}_nonfinite'.format(q)].any(), 'a zero-length bone keeps everything finite'
    assert out['zero_scale_bone_nonfinite'] and out['zero_scale_angle_nonfinite']
    for q in ('dbone', 'dangle'):
        m = out['zero_scale_{}_nonfinite'.format(q)]
        assert m[1].all() and not m[[0, 2, 3, 4, 5]].any(), 'only the degenerate sample has non-finite gradients'
    path = os.path.join(HERE, 'structure_loss.npz')
    np.savez_compressed(path, **out)
    print('structure_loss.npz', os.path.getsize(path), len(out), 'arrays')


if __name__ == '__main__':
    main()
