"""Reference pins for the geometry of the RHD reader (lib/dataset/rhd.py; build container only).

    python tests/golden/make_golden_rhd.py      # writes tests/golden/rhd_geometry.npz

The code that runs is the reference's own, compiled out of its files with ast (as make_golden_inference.py does):
RHDDataset.__getitem__ (lib/dataset/RHDDataset.py:58-124: hand choice, crop arithmetic, corner shift, idx_RHD
reorder), RandomAffineTransform (lib/dataset/transforms/transforms.py:74-175: _get_affine_matrix, _affine_joints,
__call__) and RandomHorizontalFlip (:54-71), with idx_RHD from lib/dataset/standard_legends.py. The modules cannot
be imported (cv2, kornia and matplotlib are absent), so they run in a namespace whose `cv2` only hands back given
arrays: imread returns a zero image of the stated size, cvtColor its input, warpAffine a zero image of the output
size and records the matrix it was passed. np.random and random are replaced by stubs that return fixed draws
(the two uniforms behind aug_scale and the rotation, dx / dy, the flip's uniform) and record randint's bounds.

What that pins: corner, crop_size, the reordered joints and the visibility of each fixture annotation, and per
augmentation case both matrices (IMAGE_SIZE and HEATMAP_SIZE) and the transformed joints. The pixels of
cv2.warpAffine are not pinned. Only inputs and outputs are stored.
"""
import ast
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('HRNET_REFERENCE', '/root/reference')
IMG_H, IMG_W, INPUT, HM = 320, 320, 256, 64
SCALE_TYPES = ('short', 'long')
# augmentation cases: max_rotation, min_scale, max_scale, max_translate, scale type (index), flip probability
CASES = np.array([[0, 1, 1, 0, 0, 0],               # evaluation / no WITH_DATA_AUG: crop -> IMAGE_SIZE
                  [30, 0.75, 1.25, 40, 0, 0],       # the config defaults, no flip
                  [30, 0.75, 1.25, 40, 0, 1],       # ... flipped (the shipped yaml's FLIP: true)
                  [45, 0.65, 1.35, 20, 1, 1]])      # another range, SCALE_TYPE long


def _class_or_function(path, names, ns):
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(nodes) == len(names), (path, names)
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), ns)


def _method(path, cls, name, ns):
    tree = ast.parse(open(path).read())
    c = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls][0]
    fn = [n for n in c.body if isinstance(n, ast.FunctionDef) and n.name == name]
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, 'exec'), ns)
    return ns[name]


def _assignment(path, name):
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.Assign) and any(getattr(t, 'id', None) == name for t in n.targets)]
    ns = {}
    exec(compile(ast.Module(body=node, type_ignores=[]), path, 'exec'), ns)
    return ns[name]


class _Draws(object):
    """np.random / random stand-in: random() pops the queued uniforms, randint draws from its own generator and
    records the bounds the reference computed"""

    def __init__(self, seed):
        self.queue, self.bounds, self.drawn, self.rng = [], [], [], np.random.RandomState(seed)

    def random(self):
        return self.queue.pop(0)

    def randint(self, lo, hi):
        self.bounds.append((lo, hi))
        self.drawn.append(int(self.rng.randint(int(lo), int(hi))))
        return self.drawn[-1]


def _annotations():
    """42 x 3 uv_vis (float32, as RHD's pickles): left hand visible, right hand visible, a tie, hands at the four
    image edges, a hand larger than half the image, a small one"""
    rng = np.random.RandomState(5)
    out = []

    def hand(cx, cy, span, nvis):
        uv = np.stack([cx + (rng.rand(21) - 0.5) * span, cy + (rng.rand(21) - 0.5) * span * 0.8], 1)
        vis = np.zeros(21)
        vis[rng.permutation(21)[:nvis]] = 1
        return np.concatenate([uv, vis[:, None]], 1)

    for left, right in (((160, 150, 90, 18), (60, 60, 70, 5)),          # left hand
                        ((200, 100, 80, 4), (140, 170, 100, 15)),       # right hand
                        ((100, 200, 60, 10), (220, 90, 75, 10)),        # a tie -> left
                        ((8, 12, 70, 21), (200, 200, 50, 3)),           # left / top edge (some u, v < 0)
                        ((312, 310, 80, 20), (100, 100, 50, 2)),        # right / bottom edge (some u, v > 320)
                        ((150, 40, 120, 0), (30, 300, 90, 1)),          # top-right hand chosen, bottom-left edge
                        ((160, 160, 230, 12), (50, 50, 30, 12)),        # crop_size clipped to the image width
                        ((70, 250, 9, 16), (250, 60, 40, 3))):          # a small crop
        out.append(np.concatenate([hand(*left), hand(*right)]).astype(np.float32))
    return np.stack(out)


def main():
    ds = os.path.join(REF, 'lib/dataset')
    idx_rhd = _assignment(os.path.join(ds, 'standard_legends.py'), 'idx_RHD')
    flip_index = _assignment(os.path.join(ds, 'transforms/build.py'), 'FLIP_CONFIG')['RHD']
    warped = []
    cv2 = types.SimpleNamespace(IMREAD_COLOR=1, IMREAD_IGNORE_ORIENTATION=128, COLOR_BGR2RGB=4,
                                imread=lambda path, flags: np.zeros((IMG_H, IMG_W, 3), np.uint8),
                                cvtColor=lambda img, code: img,
                                warpAffine=lambda img, m, size: (warped.append(np.array(m)),
                                                                 np.zeros((size[1], size[0], 3), np.uint8))[1])
    draws = _Draws(9)
    np_stub = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith('__')})
    np_stub.random = draws
    get_item = _method(os.path.join(ds, 'RHDDataset.py'), 'RHDDataset', '__getitem__',
                       {'np': np, 'os': os, 'cv2': cv2})
    tns = {'np': np_stub, 'cv2': cv2, 'random': types.SimpleNamespace(random=lambda: 0.5)}
    _class_or_function(os.path.join(ds, 'transforms/transforms.py'),
                       ('RandomAffineTransform', 'RandomHorizontalFlip'), tns)

    uv_vis = _annotations()
    n, nc = len(uv_vis), len(CASES)
    out = {'uv_vis': uv_vis, 'img_hw': np.array([IMG_H, IMG_W]), 'sizes': np.array([INPUT, HM]), 'cases': CASES}
    corner, crop, pose2d, vis = [], [], [], []
    u = np.random.RandomState(3).rand(n, nc, 2)
    mats_in, mats_out, joints, dxy, bounds, flip = [], [], [], [], [], []
    for i in range(n):
        me = types.SimpleNamespace(data_dir='', images=['{:05d}.png'.format(j) for j in range(n)],
                                   anno_all={j: {'uv_vis': uv_vis[j]} for j in range(n)}, reorder_idx=idx_rhd,
                                   transform=None)
        ret = get_item(me, i)
        corner.append(ret['corner'])
        crop.append(ret['crop_size'])
        pose2d.append(ret['pose2d'])
        vis.append(ret['visibility'])
        for c, (max_rot, min_s, max_s, max_t, st, prob) in enumerate(CASES):
            t = tns['RandomAffineTransform'](INPUT, HM, max_rot, min_s, max_s, SCALE_TYPES[int(st)], max_t)
            f = tns['RandomHorizontalFlip'](flip_index, HM, bool(prob))
            seen = []
            plain = t._affine_joints
            t._affine_joints = lambda j, m: (seen.append(np.array(m)), plain(j, m))[1]
            draws.queue, draws.bounds, draws.drawn = list(u[i, c]), [], []
            img, j = t(ret['imgs'], [np.array(ret['pose2d'], dtype=np.float64)])
            img, j = f(img, j)
            assert not draws.queue and len(seen) == 1 and img.shape == (INPUT, INPUT, 3)
            mats_in.append(warped.pop())
            mats_out.append(seen[0])
            joints.append(j[0])
            b = draws.bounds
            assert len(b) in (0, 2) and (not b or b[0] == b[1])
            dxy.append(draws.drawn if b else [0, 0])
            bounds.append(b[0] if b else (0, 0))
            flip.append(bool(prob))
    out.update(corner=np.array(corner, dtype=np.int64), crop_size=np.array(crop, dtype=np.int64),
               pose2d=np.stack(pose2d), visibility=np.stack(vis), u=u,
               dxy=np.array(dxy, dtype=np.int64).reshape(n, nc, 2),
               translate_bounds=np.array(bounds, dtype=np.float64).reshape(n, nc, 2),
               flip=np.array(flip).reshape(n, nc),
               mat_input=np.stack(mats_in).reshape(n, nc, 2, 3), mat_output=np.stack(mats_out).reshape(n, nc, 2, 3),
               joints=np.stack(joints).reshape(n, nc, 21, 2))
    path = os.path.join(HERE, 'rhd_geometry.npz')
    np.savez_compressed(path, **out)
    print('wrote {} ({} bytes)'.format(path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
