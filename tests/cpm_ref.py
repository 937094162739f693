"""Restatement of the reference's Convolutional Pose Machine (lib/models/CPM.py:6-170) as a table-driven walk over a state
dict with torch's CPU ops, in the dtype of its inputs: the CPU yardstick of models.CPM on the HIP path. tests/golden/
make_golden_cpm.py pins it against the reference's own module in float64.

fill_state_dict(k, seed) draws every tensor from numpy.random.RandomState(seed) in SORTED key order - weights
N(0, sqrt(2 / fan_in)), biases N(0, 0.1) - so no weights are stored anywhere (they are 127 MB).

err = rel(dev, ref64) = max|dev - ref64| / max|ref64|; a device result must stay within bound(e_ref) =
4 * e_ref + 2 * 2^-24, e_ref being the same measure of a float32 CPU run (the convention of tests/swin_ref.py).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

SEED = 20261020
K_JOINTS = 21
# name -> (batch, H, W): 8x8 maps; 5x9 maps (smaller than the 11x11 halo, not square, H no multiple of 16); 1x2 maps
CASES = {'a': (2, 64, 64), 'b': (1, 40, 72), 'c': (1, 8, 16)}


def rel(a, b, denom=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() if denom is None else denom))


def bound(e_ref):
    return 4.0 * e_ref + 2.0 * 2.0 ** -24


def conv_table(k=K_JOINTS):
    """(name, Cin, Cout, ks) of the 40 convolutions in the order the reference's constructor creates them"""
    cat = 32 + k + 2
    t = [('conv1_stage1', 3, 128, 9), ('conv2_stage1', 128, 128, 9), ('conv3_stage1', 128, 128, 9),
         ('conv4_stage1', 128, 32, 5), ('conv5_stage1', 32, 512, 9), ('conv6_stage1', 512, 512, 1),
         ('conv7_stage1', 512, k + 1, 1), ('conv1_stage2', 3, 128, 9), ('conv2_stage2', 128, 128, 9),
         ('conv3_stage2', 128, 128, 9), ('conv4_stage2', 128, 32, 5)]
    for s in range(2, 7):
        if s > 2:
            t.append(('conv1_stage%d' % s, 128, 32, 5))
        t += [('Mconv1_stage%d' % s, cat, 128, 11), ('Mconv2_stage%d' % s, 128, 128, 11), ('Mconv3_stage%d' % s, 128, 128, 11),
              ('Mconv4_stage%d' % s, 128, 128, 1), ('Mconv5_stage%d' % s, 128, k + 1, 1)]
    return t


def keys_and_shapes(k=K_JOINTS):
    out = []
    for name, ci, co, ks in conv_table(k):
        out += [(name + '.weight', (co, ci, ks, ks)), (name + '.bias', (co,))]
    return out


def fill_state_dict(k=K_JOINTS, seed=SEED):
    """name -> float64 numpy array, drawn in sorted key order"""
    shapes = dict(keys_and_shapes(k))
    rng = np.random.RandomState(seed)
    state = {}
    for key in sorted(shapes):
        shape = shapes[key]
        if key.endswith('.weight'):
            state[key] = rng.standard_normal(shape) * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        else:
            state[key] = rng.standard_normal(shape) * 0.1
    return state


def to_torch(state, dtype):
    return {k: torch.tensor(v, dtype=dtype) for k, v in state.items()}


def inputs(case, seed=SEED):
    """(image, centre map) float64 numpy arrays whose values are float16 numbers: an N(0, 0.5) image and a sigma = 3
    Gaussian (clipped as the MHP_CPM reader clips it) at a drawn centre"""
    B, H, W = CASES[case]
    rng = np.random.RandomState(seed + ord(case))
    img = (rng.standard_normal((B, 3, H, W)) * 0.5).astype(np.float16)
    yy, xx = np.mgrid[0:H, 0:W]
    cm = np.empty((B, 1, H, W))
    for b in range(B):
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        g = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 2.0 / 9.0)
        g[g < 0.0099] = 0
        cm[b, 0] = g
    return img.astype(np.float64), cm.astype(np.float16).astype(np.float64)


def forward(P, image, center):
    """the six stage outputs (B, k + 1, H / 8, W / 8); P a dict of tensors in the dtype of image and center"""
    def conv(name, x, act=True):
        w = P[name + '.weight']
        y = F.conv2d(x, w, P[name + '.bias'], padding=w.shape[2] // 2)
        return F.relu(y) if act else y

    def trunk(x, stage):
        for i in (1, 2, 3):
            x = F.max_pool2d(conv('conv%d_stage%d' % (i, stage), x), 3, 2, 1)
        return x

    pooled = F.avg_pool2d(center, 9, 8, 1)
    x = trunk(image, 1)
    for i in (4, 5, 6):
        x = conv('conv%d_stage1' % i, x)
    outs = [conv('conv7_stage1', x, act=False)]
    mid = trunk(image, 2)
    for s in range(2, 7):
        x = conv('conv4_stage2' if s == 2 else 'conv1_stage%d' % s, mid)
        x = torch.cat([x, outs[-1], pooled], 1)
        for i in (1, 2, 3, 4):
            x = conv('Mconv%d_stage%d' % (i, s), x)
        outs.append(conv('Mconv5_stage%d' % s, x, act=False))
    return outs


def run(case, dtype, seed=SEED, state=None):
    """the six outputs of a case as float64 numpy arrays, computed in `dtype`"""
    state = fill_state_dict(K_JOINTS, seed) if state is None else state
    img, cm = inputs(case, seed)
    with torch.no_grad():
        outs = forward(to_torch(state, dtype), torch.tensor(img, dtype=dtype), torch.tensor(cm, dtype=dtype))
    return [o.double().numpy() for o in outs]


def keypoints(heat):
    """integer argmax key points (B, k, 2) [u, v] of the channels 1: of a (B, k + 1, H, W) map, u = idx % W, v = idx // W"""
    h = np.asarray(heat)[:, 1:]
    B, k, H, W = h.shape
    idx = h.reshape(B, k, -1).argmax(-1)
    return np.stack((idx % W, idx // W), -1)


def top_gap(heat):
    """the smallest difference between the largest and the second largest value of a joint's map, over max|heat|"""
    h = np.asarray(heat, dtype=np.float64)
    flat = np.sort(h[:, 1:].reshape(h.shape[0], h.shape[1] - 1, -1), -1)
    if flat.shape[-1] < 2:
        return float('inf')
    return float((flat[..., -1] - flat[..., -2]).min() / np.abs(h).max())
