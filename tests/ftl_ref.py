"""Restatement of the head of the reference's FTLMultiviewNet (lib/models/FTL_encoder_decoder.py:143-214, steps 2-9 of
its forward) as a walk over a state dict with torch's CPU ops, in the dtype of its inputs: the CPU yardstick of
models.FTL_encoder_decoder on the HIP path. tests/golden/make_golden_ftl.py pins it against the reference's own forward
in float64.

Every stage after the distribution is in SLOT order b * V + v (the reference stacks the views view-major, row v * B + b, and
then reads the rows as batch-major; the two agree at B = 1). The convolutions and the transform stay unfused here: eval
BatchNorm after each convolution, decoder.layer_lst.2 and final_layer as two layers.

fill_state_dict(channels, V, K, seed, kind) draws every tensor from numpy.random.RandomState(seed) in SORTED key order:
weights N(0, sqrt(2 / fan_in)), biases N(0, 0.1), BatchNorm weight U(0.5, 1.5), bias N(0, 0.1), running_mean N(0, 0.1),
running_var U(0.5, 1.5), num_batches_tracked 0; for the MHP-scale camera set the running statistics of the two BatchNorms
behind the transforms are scaled to the size of what they see there (STAT_SCALE).

err = rel(dev, ref64) = max|dev - ref64| / max|ref64|; a device result must stay within bound(e_ref) =
4 * e_ref + 2 * 2^-24, e_ref being the same measure of a float32 CPU run (the convention of tests/swin_ref.py).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

SEED = 20261021
K_JOINTS = 21
DEC = 256                      # the decoder's width, fixed in the reference
WIDE, NARROW = (8, 16, 24, 48), (4, 8, 12, 16)       # C = 96, and C = 40 whose C / 2 = 20 is no multiple of 16
MHP_INTRINSIC = np.array([[614.878, 0, 313.219], [0, 615.479, 231.288], [0, 0, 1]])
# name -> (STAGE4.NUM_CHANNELS, V, B, (h, w) of the features, camera set). Feature sizes: (4, 8) -> 3 x 4 after the encoder
# (triplets cross rows); (8, 4) -> 4 x 3 through an odd 5 x 3; (16, 16) -> 6 x 6 through 9 x 9 (a parity class with all four
# live taps, output_padding 1)
CASES = {'a': (WIDE, 4, 1, (4, 8), 'unit'), 'b': (NARROW, 3, 2, (4, 8), 'unit'), 'c': (NARROW, 4, 2, (8, 4), 'unit'),
         'd': (WIDE, 3, 1, (8, 4), 'mhp'), 'e': (NARROW, 3, 1, (16, 16), 'unit'), 'f': (NARROW, 4, 2, (4, 8), 'mhp')}
STAGES = ('encoder_head', 'fuse_after_FTL', 'channel_expansion', 'decoder', 'heatmaps')
# what the fixture keeps of a stage's channels (the whole of the others): the wide maps would not fit a committed file
KEEP = {'channel_expansion': 4, 'decoder': 32}


def rel(a, b, denom=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() if denom is None else denom))


def bound(e_ref):
    return 4.0 * e_ref + 2.0 * 2.0 ** -24


def kept(stage, y):
    """the channels of a stage's (N, C, h, w) output that the fixture records"""
    return y[:, ::KEEP[stage]] if stage in KEEP else y


def enc_size(n):
    """Conv2d(3, stride 2, padding 2): 64 -> 33 -> 18"""
    return (n + 1) // 2 + 1


def keys_and_shapes(channels, V, K=K_JOINTS):
    """the head's state-dict entries in the reference's order"""
    C = sum(channels)
    C2 = C // 2
    out = []

    def conv_bn(prefix, w_shape, co):
        out.extend([(prefix + '.0.weight', w_shape), (prefix + '.0.bias', (co,)), (prefix + '.1.weight', (co,)),
                    (prefix + '.1.bias', (co,)), (prefix + '.1.running_mean', (co,)), (prefix + '.1.running_var', (co,)),
                    (prefix + '.1.num_batches_tracked', ())])

    conv_bn('encoder_head.layer_lst.0', (C, C, 3, 3), C)
    conv_bn('encoder_head.layer_lst.1', (C2, C, 3, 3), C2)
    conv_bn('fuse_after_FTL.layer_lst.0', (C2, C2 * V, 1, 1), C2)
    conv_bn('fuse_after_FTL.layer_lst.1', (C2, C2, 1, 1), C2)
    conv_bn('channel_expansion.layer_lst.0', (C, C2, 1, 1), C)
    conv_bn('decoder.layer_lst.0', (C, DEC, 3, 3), DEC)             # ConvTranspose2d: (Cin, Cout, 3, 3)
    conv_bn('decoder.layer_lst.1', (DEC, DEC, 3, 3), DEC)
    out += [('decoder.layer_lst.2.weight', (DEC, DEC, 3, 3)), ('decoder.layer_lst.2.bias', (DEC,)),
            ('final_layer.weight', (K, DEC, 1, 1)), ('final_layer.bias', (K,))]
    return out


# BatchNorm statistics that fit the camera set, as trained ones would: at MHP scale the gathered features are of the order
# of |t| ~ 300 and the distributed ones of |t| f ~ 2e5; without this the final softmax saturates to one pixel per map
STAT_SCALE = {'unit': {}, 'mhp': {'fuse_after_FTL.layer_lst.0.1': 300.0, 'channel_expansion.layer_lst.0.1': 2e5}}


def fill_state_dict(channels, V, K=K_JOINTS, seed=SEED, kind='unit'):
    """name -> float64 numpy array (int64 for num_batches_tracked), drawn in sorted key order; kind: the camera set whose
    scale the running statistics of the two BatchNorms behind the transforms take (STAT_SCALE)"""
    shapes = dict(keys_and_shapes(channels, V, K))
    rng = np.random.RandomState(seed)
    state = {}
    for key in sorted(shapes):
        shape = shapes[key]
        if key.endswith('num_batches_tracked'):
            state[key] = np.zeros((), dtype=np.int64)
        elif len(shape) == 4:
            fan = shape[1] * shape[2] * shape[3]
            if key.startswith('decoder.layer_lst.') and key[18] in '01':
                fan = shape[0] * 9 / 4.0                       # a transposed stride-2 layer: 9 / 4 taps per output on average
            state[key] = rng.standard_normal(shape) * math.sqrt(2.0 / fan)
        elif key.endswith('.1.weight') or key.endswith('running_var'):
            state[key] = rng.uniform(0.5, 1.5, shape)
        else:
            state[key] = rng.standard_normal(shape) * 0.1
    for prefix, f in STAT_SCALE[kind].items():
        state[prefix + '.running_mean'] *= f
        state[prefix + '.running_var'] *= f * f
    return state


def to_torch(state, dtype):
    return {k: torch.tensor(v, dtype=torch.int64 if v.dtype == np.int64 else dtype) for k, v in state.items()}


def rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def cameras(kind, B, V, rng):
    """(extrinsic (B, V, 3, 4) = [R | t], intrinsic (3, 3)) float64. 'mhp': the data set's intrinsics, |t| of a few hundred;
    'unit': K within 2x of the identity, |t| <= 1 - the set on which float32 keeps its digits (see the fixture script)"""
    ext = np.empty((B, V, 3, 4))
    for b in range(B):
        for v in range(V):
            ext[b, v, :, :3] = rotation(rng)
            d = rng.standard_normal(3)
            ext[b, v, :, 3] = d / np.linalg.norm(d) * (rng.uniform(200, 500) if kind == 'mhp' else rng.uniform(0.2, 1.0))
    if kind == 'mhp':
        return ext, MHP_INTRINSIC.copy()
    K = np.eye(3)
    K[0, 0], K[1, 1] = rng.uniform(0.6, 1.8, 2)
    K[0, 2], K[1, 2] = rng.uniform(-0.4, 0.4, 2)
    return ext, K


def inputs(case, seed=SEED):
    """(features (B * V, C, h, w) float64 whose values are float16 numbers, extrinsic, intrinsic) of a case"""
    channels, V, B, (h, w), kind = CASES[case]
    rng = np.random.RandomState(seed + ord(case))
    feat = np.abs(rng.standard_normal((B * V, sum(channels), h, w))).astype(np.float16).astype(np.float64)
    ext, K = cameras(kind, B, V, rng)
    return feat, ext, K


def affines(ext, K):
    """(gather (B, V, 12), scatter (B, V, 12)) float64 tensors in the dtype of ext: x -> x A + c with
    A = K^-T R^-T, c = -t^T R^-T (gather) and A = R^T K^T, c = t^T K^T (scatter), A row-major then c. The composed form
    that the device kernels evaluate; forward() below keeps the reference's two-step form."""
    B, V = ext.shape[:2]
    Rt, tt, Kt = ext[..., :3].transpose(2, 3), ext[..., 3:].transpose(2, 3), K.t()
    Ri = torch.inverse(Rt)
    Ag = torch.inverse(Kt) @ Ri
    cg = -(tt @ Ri)
    As = Rt @ Kt
    cs = tt @ Kt
    return (torch.cat([Ag.reshape(B, V, 9), cg.reshape(B, V, 3)], -1), torch.cat([As.reshape(B, V, 9), cs.reshape(B, V, 3)], -1))


def expectation(hm):
    """this project's CPU decode of normalised maps: (N, K, 2) [sum x h, sum y h]"""
    N, K, h, w = hm.shape
    xs = torch.arange(w, dtype=hm.dtype)
    ys = torch.arange(h, dtype=hm.dtype)
    return torch.stack([(hm.sum(2) * xs).sum(-1), (hm.sum(3) * ys).sum(-1)], -1)


def forward(P, feat, ext, K):
    """feat (B * V, C, h, w) in slot order, ext (B, V, 3, 4), K (3, 3), P a dict of tensors, all of one dtype -> dict of the
    STAGES' outputs (every one in slot order where it has views) and 'pose2d' (B, V, K, 2) in heat-map pixels"""
    B, V = ext.shape[:2]
    out = {}

    def block(prefix, x, n, stride=1, padding=0):
        for i in range(n):
            p = '{}.layer_lst.{}'.format(prefix, i)
            x = F.conv2d(x, P[p + '.0.weight'], P[p + '.0.bias'], stride=stride, padding=padding)
            x = F.relu(F.batch_norm(x, P[p + '.1.running_mean'], P[p + '.1.running_var'], P[p + '.1.weight'],
                                    P[p + '.1.bias'], False, 0.0, 1e-5))
        return x

    enc = block('encoder_head', feat, 2, 2, 2)
    out['encoder_head'] = enc
    C2, h2, w2 = enc.shape[1:]
    trip = enc.reshape(B, V, C2, h2 * w2 // 3, 3)
    Rt, tt, Kt = ext[..., :3].transpose(2, 3), ext[..., 3:].transpose(2, 3), K.t()
    canon = []
    for v in range(V):
        c = trip[:, v] @ torch.inverse(Kt)
        c = (c - tt[:, v:v + 1]) @ torch.inverse(Rt[:, v:v + 1])
        canon.append(c.reshape(B, C2, h2, w2))
    fused = block('fuse_after_FTL', torch.cat(canon, 1), 2)
    out['fuse_after_FTL'] = fused
    ft = fused.reshape(B, C2, h2 * w2 // 3, 3)
    views = []
    for v in range(V):
        e = (ft @ Rt[:, v:v + 1] + tt[:, v:v + 1]) @ Kt
        views.append(e.reshape(B, C2, h2, w2))
    x = torch.stack(views, 1).reshape(B * V, C2, h2, w2)                    # slot b * V + v
    x = block('channel_expansion', x, 1)
    out['channel_expansion'] = x
    for i, op in ((0, 0), (1, 1)):
        p = 'decoder.layer_lst.{}'.format(i)
        x = F.conv_transpose2d(x, P[p + '.0.weight'], P[p + '.0.bias'], stride=2, padding=2, output_padding=op)
        x = F.relu(F.batch_norm(x, P[p + '.1.running_mean'], P[p + '.1.running_var'], P[p + '.1.weight'], P[p + '.1.bias'],
                                False, 0.0, 1e-5))
    x = F.conv2d(x, P['decoder.layer_lst.2.weight'], P['decoder.layer_lst.2.bias'], padding=1)
    out['decoder'] = x
    y = F.conv2d(x, P['final_layer.weight'], P['final_layer.bias'])
    hm = F.softmax(y.reshape(y.shape[0], y.shape[1], -1), 2).reshape(y.shape)
    out['heatmaps'] = hm
    out['pose2d'] = expectation(hm).reshape(B, V, -1, 2)
    return out


def run(case, dtype, seed=SEED, state=None):
    """the outputs of a case as float64 numpy arrays, computed in `dtype`"""
    channels, V = CASES[case][:2]
    state = fill_state_dict(channels, V, K_JOINTS, seed, CASES[case][4]) if state is None else state
    feat, ext, K = inputs(case, seed)
    with torch.no_grad():
        out = forward(to_torch(state, dtype), torch.tensor(feat, dtype=dtype), torch.tensor(ext, dtype=dtype),
                      torch.tensor(K, dtype=dtype))
    return {k: v.double().numpy() for k, v in out.items()}
