"""Restatement of the reference's PredRNN head (lib/models/predrnn.py: SpatioTemporalLSTMCell :7-58, RNN :61-122, BasicBlock
and ResNet :132-184) as a walk over a state dict with torch's CPU ops, in the dtype of its inputs: the CPU yardstick of
models.predrnn on the HIP path. tests/golden/make_golden_predrnn.py pins it against the reference's own modules in float64.

The state dict carries the names of HRNet_PredRNN_ResNet's children: 'PredRNN.cell_list.0.conv_x.0.weight' ...,
'resnet.block1.conv1.weight' ... (the backbone's 'HRNet.*' entries are not part of it).

fill_state_dict(case, seed) draws every tensor from numpy.random.RandomState(seed) in SORTED key order, so no weights are
stored anywhere: convolution and linear weights N(0, sqrt(1 / fan_in)) (fc: sqrt(2 / fan_in)), their biases N(0, 0.1),
LayerNorm and BatchNorm weights 1 + N(0, 0.1), their biases N(0, 0.1), BatchNorm running means N(0, 0.2), running
variances uniform in [0.5, 1.5], num_batches_tracked 1.

err = rel(dev, ref64) = max|dev - ref64| / max|ref64|; a device result must stay within bound(e_ref) =
4 * e_ref + 2 * 2^-24, e_ref being the same measure of a float32 CPU run (the convention of tests/cpm_ref.py and
tests/swin_ref.py).

The second half restates the device ops one by one on NHWC maps (sample_stats, gates, out_gate, maxpool2x2): what
tests/test_predrnn_ops_gpu.py holds each kernel to.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

SEED = 20261021
JOINTS = 21
C0 = 32                          # STAGE2.NUM_CHANNELS[0] of the W32 backbone
FRAME = JOINTS + C0              # 53 channels of a frame
EPS = 1e-5
# name -> N_HIDDEN, FILTER_SIZE, map size, batch, frames. b: maps smaller than two tiles of the convolution, one layer, so
# m_t is read from the map that m_new is written to
CASES = {'a': dict(nh=[8, 8, 8], ks=3, size=8, B=2, L=3), 'b': dict(nh=[4], ks=5, size=6, B=1, L=2)}
FULL = dict(nh=[64, 64, 64, 64], ks=3, size=64)          # the yaml's config


def rel(a, b, denom=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() if denom is None else denom))


def bound(e_ref):
    return 4.0 * e_ref + 2.0 * 2.0 ** -24


def head_keys_and_shapes(case):
    """(key, shape) of the PredRNN and resnet children in the reference's state-dict order"""
    nhs, ks, s = case['nh'], case['ks'], case['size']
    out = []
    for i, nh in enumerate(nhs):
        cin = FRAME if i == 0 else nhs[i - 1]
        p = 'PredRNN.cell_list.{}.'.format(i)
        for name, ci, k in (('conv_x', cin, 7), ('conv_h', nh, 4), ('conv_m', nh, 3), ('conv_o', 2 * nh, 1)):
            out += [(p + name + '.0.weight', (k * nh, ci, ks, ks)), (p + name + '.0.bias', (k * nh,)),
                    (p + name + '.1.weight', (k * nh, s, s)), (p + name + '.1.bias', (k * nh, s, s))]
        out += [(p + 'conv_last.weight', (nh, 2 * nh, 1, 1)), (p + 'conv_last.bias', (nh,))]
    out.append(('PredRNN.conv_last.weight', (FRAME, nhs[-1], 1, 1)))
    for b in ('block1', 'block2'):
        for j in ('1', '2'):
            p = 'resnet.{}.'.format(b)
            out.append((p + 'conv' + j + '.weight', (FRAME, FRAME, 3, 3)))
            out += [(p + 'bn' + j + '.' + n, sh) for n, sh in (('weight', (FRAME,)), ('bias', (FRAME,)),
                                                                 ('running_mean', (FRAME,)), ('running_var', (FRAME,)),
                                                                 ('num_batches_tracked', ()))]
    out += [('resnet.fc1.weight', (1024, FRAME * s * s // 4)), ('resnet.fc1.bias', (1024,)),
            ('resnet.fc2.weight', (3 * JOINTS, 1024)), ('resnet.fc2.bias', (3 * JOINTS,))]
    # the reference's BasicBlock registers conv1, bn1, conv2, bn2 in that order
    return out


def fill_state_dict(case, seed=SEED):
    """name -> float64 numpy array (num_batches_tracked: int64), drawn in sorted key order"""
    shapes = dict(head_keys_and_shapes(case))
    rng = np.random.RandomState(seed)
    state = {}
    for key in sorted(shapes):
        shape = shapes[key]
        leaf = key.rsplit('.', 1)[1]
        norm = '.bn' in key or key.rsplit('.', 2)[1] == '1'            # BatchNorm, or the LayerNorm of a Sequential
        if leaf == 'num_batches_tracked':
            state[key] = np.array(1, dtype=np.int64)
        elif leaf == 'running_mean':
            state[key] = rng.standard_normal(shape) * 0.2
        elif leaf == 'running_var':
            state[key] = rng.uniform(0.5, 1.5, shape)
        elif norm and leaf == 'weight':
            state[key] = 1.0 + rng.standard_normal(shape) * 0.1
        elif leaf == 'bias':
            state[key] = rng.standard_normal(shape) * 0.1
        elif '.fc' in key:
            state[key] = rng.standard_normal(shape) * math.sqrt(2.0 / shape[1])
        else:
            state[key] = rng.standard_normal(shape) * math.sqrt(1.0 / (shape[1] * shape[2] * shape[3]))
    return state


def to_torch(state, dtype):
    return {k: torch.tensor(v, dtype=dtype if v.dtype.kind == 'f' else torch.int64) for k, v in state.items()}


def sub(P, prefix):
    """the entries of a child, its prefix stripped: what the child's load_state_dict takes"""
    return {k[len(prefix):]: v for k, v in P.items() if k.startswith(prefix)}


def frames(name, seed=SEED):
    """(B, L, 53, s, s) float64 numpy array whose values are float16 numbers: N(0, 0.5), as heat maps and features mix"""
    c = CASES[name]
    rng = np.random.RandomState(seed + ord(name))
    x = (rng.standard_normal((c['B'], c['L'], FRAME, c['size'], c['size'])) * 0.5).astype(np.float16)
    return x.astype(np.float64)


# ---- the model's head, NCHW as the reference -------------------------------------------------------------------------
def _conv_ln(P, p, x):
    w = P[p + '.0.weight']
    y = F.conv2d(x, w, P[p + '.0.bias'], padding=w.shape[2] // 2)
    return F.layer_norm(y, y.shape[1:], P[p + '.1.weight'], P[p + '.1.bias'], EPS)


def cell_forward(P, p, x, h, c, m):
    """predrnn.py:33-58: -> (h_new, c_new, m_new)"""
    nh = c.shape[1]
    i_x, f_x, g_x, i_xp, f_xp, g_xp, o_x = torch.split(_conv_ln(P, p + 'conv_x', x), nh, dim=1)
    i_h, f_h, g_h, o_h = torch.split(_conv_ln(P, p + 'conv_h', h), nh, dim=1)
    i_m, f_m, g_m = torch.split(_conv_ln(P, p + 'conv_m', m), nh, dim=1)
    c_new = torch.sigmoid(f_x + f_h + 1.0) * c + torch.sigmoid(i_x + i_h) * torch.tanh(g_x + g_h)
    m_new = torch.sigmoid(f_xp + f_m + 1.0) * m + torch.sigmoid(i_xp + i_m) * torch.tanh(g_xp + g_m)
    mem = torch.cat((c_new, m_new), 1)
    o = torch.sigmoid(o_x + o_h + _conv_ln(P, p + 'conv_o', mem))
    return o * torch.tanh(F.conv2d(mem, P[p + 'conv_last.weight'], P[p + 'conv_last.bias'])), c_new, m_new


def rnn_forward(P, x, nhs):
    """predrnn.py:84-122: x (B, L, 53, s, s) -> (B, L, 53, s, s); P the whole head's dict"""
    B, L, _, s, _ = x.shape
    zeros = lambda n: torch.zeros((B, n, s, s), dtype=x.dtype)
    h, c = [zeros(n) for n in nhs], [zeros(n) for n in nhs]
    memory = zeros(nhs[0])
    out = []
    for t in range(L):
        net = x[:, t]
        for i in range(len(nhs)):
            h[i], c[i], memory = cell_forward(P, 'PredRNN.cell_list.{}.'.format(i), net if i == 0 else h[i - 1], h[i], c[i],
                                              memory)
        out.append(F.conv2d(h[-1], P['PredRNN.conv_last.weight']))
    return torch.stack(out, 1)


def _block(P, p, x):
    def bn(y, j):
        q = p + 'bn' + j + '.'
        return F.batch_norm(y, P[q + 'running_mean'], P[q + 'running_var'], P[q + 'weight'], P[q + 'bias'], False, 0.0, EPS)
    y = F.relu(bn(F.conv2d(x, P[p + 'conv1.weight'], padding=1), '1'))
    return F.relu(bn(F.conv2d(y, P[p + 'conv2.weight'], padding=1), '2') + x)


def pose_forward(P, x):
    """predrnn.py:173-184: x (B, 53, s, s) -> (B, 63)"""
    y = _block(P, 'resnet.block2.', F.max_pool2d(_block(P, 'resnet.block1.', x), 2, 2))
    y = F.relu(F.linear(y.reshape(y.shape[0], -1), P['resnet.fc1.weight'], P['resnet.fc1.bias']))
    return F.relu(F.linear(y, P['resnet.fc2.weight'], P['resnet.fc2.bias']))


def last_frame(rnn64):
    """the tail's input of a case: the float64 RNN's last predicted frame, rounded to float16 values"""
    return np.asarray(rnn64)[:, -1].astype(np.float16).astype(np.float64)


def run(name, dtype, seed=SEED, state=None):
    """(the predicted frames, the pose of last_frame(float64 frames)) of a case as float64 numpy arrays, computed in `dtype`;
    the float64 frames are computed first, whatever dtype is"""
    c = CASES[name]
    state = fill_state_dict(c, seed) if state is None else state
    with torch.no_grad():
        x = frames(name, seed)
        y64 = rnn_forward(to_torch(state, torch.float64), torch.tensor(x, dtype=torch.float64), c['nh']).numpy()
        P = to_torch(state, dtype)
        y = rnn_forward(P, torch.tensor(x, dtype=dtype), c['nh']).double().numpy() if dtype != torch.float64 else y64
        pose = pose_forward(P, torch.tensor(last_frame(y64), dtype=dtype)).double().numpy()
    return y, pose


# ---- the device ops, NHWC --------------------------------------------------------------------------------------------
def sample_stats(x, eps=EPS):
    """x (B, ...) -> (B, 2): mean and 1 / sqrt(biased var + eps) per sample, in x's dtype"""
    flat = x.reshape(x.shape[0], -1)
    mean = flat.mean(1)
    var = ((flat - mean[:, None]) ** 2).mean(1)
    return torch.stack((mean, 1.0 / torch.sqrt(var + eps)), 1)


def layer_norm(x, w, b, eps=EPS):
    """x (B, H, W, C), w and b (H, W, C): LayerNorm over all of a sample"""
    return F.layer_norm(x, x.shape[1:], w, b, eps)


def gates(xc, hc, mc, ln, c_t, m_t, nh):
    """NHWC: raw xc (B, H, W, 7 nh), hc (.., 4 nh), mc (.., 3 nh); ln = (wx, bx, wh, bh, wm, bm) as (H, W, C); c_t, m_t
    (B, H, W, nh) -> (c_new, m_new, o_pre)"""
    i_x, f_x, g_x, i_xp, f_xp, g_xp, o_x = torch.split(layer_norm(xc, ln[0], ln[1]), nh, dim=3)
    i_h, f_h, g_h, o_h = torch.split(layer_norm(hc, ln[2], ln[3]), nh, dim=3)
    i_m, f_m, g_m = torch.split(layer_norm(mc, ln[4], ln[5]), nh, dim=3)
    c_new = torch.sigmoid(f_x + f_h + 1.0) * c_t + torch.sigmoid(i_x + i_h) * torch.tanh(g_x + g_h)
    m_new = torch.sigmoid(f_xp + f_m + 1.0) * m_t + torch.sigmoid(i_xp + i_m) * torch.tanh(g_xp + g_m)
    return c_new, m_new, o_x + o_h


def out_gate(oc, wo, bo, o_pre, last):
    return torch.sigmoid(o_pre + layer_norm(oc, wo, bo)) * torch.tanh(last)


def maxpool2x2(x):
    """x (B, H, W, C) NHWC"""
    return F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
