"""Training-mode restatement of tests/ftl_ref.py's forward with torch CPU autograd, in the dtype of its inputs: the CPU
yardstick of a trainable models.FTL_encoder_decoder. Every BatchNorm runs on batch statistics (F.batch_norm with
training=True, momentum 0.1, which updates the running statistics it is handed); the transforms keep the reference's
two-step form; decoder.layer_lst.2 and final_layer stay two layers. The loss is mean((pose2d - gt)^2) against drawn
targets in heat-map pixels.

run(case, dtype) -> dict of float64 numpy arrays: 'loss', 'heatmaps', 'pose2d', 'grad/<parameter>' for every head
parameter, 'stat/<buffer>' for every running statistic after the step, and 'scale/<parameter>' for the biases whose true
gradient is zero (a convolution bias in front of a batch-statistic BatchNorm; the last two biases, because the softmax is
shift-invariant): max_c sum_pixels |dz| of the layer's pre-BatchNorm gradient (the logits' gradient for the last two), the
scale on which their float error is measured.

forward_layers(...) is an independent per-layer restatement (hand-written batch statistics, the composed affine
transforms of ftl_ref.affines, the folded output convolution) that tests/test_ftl_train_cpu.py pins run() against.
"""
import numpy as np
import torch
import torch.nn.functional as F

import ftl_ref as R

MOMENTUM, EPS = 0.1, 1e-5
BN_BLOCKS = ('encoder_head.layer_lst.0', 'encoder_head.layer_lst.1', 'fuse_after_FTL.layer_lst.0',
             'fuse_after_FTL.layer_lst.1', 'channel_expansion.layer_lst.0', 'decoder.layer_lst.0', 'decoder.layer_lst.1')
ZERO_GRAD_BIASES = tuple(p + '.0.bias' for p in BN_BLOCKS) + ('decoder.layer_lst.2.bias', 'final_layer.bias')


def is_parameter(key):
    return not key.endswith(('running_mean', 'running_var', 'num_batches_tracked'))


def targets(case, seed=R.SEED):
    """the drawn 2-D targets (B, V, K, 2) of a case, float16-valued, inside the heat map"""
    channels, V, B, (h, w), kind = R.CASES[case]
    rng = np.random.RandomState(seed + 1000 + ord(case))
    gt = rng.uniform(0, 1, (B, V, R.K_JOINTS, 2)) * np.array([w - 1, h - 1])
    return gt.astype(np.float16).astype(np.float64)


def forward_train(P, feat, ext, K):
    """ftl_ref.forward on batch statistics. P: parameters (requires_grad as the caller set it) and running statistics
    (updated in place). Returns (dict of 'heatmaps', 'pose2d', 'logits', pre: block prefix -> its pre-BatchNorm map)"""
    B, V = ext.shape[:2]
    pre = {}

    def bn_relu(p, x):
        pre[p] = x
        return F.relu(F.batch_norm(x, P[p + '.1.running_mean'], P[p + '.1.running_var'], P[p + '.1.weight'], P[p + '.1.bias'],
                                   True, MOMENTUM, EPS))

    def block(prefix, x, n, stride=1, padding=0):
        for i in range(n):
            p = '{}.layer_lst.{}'.format(prefix, i)
            x = bn_relu(p, F.conv2d(x, P[p + '.0.weight'], P[p + '.0.bias'], stride=stride, padding=padding))
        return x

    enc = block('encoder_head', feat, 2, 2, 2)
    C2, h2, w2 = enc.shape[1:]
    trip = enc.reshape(B, V, C2, h2 * w2 // 3, 3)
    Rt, tt, Kt = ext[..., :3].transpose(2, 3), ext[..., 3:].transpose(2, 3), K.t()
    canon = []
    for v in range(V):
        c = trip[:, v] @ torch.inverse(Kt)
        c = (c - tt[:, v:v + 1]) @ torch.inverse(Rt[:, v:v + 1])
        canon.append(c.reshape(B, C2, h2, w2))
    fused = block('fuse_after_FTL', torch.cat(canon, 1), 2)
    ft = fused.reshape(B, C2, h2 * w2 // 3, 3)
    views = [((ft @ Rt[:, v:v + 1] + tt[:, v:v + 1]) @ Kt).reshape(B, C2, h2, w2) for v in range(V)]
    x = torch.stack(views, 1).reshape(B * V, C2, h2, w2)                    # slot b * V + v
    x = block('channel_expansion', x, 1)
    for i, op in ((0, 0), (1, 1)):
        p = 'decoder.layer_lst.{}'.format(i)
        x = bn_relu(p, F.conv_transpose2d(x, P[p + '.0.weight'], P[p + '.0.bias'], stride=2, padding=2, output_padding=op))
    x = F.conv2d(x, P['decoder.layer_lst.2.weight'], P['decoder.layer_lst.2.bias'], padding=1)
    y = F.conv2d(x, P['final_layer.weight'], P['final_layer.bias'])
    hm = F.softmax(y.reshape(y.shape[0], y.shape[1], -1), 2).reshape(y.shape)
    return {'heatmaps': hm, 'pose2d': R.expectation(hm).reshape(B, V, -1, 2), 'logits': y}, pre


def loss_of(pose2d, gt):
    return ((pose2d - gt) ** 2).mean()


def _bn_hand(x, gamma, beta):
    mean = x.mean((0, 2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean((0, 2, 3), keepdim=True)
    return F.relu((x - mean) / torch.sqrt(var + EPS) * gamma.reshape(1, -1, 1, 1) + beta.reshape(1, -1, 1, 1))


def forward_layers(P, feat, ext, K):
    """the same function, restated independently: batch statistics by hand, the composed transforms x A + c of
    ftl_ref.affines, decoder.layer_lst.2 and final_layer folded into one 3x3 convolution. Returns the same dict (no pre)"""
    B, V = ext.shape[:2]

    def cbr(p, x, **kw):
        return _bn_hand(F.conv2d(x, P[p + '.0.weight'], P[p + '.0.bias'], **kw), P[p + '.1.weight'], P[p + '.1.bias'])

    x = cbr('encoder_head.layer_lst.0', feat, stride=2, padding=2)
    enc = cbr('encoder_head.layer_lst.1', x, stride=2, padding=2)
    C2, h2, w2 = enc.shape[1:]
    cg, cs = R.affines(ext, K)

    def affine(t, coef):                       # t (..., T, 3), coef (..., 12) broadcast over the channels
        A, c = coef[..., :9].reshape(coef.shape[:-1] + (1, 3, 3)), coef[..., 9:].reshape(coef.shape[:-1] + (1, 1, 3))
        return t @ A + c

    trip = enc.reshape(B, V, C2, h2 * w2 // 3, 3)
    cat = affine(trip, cg).reshape(B, V * C2, h2, w2)
    f = cbr('fuse_after_FTL.layer_lst.1', cbr('fuse_after_FTL.layer_lst.0', cat))
    ft = f.reshape(B, 1, C2, h2 * w2 // 3, 3).expand(B, V, C2, h2 * w2 // 3, 3)
    x = affine(ft, cs).reshape(B * V, C2, h2, w2)
    x = cbr('channel_expansion.layer_lst.0', x)
    for i, op in ((0, 0), (1, 1)):
        p = 'decoder.layer_lst.{}'.format(i)
        x = _bn_hand(F.conv_transpose2d(x, P[p + '.0.weight'], P[p + '.0.bias'], stride=2, padding=2, output_padding=op),
                     P[p + '.1.weight'], P[p + '.1.bias'])
    wf = P['final_layer.weight'].reshape(P['final_layer.weight'].shape[0], -1)
    w_out = torch.einsum('km,mcrs->kcrs', wf, P['decoder.layer_lst.2.weight'])
    b_out = wf @ P['decoder.layer_lst.2.bias'] + P['final_layer.bias']
    y = F.conv2d(x, w_out, b_out, padding=1)
    hm = F.softmax(y.reshape(y.shape[0], y.shape[1], -1), 2).reshape(y.shape)
    return {'heatmaps': hm, 'pose2d': R.expectation(hm).reshape(B, V, -1, 2), 'logits': y}


def tensors(case, dtype, seed=R.SEED, state=None):
    """(P with requires_grad on the parameters, feat, ext, K, gt) of a case as torch tensors of dtype"""
    channels, V = R.CASES[case][:2]
    state = R.fill_state_dict(channels, V, R.K_JOINTS, seed, R.CASES[case][4]) if state is None else state
    P = R.to_torch(state, dtype)
    for k, v in P.items():
        if is_parameter(k):
            v.requires_grad_()
    feat, ext, K = R.inputs(case, seed)
    t = lambda a: torch.tensor(a, dtype=dtype)
    return P, t(feat), t(ext), t(K), t(targets(case, seed))


_RUNS = {}


def run(case, dtype, seed=R.SEED):
    """one training step's loss, heat maps and gradients of a case in dtype, as float64 numpy arrays; computed once"""
    key = (case, dtype, seed)
    if key in _RUNS:
        return _RUNS[key]
    P, feat, ext, K, gt = tensors(case, dtype, seed)
    out, pre = forward_train(P, feat, ext, K)
    for v in list(pre.values()) + [out['logits']]:
        v.retain_grad()
    loss = loss_of(out['pose2d'], gt)
    loss.backward()
    n = lambda v: v.detach().double().numpy()
    res = {'loss': n(loss), 'heatmaps': n(out['heatmaps']), 'pose2d': n(out['pose2d'])}
    for k, v in P.items():
        if is_parameter(k):
            res['grad/' + k] = n(v.grad)
        else:
            res['stat/' + k] = n(v)
    scale = lambda g: float(g.detach().double().abs().sum((0, 2, 3)).max())
    for p in BN_BLOCKS:
        res['scale/' + p + '.0.bias'] = scale(pre[p].grad)
    res['scale/decoder.layer_lst.2.bias'] = res['scale/final_layer.bias'] = scale(out['logits'].grad)
    _RUNS[key] = res
    return res
