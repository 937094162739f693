"""The gradient oracle of CPM training. It builds on tests/cpm_ref.py (left alone) and restates the model with its
DECISIONS made explicit: relu(z) = z * mask and the max pool as a gather at given indices. Run freely, the decisions are
the restatement's own (mask = z > 0, indices = F.max_pool2d's: the first maximum in scan order) and it is cpm_ref.forward;
run with decisions handed in, it is the function the device differentiated: a float32 forward and a float64 one disagree on
a few ReLU signs and arg-maxima among ~10^5 units (those within rounding of zero or of a tie), and one flip moves a
gradient by far more than the bound, so the tests read the masks and indices from the trainable model's saved activations
(decisions_of) and give them to the float64 and the float32 restatement alike."""
import numpy as np
import torch
import torch.nn.functional as F

import cpm_ref as R

CASES = {'p': (2, 24, 40), 'q': (1, 8, 16)}     # 3 x 5 maps, 1 x 2 maps
ALL_STAGES = (1, 1, 1, 1, 1, 1)
LAST_STAGE = (0, 0, 0, 0, 0, 1)


def inputs(case, seed=R.SEED):
    """(image, centre map, target) float64 numpy arrays with float16 values; the image and centre map as cpm_ref.inputs
    draws them, the target a clipped sigma = 1 Gaussian per joint with the background channel in front"""
    B, H, W = CASES[case]
    rng = np.random.RandomState(seed + 7 * ord(case))
    img = (rng.standard_normal((B, 3, H, W)) * 0.5).astype(np.float16)
    yy, xx = np.mgrid[0:H, 0:W]
    cm = np.empty((B, 1, H, W))
    for b in range(B):
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        g = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 2.0 / 9.0)
        g[g < 0.0099] = 0
        cm[b, 0] = g
    h, w = H // 8, W // 8
    yy, xx = np.mgrid[0:h, 0:w]
    tgt = np.empty((B, R.K_JOINTS + 1, h, w))
    for b in range(B):
        for j in range(1, R.K_JOINTS + 1):
            cx, cy = rng.uniform(0, w), rng.uniform(0, h)
            tgt[b, j] = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 2.0)
        tgt[b, 0] = 1 - tgt[b, 1:].max(0)
    f16 = lambda a: a.astype(np.float16).astype(np.float64)
    return img.astype(np.float64), f16(cm), f16(tgt)


def sample_index(case, sizes, samples=1024):
    """(len(sizes), samples) flat indices, drawn with replacement per tensor: where tests/golden/cpm_train.npz samples the
    gradients"""
    rng = np.random.RandomState(R.SEED + ord(case))
    return np.stack([rng.randint(0, n, samples) for n in sizes])


def forward(P, image, center, dec=None, rec=None):
    """the six stage outputs. dec: None (own decisions) or a dict name -> bool mask (ReLU) / int64 indices (pool);
    rec: a dict that receives the decisions taken"""
    def relu(name, z):
        mask = (z > 0) if dec is None else dec[name]
        if rec is not None:
            rec[name] = mask
        return z * mask.to(z.dtype)

    def conv(name, x, act=True):
        w = P[name + '.weight']
        y = F.conv2d(x, w, P[name + '.bias'], padding=w.shape[2] // 2)
        return relu(name, y) if act else y

    def pool(name, a):
        if dec is None:
            idx = F.max_pool2d(a.detach(), 3, 2, 1, return_indices=True)[1]
        else:
            idx = dec[name]
        if rec is not None:
            rec[name] = idx
        return a.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)

    def trunk(x, stage):
        for i in (1, 2, 3):
            x = pool('pool%d_stage%d' % (i, stage), conv('conv%d_stage%d' % (i, stage), x))
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


def heatmap_loss(pred, gt):
    """HeatmapLoss 'l2' (lib/core/loss.py): mean over (b, k) of the sum over (h, w) of the squared difference"""
    return ((pred - gt) ** 2).sum((2, 3)).mean()


def loss_of(outs, target, weights):
    total = None
    for o, wgt in zip(outs, weights):
        if wgt:
            term = heatmap_loss(o, target) * wgt
            total = term if total is None else total + term
    return total


def loss_and_grads(state, img, cm, tgt, weights, dtype, dec=None, rec=None):
    """(loss, name -> gradient) as float64 numpy, computed in `dtype` on the CPU"""
    P = {k: torch.tensor(v, dtype=dtype).requires_grad_(True) for k, v in state.items()}
    t = lambda a: torch.tensor(a, dtype=dtype)
    loss = loss_of(forward(P, t(img), t(cm), dec, rec), t(tgt), weights)
    loss.backward()
    return float(loss.detach().double()), {k: v.grad.double().numpy() for k, v in P.items()}


def decisions_of(model):
    """the decisions of a trainable models.CPM's training forward, from its saved activations (model.tape, NHWC on the
    device): a ReLU passed where its output is > 0; a pool took the first position in scan order that equals the pooled
    value, which is what F.max_pool2d returns on the device's own float32 input"""
    tape = model.tape
    nchw = lambda t, c=None: t[..., :c].permute(0, 3, 1, 2).contiguous().cpu()
    dec = {}
    for st in (1, 2):
        for i in (1, 2, 3):
            a = nchw(tape['a%d_%d' % (i, st)])
            dec['conv%d_stage%d' % (i, st)] = a > 0
            pooled, idx = F.max_pool2d(a, 3, 2, 1, return_indices=True)
            assert torch.equal(pooled, nchw(tape['p%d_%d' % (i, st)]))
            dec['pool%d_stage%d' % (i, st)] = idx
    for i in (4, 5, 6):
        dec['conv%d_stage1' % i] = nchw(tape['y%d' % i]) > 0
    for s in range(2, 7):
        dec['conv4_stage2' if s == 2 else 'conv1_stage%d' % s] = nchw(tape['cats'][s - 2], 32) > 0
        for i in (1, 2, 3, 4):
            dec['Mconv%d_stage%d' % (i, s)] = nchw(tape['m%d_%d' % (i, s)]) > 0
    return dec
