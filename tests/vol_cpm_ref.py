"""Restatement of the CPM_volumetric backbone (reference lib/models/CPM_volumetric.py:110-222) and of the feature path of
VolumetricTriangulationNet_CPM, built from tests/cpm_ref.py (state dict, inputs, error measure), F.interpolate and
tests/vol_ref.py (the lift). tests/golden/make_golden_vol_cpm.py pins `backbone` against the reference's own module in
float64 at cpm_ref.CASES b and c, and checks there that the commuted feature path is the reference's.

backbone(P, image, center, hm)          the 8-tuple's tensors in the REFERENCE's layout: five stride-8 maps, stage 6's
                                        maps up-sampled to hm = (H, W), the 128-channel features of Mconv4_stage6 (NCHW,
                                        stride 8: not up-sampled, see below)
features_reference(feat, w, b, hm)      the reference's order: up-sample the 128 channels, then the 1x1 convolution
features_commuted(feat, w, b, hm)       this project's order: the 1x1 convolution at stride 8, then up-sample 32 channels

ReLU decisions (dec / rec) follow tests/cpm_train_ref.py: a ReLU named in `dec` uses the mask handed in. Only the masks of
Mconv3_stage6 and Mconv4_stage6 lie on the path of a gradient of the three trained layers (the walk stops at
Mconv3_stage6's weight gradient); every other decision moves the forward values continuously."""
import numpy as np
import torch
import torch.nn.functional as F

import cpm_ref as R

INTER = 128
BASE_JOINT = 9
TRAINED = ('Mconv3_stage6', 'Mconv4_stage6', 'Mconv5_stage6')


def upsample(x, hm):
    return F.interpolate(x, size=tuple(hm), mode='bilinear', align_corners=True)


def backbone(P, image, center, hm, dec=None, rec=None):
    """-> (five stride-8 maps, stage 6's maps at hm, Mconv4_stage6's ReLU output (B, 128, H / 8, W / 8))"""
    def conv(name, x, act=True):
        w = P[name + '.weight']
        y = F.conv2d(x, w, P[name + '.bias'], padding=w.shape[2] // 2)
        if not act:
            return y
        mask = dec[name] if dec is not None and name in dec else (y > 0)
        if rec is not None:
            rec[name] = mask
        return y * mask.to(y.dtype)

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
    return outs[:5], upsample(outs[5], hm), x


def features_reference(feat, w, b, hm):
    return F.conv2d(upsample(feat, hm), w, b)


def features_commuted(feat, w, b, hm):
    return upsample(F.conv2d(feat, w, b), hm)


def lift(net, w, b, heat, feat, proj, cuboid_side, S, thetas, softmax=False, method='softmax', multiplier=1.0,
         dtype=torch.float64):
    """tests/vol_ref.lift for this model: heat (B * V, k + 1, H, W) with the background in channel 0, so the decode reads
    channels 1:, by arg-max unless `softmax` (MODEL.HEATMAP_SOFTMAX); feat (B * V, 128, H / 8, W / 8) goes through the
    REFERENCE's order (up-sample, then the 1x1 convolution) -> (key points, p, coord, base, pose2d (B, V, k, 2))"""
    import triangulate_ref as T
    import vol_ref as VOL
    from oracle import hrnet_cpu as O
    B, V = proj.shape[:2]
    pred = O.get_final_preds(heat[:, 1:].detach().double(), softmax).double().numpy().reshape(B, V, -1, 2)
    base = T.triangulate_batch(proj, pred[:, :, VOL.BASE_JOINT:VOL.BASE_JOINT + 1])[:, 0]
    coord = VOL.coord_volumes(base, cuboid_side, S, thetas)
    feats = features_reference(feat, w, b, heat.shape[2:])
    vol = VOL._Unproject.apply(feats.reshape(B, V, *feats.shape[1:]), proj, coord, method)
    out = net(vol)
    K = out.shape[1]
    p = torch.softmax(multiplier * out.reshape(B, K, -1), dim=2)
    kp = torch.einsum('bjn,bnc->bjc', p, torch.from_numpy(coord.reshape(B, -1, 3)).to(dtype))
    return kp, p.reshape(out.shape), torch.from_numpy(coord), torch.from_numpy(base), pred


def process_weights(seed=R.SEED):
    """(w (32, 128, 1, 1), b (32,)) float64 numpy with float32 values"""
    rng = np.random.RandomState(seed + 5)
    w = rng.standard_normal((32, INTER, 1, 1)) * np.sqrt(2.0 / INTER)
    b = rng.standard_normal(32) * 0.1
    return w.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)


def short_targets(case, hm, seed=R.SEED):
    """(heat-map target (B, k + 1, H, W), weights of the feature term (B, 32, H, W)) float64 numpy with float16 values"""
    B = R.CASES[case][0]
    rng = np.random.RandomState(seed + 11 * ord(case))
    f16 = lambda a: a.astype(np.float16).astype(np.float64)
    return f16(rng.uniform(0, 1, (B, R.K_JOINTS + 1) + tuple(hm))), f16(rng.standard_normal((B, 32) + tuple(hm)))


def short_loss(heat, feats, tgt, wts):
    """HeatmapLoss 'l2' on the lifted maps plus a linear functional of the lifted, processed features"""
    return ((heat - tgt) ** 2).sum((2, 3)).mean() + (feats * wts).sum() / feats.shape[0]


def short_loss_and_grads(state, case, hm, dtype, dec=None):
    """(loss, name -> gradient) of the three trained layers and of process_features, float64 numpy, computed in `dtype`"""
    img, cm = R.inputs(case)
    w, b = process_weights()
    tgt, wts = short_targets(case, hm)
    t = lambda a: torch.tensor(a, dtype=dtype)
    P = {k: t(v) for k, v in state.items()}
    leaves = {}
    for name in TRAINED:
        for part in ('.weight', '.bias'):
            leaves['backbone.' + name + part] = P[name + part].requires_grad_(True)
    leaves['process_features.0.weight'], leaves['process_features.0.bias'] = t(w).requires_grad_(True), t(b).requires_grad_(True)
    _low, heat, feat = backbone(P, t(img), t(cm), hm, dec)
    feats = features_commuted(feat, leaves['process_features.0.weight'], leaves['process_features.0.bias'], hm)
    loss = short_loss(heat, feats, t(tgt), t(wts))
    loss.backward()
    return float(loss.detach().double()), {k: v.grad.double().numpy() for k, v in leaves.items()}
