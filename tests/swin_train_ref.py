"""The training-only pieces of the SwinPose restatement (tests/swin_ref.py holds the rest): the decoder step with
batch-statistic BatchNorm, the block with a per-sample scale on each residual branch (timm's DropPath: flag / keep_prob),
and the head built from them. Plain torch tensor ops in the dtype of the inputs, differentiable as they stand.

drop_path_rates(depths, rate) is the reference's schedule: block k of the whole network has linspace(0, rate, sum(depths))[k]
(reference lib/models/swin_transformer.py:640, rate 0.2 by default).
"""
import numpy as np
import torch

import swin_ref as R


def drop_path_rates(depths, rate=0.2):
    return [float(v) for v in torch.linspace(0, rate, sum(depths))]


def factors(depths, batch, rate, seed, keep_all=False):
    """per block two float64 vectors (B,): flag / keep_prob with flag ~ Bernoulli(keep_prob), from RandomState(seed)"""
    rng = np.random.RandomState(seed)
    out = []
    for r in drop_path_rates(depths, rate):
        keep = 1.0 - r
        pair = []
        for _ in range(2):
            flag = np.ones(batch) if keep_all else (rng.uniform(size=batch) < keep).astype(np.float64)
            pair.append(flag / keep)
        out.append(pair)
    return out


def block(x, H, W, P, b, heads, ws, shift, s1, s2):
    """swin_ref.block with the two branches scaled per sample by s1, s2 (B,)"""
    h = R.layer_norm(x, P[b + 'norm1.weight'], P[b + 'norm1.bias'])
    h = R.window_attention(h, H, W, P[b + 'attn.qkv.weight'], P[b + 'attn.qkv.bias'],
                           P[b + 'attn.relative_position_bias_table'], heads, ws, shift)
    x = x + s1.reshape(-1, 1, 1) * (h @ P[b + 'attn.proj.weight'].t() + P[b + 'attn.proj.bias'])
    h = R.layer_norm(x, P[b + 'norm2.weight'], P[b + 'norm2.bias'])
    h = R.gelu(h @ P[b + 'feed_forward.fc1.weight'].t() + P[b + 'feed_forward.fc1.bias'])
    return x + s2.reshape(-1, 1, 1) * (h @ P[b + 'feed_forward.fc2.weight'].t() + P[b + 'feed_forward.fc2.bias'])


def swin(x, P, cfg, fac, ws=R.WS):
    s = 'swinTransformer.'
    w = P[s + 'patch_embed.proj.weight']
    rows, H, W = R.embed_rows(x, cfg['patch'])
    t = rows @ w.reshape(w.shape[0], -1).t() + P[s + 'patch_embed.proj.bias']
    t = R.layer_norm(t, P[s + 'patch_embed.norm.weight'], P[s + 'patch_embed.norm.bias']).reshape(x.shape[0], H * W, -1)
    n, k = len(cfg['depths']), 0
    for i, depth in enumerate(cfg['depths']):
        for j in range(depth):
            s1, s2 = (torch.as_tensor(f, dtype=x.dtype) for f in fac[k])
            t = block(t, H, W, P, s + 'layers.{}.blocks.{}.'.format(i, j), R.HEADS[i], ws, 0 if j % 2 == 0 else ws // 2,
                      s1, s2)
            k += 1
        if i < n - 1:
            d = s + 'layers.{}.downsample.'.format(i)
            t = R.layer_norm(R.merge_gather(t, H, W), P[d + 'norm.weight'], P[d + 'norm.bias']) @ P[d + 'reduction.weight'].t()
            H, W = (H + 1) // 2, (W + 1) // 2
    key = s + 'norm{}.'.format(n - 1)
    return R.layer_norm(t, P[key + 'weight'], P[key + 'bias']), H, W


def conv_transpose(x, w, b):
    """ConvTranspose2d(3, 2, 1, 1) from its definition, as swin_ref.decoder_step"""
    B, Ci, H, W = x.shape
    full = x.new_zeros(B, w.shape[1], 2 * H + 2, 2 * W + 2)
    for kh in range(3):
        for kw in range(3):
            full[:, :, kh:kh + 2 * H:2, kw:kw + 2 * W:2] += torch.einsum('bihw,io->bohw', x, w[:, :, kh, kw])
    return full[:, :, 1:2 * H + 1, 1:2 * W + 1] + b.reshape(1, -1, 1, 1)


def batch_norm_train(y, gamma, beta, eps=1e-5):
    """y NCHW -> (normalised with the batch's biased variance, batch mean, UNBIASED batch variance)"""
    mean = y.mean(dim=(0, 2, 3))
    d = y - mean.reshape(1, -1, 1, 1)
    var = (d * d).mean(dim=(0, 2, 3))
    n = y.numel() // y.shape[1]
    out = d / torch.sqrt(var.reshape(1, -1, 1, 1) + eps) * gamma.reshape(1, -1, 1, 1) + beta.reshape(1, -1, 1, 1)
    return out, mean, var * (n / max(n - 1, 1))


def decoder_step(x, P, s, eps=1e-5):
    """NCHW x -> (ConvTranspose2d, Conv2d 1x1, training BatchNorm, ReLU; batch mean; unbiased batch variance)"""
    b = 'decoder.{}.'
    y = conv_transpose(x, P[b.format(4 * s) + 'weight'], P[b.format(4 * s) + 'bias'])
    w1 = P[b.format(4 * s + 1) + 'weight']
    y = torch.einsum('bihw,oi->bohw', y, w1[:, :, 0, 0]) + P[b.format(4 * s + 1) + 'bias'].reshape(1, -1, 1, 1)
    n = b.format(4 * s + 2)
    y, mean, var = batch_norm_train(y, P[n + 'weight'], P[n + 'bias'], eps)
    return torch.relu(y), mean, var


def head(x, P, cfg, fac):
    """NCHW features -> (heat maps (B, J, Hm, Wm), [(batch mean, unbiased variance) per decoder step]), training mode"""
    t, H, W = swin(x, P, cfg, fac)
    y = t.reshape(x.shape[0], H, W, -1).permute(0, 3, 1, 2)
    stats = []
    for s in range(cfg['steps']):
        y, mean, var = decoder_step(y, P, s)
        stats.append((mean, var))
    last = 'decoder.{}.'.format(4 * cfg['steps'])
    y = torch.einsum('bihw,oi->bohw', y, P[last + 'weight'][:, :, 0, 0]) + P[last + 'bias'].reshape(1, -1, 1, 1)
    return torch.softmax(y.flatten(2) * P['trainable_temp'], dim=2).reshape(y.shape), stats


def targets(cfg, size, seed=R.SEED):
    """fixed heat-map targets (B, J, size, size), positive, each map summing to 1"""
    rng = np.random.RandomState(seed + 2)
    t = rng.uniform(0.0, 1.0, (cfg['batch'], cfg['joints'], size, size)) ** 4
    return t / t.sum(axis=(2, 3), keepdims=True)


def loss(heatmaps, target):
    """sum of squared differences, scaled so that the loss is O(1)"""
    return ((heatmaps - target) ** 2).sum() * heatmaps.shape[-1] * heatmaps.shape[-2] / heatmaps.shape[0]
