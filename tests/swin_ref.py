"""Restatement of the reference's SwinPose head (lib/models/swin_transformer.py: SwinTransformer :569-722, the decoder
:784-811 and the spatial softmax :824-827) in plain torch tensor ops, in the dtype of its inputs: the CPU yardstick of the
HIP path. It follows the reference's own route - pad, roll, window partition, mask, reverse - so it shares nothing with the
device kernel's arithmetic token lookup.

fill_state_dict(keys_and_shapes, seed) draws every tensor from numpy.random.RandomState(seed) in SORTED key order, so no
weights are stored anywhere. All biases and the bias tables are non-zero (zero biases would hide the rule that a padded
token's q, k, v are the qkv bias); BatchNorm running variances are in [0.5, 2) and about a third of the gammas negative.

err = rel(dev, ref64) = max|dev - ref64| / max|ref64|; a device result must stay within bound(e_ref) =
4 * e_ref + 2 * 2^-24, e_ref being the same measure of this restatement run in float32 on the CPU.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

HEADS = (3, 6, 12, 24)         # SwinTransformer's defaults: SwinPose does not pass NUM_HEADS (:765-773)
WS = 7
SEED = 20261019
CASE_A = dict(cin=480, size=(16, 16), patch=2, emb=48, depths=(2, 2, 2, 2), batch=2, steps=4, joints=21)
CASE_B = dict(cin=3, size=(41, 25), patch=4, emb=96, depths=(2, 2, 2, 2), batch=1, steps=0, joints=21)
FULL = dict(cin=480, size=(64, 64), patch=2, emb=96, depths=(2, 2, 18, 2), batch=1, steps=4, joints=21)
FULL_NO_BACKBONE = dict(cin=3, size=(256, 256), patch=2, emb=96, depths=(2, 2, 18, 2), batch=1, steps=2, joints=21)


def rel(a, b, denom=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() if denom is None else denom))


def bound(e_ref):
    return 4.0 * e_ref + 2.0 * 2.0 ** -24


def rel_index(ws):
    """relative_position_index (:217-226), arithmetically: (ws^2, ws^2) long"""
    n = torch.arange(ws * ws)
    r, c = n // ws, n % ws
    return (r[:, None] - r[None, :] + ws - 1) * (2 * ws - 1) + (c[:, None] - c[None, :] + ws - 1)


# ---- the state dict ----------------------------------------------------------------------------------------------------
def head_keys(cfg, ws=WS):
    """the state-dict entries of SwinPose without backbone.*, in the reference's order, with shapes"""
    e, p, cin = cfg['emb'], cfg['patch'], cfg['cin']
    keys = [('trainable_temp', ()),
            ('swinTransformer.patch_embed.proj.weight', (e, cin, p, p)), ('swinTransformer.patch_embed.proj.bias', (e,)),
            ('swinTransformer.patch_embed.norm.weight', (e,)), ('swinTransformer.patch_embed.norm.bias', (e,))]
    nst = len(cfg['depths'])
    for i, depth in enumerate(cfg['depths']):
        d = e * 2 ** i
        for j in range(depth):
            b = 'swinTransformer.layers.{}.blocks.{}.'.format(i, j)
            keys += [(b + 'norm1.weight', (d,)), (b + 'norm1.bias', (d,)),
                     (b + 'attn.relative_position_bias_table', ((2 * ws - 1) ** 2, HEADS[i])),
                     (b + 'attn.relative_position_index', (ws * ws, ws * ws)),
                     (b + 'attn.qkv.weight', (3 * d, d)), (b + 'attn.qkv.bias', (3 * d,)),
                     (b + 'attn.proj.weight', (d, d)), (b + 'attn.proj.bias', (d,)),
                     (b + 'norm2.weight', (d,)), (b + 'norm2.bias', (d,)),
                     (b + 'feed_forward.fc1.weight', (4 * d, d)), (b + 'feed_forward.fc1.bias', (4 * d,)),
                     (b + 'feed_forward.fc2.weight', (d, 4 * d)), (b + 'feed_forward.fc2.bias', (d,))]
        if i < nst - 1:
            b = 'swinTransformer.layers.{}.downsample.'.format(i)
            keys += [(b + 'reduction.weight', (2 * d, 4 * d)), (b + 'norm.weight', (4 * d,)), (b + 'norm.bias', (4 * d,))]
    for i in range(nst):
        keys += [('swinTransformer.norm{}.weight'.format(i), (e * 2 ** i,)), ('swinTransformer.norm{}.bias'.format(i), (e * 2 ** i,))]
    top = e * 2 ** (nst - 1)
    for s in range(cfg['steps']):
        ci, co, b = top // 2 ** s, top // 2 ** (s + 1), 'decoder.{}.'
        keys += [(b.format(4 * s) + 'weight', (ci, co, 3, 3)), (b.format(4 * s) + 'bias', (co,)),
                 (b.format(4 * s + 1) + 'weight', (co, co, 1, 1)), (b.format(4 * s + 1) + 'bias', (co,)),
                 (b.format(4 * s + 2) + 'weight', (co,)), (b.format(4 * s + 2) + 'bias', (co,)),
                 (b.format(4 * s + 2) + 'running_mean', (co,)), (b.format(4 * s + 2) + 'running_var', (co,)),
                 (b.format(4 * s + 2) + 'num_batches_tracked', ())]
    if cfg['steps']:
        last = 'decoder.{}.'.format(4 * cfg['steps'])
        keys += [(last + 'weight', (cfg['joints'], top // 2 ** cfg['steps'], 1, 1)), (last + 'bias', (cfg['joints'],))]
    return keys


def _is_norm(key):
    stem = key.rsplit('.', 1)[0].rsplit('.', 1)[-1]
    return stem.startswith('norm')


def fill_state_dict(keys_and_shapes, seed=SEED):
    """numpy arrays (float64; the two integer entries int64) drawn from numpy.random.RandomState(seed) in SORTED key order:
    LayerNorm gains U(0.5, 1.5) and biases N(0, 0.2); bias tables N(0, 0.5); matrices and convolutions N(0, 1 / sqrt(fan_in))
    (a transposed convolution (Cin, Cout, 3, 3): fan_in = 9 Cin / 4, the taps that meet one output); other biases N(0, 0.1);
    BatchNorm: |gamma| U(0.5, 1.5) with a third negative, beta N(0, 0.2), running_mean N(0, 0.3), running_var U(0.5, 2);
    trainable_temp U(0.8, 1.5). relative_position_index is computed, num_batches_tracked 0."""
    rng = np.random.RandomState(seed)
    bn = {k.rsplit('.', 1)[0] for k, _ in keys_and_shapes if k.endswith('running_var')}
    out = {}
    for key, shape in sorted(keys_and_shapes):
        shape = tuple(int(s) for s in shape)
        stem, leaf = key.rsplit('.', 1) if '.' in key else ('', key)
        if leaf == 'relative_position_index':
            v = rel_index(int(round(math.sqrt(shape[0])))).numpy().astype(np.int64)
        elif leaf == 'num_batches_tracked':
            v = np.zeros((), dtype=np.int64)
        elif key == 'trainable_temp':
            v = rng.uniform(0.8, 1.5, shape)
        elif leaf == 'relative_position_bias_table':
            v = rng.normal(0.0, 0.5, shape)
        elif stem in bn:
            if leaf == 'weight':
                v = rng.uniform(0.5, 1.5, shape) * np.where(rng.uniform(size=shape) < 1.0 / 3.0, -1.0, 1.0)
            elif leaf == 'running_var':
                v = rng.uniform(0.5, 2.0, shape)
            else:
                v = rng.normal(0.0, 0.3 if leaf == 'running_mean' else 0.2, shape)
        elif _is_norm(key):
            v = rng.uniform(0.5, 1.5, shape) if leaf == 'weight' else rng.normal(0.0, 0.2, shape)
        elif len(shape) == 4 and key.startswith('decoder.') and shape[2] == 3:
            v = rng.normal(0.0, 1.0 / math.sqrt(shape[0] * 9 / 4.0), shape)
        elif len(shape) >= 2:
            v = rng.normal(0.0, 1.0 / math.sqrt(float(np.prod(shape[1:]))), shape)
        else:
            v = rng.normal(0.0, 0.1, shape)
        out[key] = v
    return out


def to_torch(state, dtype):
    return {k: torch.tensor(np.asarray(v), dtype=torch.int64 if np.asarray(v).dtype == np.int64 else dtype)
            for k, v in state.items()}


def inputs(cfg, seed=SEED):
    """N(0, 1) rounded to float16 values (exact in every wider format; the fixture stores them as float16), float64"""
    rng = np.random.RandomState(seed + 1)
    return rng.normal(0.0, 1.0, (cfg['batch'], cfg['cin']) + tuple(cfg['size'])).astype(np.float16).astype(np.float64)


# ---- the ops -----------------------------------------------------------------------------------------------------------
def layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def window_partition(x, ws):
    B, H, W, C = x.shape
    return x.reshape(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def window_reverse(w, ws, B, H, W):
    return w.reshape(B, H // ws, W // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, -1)


def shift_mask(Hp, Wp, ws, shift, dtype):
    """(nW, ws^2, ws^2) of 0 / -100 (:494-510)"""
    band = lambda n: (torch.arange(n) >= n - ws).to(dtype) + (torch.arange(n) >= n - shift).to(dtype)
    img = (3 * band(Hp)[:, None] + band(Wp)[None, :]).reshape(1, Hp, Wp, 1)   # region ids 0 .. 8 of the shifted grid
    m = window_partition(img, ws).reshape(-1, ws * ws)
    d = m[:, None, :] - m[:, :, None]
    return torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))


def window_attention_padded(xp, qkv_w, qkv_b, table, heads, ws, shift, scale):
    """xp (B, Hp, Wp, C), already padded with zeros -> the attention output (B, Hp, Wp, C) before proj (:237-266, :340-363)"""
    B, Hp, Wp, C = xp.shape
    if shift > 0:
        xp = torch.roll(xp, shifts=(-shift, -shift), dims=(1, 2))
    xw = window_partition(xp, ws)                                          # (B nW, N, C)
    N = ws * ws
    qkv = (xw @ qkv_w.t() + qkv_b).reshape(-1, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    attn = (qkv[0] * scale) @ qkv[1].transpose(-2, -1)                     # (B nW, heads, N, N)
    attn = attn + table[rel_index(ws).reshape(-1)].reshape(N, N, heads).permute(2, 0, 1).unsqueeze(0)
    if shift > 0:
        mask = shift_mask(Hp, Wp, ws, shift, xp.dtype)
        nW = mask.shape[0]
        attn = (attn.reshape(B, nW, heads, N, N) + mask[None, :, None]).reshape(-1, heads, N, N)
    out = (torch.softmax(attn, dim=-1) @ qkv[2]).transpose(1, 2).reshape(-1, N, C)
    out = window_reverse(out, ws, B, Hp, Wp)
    if shift > 0:
        out = torch.roll(out, shifts=(shift, shift), dims=(1, 2))
    return out


def window_attention(h, H, W, qkv_w, qkv_b, table, heads, ws, shift):
    """h (B, H W, C), the normalised tokens -> (B, H W, C): pad, attention, crop (:330-368 without proj)"""
    B, L, C = h.shape
    x = F.pad(h.reshape(B, H, W, C), (0, 0, 0, (ws - W % ws) % ws, 0, (ws - H % ws) % ws))
    out = window_attention_padded(x, qkv_w, qkv_b, table, heads, ws, shift, (C // heads) ** -0.5)
    return out[:, :H, :W, :].reshape(B, L, C)


def attention_from_qkv(qkv, qkv_b, table, H, W, heads, ws, shift, scale):
    """what hrnet_swin_attention computes, from a given qkv (B, H W, 3 C) of the unpadded tokens: the padded tokens' rows
    are the qkv bias. Written with an identity qkv linear over the 3 C channels of the padded map."""
    B, L, C3 = qkv.shape
    C = C3 // 3
    x = qkv.reshape(B, H, W, C3)
    pr, pb = (ws - W % ws) % ws, (ws - H % ws) % ws
    xp = qkv_b.reshape(1, 1, 1, C3).expand(B, H + pb, W + pr, C3).clone()
    xp[:, :H, :W] = x
    Hp, Wp = H + pb, W + pr
    if shift > 0:
        xp = torch.roll(xp, shifts=(-shift, -shift), dims=(1, 2))
    xw = window_partition(xp, ws)
    N = ws * ws
    t = xw.reshape(-1, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    attn = (t[0] * scale) @ t[1].transpose(-2, -1)
    attn = attn + table[rel_index(ws).reshape(-1)].reshape(N, N, heads).permute(2, 0, 1).unsqueeze(0)
    if shift > 0:
        mask = shift_mask(Hp, Wp, ws, shift, qkv.dtype)
        attn = (attn.reshape(B, mask.shape[0], heads, N, N) + mask[None, :, None]).reshape(-1, heads, N, N)
    out = (torch.softmax(attn, dim=-1) @ t[2]).transpose(1, 2).reshape(-1, N, C)
    out = window_reverse(out, ws, B, Hp, Wp)
    if shift > 0:
        out = torch.roll(out, shifts=(shift, shift), dims=(1, 2))
    return out[:, :H, :W, :].reshape(B, L, C)


def block(x, H, W, P, b, heads, ws, shift):
    h = layer_norm(x, P[b + 'norm1.weight'], P[b + 'norm1.bias'])
    h = window_attention(h, H, W, P[b + 'attn.qkv.weight'], P[b + 'attn.qkv.bias'],
                         P[b + 'attn.relative_position_bias_table'], heads, ws, shift)
    x = x + h @ P[b + 'attn.proj.weight'].t() + P[b + 'attn.proj.bias']
    h = layer_norm(x, P[b + 'norm2.weight'], P[b + 'norm2.bias'])
    h = gelu(h @ P[b + 'feed_forward.fc1.weight'].t() + P[b + 'feed_forward.fc1.bias'])
    return x + h @ P[b + 'feed_forward.fc2.weight'].t() + P[b + 'feed_forward.fc2.bias']


def merge_gather(x, H, W):
    """(B, H W, C) -> (B, ceil(H / 2) ceil(W / 2), 4 C) (:400-412)"""
    B, L, C = x.shape
    x = F.pad(x.reshape(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
    x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    return x.reshape(B, -1, 4 * C)


def embed_rows(x, p):
    """NCHW -> (B Hp Wp, Cin p p), column c p p + kh p + kw, zero padded right and below (:553-559 as a matrix)"""
    B, Cin, H, W = x.shape
    x = F.pad(x, (0, (p - W % p) % p, 0, (p - H % p) % p))
    Hp, Wp = x.shape[2] // p, x.shape[3] // p
    rows = x.reshape(B, Cin, Hp, p, Wp, p).permute(0, 2, 4, 1, 3, 5).reshape(B * Hp * Wp, Cin * p * p)
    return rows, Hp, Wp


def swin(x, P, cfg, ws=WS):
    """NCHW x -> the last stage's normalised tokens (B, H W, C), H, W (:697-721, last output)"""
    s = 'swinTransformer.'
    w = P[s + 'patch_embed.proj.weight']
    rows, H, W = embed_rows(x, cfg['patch'])
    t = rows @ w.reshape(w.shape[0], -1).t() + P[s + 'patch_embed.proj.bias']
    t = layer_norm(t, P[s + 'patch_embed.norm.weight'], P[s + 'patch_embed.norm.bias']).reshape(x.shape[0], H * W, -1)
    n = len(cfg['depths'])
    for i, depth in enumerate(cfg['depths']):
        for j in range(depth):
            t = block(t, H, W, P, s + 'layers.{}.blocks.{}.'.format(i, j), HEADS[i], ws, 0 if j % 2 == 0 else ws // 2)
        if i < n - 1:
            d = s + 'layers.{}.downsample.'.format(i)
            t = layer_norm(merge_gather(t, H, W), P[d + 'norm.weight'], P[d + 'norm.bias']) @ P[d + 'reduction.weight'].t()
            H, W = (H + 1) // 2, (W + 1) // 2
    k = s + 'norm{}.'.format(n - 1)
    return layer_norm(t, P[k + 'weight'], P[k + 'bias']), H, W


def decoder_step(x, P, s, eps=1e-5):
    """NCHW x -> ConvTranspose2d(3, 2, 1, 1), Conv2d 1x1, eval BatchNorm, ReLU (:790-801), from the definitions: the
    transposed convolution scatters x[i] w[:, :, kh, kw] to output (2 i - 1 + kh, 2 j - 1 + kw)"""
    b = 'decoder.{}.'
    w = P[b.format(4 * s) + 'weight']                                       # (Cin, Cout, 3, 3)
    B, Ci, H, W = x.shape
    full = x.new_zeros(B, w.shape[1], 2 * H + 2, 2 * W + 2)                 # output index + 1
    for kh in range(3):
        for kw in range(3):
            full[:, :, kh:kh + 2 * H:2, kw:kw + 2 * W:2] += torch.einsum('bihw,io->bohw', x, w[:, :, kh, kw])
    y = full[:, :, 1:2 * H + 1, 1:2 * W + 1] + P[b.format(4 * s) + 'bias'].reshape(1, -1, 1, 1)
    w1 = P[b.format(4 * s + 1) + 'weight']
    y = torch.einsum('bihw,oi->bohw', y, w1[:, :, 0, 0]) + P[b.format(4 * s + 1) + 'bias'].reshape(1, -1, 1, 1)
    n = b.format(4 * s + 2)
    y = (y - P[n + 'running_mean'].reshape(1, -1, 1, 1)) / torch.sqrt(P[n + 'running_var'].reshape(1, -1, 1, 1) + eps)
    return torch.relu(y * P[n + 'weight'].reshape(1, -1, 1, 1) + P[n + 'bias'].reshape(1, -1, 1, 1))


def head(x, P, cfg):
    """NCHW features -> heat maps (B, J, Hm, Wm): swinTransformer, decoder, spatial softmax (:820-827)"""
    t, H, W = swin(x, P, cfg)
    y = t.reshape(x.shape[0], H, W, -1).permute(0, 3, 1, 2)
    for s in range(cfg['steps']):
        y = decoder_step(y, P, s)
    last = 'decoder.{}.'.format(4 * cfg['steps'])
    y = torch.einsum('bihw,oi->bohw', y, P[last + 'weight'][:, :, 0, 0]) + P[last + 'bias'].reshape(1, -1, 1, 1)
    return torch.softmax(y.flatten(2) * P['trainable_temp'], dim=2).reshape(y.shape)


def run(cfg, dtype, seed=SEED, x=None):
    """the case's result as a float64 numpy array: heat maps (steps > 0) or the last stage's tokens"""
    P = to_torch(fill_state_dict(head_keys(cfg), seed), dtype)
    x = torch.tensor(inputs(cfg, seed) if x is None else np.asarray(x), dtype=dtype)
    with torch.no_grad():
        y = head(x, P, cfg) if cfg['steps'] else swin(x, P, cfg)[0]
    return y.double().numpy()
