"""Plain-torch restatement of the PoseFormer head of pose_hrnet_transformer (reference
lib/models/pose_hrnet_transformer.py:21-85 Mlp / Attention / Block, :162-192 the modules, :195-237 the forward) and of
each op the HIP kernels implement, runnable in float64 and float32 on the CPU. Functional: the parameters come as a
dict with the reference's state-dict keys.

tests/golden/make_golden_poseformer.py checks `head` against the reference's own float64 run (1e-10 of max|y|) and
records the numbers below in tests/golden/poseformer.npz.

Recorded with fill_state_dict(seed 20261019) and poses uniform in [0, 64), the restatement in float32 against float64,
as a fraction of max|.| (make_golden_poseformer.py prints them):
    (S, F, J) = (4, 9, 21): max|y| 2.62, forward 7.0e-07, pose gradient 5.3e-07, worst stored parameter gradient 1.9e-06
    (2, 5, 21):             max|y| 2.95, forward 5.3e-07, pose gradient 1.1e-06, worst stored parameter gradient 1.7e-06
    (1, 1, 21):             max|y| 2.59, forward 5.5e-07, pose gradient 8.6e-07, worst stored parameter gradient 2.0e-05
(the reference's own float32 forward: 7.7e-07, 4.8e-07, 5.6e-07). The head has 110 state-dict entries and, at F = 9,
14,552,276 parameters.
"""
import math

import numpy as np
import torch

EMBED = 32                     # reference :109
DEPTH = 4                      # :110
HEADS = 8                      # :111
MLP_RATIO = 2                  # :112
DROP_PATH_RATE = 0.2           # :117
NORM_EPS = 1e-6                # :119
HEAD_NORM_EPS = 1e-5           # :190, a plain nn.LayerNorm
SEED = 20261019


def drop_rates():
    """torch.linspace(0, 0.2, 4) (:169), spatial block i and temporal block i share rate i"""
    return [float(x) for x in torch.linspace(0, DROP_PATH_RATE, DEPTH)]


def _block_keys(prefix, dim):
    hid = int(dim * MLP_RATIO)
    return [(prefix + '.norm1.weight', (dim,)), (prefix + '.norm1.bias', (dim,)),
            (prefix + '.attn.qkv.weight', (3 * dim, dim)), (prefix + '.attn.qkv.bias', (3 * dim,)),
            (prefix + '.attn.proj.weight', (dim, dim)), (prefix + '.attn.proj.bias', (dim,)),
            (prefix + '.norm2.weight', (dim,)), (prefix + '.norm2.bias', (dim,)),
            (prefix + '.mlp.fc1.weight', (hid, dim)), (prefix + '.mlp.fc1.bias', (hid,)),
            (prefix + '.mlp.fc2.weight', (dim, hid)), (prefix + '.mlp.fc2.bias', (dim,))]


def head_keys(F, J):
    """the head's state-dict entries (everything but backbone.*) in the reference's order, with shapes"""
    D = EMBED * J
    keys = [('Spatial_pos_embed', (1, J, EMBED)), ('Temporal_pos_embed', (1, F, D)),
            ('Spatial_patch_to_embedding.weight', (EMBED, 2)), ('Spatial_patch_to_embedding.bias', (EMBED,))]
    for i in range(DEPTH):
        keys += _block_keys('Spatial_blocks.{}'.format(i), EMBED)
    for i in range(DEPTH):
        keys += _block_keys('blocks.{}'.format(i), D)
    keys += [('Spatial_norm.weight', (EMBED,)), ('Spatial_norm.bias', (EMBED,)),
             ('Temporal_norm.weight', (D,)), ('Temporal_norm.bias', (D,)),
             ('weighted_mean.weight', (1, F, 1)), ('weighted_mean.bias', (1,)),
             ('head.0.weight', (D,)), ('head.0.bias', (D,)), ('head.1.weight', (2 * J, D)), ('head.1.bias', (2 * J,))]
    return keys


def _is_norm(key):
    stem = key.rsplit('.', 1)[0]
    return stem.endswith(('norm1', 'norm2', 'Spatial_norm', 'Temporal_norm', 'head.0'))


def fill_state_dict(keys_and_shapes, seed=SEED):
    """float64 numpy arrays drawn from numpy.random.default_rng(seed) in SORTED key order:
    position embeddings N(0, 0.5); norm gains U(0.5, 1.5), norm biases N(0, 0.2); matrices N(0, 1 / sqrt(fan_in)) with
    fan_in = shape[1]; other biases N(0, 0.1)"""
    rng = np.random.default_rng(seed)
    out = {}
    for key, shape in sorted(keys_and_shapes):
        if key.endswith('pos_embed'):
            v = rng.normal(0.0, 0.5, shape)
        elif _is_norm(key):
            v = rng.uniform(0.5, 1.5, shape) if key.endswith('weight') else rng.normal(0.0, 0.2, shape)
        elif len(shape) >= 2:
            v = rng.normal(0.0, 1.0 / math.sqrt(shape[1]), shape)
        else:
            v = rng.normal(0.0, 0.1, shape)
        out[key] = v
    return out


def to_torch(state, dtype, requires_grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(requires_grad) for k, v in state.items()}


# ---- the ops ----------------------------------------------------------------------------------------------------------
def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def linear(x, w, b=None, act=None, residual=None, row_scale=None):
    y = x @ w.t()
    if b is not None:
        y = y + b
    if act == 'gelu':
        y = gelu(y)
    if row_scale is not None:
        y = y * row_scale.reshape(y.shape[:-1] + (1,))
    if residual is not None:
        y = residual + y
    return y


def attention(qkv, heads, scale):
    """qkv (S, N, 3 C) packed [q | k | v], each (heads, hd) -> (S, N, C) (reference :53-62)"""
    S, N, C3 = qkv.shape
    C = C3 // 3
    t = qkv.reshape(S, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    a = torch.softmax((q @ k.transpose(-2, -1)) * scale, dim=-1)
    return (a @ v).transpose(1, 2).reshape(S, N, C)


def frame_mean(x, w, b=None):
    """Conv1d(F -> 1, kernel 1) over (S, F, D) (reference :187, :219)"""
    y = (x * w.reshape(1, -1, 1)).sum(1)
    return y if b is None else y + b.reshape(1, 1)


def block(x, P, prefix, dim, scale_a=None, scale_m=None):
    """x (sequences, N, dim); scale_a / scale_m: per-sequence stochastic-depth factors keep / (1 - r), or None"""
    n, N = x.shape[:2]
    rs = lambda s: None if s is None else s.reshape(n, 1).expand(n, N)
    h = layer_norm(x, P[prefix + '.norm1.weight'], P[prefix + '.norm1.bias'], NORM_EPS)
    qkv = linear(h, P[prefix + '.attn.qkv.weight'], P[prefix + '.attn.qkv.bias'])
    a = attention(qkv, HEADS, (dim // HEADS) ** -0.5)
    x = linear(a, P[prefix + '.attn.proj.weight'], P[prefix + '.attn.proj.bias'], residual=x, row_scale=rs(scale_a))
    h = layer_norm(x, P[prefix + '.norm2.weight'], P[prefix + '.norm2.bias'], NORM_EPS)
    h = linear(h, P[prefix + '.mlp.fc1.weight'], P[prefix + '.mlp.fc1.bias'], act='gelu')
    return linear(h, P[prefix + '.mlp.fc2.weight'], P[prefix + '.mlp.fc2.bias'], residual=x, row_scale=rs(scale_m))


def head(p, P, drop_flags=None):
    """p (S, F, J, 2) poses in heat-map pixels, P the head's parameters -> (S, J, 2). drop_flags: None (eval mode) or 16
    tensors of 0 / 1 keep flags - spatial blocks then temporal blocks, two per block (attention branch, mlp branch), of
    S * F values (spatial) and S values (temporal); a kept branch is divided by 1 - r, a dropped one is zero"""
    S, F, J, _ = p.shape
    D = EMBED * J
    rates = drop_rates()

    def scale(idx, i):
        if drop_flags is None:
            return None
        return drop_flags[idx].to(p.dtype) / (1.0 - rates[i])

    x = linear(p.reshape(S * F, J, 2), P['Spatial_patch_to_embedding.weight'], P['Spatial_patch_to_embedding.bias'])
    x = x + P['Spatial_pos_embed']
    for i in range(DEPTH):
        x = block(x, P, 'Spatial_blocks.{}'.format(i), EMBED, scale(2 * i, i), scale(2 * i + 1, i))
    x = layer_norm(x, P['Spatial_norm.weight'], P['Spatial_norm.bias'], NORM_EPS)
    x = x.reshape(S, F, D) + P['Temporal_pos_embed']
    for i in range(DEPTH):
        x = block(x, P, 'blocks.{}'.format(i), D, scale(2 * DEPTH + 2 * i, i), scale(2 * DEPTH + 2 * i + 1, i))
    x = layer_norm(x, P['Temporal_norm.weight'], P['Temporal_norm.bias'], NORM_EPS)
    x = frame_mean(x, P['weighted_mean.weight'], P['weighted_mean.bias'])
    x = layer_norm(x, P['head.0.weight'], P['head.0.bias'], HEAD_NORM_EPS)
    return linear(x, P['head.1.weight'], P['head.1.bias']).reshape(S, J, 2)


# ---- the fixture's conventions -----------------------------------------------------------------------------------------
SHAPES = ((4, 9, 21), (2, 5, 21), (1, 1, 21))
# the parameter gradients the fixture stores: every parameter of one spatial block, one of each kind of one temporal
# block, both position embeddings, both final norms, weighted_mean.*, head.*
STORED = (['Spatial_pos_embed', 'Temporal_pos_embed', 'Spatial_patch_to_embedding.weight',
           'Spatial_patch_to_embedding.bias'] + [k for k, _ in _block_keys('Spatial_blocks.1', EMBED)] +
          [k for k, _ in _block_keys('blocks.2', EMBED)] +
          ['Spatial_norm.weight', 'Spatial_norm.bias', 'Temporal_norm.weight', 'Temporal_norm.bias',
           'weighted_mean.weight', 'weighted_mean.bias', 'head.0.weight', 'head.0.bias', 'head.1.weight', 'head.1.bias'])


def sample(g):
    """what the fixture keeps of a gradient: all of a small tensor, rows ::29 and columns ::23 of a matrix of more than
    8192 elements (the temporal matrices are up to 2016 x 672)"""
    g = np.asarray(g)
    return g[::29, ::23] if g.ndim == 2 and g.size > 8192 else g


def tag(S, F, J):
    return 's{}f{}j{}'.format(S, F, J)


def inputs(S, F, J, seed=SEED):
    """(poses (S, F, J, 2) uniform in [0, 64), cotangent g (S, J, 2) standard normal), float64 numpy"""
    rng = np.random.default_rng((seed, S, F, J))
    return rng.uniform(0.0, 64.0, (S, F, J, 2)), rng.normal(0.0, 1.0, (S, J, 2))


def run(p, g, state, dtype, drop_flags=None, wanted=STORED):
    """the restatement's forward and gradients of sum(y * g): (y, dp, {key: full gradient}) as float64 numpy"""
    P = to_torch(state, dtype, requires_grad=True)
    pt = torch.tensor(p, dtype=dtype, requires_grad=True)
    y = head(pt, P, drop_flags)
    (y * torch.tensor(g, dtype=dtype)).sum().backward()
    grads = {k: (P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])).double().numpy() for k in wanted}
    return y.detach().double().numpy(), pt.grad.double().numpy(), grads


def rel(a, b, denom=None):
    """max|a - b| / max|b| (or / denom)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = float(np.abs(b).max()) if denom is None else float(denom)
    return float(np.abs(a - b).max()) / d if d > 0 else float(np.abs(a - b).max())


def bound(e_ref):
    """the project's convention (tests/test_v2v_gpu.py): four times the float32 restatement's own error plus two float32
    roundings"""
    return 4.0 * e_ref + 2.0 * 2.0 ** -24
