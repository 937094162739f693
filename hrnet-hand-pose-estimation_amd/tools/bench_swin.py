"""Timing of the SwinPose head of swin_transformer (csrc/swin.hip and csrc/transformer.hip through hipnet.swin and
hipnet.transformer, the decoder on the f32 NHWC convolution entry) at the v3 yaml's size - 480-channel 64x64 features,
PATCH_SIZE 2, EMB_DIM 96, DEPTHS 2 / 2 / 18 / 2 - against the same head built from torch ops on the device:

    python tools/bench_swin.py [--batches 1 32] [--repeats 20] [--warmup 3]
    python tools/bench_swin.py --counts-only          (no device: launches and bytes per stage)
    python tools/bench_swin.py --train [--counts-only]   (the head's training step: forward + backward)

`counts(B)` is the cost model: per stage (embed, stage0 .. stage3 with their patch merging, norm, decoder) the launches of
one eval forward, the bytes of weights read and of activations read and written, and the floor those bytes give at the
achievable HBM rate.

The baseline is the reference's composition (lib/models/swin_transformer.py: pad, roll, window partition, masked attention,
reverse; F.conv_transpose2d, F.conv2d, F.batch_norm) from torch ops on the model's own parameters, in the same process on the
same inputs, eval mode under no_grad, timed with device events after a warm-up, alternating with the HIP path; medians
with the spread (min .. max) over the repeats, for the whole head and per stage. Without a HIP device the timing mode
fails: there is no fallback.

--train times one training step of the head, forward + backward (hipnet.swin_train and hipnet.transformer under autograd,
SwinPose(trainable=True, drop_path_rate=0) in training mode: batch-statistic BatchNorm, every activation materialised)
against the same head from torch ops with autograd on the same parameters, alternating, medians of --repeats after
--warmup, and appends the spread to profiles/swin_train_times.txt. `train_counts(B)` is its cost model: kernel launches
of the forward and of the backward per stage, and the bytes they move. No ratio is promised.
"""
import argparse
import json
import os
import statistics
import sys

import _init_paths  # noqa: F401

HBM_BYTES_PER_S = 6.3e12          # achievable HBM rate of the MI355X
HEADS, WS = (3, 6, 12, 24), 7
YAML = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'experiments', 'RHD',
                    'RHD_HRNet_w32_SwinTransformer_v3.yaml')
SHAPE = dict(cin=480, size=64, patch=2, emb=96, depths=(2, 2, 18, 2), steps=4, joints=21)


def counts(B, shape=SHAPE):
    """launches, weight bytes and activation bytes of one eval forward of the head, per stage and in total"""
    stages = {}

    def add(name, launches, weights, acts):
        s = stages.setdefault(name, {'launches': 0, 'weight_bytes': 0, 'activation_bytes': 0})
        s['launches'] += launches
        s['weight_bytes'] += 4 * weights
        s['activation_bytes'] += 4 * acts

    e, p, cin = shape['emb'], shape['patch'], shape['cin']
    H = W = (shape['size'] + p - 1) // p
    K = cin * p * p
    rows = B * H * W
    add('embed', 3, K * e + e + 2 * e, B * cin * shape['size'] ** 2 + 2 * rows * K + 3 * rows * e)
    for i, depth in enumerate(shape['depths']):
        c, name = e * 2 ** i, 'stage{}'.format(i)
        rows = B * H * W
        table = (2 * WS - 1) ** 2 * HEADS[i]
        for _ in range(depth):
            # LayerNorm, qkv, attention, proj + residual, LayerNorm, fc1 + GELU, fc2 + residual
            add(name, 7, 2 * c + 3 * c * c + 3 * c + table + 3 * c + c * c + c + 2 * c + 8 * c * c + 5 * c,
                rows * (2 * c + 4 * c + 4 * c + 3 * c + 2 * c + 5 * c + 6 * c))
        if i < len(shape['depths']) - 1:
            H2, W2 = (H + 1) // 2, (W + 1) // 2
            add(name, 2, 8 * c + 8 * c * c, rows * c + B * H2 * W2 * (4 * c + 4 * c + 2 * c))
            H, W = H2, W2
    c = e * 2 ** (len(shape['depths']) - 1)
    add('norm', 1, 2 * c, 2 * B * H * W * c)
    for s in range(shape['steps']):
        co = c // 2
        # transposed convolution + bias (reads the folded scale / shift of the step before), then the 1x1
        add('decoder', 2, 9 * c * co + co + (2 * c if s else 0) + co * co, B * H * W * c + 3 * B * 4 * H * W * co)
        c, H, W = co, 2 * H, 2 * W
    jp = (shape['joints'] + 15) // 16 * 16
    add('decoder', 3, c * jp + jp + 2 * c + 1, B * H * W * (c + 2 * jp + 3 * shape['joints']))
    total = {k: sum(s[k] for s in stages.values()) for k in ('launches', 'weight_bytes', 'activation_bytes')}
    total['floor_us'] = 1e6 * (total['weight_bytes'] + total['activation_bytes']) / HBM_BYTES_PER_S
    return {'launches_per_block': 7, 'blocks': sum(shape['depths']), 'stages': stages, 'total': total}


def train_counts(B, shape=SHAPE):
    """launches (forward, backward) and bytes of one training step of the head, per stage and in total. Launches are the
    kernels inside the C entries: LayerNorm backward 3 (dx, column partials, their sum), linear backward 2 (dx; dW with
    db), attention backward 2 (the window kernel, the partial-row sum), BatchNorm statistics 3, apply 1, backward 3, weight
    gradient 2 (slabs, reduce), bias gradient 2, packing 1. torch's own launches (the gradient accumulation where a tensor
    feeds two consumers: 3 per block; the zero-padded copies of the decoder's vectors) are listed apart."""
    stages = {}

    def add(name, fwd, bwd, weights, acts, torch_ops=0):
        s = stages.setdefault(name, {'forward_launches': 0, 'backward_launches': 0, 'torch_launches': 0,
                                     'weight_bytes': 0, 'activation_bytes': 0})
        s['forward_launches'] += fwd
        s['backward_launches'] += bwd
        s['torch_launches'] += torch_ops
        s['weight_bytes'] += 4 * weights
        s['activation_bytes'] += 4 * acts

    e, p, cin = shape['emb'], shape['patch'], shape['cin']
    H = W = (shape['size'] + p - 1) // p
    K = cin * p * p
    rows = B * H * W
    # rows gather, linear, LayerNorm | LayerNorm, linear (dx for the feature gradient, dW), rows scatter
    add('embed', 3, 3 + 2 + 1, 3 * (K * e + 3 * e), B * cin * shape['size'] ** 2 * 2 + rows * (6 * K + 11 * e))
    for i, depth in enumerate(shape['depths']):
        c, name = e * 2 ** i, 'stage{}'.format(i)
        rows = B * H * W
        table = (2 * WS - 1) ** 2 * HEADS[i]
        nwin = ((H + WS - 1) // WS) * ((W + WS - 1) // WS)
        scratch = 2 * 2 * B * nwin * HEADS[i] * ((2 * WS - 1) ** 2 + 2 * c // HEADS[i])
        for _ in range(depth):
            # forward as inference + the stored GELU pre-activation; backward: 2 LayerNorms (x and dy twice, dx), 4 linears
            # (dy twice, x, dx, the pre-activation twice), the attention (qkv, dout, dqkv, the f64 partial rows twice)
            add(name, 7, 2 * 3 + 4 * 2 + 2, 3 * (12 * c * c + 13 * c + table),
                rows * (26 + 4) * c + rows * (10 + 8 + 7 + 4 + 18 + 10) * c + scratch, torch_ops=3)
        if i < len(shape['depths']) - 1:
            H2, W2 = (H + 1) // 2, (W + 1) // 2
            r2 = B * H2 * W2
            add(name, 3, 2 + 3 + 1, 3 * (8 * c + 8 * c * c), rows * c * 2 + r2 * (4 * c * 4 + 2 * c) + r2 * (4 * c * 8 + 2 * c * 2))
            H, W = H2, W2
    c = e * 2 ** (len(shape['depths']) - 1)
    add('norm', 1, 3, 3 * 2 * c, 7 * B * H * W * c)
    for s in range(shape['steps']):
        co = c // 2
        big = B * 4 * H * W * co
        # pack 2, convolutions 2, statistics 3, apply 1 | BatchNorm 3, 1x1: weight gradient 2, pack 1, input gradient 1;
        # transposed: bias gradient 2, weight gradient 2, pack 1, input gradient 1
        add('decoder', 8, 13, 4 * (9 * c * co + co * co) + 12 * co, B * H * W * c * 4 + big * (2 + 2 + 3 + 2) + big * (5 + 4 + 3),
            torch_ops=8)
        c, H, W = co, 2 * H, 2 * W
    jp = (shape['joints'] + 15) // 16 * 16
    # pack, 1x1, layout, softmax | softmax, layout, pack, input gradient, weight gradient 2, bias gradient 2
    add('decoder', 4, 8, 4 * (c * jp + jp), B * H * W * (3 * c + 6 * jp + 8 * shape['joints']), torch_ops=3)
    total = {k: sum(s[k] for s in stages.values()) for k in ('forward_launches', 'backward_launches', 'torch_launches',
                                                             'weight_bytes', 'activation_bytes')}
    total['floor_us'] = 1e6 * (total['weight_bytes'] + total['activation_bytes']) / HBM_BYTES_PER_S
    return {'blocks': sum(shape['depths']), 'stages': stages, 'total': total}


# ---- the head from torch ops ------------------------------------------------------------------------------------------
def _shift_mask(Hp, Wp, ws, shift, device):
    import torch
    band = lambda n: ((torch.arange(n, device=device) >= n - ws).float() +
                      (torch.arange(n, device=device) >= n - shift).float())
    img = 3 * band(Hp)[:, None] + band(Wp)[None, :]        # region ids of the shifted grid
    m = img.reshape(1, Hp // ws, ws, Wp // ws, ws, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws)
    d = m.unsqueeze(1) - m.unsqueeze(2)
    return d.masked_fill(d != 0, -100.0).masked_fill(d == 0, 0.0)


def _torch_block(x, H, W, blk, mask):
    import torch
    import torch.nn.functional as Fn
    B, L, C = x.shape
    ws, shift, a = blk.window_size, blk.shift_size, blk.attn
    h = Fn.layer_norm(x, (C,), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps).view(B, H, W, C)
    h = Fn.pad(h, (0, 0, 0, (ws - W % ws) % ws, 0, (ws - H % ws) % ws))
    Hp, Wp = h.shape[1], h.shape[2]
    if shift > 0:
        h = torch.roll(h, shifts=(-shift, -shift), dims=(1, 2))
    h = h.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)
    N = ws * ws
    qkv = Fn.linear(h, a.qkv.weight, a.qkv.bias).reshape(-1, N, 3, a.num_heads, C // a.num_heads).permute(2, 0, 3, 1, 4)
    attn = (qkv[0] * a.scale) @ qkv[1].transpose(-2, -1)
    bias = a.relative_position_bias_table[a.relative_position_index.view(-1)].view(N, N, -1).permute(2, 0, 1).contiguous()
    attn = attn + bias.unsqueeze(0)
    if shift > 0:
        nW = mask.shape[0]
        attn = (attn.view(-1, nW, a.num_heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, a.num_heads, N, N)
    h = (torch.softmax(attn, dim=-1) @ qkv[2]).transpose(1, 2).reshape(-1, N, C)
    h = Fn.linear(h, a.proj.weight, a.proj.bias)
    h = h.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift > 0:
        h = torch.roll(h, shifts=(shift, shift), dims=(1, 2))
    x = x + h[:, :H, :W, :].reshape(B, L, C)
    f = blk.feed_forward
    h = Fn.layer_norm(x, (C,), blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
    return x + Fn.linear(Fn.gelu(Fn.linear(h, f.fc1.weight, f.fc1.bias)), f.fc2.weight, f.fc2.bias)


class TorchPath(object):
    def __init__(self, model):
        self.m = model

    def embed(self, x):
        import torch.nn.functional as Fn
        pe = self.m.swinTransformer.patch_embed
        p = pe.patch_size
        x = Fn.pad(x, (0, (p - x.shape[3] % p) % p, 0, (p - x.shape[2] % p) % p))
        x = Fn.conv2d(x, pe.proj.weight, pe.proj.bias, stride=p)
        H, W = x.shape[2], x.shape[3]
        return Fn.layer_norm(x.flatten(2).transpose(1, 2), (pe.embed_dim,), pe.norm.weight, pe.norm.bias, pe.norm.eps), H, W

    def stage(self, i, t, H, W):
        import torch
        import torch.nn.functional as Fn
        layer = self.m.swinTransformer.layers[i]
        ws = layer.window_size
        Hp, Wp = (H + ws - 1) // ws * ws, (W + ws - 1) // ws * ws
        mask = _shift_mask(Hp, Wp, ws, layer.shift_size, t.device)
        for blk in layer.blocks:
            t = _torch_block(t, H, W, blk, mask)
        if layer.downsample is not None:
            d = layer.downsample
            B, L, C = t.shape
            x = Fn.pad(t.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
            x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).view(B, -1, 4 * C)
            t = Fn.linear(Fn.layer_norm(x, (4 * C,), d.norm.weight, d.norm.bias, d.norm.eps), d.reduction.weight)
            H, W = (H + 1) // 2, (W + 1) // 2
        return t, H, W

    def norm(self, t, H, W):
        import torch.nn.functional as Fn
        n = getattr(self.m.swinTransformer, 'norm{}'.format(self.m.swinTransformer.num_layers - 1))
        return Fn.layer_norm(t, (t.shape[2],), n.weight, n.bias, n.eps), H, W

    def decoder(self, t, H, W):
        import torch
        y = self.m.decoder(t.view(t.shape[0], H, W, -1).permute(0, 3, 1, 2).contiguous())
        return torch.softmax(y.flatten(2) * self.m.trainable_temp, dim=2).view(y.shape)


class HipPath(object):
    def __init__(self, model):
        self.m = model

    def embed(self, x):
        return self.m.swinTransformer.patch_embed.run(x)

    def stage(self, i, t, H, W):
        layer = self.m.swinTransformer.layers[i]
        for blk in layer.blocks:
            t = blk.run(t, H, W)
        if layer.downsample is not None:
            t = layer.downsample.run(t, H, W)
            H, W = (H + 1) // 2, (W + 1) // 2
        return t, H, W

    def norm(self, t, H, W):
        from hipnet import transformer as T
        n = getattr(self.m.swinTransformer, 'norm{}'.format(self.m.swinTransformer.num_layers - 1))
        return T.layer_norm(t, n.weight, n.bias, n.eps), H, W

    def decoder(self, t, H, W):
        return self.m.decoder_forward(t, H, W)


def _stages(path, n):
    """[(name, fn(state) -> state)]: state is the argument tuple of the next stage"""
    out = [('embed', lambda s: path.embed(*s))]
    for i in range(n):
        out.append(('stage{}'.format(i), lambda s, i=i: path.stage(i, *s)))
    out.append(('norm', lambda s: path.norm(*s)))
    out.append(('decoder', lambda s: (path.decoder(*s),)))
    return out


def _time(fn, start, stop):
    import torch
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3          # us


def measure(B, repeats, warmup):
    import torch
    from config import get_cfg_defaults
    from models import swin_transformer
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    torch.manual_seed(0)
    model = swin_transformer.get_pose_net(cfg, is_train=False).cuda().eval()
    with torch.no_grad():
        for k, v in model.named_parameters():                # non-trivial tables, biases and BatchNorm statistics
            if k.endswith(('relative_position_bias_table', '.bias')):
                v.normal_(0.0, 0.2)
        for k, v in model.named_buffers():
            if k.endswith('running_var'):
                v.uniform_(0.5, 2.0)
            elif k.endswith('running_mean'):
                v.normal_(0.0, 0.3)
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(B, SHAPE['cin'], SHAPE['size'], SHAPE['size'], device='cuda', generator=g)
    n = model.swinTransformer.num_layers
    paths = {'hip': _stages(HipPath(model), n), 'torch': _stages(TorchPath(model), n)}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {}
    with torch.no_grad():
        states, outs = {}, {}
        for name, stages in paths.items():                   # the inputs of every stage, and the result
            s, states[name] = (x,), []
            for _, fn in stages:
                states[name].append(s)
                s = fn(s)
            outs[name] = s[0]
        diff = float((outs['hip'] - outs['torch']).abs().max() / outs['torch'].abs().max())

        def whole(stages):
            s = (x,)
            for _, fn in stages:
                s = fn(s)

        for r in range(warmup + repeats):
            for name, stages in paths.items():
                t = _time(lambda: whole(stages), start, stop)
                if r >= warmup:
                    times.setdefault('head_' + name, []).append(t)
                for (label, fn), s in zip(stages, states[name]):
                    t = _time(lambda: fn(s), start, stop)
                    if r >= warmup:
                        times.setdefault(label + '_' + name, []).append(t)
    out = {k: {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)} for k, v in times.items()}
    out['relative_difference_of_the_two_heads'] = diff
    return out


def measure_train(B, repeats, warmup):
    """forward + backward of the head in training mode: the HIP path under autograd and the torch composition under
    autograd, on the same parameters and inputs, alternating; the gradient of a fixed random weighting of the heat maps"""
    import torch
    from config import get_cfg_defaults
    from models import swin_transformer
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    torch.manual_seed(0)
    model = swin_transformer.get_pose_net(cfg, is_train=True, trainable=True, drop_path_rate=0.).cuda().train()
    with torch.no_grad():
        for k, v in model.named_parameters():
            if k.endswith(('relative_position_bias_table', '.bias')):
                v.normal_(0.0, 0.2)
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(B, SHAPE['cin'], SHAPE['size'], SHAPE['size'], device='cuda', generator=g).requires_grad_(True)
    wgt = torch.randn(B, SHAPE['joints'], SHAPE['size'], SHAPE['size'], device='cuda', generator=g)
    params = [v for k, v in model.named_parameters() if not k.startswith('backbone.') and v.requires_grad]
    tp, n = TorchPath(model), model.swinTransformer.num_layers

    def torch_head():
        s = tp.embed(x)
        for i in range(n):
            s = tp.stage(i, *s)
        return tp.decoder(*tp.norm(*s))

    heads = {'hip': lambda: model.head_forward(x), 'torch': torch_head}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times, grads = {}, {}

    def step(name):
        out = heads[name]()
        grads[name] = torch.autograd.grad((out * wgt).sum(), [x] + params, allow_unused=True)[0]

    for r in range(warmup + repeats):
        for name in heads:
            t = _time(lambda: step(name), start, stop)
            if r >= warmup:
                times.setdefault('train_' + name, []).append(t)
            t = _time(lambda: heads[name](), start, stop)
            if r >= warmup:
                times.setdefault('forward_' + name, []).append(t)
    out = {k: {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)} for k, v in times.items()}
    out['relative_difference_of_the_two_feature_gradients'] = float(
        (grads['hip'] - grads['torch']).abs().max() / grads['torch'].abs().max())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32])
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--counts-only', action='store_true')
    ap.add_argument('--train', action='store_true', help='time the training step of the head (forward + backward)')
    args = ap.parse_args(argv)
    if not args.counts_only:
        import torch
        if not torch.cuda.is_available():
            sys.exit('bench_swin: no HIP device: the timings need one (--counts-only prints the cost model)')
    if args.train:
        lines = []
        for B in args.batches:
            row = {'B': B, 'train_counts': train_counts(B)}
            if not args.counts_only:
                row['times'] = t = measure_train(B, args.repeats, args.warmup)
                row['train_ratio_torch_over_hip'] = t['train_torch']['median_us'] / t['train_hip']['median_us']
                lines.append('B {:3d}  '.format(B) + '  '.join('{} {:.0f} ({:.0f} .. {:.0f}) us'.format(
                    k, v['median_us'], v['min_us'], v['max_us']) for k, v in sorted(t.items()) if isinstance(v, dict)))
            print(json.dumps(row))
        if lines:
            path = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), 'profiles',
                                'swin_train_times.txt')
            with open(path, 'a') as f:
                f.write('bench_swin.py --train: median (min .. max) of {} after {} warm-ups\n'.format(
                    args.repeats, args.warmup) + '\n'.join(lines) + '\n')
        return
    for B in args.batches:
        row = {'B': B, 'counts': counts(B)}
        if not args.counts_only:
            row['times'] = t = measure(B, args.repeats, args.warmup)
            row['head_ratio_torch_over_hip'] = t['head_torch']['median_us'] / t['head_hip']['median_us']
        print(json.dumps(row))


if __name__ == '__main__':
    main()
