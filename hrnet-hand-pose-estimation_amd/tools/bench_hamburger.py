"""Timing of the HamNet head of pose_hrnet_hamburger (csrc/nmf.hip through hipnet.nmf, the convolutions on the f32 NHWC
convolution entry) at the v2 yaml's size - 480-channel 64x64 features, EMB_DIM 512, R 512, DUAL_HAM, six steps - against
the same head built from torch ops on the device:

    python tools/bench_hamburger.py [--batches 1 4] [--repeats 10] [--warmup 2] [--out <file>]
    python tools/bench_hamburger.py --counts-only          (no device: launches, FLOPs and bytes per stage)

`counts(B)` is the cost model: per stage (layout, squeeze, lower_bread, ham_spatial, ham_channel, cheese, upper_bread,
align, fc) the launches of one eval forward through the C ABI, the torch element-wise launches beside them, the FLOPs of
the products, the bytes every launch must at least read and write, and the floor those give at the f32 MFMA rate and the
achievable HBM rate.

The baseline is the reference's composition (lib/models/hamburger/: F.conv2d, F.batch_norm, view / transpose, torch.bmm,
element-wise ratio, torch.cat) from torch ops on the model's own parameters, in the same process, on the same features and
the same bases, eval mode under no_grad, timed with device events after a warm-up, alternating with the HIP path; medians
with the spread (min .. max) over the repeats, for the whole head and for the two hams alone. The host draw of the bases
(torch.rand on the CPU generator, as the reference draws them) and their upload are timed apart: both heads pay them.
The result is appended to --out (default profiles/hamburger_head_times.txt). Without a HIP device the timing mode fails:
there is no fallback. No ratio is promised.

    python tools/bench_hamburger.py --train [--counts-only]

times one training step of the head - forward and backward with every parameter gradient, HamNet(trainable=True) through
hipnet.burger_train and hipnet.nmf_train - against the same head from torch ops under autograd (F.batch_norm on batch
statistics, the TRAIN_STEPS updates under no_grad, compute_coef with gradient): same parameters, bases and keep mask.
`train_counts(B)` is its cost model, with the stages `mix` and `dropout` of csrc/burger_train.hip.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import _init_paths  # noqa: F401

HBM_BYTES_PER_S = 6.3e12          # achievable HBM rate of the MI355X
F32_MFMA_FLOPS = 155e12           # measured f32 MFMA rate (there is no xf32 on gfx950)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
YAML = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'experiments', 'RHD',
                    'RHD_HRNet_w32_Hamburger_v2.yaml')
SHAPE = dict(cin=480, size=64, emb=512, R=512, S=1, dual=True, spatial=True, cheese=1, steps=6, joints=21, align=256)


def ham_counts(G, D, N, R, steps, split):
    """one NMF2D on G matrices (D, N): launches, FLOPs and the floats every launch reads and writes at least; split(G, K, R)
    tells whether the Gram matrix over K rows takes the second, adding launch"""
    gram = lambda K: (2 if split(G, K, R) else 1, 2 * G * K * R * R, G * (K * R + R * R))
    upd = lambda M, K: (1, 2 * G * M * R * (K + R), G * (2 * M * R + K * R + M * K + R * R))
    ops = [(1, 2 * G * N * D * R, G * (D * N + D * R + N * R)), (1, 0, 2 * G * N * R)]         # logits, softmax
    for _ in range(steps):
        ops += [gram(D), upd(N, D), gram(N), upd(D, N)]
    ops += [gram(D), upd(N, D), (1, 2 * G * D * N * R, G * (D * R + N * R + D * N))]           # last update, reconstruction
    return tuple(sum(o[i] for o in ops) for i in range(3))


def counts(B, shape=SHAPE, split=None):
    """launches, FLOPs and bytes of one eval forward of the head, per stage and in total"""
    if split is None:
        from hipnet import nmf
        split = lambda G, K, R: nmf.gram_scratch(G, K, R) > 0
    stages = {}

    def add(name, launches, flops, weights, acts, torch_launches=0):
        s = stages.setdefault(name, {'launches': 0, 'torch_launches': 0, 'flops': 0, 'weight_bytes': 0, 'activation_bytes': 0})
        s['launches'] += launches
        s['torch_launches'] += torch_launches
        s['flops'] += flops
        s['weight_bytes'] += 4 * weights
        s['activation_bytes'] += 4 * acts

    pad = lambda c: (c + 15) // 16 * 16
    P = B * shape['size'] ** 2
    e, cin, R, S_ = shape['emb'], shape['cin'], shape['R'], shape['S']
    c = S_ * e * (2 if shape['dual'] else 1)
    mid = c // (shape['cheese'] * (2 if shape['dual'] else 1))

    def conv(name, ci, co, ks, extra=0, torch_launches=0, affine=0):
        # a 3x3 runs as nine accumulating 1x1 launches: x is read nine times, y written nine times and read eight
        launches, acts = (9, 9 * pad(ci) + 17 * pad(co)) if ks == 3 else (1, pad(ci) + pad(co))
        add(name, launches, 2 * P * ci * co * ks * ks, pad(co) * ks * ks * pad(ci) + pad(co) + 2 * affine, P * (acts + extra),
            torch_launches)

    add('layout', 1, 0, 0, P * (cin + pad(cin)))
    conv('squeeze', cin, e, 3)
    conv('lower_bread', e, c, 1, extra=2 * pad(c), torch_launches=1, affine=pad(e))        # + the ReLU in place
    hw = shape['size'] ** 2
    hams = [(True, c // 2), (False, c // 2)] if shape['dual'] else [(bool(shape['spatial']), c)]
    for spatial, ch in hams:
        G, D, N = (B * S_, ch // S_, hw) if spatial else (B * S_, hw, ch // S_)
        launches, flops, floats = ham_counts(G, D, N, R, shape['steps'], split)
        # the bases: uploaded, then normalised by three torch launches (norm, clamp, divide)
        add('ham_spatial' if spatial else 'ham_channel', launches, flops, 0, floats + 3 * G * D * R, torch_launches=3)
    add('cheese', 1, 2 * P * c * mid, c * pad(mid), P * (c + pad(mid)))                     # a product of the NMF engine
    # addcmul, relu_, mul_ for coef_shortcut * relu(bn(z)); the accumulating 1x1; the block's relu_
    conv('upper_bread', mid, e, 1, extra=9 * pad(e), torch_launches=4, affine=pad(mid))
    conv('align', e, shape['align'], 3)
    jp = pad(shape['joints'])
    conv('fc', shape['align'], shape['joints'], 1, affine=pad(shape['align']))
    add('fc', 2, 0, 1, P * (jp + 3 * shape['joints']))                                      # layout, softmax
    total = {k: sum(s[k] for s in stages.values()) for k in ('launches', 'torch_launches', 'flops', 'weight_bytes',
                                                             'activation_bytes')}
    for s in list(stages.values()) + [total]:
        s['floor_us'] = 1e6 * max(s['flops'] / F32_MFMA_FLOPS, (s['weight_bytes'] + s['activation_bytes']) / HBM_BYTES_PER_S)
    return {'stages': stages, 'total': total}


# ---- the head from torch ops ------------------------------------------------------------------------------------------
def _torch_nmf2d(x, bases, steps, spatial, S_):
    import torch
    B, C, H, W = x.shape
    X = x.reshape(B * S_, C // S_, H * W)
    if not spatial:
        X = X.transpose(1, 2)
    coef = torch.softmax(torch.bmm(X.transpose(1, 2), bases), dim=-1)

    def coef_step(coef, bases):
        return coef * torch.bmm(X.transpose(1, 2), bases) / (coef.bmm(bases.transpose(1, 2).bmm(bases)) + 1e-6)

    for _ in range(steps):
        coef = coef_step(coef, bases)
        bases = bases * torch.bmm(X, coef) / (bases.bmm(coef.transpose(1, 2).bmm(coef)) + 1e-6)
    out = torch.bmm(bases, coef_step(coef, bases).transpose(1, 2))
    return (out if spatial else out.transpose(1, 2)).reshape(B, C, H, W)


def _torch_cbr(m, x):
    import torch
    import torch.nn.functional as Fn
    y = Fn.conv2d(x, m.conv.weight, padding=m.conv.padding)
    return torch.relu(Fn.batch_norm(y, m.bn.running_mean, m.bn.running_var, m.bn.weight, m.bn.bias, False, 0.0, m.bn.eps))


def torch_hams(model, low, bases):
    import torch
    import torch.nn.functional as Fn
    parts = [_torch_nmf2d(low[:, c0:c0 + ch], Fn.normalize(b, dim=1), ham.eval_steps, ham.spatial, ham.S)
             for (ham, c0, ch), b in zip(model.hamburger.hams(), bases)]
    return torch.cat(parts, dim=1)


def torch_head(model, features, bases):
    import torch
    import torch.nn.functional as Fn
    h = model.hamburger
    z = _torch_cbr(model.squeeze, features)
    low = torch.relu(Fn.conv2d(z, h.lower_bread[0].weight, h.lower_bread[0].bias))
    y = Fn.conv2d(_torch_cbr(h.cheese, torch_hams(model, low, bases)), h.upper_bread.weight)
    y = _torch_cbr(model.align, torch.relu(h.coef_ham * y + h.coef_shortcut * z))
    y = Fn.conv2d(y, model.fc[1].weight, model.fc[1].bias)
    return torch.softmax(y.flatten(2) * model.trainable_temp, dim=2).view(y.shape)


def hip_hams(model, low_nhwc, bases):
    """the two hams alone, as head_forward runs them: views of the NHWC map in, the cheese input out"""
    import torch
    from hipnet import nmf
    out = torch.empty_like(low_nhwc)
    for (ham, c0, ch), b in zip(model.hamburger.hams(), bases):
        nmf.nmf2d(low_nhwc.permute(0, 3, 1, 2)[:, c0:c0 + ch], nmf.normalise_bases(b), ham.eval_steps, ham.spatial, ham.S,
                  out=out.permute(0, 3, 1, 2)[:, c0:c0 + ch])
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
    from models import pose_hrnet_hamburger
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    torch.manual_seed(0)
    model = pose_hrnet_hamburger.get_pose_net(cfg, is_train=False)
    del model.backbone                                          # the head alone: the features are given
    model = model.cuda().eval()
    with torch.no_grad():
        model.hamburger.coef_ham.fill_(0.7)                     # ZERO_HAM starts it at 0, which would hide the hams
        for k, v in model.named_buffers():
            if k.endswith('running_var'):
                v.uniform_(0.5, 2.0)
            elif k.endswith('running_mean'):
                v.normal_(0.0, 0.3)
    g = torch.Generator(device='cuda').manual_seed(1)
    hw = SHAPE['size']
    features = torch.randn(B, SHAPE['cin'], hw, hw, device='cuda', generator=g)
    t0 = time.perf_counter()
    host = model.draw_bases(B, hw, hw)
    t1 = time.perf_counter()
    bases = [b.cuda() for b in host]
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {}
    with torch.no_grad():
        h = model.hamburger
        low = torch.relu(torch.nn.functional.conv2d(_torch_cbr(model.squeeze, features), h.lower_bread[0].weight,
                                                    h.lower_bread[0].bias))
        low_nhwc = low.permute(0, 2, 3, 1).contiguous()
        runs = {'head_hip': lambda: model.head_forward(features, bases), 'head_torch': lambda: torch_head(model, features, bases),
                'hams_hip': lambda: hip_hams(model, low_nhwc, bases), 'hams_torch': lambda: torch_hams(model, low, bases)}
        a, b = runs['head_hip'](), runs['head_torch']()
        diff = float((a - b).abs().max() / b.abs().max())
        a, b = runs['hams_hip']().permute(0, 3, 1, 2), runs['hams_torch']()
        ham_diff = float((a - b).abs().max() / b.abs().max())
        for r in range(warmup + repeats):
            for name, fn in runs.items():
                t = _time(fn, start, stop)
                if r >= warmup:
                    times.setdefault(name, []).append(t)
    out = {k: {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)} for k, v in times.items()}
    out['bases_host_draw_us'], out['bases_upload_us'] = 1e6 * (t1 - t0), 1e6 * (t2 - t1)
    out['bases_bytes'] = sum(4 * b.numel() for b in host)
    out['relative_difference_of_the_two_heads'] = diff
    out['relative_difference_of_the_two_ham_outputs'] = ham_diff
    return out


# ---- the training step (--train) ---------------------------------------------------------------------------------------
TRAIN_STAGES = ['layout', 'squeeze', 'lower_bread', 'ham_spatial', 'ham_channel', 'cheese', 'upper_bread', 'mix', 'align',
                'dropout', 'fc']


def train_counts(B, shape=SHAPE, split=None):
    """launches through the C ABI, FLOPs and bytes of one training step of the head (forward + backward with every
    parameter gradient, no feature gradient), per stage and in total. A BatchNorm is 3 + 1 launches forward (two sum
    passes, finalize; apply) and 3 backward; a weight gradient is the slab launch and its reduce; a 3x3 is nine taps in
    both directions; a ham's backward is one update and one reconstruction."""
    if split is None:
        from hipnet import nmf
        split = lambda G, K, R: nmf.gram_scratch(G, K, R) > 0
    stages = {name: {'launches': 0, 'torch_launches': 0, 'flops': 0, 'weight_bytes': 0, 'activation_bytes': 0}
              for name in TRAIN_STAGES}

    def add(name, launches, flops, weights, acts, torch_launches=0):
        s = stages[name]
        s['launches'] += launches
        s['torch_launches'] += torch_launches
        s['flops'] += flops
        s['weight_bytes'] += 4 * weights
        s['activation_bytes'] += 4 * acts

    pad = lambda c: (c + 15) // 16 * 16
    hw = shape['size'] ** 2
    P = B * hw
    e, cin, R, S_ = shape['emb'], shape['cin'], shape['R'], shape['S']
    c = S_ * e * (2 if shape['dual'] else 1)
    mid = c // (shape['cheese'] * (2 if shape['dual'] else 1))
    al, j = shape['align'], shape['joints']

    def conv(name, ci, co, ks, bn, dgrad, bias=False, relu=False):
        taps = ks * ks
        w = pad(co) * taps * pad(ci)
        prod = 2 * P * ci * co * taps
        # forward: pack (+ the tap-major copy of a 3x3, one torch launch), the taps
        add(name, 1 + taps, prod, 2 * w, P * (taps * pad(ci) + (2 * taps - 1) * pad(co)), torch_launches=(ks == 3) + 2 * bn + bias)
        if bn:                     # stats (z twice), apply (z, y); backward: sums (dy, z, y), apply (dy, z, y, dz)
            add(name, 4 + 3, 0, 0, P * pad(co) * (2 + 2 + 3 + 4))
        if relu:                   # relu_ in place; hrnet_grad_term backward
            add(name, 1, 0, 0, P * pad(co) * 5, torch_launches=1)
        add(name, 2, prod, 2 * w, P * (pad(ci) + pad(co)))                                  # weight gradient
        if bias:
            add(name, 2, 0, 0, P * pad(co))
        if dgrad:
            add(name, 1 + taps, prod, 2 * w, P * (taps * pad(co) + (2 * taps - 1) * pad(ci)), torch_launches=(ks == 3))

    add('layout', 1, 0, 0, P * (cin + pad(cin)))
    conv('squeeze', cin, e, 3, True, False)
    conv('lower_bread', e, c, 1, False, True, bias=True, relu=True)
    hams = [(True, c // 2), (False, c // 2)] if shape['dual'] else [(bool(shape['spatial']), c)]
    for spatial, ch in hams:
        G, D, N = (B * S_, ch // S_, hw) if spatial else (B * S_, hw, ch // S_)
        launches, flops, floats = ham_counts(G, D, N, R, shape['steps'], split)
        # backward: the update with dY where X sits, the reconstruction into dlow; dlow is zeroed once per burger
        add('ham_spatial' if spatial else 'ham_channel', launches + 2, flops + 2 * G * N * R * (D + R) + 2 * G * D * N * R, 0,
            floats + 3 * G * D * R + G * (2 * N * R + D * R + D * N + R * R) + G * (D * R + N * R + D * N), torch_launches=3)
    add('ham_spatial', 0, 0, 0, P * pad(c), torch_launches=1)
    conv('cheese', c, mid, 1, True, True)
    conv('upper_bread', mid, e, 1, False, True)
    add('mix', 1 + 2, 0, 0, P * pad(e) * (3 + 6))            # forward: u, s, out; backward: g, out, u, s, du, ds + reduce
    conv('align', e, al, 3, True, True)
    add('dropout', 2, 0, 0, P * pad(al) * 4)
    conv('fc', al, j, 1, False, True, bias=True)
    add('fc', 2 + 2, 0, 1, P * (2 * pad(j) + 8 * j))          # layout and softmax, both directions
    total = {k: sum(s[k] for s in stages.values()) for k in ('launches', 'torch_launches', 'flops', 'weight_bytes',
                                                             'activation_bytes')}
    for s in list(stages.values()) + [total]:
        s['floor_us'] = 1e6 * max(s['flops'] / F32_MFMA_FLOPS, (s['weight_bytes'] + s['activation_bytes']) / HBM_BYTES_PER_S)
    return {'stages': stages, 'total': total}


def _torch_nmf2d_train(x, bases, steps, spatial, S_):
    import torch
    B, C, H, W = x.shape
    X = x.reshape(B * S_, C // S_, H * W)
    if not spatial:
        X = X.transpose(1, 2)
    with torch.no_grad():
        Xd = X.detach()
        coef = torch.softmax(torch.bmm(Xd.transpose(1, 2), bases), dim=-1)
        for _ in range(steps):
            coef = coef * torch.bmm(Xd.transpose(1, 2), bases) / (coef.bmm(bases.transpose(1, 2).bmm(bases)) + 1e-6)
            bases = bases * torch.bmm(Xd, coef) / (bases.bmm(coef.transpose(1, 2).bmm(coef)) + 1e-6)
    coef = coef * torch.bmm(X.transpose(1, 2), bases) / (coef.bmm(bases.transpose(1, 2).bmm(bases)) + 1e-6)
    out = torch.bmm(bases, coef.transpose(1, 2))
    return (out if spatial else out.transpose(1, 2)).reshape(B, C, H, W)


def _torch_cbr_train(m, x):
    import torch
    import torch.nn.functional as Fn
    y = Fn.conv2d(x, m.conv.weight, padding=m.conv.padding)
    # the running statistics are copies: the HIP path owns the model's
    return torch.relu(Fn.batch_norm(y, m.bn.running_mean.clone(), m.bn.running_var.clone(), m.bn.weight, m.bn.bias, True,
                                    m.bn.momentum, m.bn.eps))


def torch_head_train(model, features, bases, keep, steps):
    """the reference's composition in training mode from torch ops under autograd, on the model's own parameters"""
    import torch
    import torch.nn.functional as Fn
    h = model.hamburger
    z = _torch_cbr_train(model.squeeze, features)
    low = torch.relu(Fn.conv2d(z, h.lower_bread[0].weight, h.lower_bread[0].bias))
    parts = [_torch_nmf2d_train(low[:, c0:c0 + ch], Fn.normalize(b, dim=1), steps, ham.spatial, ham.S)
             for (ham, c0, ch), b in zip(h.hams(), bases)]
    y = Fn.conv2d(_torch_cbr_train(h.cheese, torch.cat(parts, dim=1)), h.upper_bread.weight)
    y = _torch_cbr_train(model.align, torch.relu(h.coef_ham * y + h.coef_shortcut * z))
    y = Fn.conv2d(y * keep.reshape(keep.shape[0], -1, 1, 1), model.fc[1].weight, model.fc[1].bias)
    return torch.softmax(y.flatten(2) * model.trainable_temp, dim=2).view(y.shape)


def stage_times(model, features, bases, keep, repeats, warmup):
    """forward + backward of every stage alone, on the activations of one forward: {stage: {'hip': us, 'torch': us}}
    (medians). A stage's input requires a gradient where the training step forms one (not the features)."""
    import torch
    import torch.nn.functional as Fn
    from hipnet import burger_train as BT
    from hipnet import nhwc
    from hipnet import nmf_train as NT
    from models.pose_hrnet_softmax import _SpatialSoftmax
    h = model.hamburger
    steps, J = model.train_steps, model.num_joints
    nb = [Fn.normalize(b, dim=1) for b in bases]
    specs = [(ham.spatial, c0, ch, ham.S) for ham, c0, ch in h.hams()]
    kview = keep.reshape(keep.shape[0], -1, 1, 1)
    t_hams = lambda low: torch.cat([_torch_nmf2d_train(low[:, c0:c0 + ch], b, steps, sp, S_)
                                    for (sp, c0, ch, S_), b in zip(specs, nb)], dim=1)
    t_fc = lambda x: torch.softmax(Fn.conv2d(x, model.fc[1].weight, model.fc[1].bias).flatten(2) * model.trainable_temp,
                                   dim=2)
    with torch.no_grad():
        z = _torch_cbr_train(model.squeeze, features)
        low = torch.relu(Fn.conv2d(z, h.lower_bread[0].weight, h.lower_bread[0].bias))
        ham = t_hams(low)
        mid = _torch_cbr_train(h.cheese, ham)
        up = Fn.conv2d(mid, h.upper_bread.weight)
        blk = torch.relu(h.coef_ham * up + h.coef_shortcut * z)
        al = _torch_cbr_train(model.align, blk)
    s_nchw, s_nhwc = z.clone().requires_grad_(True), z.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    # stage: (input NCHW, its gradient is formed, the HIP op on NHWC, the torch op on NCHW)
    stages = {
        'squeeze': (features, False, lambda x: BT.conv_bn_relu_train(x, model.squeeze.conv, model.squeeze.bn, 3),
                    lambda x: _torch_cbr_train(model.squeeze, x)),
        'lower_bread': (z, True, lambda x: nhwc.conv1x1_train(x, h.lower_bread[0], True),
                        lambda x: torch.relu(Fn.conv2d(x, h.lower_bread[0].weight, h.lower_bread[0].bias))),
        'hams': (low, True, lambda x: NT.hams_train(x, specs, nb, steps), t_hams),
        'cheese': (ham, True, lambda x: BT.conv_bn_relu_train(x, h.cheese.conv, h.cheese.bn, 1),
                   lambda x: _torch_cbr_train(h.cheese, x)),
        'upper_bread': (mid, True, lambda x: nhwc.conv1x1_train(x, h.upper_bread), lambda x: Fn.conv2d(x, h.upper_bread.weight)),
        'mix': (up, True, lambda x: BT.burger_mix(x, s_nhwc, h.coef_ham, h.coef_shortcut),
                lambda x: torch.relu(h.coef_ham * x + h.coef_shortcut * s_nchw)),
        'align': (blk, True, lambda x: BT.conv_bn_relu_train(x, model.align.conv, model.align.bn, 3),
                  lambda x: _torch_cbr_train(model.align, x)),
        'dropout': (al, True, lambda x: BT.dropout2d(x, keep), lambda x: x * kview),
        'fc': (al, True, lambda x: _SpatialSoftmax.apply(nhwc.to_nchw(nhwc.conv1x1_train(x, model.fc[1]), J),
                                                         model.trainable_temp), t_fc),
    }
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    params = [p for p in model.parameters() if p.requires_grad]
    out = {}
    for name, (x, need, hip, ref) in stages.items():
        res = {}
        for side, fn, inp in (('hip', hip, x.permute(0, 2, 3, 1).contiguous()), ('torch', ref, x)):
            inp = inp.detach().requires_grad_(need)
            g = torch.randn_like(fn(inp))

            def run():
                inp.grad = None
                for p in params:
                    p.grad = None
                fn(inp).backward(g)
            ts = [_time(run, start, stop) for _ in range(warmup + repeats)][warmup:]
            res[side] = statistics.median(ts)
        out[name] = res
    return out


def measure_train(B, repeats, warmup):
    import torch
    from config import get_cfg_defaults
    from models import pose_hrnet_hamburger
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    torch.manual_seed(0)
    model = pose_hrnet_hamburger.get_pose_net(cfg, is_train=False, trainable=True)
    del model.backbone
    model = model.cuda().train()
    with torch.no_grad():
        model.hamburger.coef_ham.fill_(0.7)
    g = torch.Generator(device='cuda').manual_seed(1)
    hw = SHAPE['size']
    features = torch.randn(B, SHAPE['cin'], hw, hw, device='cuda', generator=g)
    bases = [b.cuda() for b in model.draw_bases(B, hw, hw)]
    keep = model.draw_drop_keep(B, features.device)
    weight = torch.randn(B, SHAPE['joints'], hw, hw, device='cuda', generator=g)
    names = [k for k, p in model.named_parameters() if p.requires_grad]

    def step(head, m, w):
        params = [p for p in m.parameters() if p.requires_grad]

        def run():
            for p in params:
                p.grad = None
            (head() * w).sum().backward()
            return [p.grad for p in params]
        return run

    runs = {'train_hip': step(lambda: model.head_forward(features, bases, keep), model, weight),
            'train_torch': step(lambda: torch_head_train(model, features, bases, keep, model.train_steps), model, weight)}
    a, b = runs['train_hip'](), runs['train_torch']()
    # both against the same composition in float64 on the device (fc.1.bias is left out: its gradient is zero by the
    # softmax's shift invariance)
    m64 = copy.deepcopy(model).double()
    ref = step(lambda: torch_head_train(m64, features.double(), [t.double() for t in bases], keep.double(), model.train_steps),
               m64, weight.double())()
    rel = lambda x, y: float((x.double() - y).abs().max() / y.abs().max().clamp_min(1e-300))
    errs = {side: max((rel(x, y), k) for x, y, k in zip(g, ref, names) if k != 'fc.1.bias')
            for side, g in (('hip', a), ('torch', b))}
    diff = max(rel(x, y) for x, y, k in zip(a, b, names) if k != 'fc.1.bias')
    del m64, ref
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {}
    for r in range(warmup + repeats):
        for name, fn in runs.items():
            t = _time(fn, start, stop)
            if r >= warmup:
                times.setdefault(name, []).append(t)
    out = {k: {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)} for k, v in times.items()}
    out['largest_relative_difference_of_a_gradient'] = diff
    out['largest_gradient_error_against_float64'] = {side: {'err': e, 'parameter': k} for side, (e, k) in errs.items()}
    out['stages_us'] = stage_times(model, features, bases, keep, repeats, warmup)
    return out


def main_train(args):
    lines = []
    for B in args.batches:
        row = {'B': B, 'train': True, 'counts': train_counts(B)}
        if not args.counts_only:
            row['times'] = t = measure_train(B, args.repeats, args.warmup)
            row['train_ratio_torch_over_hip'] = t['train_torch']['median_us'] / t['train_hip']['median_us']
            lines.append('B {:3d}  '.format(B) + '  '.join('{} {:.0f} ({:.0f} .. {:.0f}) us'.format(
                k, v['median_us'], v['min_us'], v['max_us']) for k, v in sorted(t.items())
                if isinstance(v, dict) and 'median_us' in v))
            lines.append('       torch / hip: training step of the head {:.2f}; floor {:.0f} us; largest difference of a '
                         'gradient {:.2g}'.format(row['train_ratio_torch_over_hip'], row['counts']['total']['floor_us'],
                                                  t['largest_relative_difference_of_a_gradient']))
            e = t['largest_gradient_error_against_float64']
            lines.append('       largest gradient error against the float64 composition: hip {:.2g} ({}), torch {:.2g} '
                         '({})'.format(e['hip']['err'], e['hip']['parameter'], e['torch']['err'], e['torch']['parameter']))
            lines.append('       stage alone, forward + backward, hip / torch us: ' + ', '.join(
                '{} {:.0f} / {:.0f}'.format(k, v['hip'], v['torch']) for k, v in t['stages_us'].items()))
        print(json.dumps(row))
    if lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('bench_hamburger.py --train: forward + backward of the head, median (min .. max) of {} after {} '
                    'warm-ups\n'.format(args.repeats, args.warmup) + '\n'.join(lines) + '\n')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--counts-only', action='store_true')
    ap.add_argument('--train', action='store_true', help='time forward + backward of the head in training mode')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hamburger_head_times.txt'))
    args = ap.parse_args(argv)
    if not args.counts_only:
        import torch
        if not torch.cuda.is_available():
            sys.exit('bench_hamburger: no HIP device: the timings need one (--counts-only prints the cost model)')
    if args.train:
        return main_train(args)
    lines = []
    for B in args.batches:
        row = {'B': B, 'counts': counts(B)}
        if not args.counts_only:
            row['times'] = t = measure(B, args.repeats, args.warmup)
            row['head_ratio_torch_over_hip'] = t['head_torch']['median_us'] / t['head_hip']['median_us']
            row['hams_ratio_torch_over_hip'] = t['hams_torch']['median_us'] / t['hams_hip']['median_us']
            tot = row['counts']['total']
            hams = sum(row['counts']['stages'][k]['flops'] for k in ('ham_spatial', 'ham_channel'))
            lines.append('B {:3d}  '.format(B) + '  '.join('{} {:.0f} ({:.0f} .. {:.0f}) us'.format(
                k, v['median_us'], v['min_us'], v['max_us']) for k, v in sorted(t.items()) if isinstance(v, dict)))
            lines.append('       torch / hip: head {:.2f}, hams {:.2f}; hams {:.1f} GFLOP -> {:.1f} TFLOP/s on the HIP path, '
                         '{:.1f} on torch; head floor {:.0f} us; bases {:.1f} MB: host draw {:.0f} us, upload {:.0f} us; '
                         'difference of the two heads {:.2g}'.format(
                             row['head_ratio_torch_over_hip'], row['hams_ratio_torch_over_hip'], hams / 1e9,
                             hams / t['hams_hip']['median_us'] / 1e6, hams / t['hams_torch']['median_us'] / 1e6,
                             tot['floor_us'], t['bases_bytes'] / 1e6, t['bases_host_draw_us'], t['bases_upload_us'],
                             t['relative_difference_of_the_two_heads']))
        print(json.dumps(row))
    if lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('bench_hamburger.py: median (min .. max) of {} after {} warm-ups\n'.format(args.repeats, args.warmup) +
                    '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
