"""Timing of CPM (models.CPM on hrnet_conv2d_kxk, csrc/conv_kxk.hip) at 256 x 256 against the same model built from torch
ops (F.conv2d = MIOpen, F.max_pool2d, F.avg_pool2d, torch.cat) on the same device with the same weights:

    python tools/bench_cpm.py [--batches 1 16] [--repeats 20] [--warmup 3]
    python tools/bench_cpm.py --counts-only          (no device: launches, FLOPs and bytes per layer)

It times the whole model and the three dominant layers alone - 9x9 3 -> 128 at 256^2 (conv1_stage1), 9x9 128 -> 128 at
128^2 (conv2_stage1) and 11x11 128 -> 128 at 32^2 (Mconv2_stage2), each with bias and ReLU - the HIP path on NHWC maps,
torch on NCHW ones, each in its own layout. Device events around each call after a warm-up, the two paths alternating
inside one loop; medians with the spread (min .. max) over the repeats, and the achieved TFLOP/s against the 155 TF that
the f32 MFMA reaches on this device. The yardstick is always torch's op in the same run, never an earlier run of this
kernel. Lines are appended to profiles/cpm_times.txt. Without a HIP device the timing mode fails: there is no fallback.

    python tools/bench_cpm.py --train [--batches 1 16]   (the training step and the dominant layers' gradients)

--train measures the training step of models.CPM(trainable=True) - forward, last-stage loss, backward, FlatAdam - against
torch autograd + torch.optim.Adam on the same weights, and hrnet_conv2d_kxk_wgrad / _dgrad of the same three layers
against torch.nn.grad.conv2d_weight / conv2d_input (MIOpen, f32), in the same run: medians of 10 after 3 warm-ups,
appended to profiles/cpm_train_times.txt. `train_counts(B)` is its cost model: three times the forward's FLOPs, minus the
image layers' data gradient. --train --counts-only prints it without a device.

`counts(B)` is the cost model: per layer the launches of one forward, 2 * MACs, and the bytes of weights and
activations.
"""
import argparse
import json
import os
import statistics
import sys

import _init_paths  # noqa: F401

F32_MFMA_FLOPS = 155e12           # measured peak of the f32 MFMA on the MI355X
SIZE, JOINTS = 256, 21
DOMINANT = (('conv1_stage1', 1), ('conv2_stage1', 2), ('Mconv2_stage2', 8))       # (layer, stride of its map)


def _trunk_index(name):
    """1, 2, 3 for the three convolutions in front of a max-pool (conv{1,2,3}_stage{1,2}), 0 for every other layer"""
    if name.startswith('conv') and name[-1] in '12' and name[4] in '123':
        return int(name[4])
    return 0


def layer_sizes(size=SIZE, k=JOINTS):
    """[(name, Cin, Cout, ks, map side)] of the 40 convolutions"""
    from models.CPM import layer_table
    return [(name, ci, co, ks, size // 2 ** (_trunk_index(name) - 1) if _trunk_index(name) else size // 8)
            for name, ci, co, ks in layer_table(k)]


def counts(B, size=SIZE, k=JOINTS):
    """launches, FLOPs (2 * MACs of the real channels) and bytes of one forward, per layer and in total"""
    layers, total = {}, {'launches': 0, 'flops': 0, 'weight_bytes': 0, 'activation_bytes': 0}
    for name, ci, co, ks, side in layer_sizes(size, k):
        pooled = _trunk_index(name) > 0
        row = {'launches': 2 if pooled else 1, 'flops': 2 * B * side * side * co * ci * ks * ks,
               'weight_bytes': 4 * (co * ci * ks * ks + co),
               'activation_bytes': 4 * B * side * side * (ci + co) + (4 * B * side * side * co * 5 // 4 if pooled else 0)}
        layers[name] = row
        for key in total:
            total[key] += row[key]
    # layout in (1), centre pool (1), six layouts out
    total['launches'] += 8
    total['mfma_floor_us'] = 1e6 * total['flops'] / F32_MFMA_FLOPS
    return {'layers': layers, 'total': total}


def train_counts(B, size=SIZE, k=JOINTS):
    """FLOPs of one training step: the forward, the weight gradient (as many MACs again) and the data gradient (again as
    many, except for the two image layers, whose input needs none)"""
    c = counts(B, size, k)
    layers = {}
    for name, ci, co, ks, side in layer_sizes(size, k):
        f = c['layers'][name]['flops']
        layers[name] = {'forward': f, 'wgrad': f, 'dgrad': 0 if ci == 3 else f}
    total = {key: sum(row[key] for row in layers.values()) for key in ('forward', 'wgrad', 'dgrad')}
    total['flops'] = total['forward'] + total['wgrad'] + total['dgrad']
    total['mfma_floor_us'] = 1e6 * total['flops'] / F32_MFMA_FLOPS
    return {'layers': layers, 'total': total}


def measure_train(B, repeats, warmup):
    """the training step (forward, last-stage loss, backward, Adam) of models.CPM(trainable=True) against torch autograd on
    the same weights, and the weight and data gradients of the three dominant layers against torch.nn.grad (MIOpen, f32),
    the two paths alternating inside one loop"""
    import torch
    import torch.nn.functional as F
    from hipnet import conv_kxk_train as T
    from hipnet.optim import FlatAdam
    from models import CPM
    torch.manual_seed(0)
    model = CPM.CPM(JOINTS, trainable=True)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith('.weight'):
                p.normal_(0.0, (2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
            else:
                p.normal_(0.0, 0.1)
    model = model.cuda().train()
    P = {k: v.detach().clone().requires_grad_(True) for k, v in model.named_parameters()}
    g = torch.Generator(device='cuda').manual_seed(1)
    image = torch.randn(B, 3, SIZE, SIZE, device='cuda', generator=g) * 0.5
    yy, xx = torch.meshgrid(torch.arange(SIZE, device='cuda'), torch.arange(SIZE, device='cuda'), indexing='ij')
    center = torch.exp(-((xx - 130.0) ** 2 + (yy - 120.0) ** 2) / 18.0)[None, None].repeat(B, 1, 1, 1).contiguous()
    target = torch.rand(B, JOINTS + 1, SIZE // 8, SIZE // 8, device='cuda', generator=g)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    opt_hip, opt_torch = FlatAdam(model, lr=1e-4), torch.optim.Adam(list(P.values()), lr=1e-4)

    def step_hip():
        opt_hip.zero_grad()
        CPM.cpm_loss(model(image, center), target).backward()
        opt_hip.step()

    def step_torch():
        opt_torch.zero_grad()
        (((torch_forward(P, image, center)[-1] - target) ** 2).sum((2, 3)).mean()).backward()
        opt_torch.step()

    jobs = {'step_hip': step_hip, 'step_torch': step_torch}
    sizes = {n: (ci, co, ks, side) for n, ci, co, ks, side in layer_sizes()}
    for name, _ in DOMINANT:
        ci, co, ks, side = sizes[name]
        cip = (ci + 3) // 4 * 4
        x_nchw = torch.randn(B, ci, side, side, device='cuda', generator=g)
        dy_nchw = torch.randn(B, co, side, side, device='cuda', generator=g)
        x_nhwc = torch.zeros(B, side, side, cip, device='cuda')
        x_nhwc[..., :ci] = x_nchw.permute(0, 2, 3, 1)
        dy_nhwc = dy_nchw.permute(0, 2, 3, 1).contiguous()
        w = P[name + '.weight'].detach()
        scratch = torch.empty(T.wgrad_plan(B, side, side, cip, co, ks)[0] // 4, device='cuda')
        dw, db = torch.empty_like(w), torch.empty(co, device='cuda')
        jobs[name + '_wgrad_hip'] = lambda x=x_nhwc, dy=dy_nhwc, s=scratch, dw=dw, db=db, cip=cip, ci=ci, co=co, ks=ks: \
            T.wgrad(x, dy, s, dw, db, cip, ci, 0, co, 0, ks)
        jobs[name + '_wgrad_torch'] = lambda x=x_nchw, dy=dy_nchw, w=w, ks=ks: \
            (torch.nn.grad.conv2d_weight(x, w.shape, dy, padding=ks // 2), dy.sum((0, 2, 3)))
        if ci != 3:
            wt = T.pack_dgrad(w, co)
            dx = torch.empty(B, side, side, ci, device='cuda')
            jobs[name + '_dgrad_hip'] = lambda dy=dy_nhwc, wt=wt, dx=dx, ci=ci, co=co, ks=ks: \
                T.dgrad(dy, wt, dx, None, co, 0, ci, 0, 0, ks, False)
            jobs[name + '_dgrad_torch'] = lambda x=x_nchw, dy=dy_nchw, w=w, ks=ks: \
                torch.nn.grad.conv2d_input(x.shape, w, dy, padding=ks // 2)
    times = {}
    for r in range(warmup + repeats):
        for label, fn in jobs.items():
            t = _time(fn, start, stop)
            if r >= warmup:
                times.setdefault(label, []).append(t)
    out = {k: {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)} for k, v in times.items()}
    c = train_counts(B)
    for k, v in out.items():
        what = k.rsplit('_', 1)[0]
        flops = c['total']['flops'] if what == 'step' else c['layers'][what.rsplit('_', 1)[0]]['wgrad']
        v['tflops'] = flops / v['median_us'] / 1e6
    with torch.no_grad():
        gh = {k: p.grad for k, p in model.named_parameters()}
        out['relative_difference_of_the_last_gradients'] = max(
            float((gh[k] - P[k].grad).abs().max() / P[k].grad.abs().max().clamp_min(1e-30)) for k in P)
    return out


def torch_forward(P, image, center):
    """the reference's composition (lib/models/CPM.py:68-170) from torch ops on a dict of parameters, NCHW"""
    import torch
    import torch.nn.functional as F

    def conv(name, x, act=True):
        w = P[name + '.weight']
        y = F.conv2d(x, w, P[name + '.bias'], padding=w.shape[2] // 2)
        return F.relu(y) if act else y

    def trunk(x, stage):
        for i in (1, 2, 3):
            x = F.max_pool2d(conv('conv{}_stage{}'.format(i, stage), x), 3, 2, 1)
        return x

    pooled = F.avg_pool2d(center, 9, 8, 1)
    x = trunk(image, 1)
    for i in (4, 5, 6):
        x = conv('conv{}_stage1'.format(i), x)
    outs = [conv('conv7_stage1', x, act=False)]
    mid = trunk(image, 2)
    for s in range(2, 7):
        x = conv('conv4_stage2' if s == 2 else 'conv1_stage{}'.format(s), mid)
        x = torch.cat([x, outs[-1], pooled], 1)
        for i in (1, 2, 3, 4):
            x = conv('Mconv{}_stage{}'.format(i, s), x)
        outs.append(conv('Mconv5_stage{}'.format(s), x, act=False))
    return outs


def _time(fn, start, stop):
    import torch
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3          # us


def measure(B, repeats, warmup):
    import torch
    import torch.nn.functional as F
    from hipnet import conv_kxk as K
    from models import CPM
    torch.manual_seed(0)
    model = CPM.CPM(JOINTS)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith('.weight'):
                p.normal_(0.0, (2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
            else:
                p.normal_(0.0, 0.1)
    model = model.cuda().eval()
    P = {k: v.detach() for k, v in model.named_parameters()}
    g = torch.Generator(device='cuda').manual_seed(1)
    image = torch.randn(B, 3, SIZE, SIZE, device='cuda', generator=g) * 0.5
    yy, xx = torch.meshgrid(torch.arange(SIZE, device='cuda'), torch.arange(SIZE, device='cuda'), indexing='ij')
    center = torch.exp(-((xx - 130.0) ** 2 + (yy - 120.0) ** 2) / 18.0)[None, None].repeat(B, 1, 1, 1).contiguous()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sizes = {n: (ci, co, ks, side) for n, ci, co, ks, side in layer_sizes()}
    with torch.no_grad():
        hip_out, torch_out = model(image, center), torch_forward(P, image, center)
        diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(hip_out, torch_out))
        jobs = {'model_hip': lambda: model(image, center), 'model_torch': lambda: torch_forward(P, image, center)}
        plan = model._packed()
        for name, _ in DOMINANT:
            ci, co, ks, side = sizes[name]
            cip = (ci + 3) // 4 * 4
            x_nchw = torch.randn(B, ci, side, side, device='cuda', generator=g)
            x_nhwc = torch.zeros(B, side, side, cip, device='cuda')
            x_nhwc[..., :ci] = x_nchw.permute(0, 2, 3, 1)
            w, b = plan[name][0], plan[name][1]
            jobs[name + '_hip'] = lambda x=x_nhwc, w=w, b=b, co=co, ks=ks: K.conv_kxk(x, w, co, ks, bias=b, relu=True)
            jobs[name + '_torch'] = lambda x=x_nchw, n=name, ks=ks: F.relu(F.conv2d(x, P[n + '.weight'], P[n + '.bias'],
                                                                                   padding=ks // 2))
        times = {}
        for r in range(warmup + repeats):
            for label, fn in jobs.items():
                t = _time(fn, start, stop)
                if r >= warmup:
                    times.setdefault(label, []).append(t)
    out = {k: {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)} for k, v in times.items()}
    c = counts(B)
    flops = dict({n: c['layers'][n]['flops'] for n, _ in DOMINANT}, model=c['total']['flops'])
    for k, v in out.items():
        v['tflops'] = flops[k.rsplit('_', 1)[0]] / v['median_us'] / 1e6
    out['relative_difference_of_the_two_models'] = diff
    return out


def main_train(args):
    repeats = 10 if args.repeats == 20 else args.repeats
    lines = []
    for B in args.batches:
        row = {'B': B, 'train_counts': train_counts(B)}
        if not args.counts_only:
            row['times'] = t = measure_train(B, repeats, args.warmup)
            for name in sorted({k.rsplit('_', 1)[0] for k in t if k.endswith('_hip')}):
                h, o = t[name + '_hip'], t[name + '_torch']
                row[name + '_ratio_torch_over_hip'] = o['median_us'] / h['median_us']
                lines.append('B {:3d}  {:20s} hip {:.0f} ({:.0f} .. {:.0f}) us {:.1f} TF ({:.0f} % of 155)  torch {:.0f} '
                             '({:.0f} .. {:.0f}) us {:.1f} TF  torch / hip {:.2f}'.format(
                                 B, name, h['median_us'], h['min_us'], h['max_us'], h['tflops'], 100 * h['tflops'] / 155,
                                 o['median_us'], o['min_us'], o['max_us'], o['tflops'], o['median_us'] / h['median_us']))
        print(json.dumps(row))
    if lines:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), 'profiles',
                            'cpm_train_times.txt')
        with open(path, 'a') as f:
            f.write('bench_cpm.py --train: median (min .. max) of {} after {} warm-ups\n'.format(repeats, args.warmup) +
                    '\n'.join(lines) + '\n')
        print('\n'.join(lines))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--counts-only', action='store_true')
    ap.add_argument('--train', action='store_true', help='the training step and the gradients of the dominant layers '
                    '(medians of 10 after 3 warm-ups unless --repeats / --warmup say otherwise)')
    args = ap.parse_args(argv)
    if not args.counts_only:
        import torch
        if not torch.cuda.is_available():
            sys.exit('bench_cpm: no HIP device: the timings need one (--counts-only prints the cost model)')
    if args.train:
        return main_train(args)
    lines = []
    for B in args.batches:
        row = {'B': B, 'counts': counts(B)}
        if not args.counts_only:
            row['times'] = t = measure(B, args.repeats, args.warmup)
            for name in ['model'] + [n for n, _ in DOMINANT]:
                h, o = t[name + '_hip'], t[name + '_torch']
                row[name + '_ratio_torch_over_hip'] = o['median_us'] / h['median_us']
                lines.append('B {:3d}  {:14s} hip {:.0f} ({:.0f} .. {:.0f}) us {:.1f} TF ({:.0f} % of 155)  torch {:.0f} '
                             '({:.0f} .. {:.0f}) us {:.1f} TF  torch / hip {:.2f}'.format(
                                 B, name, h['median_us'], h['min_us'], h['max_us'], h['tflops'], 100 * h['tflops'] / 155,
                                 o['median_us'], o['min_us'], o['max_us'], o['tflops'], o['median_us'] / h['median_us']))
        print(json.dumps(row))
    if lines:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), 'profiles',
                            'cpm_times.txt')
        with open(path, 'a') as f:
            f.write('bench_cpm.py: median (min .. max) of {} after {} warm-ups\n'.format(args.repeats, args.warmup) +
                    '\n'.join(lines) + '\n')
        print('\n'.join(lines))


if __name__ == '__main__':
    main()
