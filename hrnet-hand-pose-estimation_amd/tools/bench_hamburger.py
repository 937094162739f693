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
"""
import argparse
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--counts-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hamburger_head_times.txt'))
    args = ap.parse_args(argv)
    if not args.counts_only:
        import torch
        if not torch.cuda.is_available():
            sys.exit('bench_hamburger: no HIP device: the timings need one (--counts-only prints the cost model)')
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
