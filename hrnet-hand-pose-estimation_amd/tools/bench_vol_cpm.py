"""Timing of the joint between the CPM backbone and the volumetric half of MODEL.NAME vol_CPM (hipnet.upsample_slice on
csrc/upsample_slice.hip), and of the model's forward and training step:

    python tools/bench_vol_cpm.py [--repeats 30] [--warmup 5] [--no-model]
    python tools/bench_vol_cpm.py --counts-only          (no device: launches and bytes of the bridge and of the step)

The bridge: hrnet_upsample_slice_nchw and its transpose at N = 4 and 16, 32 x 32 -> 64 x 64, C = 22 (the heat maps, channels
32 .. 53 of the 56-wide concatenated map) and C = 32 (the processed features, a whole 32-wide map), against the same from
torch ops on the same device: x[..., c0 : c0 + C].permute(0, 3, 1, 2) -> F.interpolate(bilinear, align_corners=True), and
torch.autograd.grad back to the NHWC map. Device events around each call after a warm-up, the two paths alternating inside
one loop; medians with the spread (min .. max) over the repeats, and the achieved GB/s on the bytes the operation NEEDS
(`bridge_counts`: the slice read once, the NCHW map written once; the backward the mirror) - it is a layout change, so
bytes over the device's memory rate is its floor. A call of a few microseconds is mostly launch overhead: the N = 16 rows
are the ones to read, and the yardstick is always torch's op in the same run.

The model: VolumetricTriangulationNet_CPM at 256 x 256 images, 64 x 64 heat maps, VOLUME_SIZE 64, V = 4 views, B = 1: the
eval forward under no_grad and one training step (forward, the three losses of the shipped yaml, backward, the Adam step
of tools/train_vol.py) with drawn weights. There is no torch yardstick for the whole model here; the step is reported
beside `step_counts` (launches of the short backward against the 40-layer walk it replaces).

Lines are appended to profiles/vol_cpm_times.txt. Without a HIP device the timing mode fails: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import _init_paths  # noqa: F401

BRIDGE = [(N, 32, 32, Cp, c0, C, 64, 64) for N in (4, 16) for Cp, c0, C in ((56, 32, 22), (32, 0, 32))]
PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bridge_counts(N, h, w, Cp, c0, C, H, W):
    """launches and the bytes the operation needs, per direction"""
    need = 4 * N * C * (h * w + H * W)
    return {'forward': {'launches': 1, 'bytes': need}, 'backward': {'launches': 1, 'bytes': need},
            'torch_forward_ops': 2, 'workgroups_forward': N * -(-H * W // 64) * -(-C // 32),
            'workgroups_backward': N * -(-h * w // 64) * -(-C // 32)}


def step_counts(k=21):
    """launches of the backbone's part of one training step: the short backward of models.CPM_volumetric against the
    40-layer walk of models.CPM it replaces (weight gradient 2 launches, data gradient 1, pool backward 1)"""
    short = 1 + (2 + 1) + (2 + 1) + 2                  # up-sample transpose; Mconv5, Mconv4: wgrad + dgrad; Mconv3: wgrad
    full = 40 * 2 + (40 - 2 + 5) + 6 + 6               # every wgrad; dgrads (Mconv1 has two); pools; layout of six gradients
    return {'short_backward_launches': short, 'full_backward_launches': full, 'bridge_launches_forward': 2,
            'bridge_launches_backward': 2, 'process_features_launches': {'forward': 2, 'backward': 4}}


def _time(fn, start, stop):
    import torch
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3          # us


def _stats(v):
    return {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)}


def measure_bridge(case, repeats, warmup):
    import torch
    import torch.nn.functional as F
    from hipnet import upsample_slice as S
    N, h, w, Cp, c0, C, H, W = case
    g = torch.Generator(device='cuda').manual_seed(2)
    x = torch.randn(N, h, w, Cp, device='cuda', generator=g)
    gy = torch.randn(N, C, H, W, device='cuda', generator=g)
    out, dx = torch.empty(N, C, H, W, device='cuda'), torch.zeros(N, h, w, Cp, device='cuda')
    xr = x.clone().requires_grad_(True)

    def torch_fwd(t=x):
        return F.interpolate(t[..., c0:c0 + C].permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=True)

    y = torch_fwd(xr)
    jobs = {'forward_hip': lambda: S.forward(x, out, c0, C), 'forward_torch': torch_fwd,
            'backward_hip': lambda: S.backward(gy, dx, c0, C, False),
            'backward_torch': lambda: torch.autograd.grad(y, xr, gy, retain_graph=True)}
    diff = float((S.forward(x, out, c0, C) - torch_fwd()).abs().max())
    dref = torch.autograd.grad(y, xr, gy, retain_graph=True)[0]
    ddiff = float((S.backward(gy, dx, c0, C, False) - dref)[..., c0:c0 + C].abs().max() / dref.abs().max())
    times = {}
    for r in range(warmup + repeats):
        for label, fn in jobs.items():
            t = _time(fn, *_events())
            if r >= warmup:
                times.setdefault(label, []).append(t)
    res = {k: _stats(v) for k, v in times.items()}
    need = bridge_counts(*case)['forward']['bytes']
    for v in res.values():
        v['GBps_on_needed_bytes'] = need / v['median_us'] / 1e3
    res['max_abs_difference_forward'], res['relative_difference_backward'] = diff, ddiff
    return res


_EVENTS = []


def _events():
    import torch
    if not _EVENTS:
        _EVENTS.extend([torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)])
    return _EVENTS


def build_model(B=1, V=4, seed=0):
    import torch
    from config import cfg
    from models.triangulation import VolumetricTriangulationNet_CPM
    c = cfg.clone()
    c.defrost()
    c.merge_from_file(os.path.join(PKG, 'experiments', 'MHP', 'MHP_VolTriangulation_CPM_v1.yaml'))
    torch.manual_seed(seed)
    model = VolumetricTriangulationNet_CPM(c, is_train=True)
    with torch.no_grad():
        for m in model.backbone.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.normal_(0.0, (2.0 / m.weight[0].numel()) ** 0.5)
                m.bias.normal_(0.0, 0.1)
    return c, model.cuda()


def measure_model(repeats, warmup, B=1, V=4):
    import math
    import torch
    from core.loss import HeatmapLoss, Joints3DMSELoss, VolumetricCELoss
    import train_vol
    c, model = build_model(B, V)
    g = torch.Generator(device='cuda').manual_seed(3)
    img = torch.randn(B, V, 3, 256, 256, device='cuda', generator=g) * 0.5
    cm = torch.rand(B, V, 1, 256, 256, device='cuda', generator=g)
    # V cameras on a ring of 600 mm looking at the origin, principal point at the centre of the 64 x 64 maps
    proj = torch.zeros(B, V, 3, 4, device='cuda')
    for v in range(V):
        a = 2 * math.pi * v / V
        R = torch.tensor([[math.cos(a), 0., -math.sin(a)], [0., 1., 0.], [math.sin(a), 0., math.cos(a)]])
        Km = torch.tensor([[80., 0., 32.], [0., 80., 32.], [0., 0., 1.]])
        proj[:, v] = (Km @ torch.cat([R, torch.tensor([[0.], [0.], [600.]])], 1)).cuda()
    tgt = torch.rand(B * V, 22, 64, 64, device='cuda', generator=g)
    gt = torch.randn(B, 21, 3, device='cuda', generator=g) * 20
    ones = torch.ones(B, 21, 1, device='cuda')
    opt = train_vol.build_optimizer(c, model)
    j3d, ce, hl = Joints3DMSELoss(), VolumetricCELoss(), HeatmapLoss()

    def forward():
        model.eval()
        with torch.no_grad():
            model(img, cm, proj)

    def step():
        model.train()
        out = model(img, cm, proj, theta=[0.0] * B)
        total = j3d(out[0], gt) + 0.01 * ce(out[5], out[3], gt, ones) + 0.1 * hl(out[2].reshape(B * V, 22, 64, 64), tgt)
        opt.zero_grad()
        total.backward()
        opt.step()

    times = {}
    for r in range(warmup + repeats):
        for label, fn in (('forward', forward), ('train_step', step)):
            t = _time(fn, *_events())
            if r >= warmup:
                times.setdefault(label, []).append(t)
    return {k: _stats(v) for k, v in times.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--counts-only', action='store_true')
    ap.add_argument('--no-model', action='store_true', help='the bridge only')
    args = ap.parse_args(argv)
    if not args.counts_only:
        import torch
        if not torch.cuda.is_available():
            sys.exit('bench_vol_cpm: no HIP device: the timings need one (--counts-only prints the cost model)')
    lines = []
    for case in BRIDGE:
        row = {'case': dict(zip(('N', 'h', 'w', 'Cp', 'c0', 'C', 'H', 'W'), case)), 'counts': bridge_counts(*case)}
        if not args.counts_only:
            row['times'] = t = measure_bridge(case, args.repeats, args.warmup)
            for name in ('forward', 'backward'):
                a, o = t[name + '_hip'], t[name + '_torch']
                lines.append('bridge N {} C {:2d} of {} {:8s} hip {:.1f} ({:.1f} .. {:.1f}) us {:.0f} GB/s  torch {:.1f} ({:.1f} .. '
                             '{:.1f}) us {:.0f} GB/s  torch / hip {:.2f}'.format(
                                 case[0], case[5], case[3], name, a['median_us'], a['min_us'], a['max_us'],
                                 a['GBps_on_needed_bytes'], o['median_us'], o['min_us'], o['max_us'],
                                 o['GBps_on_needed_bytes'], o['median_us'] / a['median_us']))
        print(json.dumps(row))
    row = {'step_counts': step_counts()}
    if not args.counts_only and not args.no_model:
        row['times'] = t = measure_model(max(3, args.repeats // 3), max(2, args.warmup // 2))
        for name in ('forward', 'train_step'):
            lines.append('model B x V 1 x 4, 256 x 256, volume 64  {:10s} {:.0f} ({:.0f} .. {:.0f}) us'.format(
                name, t[name]['median_us'], t[name]['min_us'], t[name]['max_us']))
    print(json.dumps(row))
    if lines:
        path = os.path.join(os.path.dirname(PKG), 'profiles', 'vol_cpm_times.txt')
        with open(path, 'a') as f:
            f.write('bench_vol_cpm.py: median (min .. max) of {} after {} warm-ups\n'.format(args.repeats, args.warmup) +
                    '\n'.join(lines) + '\n')
        print('\n'.join(lines))


if __name__ == '__main__':
    main()
