"""Timing of the PredRNN head of models.predrnn (hipnet.predrnn on csrc/predrnn.hip + hipnet.conv_kxk) at the yaml's size
(four layers of 64 hidden channels, 3 x 3 filters, 64 x 64 maps of 53 channels) against the same head built from torch ops
on the same device with the same parameters (F.conv2d = MIOpen, F.layer_norm, torch.sigmoid / tanh, torch.cat, F.batch_norm,
F.max_pool2d, F.linear):

    python tools/bench_predrnn.py [--shapes 1x8 4x8] [--repeats 20] [--warmup 3]
    python tools/bench_predrnn.py --counts-only          (no device: launches per cell, FLOPs and bytes per stage)

It times, at B x L = 1 x 8 and 4 x 8, the head (RNN over L frames, the last frame's prediction, the ResNet tail; the
backbone is not part of it) and ONE cell alone (layer 1: 64 -> 7 * 64 conv_x; its own conv_x included). Device events around
each call after a warm-up, the two paths alternating inside one loop; medians with the spread (min .. max) over the
repeats. The yardstick is always torch's ops in the same run. The two paths' outputs are compared once (relative
difference over the largest value). Lines are appended to profiles/predrnn_times.txt with the date and the command.
Without a HIP device the timing mode fails: there is no fallback.

`counts(B, L)` is the cost model: per stage of a cell the launches, 2 * MACs, and the bytes of activations, of weights and -
listed separately - of the LayerNorm parameters, which are as large as a sample's map and are read by every cell step.
"""
import argparse
import datetime
import json
import os
import statistics
import sys

import _init_paths  # noqa: F401

NH, LAYERS, KS, SIZE, FRAME = 64, 4, 3, 64, 53
HERE = os.path.dirname(os.path.abspath(__file__))
YAML = os.path.join(os.path.dirname(HERE), 'experiments', 'Pred_RNN', 'PredRNN_8frames_256x256_adam_lr1e-3.yaml')
OUT = os.path.join(os.path.dirname(os.path.dirname(HERE)), 'profiles', 'predrnn_times.txt')


def cell_counts(B, cin, nh=NH, ks=KS, size=SIZE):
    """the stages of one cell step in launch order: launches (kernels), FLOPs, activation / weight / LayerNorm-parameter
    bytes. cin: the input channels of conv_x (56 for layer 0, nh above)"""
    hw, f = size * size, 4
    conv = lambda ci, co, k: {'launches': 1, 'flops': 2 * B * hw * ci * co * k * k,
                              'activation_bytes': f * B * hw * (ci + co), 'weight_bytes': f * (co * ci * k * k + co), 'ln_bytes': 0}
    ew = lambda launches, read, write, ln: {'launches': launches, 'flops': 0, 'activation_bytes': f * B * hw * (read + write),
                                            'weight_bytes': 0, 'ln_bytes': f * hw * ln}
    return [('conv_x', conv(cin, 7 * nh, ks)), ('conv_h', conv(nh, 4 * nh, ks)), ('conv_m', conv(nh, 3 * nh, ks)),
            ('sample_stats(xc, hc, mc)', ew(2, 14 * nh, 0, 0)),
            ('stlstm_gates', ew(1, 16 * nh, 3 * nh, 28 * nh)),
            ('conv_o', conv(2 * nh, nh, ks)), ('conv_last', conv(2 * nh, nh, 1)),
            ('sample_stats(oc)', ew(2, nh, 0, 0)),
            ('stlstm_out', ew(1, 3 * nh, nh, 2 * nh))]


def counts(B, L, nh=NH, layers=LAYERS, ks=KS, size=SIZE):
    from hipnet.predrnn import LAUNCHES_PER_CELL
    upper = cell_counts(B, nh, nh, ks, size)
    keys = ('launches', 'flops', 'activation_bytes', 'weight_bytes', 'ln_bytes')
    cell = {k: sum(row[k] for _, row in upper) for k in keys}
    first = {k: sum(row[k] for _, row in cell_counts(B, (FRAME + 3) // 4 * 4, nh, ks, size)) for k in keys}
    assert cell['launches'] == LAUNCHES_PER_CELL['kernels']
    rnn = {k: L * (first[k] + (layers - 1) * cell[k]) for k in keys}
    rnn['launches'] -= L - 1                      # layer 0's conv_x runs once for all L frames
    return {'launches_per_cell': dict(LAUNCHES_PER_CELL), 'cell_stages': [dict(stage=n, **row) for n, row in upper],
            'cell': cell, 'rnn': rnn, 'B': B, 'L': L}


# ---- the same head from torch ops ------------------------------------------------------------------------------------
def torch_cell(P, p, x, h, c, m, nh):
    import torch
    import torch.nn.functional as F

    def conv_ln(name, t):
        w = P[p + name + '.0.weight']
        y = F.conv2d(t, w, P[p + name + '.0.bias'], padding=w.shape[2] // 2)
        return F.layer_norm(y, y.shape[1:], P[p + name + '.1.weight'], P[p + name + '.1.bias'])

    i_x, f_x, g_x, i_xp, f_xp, g_xp, o_x = torch.split(conv_ln('conv_x', x), nh, dim=1)
    i_h, f_h, g_h, o_h = torch.split(conv_ln('conv_h', h), nh, dim=1)
    i_m, f_m, g_m = torch.split(conv_ln('conv_m', m), nh, dim=1)
    c_new = torch.sigmoid(f_x + f_h + 1.0) * c + torch.sigmoid(i_x + i_h) * torch.tanh(g_x + g_h)
    m_new = torch.sigmoid(f_xp + f_m + 1.0) * m + torch.sigmoid(i_xp + i_m) * torch.tanh(g_xp + g_m)
    mem = torch.cat((c_new, m_new), 1)
    o = torch.sigmoid(o_x + o_h + conv_ln('conv_o', mem))
    return o * torch.tanh(F.conv2d(mem, P[p + 'conv_last.weight'], P[p + 'conv_last.bias'])), c_new, m_new


def torch_head(P, x, nhs):
    """x (B, L, 53, s, s) -> (B, 63): the reference's RNN (last frame's prediction only) and ResNet"""
    import torch
    import torch.nn.functional as F
    B, L, _, s, _ = x.shape
    h = [torch.zeros((B, n, s, s), device=x.device) for n in nhs]
    c = [torch.zeros((B, n, s, s), device=x.device) for n in nhs]
    memory = torch.zeros((B, nhs[0], s, s), device=x.device)
    for t in range(L):
        for i in range(len(nhs)):
            h[i], c[i], memory = torch_cell(P, 'PredRNN.cell_list.{}.'.format(i), x[:, t] if i == 0 else h[i - 1], h[i], c[i],
                                            memory, nhs[i])
    y = F.conv2d(h[-1], P['PredRNN.conv_last.weight'])

    def block(p, t):
        def bn(v, j):
            q = p + 'bn' + j + '.'
            return F.batch_norm(v, P[q + 'running_mean'], P[q + 'running_var'], P[q + 'weight'], P[q + 'bias'], False, 0.0, 1e-5)
        u = F.relu(bn(F.conv2d(t, P[p + 'conv1.weight'], padding=1), '1'))
        return F.relu(bn(F.conv2d(u, P[p + 'conv2.weight'], padding=1), '2') + t)

    y = block('resnet.block2.', F.max_pool2d(block('resnet.block1.', y), 2, 2))
    y = F.relu(F.linear(y.reshape(B, -1), P['resnet.fc1.weight'], P['resnet.fc1.bias']))
    return F.relu(F.linear(y, P['resnet.fc2.weight'], P['resnet.fc2.bias']))


def _time(fn, start, stop):
    import torch
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3          # us


def measure(B, L, repeats, warmup, model=None):
    import torch
    from config import get_cfg_defaults
    from hipnet import nhwc
    from hipnet import predrnn as P
    from models import predrnn
    if model is None:
        cfg = get_cfg_defaults()
        cfg.merge_from_file(YAML)
        torch.manual_seed(0)
        model = predrnn.get_pose_net(cfg, is_train=False)
        with torch.no_grad():
            for name, p in list(model.PredRNN.named_parameters()) + list(model.resnet.named_parameters()):
                if p.ndim == 3:                                   # LayerNorm: about 1 and about 0
                    p.copy_((1.0 if name.endswith('weight') else 0.0) + 0.1 * torch.randn_like(p))
            for bn in (m for m in model.resnet.modules() if isinstance(m, torch.nn.BatchNorm2d)):
                bn.running_mean.normal_(0.0, 0.2)
                bn.running_var.uniform_(0.5, 1.5)
        model = model.cuda().eval()
    s, fw, nh = model.RNN_feat_size, model.frame_width(), NH
    Pd = {'PredRNN.' + k: v.detach() for k, v in model.PredRNN.state_dict().items()}
    Pd.update({'resnet.' + k: v.detach() for k, v in model.resnet.state_dict().items()})
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(B, L, FRAME, s, s, device='cuda', generator=g) * 0.5
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        fm = nhwc.nchw_to_nhwc(x.transpose(0, 1).reshape(L * B, FRAME, s, s).contiguous(), fw, nhwc.F32).view(L, B, s, s, fw)
        cells = model._packed()['cells']
        rnd = lambda *shape: torch.randn(*shape, device='cuda', generator=g)
        xin, hid, cm, mm = rnd(B, s, s, nh), rnd(B, s, s, nh), rnd(B, s, s, 2 * nh), rnd(B, s, s, 2 * nh)
        to_nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
        xin_t, hid_t, c_t, m_t = to_nchw(xin), to_nchw(hid), to_nchw(cm[..., :nh]), to_nchw(mm[..., nh:])
        jobs = {'head_hip': lambda: model._tail(model._rnn(fm, False)[0]),
                'head_torch': lambda: torch_head(Pd, x, model.PredRNN.num_hidden),
                # the cell writes its memory map in place: the state drifts over the repeats, the work does not
                'cell_hip': lambda: P.cell(cells[1], xin, 0, hid, cm, mm, nh),
                'cell_torch': lambda: torch_cell(Pd, 'PredRNN.cell_list.1.', xin_t, hid_t, c_t, m_t, nh)}
        a, b = jobs['head_hip'](), jobs['head_torch']()
        diff = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
        times = {}
        for r in range(warmup + repeats):
            for label, fn in jobs.items():
                t = _time(fn, start, stop)
                if r >= warmup:
                    times.setdefault(label, []).append(t)
    out = {k: {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)} for k, v in times.items()}
    out['relative_difference_of_the_heads'] = diff
    return out, model


def main(argv=None):
    ap = argparse.ArgumentParser(description='time the PredRNN head against torch ops')
    ap.add_argument('--shapes', nargs='+', default=['1x8', '4x8'], help='B x L, e.g. 1x8 4x8')
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--counts-only', action='store_true')
    args = ap.parse_args(argv)
    shapes = [tuple(int(v) for v in s.lower().split('x')) for s in args.shapes]
    if args.counts_only:
        for B, L in shapes:
            print(json.dumps(counts(B, L)))
        return 0
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_predrnn: no HIP device: the timing mode measures on the GPU and has no fallback (--counts-only '
                 'needs none)')
    lines = ['{}  python tools/bench_predrnn.py {}'.format(datetime.date.today().isoformat(), ' '.join(sys.argv[1:])),
             'bench_predrnn.py: median (min .. max) of {} after {} warm-ups; head = RNN over L frames + ResNet tail, cell = '
             'one layer-1 cell step; f32, {} x {} maps, {} layers of {} hidden channels, {} x {} filters'.format(
                 args.repeats, args.warmup, SIZE, SIZE, LAYERS, NH, KS, KS)]
    model = None
    for B, L in shapes:
        res, model = measure(B, L, args.repeats, args.warmup, model)
        c = counts(B, L)
        for what, flops in (('head', c['rnn']['flops']), ('cell', c['cell']['flops'])):
            h, t = res[what + '_hip'], res[what + '_torch']
            lines.append('B x L {:2d} x {}  {}  hip {:.0f} ({:.0f} .. {:.0f}) us {:.1f} TF  torch {:.0f} ({:.0f} .. {:.0f}) us '
                         '{:.1f} TF  torch / hip {:.2f}'.format(
                             B, L, what, h['median_us'], h['min_us'], h['max_us'], flops / h['median_us'] / 1e6,
                             t['median_us'], t['min_us'], t['max_us'], flops / t['median_us'] / 1e6,
                             t['median_us'] / h['median_us']))
        lines.append('B x L {:2d} x {}  heads differ by {:.2e} of the largest output'.format(
            B, L, res['relative_difference_of_the_heads']))
    lines.append('(TF: the convolutions\' 2 * MACs of the cost model over the time; the head\'s figure leaves the tail\'s FLOPs out)')
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'a') as f:
        f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
