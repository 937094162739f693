"""Timing of the head of FTLMultiviewNet (models.FTL_encoder_decoder on csrc/ftl.hip) at 480 channels and 64 x 64
features against the same head built from torch ops (F.conv2d, F.conv_transpose2d = MIOpen, matmul, torch.cat) on the
same device with the same weights:

    python tools/bench_ftl.py [--batches 1 4] [--views 4] [--repeats 20] [--warmup 3]
    python tools/bench_ftl.py --counts-only          (no device: launches, FLOPs issued and useful, bytes per stage)
    python tools/bench_ftl.py --train [--counts-only]  (the head's training step: forward on batch statistics + backward)

It times the whole head (features in, heat maps out) and its three dominant layers alone - encoder_head.0 (Conv2d 3x3
stride 2 padding 2, 480 -> 480, 64 -> 33), decoder.0 (ConvTranspose2d 480 -> 256, 18 -> 33) and decoder.1 (ConvTranspose2d
256 -> 256 with output_padding 1, 33 -> 64), each with its BatchNorm folded in and the ReLU - the HIP path on NHWC maps,
torch on NCHW ones, each in its own layout. The torch head gets the same algebra as the HIP one: BatchNorm folded into
the weights, decoder.2 and final_layer composed into one 3x3 convolution, the transforms as one composed x A + c; what
is compared is kernels, not arithmetic tricks. Device events around each call after a warm-up, the two paths alternating
inside one loop; medians with the spread (min .. max) over the repeats, and the achieved TFLOP/s on the USEFUL FLOPs
against the 155 TF that the f32 MFMA reaches on this device. The yardstick is always torch's op in the same run. Lines
are appended to profiles/ftl_times.txt. Without a HIP device the timing mode fails: there is no fallback.

--train times the head's forward + backward of a trainable model (hipnet.ftl_train.HeadFn, from the features to the
gradient of every head parameter, started from a fixed heat-map gradient) against the same head from torch ops under
autograd (F.conv2d / F.conv_transpose2d / F.batch_norm in training mode, unfolded, torch.autograd.grad to the same
parameters), whole and per backward stage: the weight gradients of the four 3x3 layers with stride 2
(hrnet_conv2d_3x3g_wgrad against the weight gradient autograd takes for the same layer), the data gradients that run on
the forward kernel (against autograd's input gradient) and the two transforms' backward. `train_counts(B, V)` is its
cost model per backward stage: launches, FLOPs useful, bytes.

`counts(B, V)` is the cost model: per stage the launches, 2 * MACs issued (every MFMA of every workgroup: border pixels
of the 8 x 16 tiles, padded channels) and useful (real weight times real input), and the bytes of weights and activations.
"""
import argparse
import json
import os
import statistics
import sys

import _init_paths  # noqa: F401

F32_MFMA_FLOPS = 155e12           # measured peak of the f32 MFMA on the MI355X
CHANNELS, SIZE, JOINTS, DEC = 480, 64, 21, 256
DOMINANT = ('encoder_head.0', 'decoder.0', 'decoder.1')


def stages(B, V, C=CHANNELS, size=SIZE, K=JOINTS):
    """[(name, kind, N, Hin, Cin, Cout, Hout, (stride, pad_lo, z))] of the head's launches in order; kind 'g' =
    hrnet_conv2d_3x3g, 'p' = hrnet_conv2d_kxk ks 1, 't' = a transform"""
    from hipnet.ftl import out_size
    s1 = out_size(size, 2, 2)
    s2 = out_size(s1, 2, 2)
    s3 = out_size(s2, 1, 0, 2, 0)
    s4 = out_size(s3, 1, 0, 2, 1)
    C2, N = C // 2, B * V
    return [('encoder_head.0', 'g', N, size, C, C, s1, (2, 2, 1)), ('encoder_head.1', 'g', N, s1, C, C2, s2, (2, 2, 1)),
            ('ftl_gather', 't', N, s2, C2, C2, s2, None), ('fuse_after_FTL.0', 'p', B, s2, V * C2, C2, s2, None),
            ('fuse_after_FTL.1', 'p', B, s2, C2, C2, s2, None), ('ftl_scatter', 't', N, s2, C2, C2, s2, None),
            ('channel_expansion.0', 'p', N, s2, C2, C, s2, None), ('decoder.0', 'g', N, s2, C, DEC, s3, (1, 0, 2)),
            ('decoder.1', 'g', N, s3, DEC, DEC, s4, (1, 0, 2)), ('decoder.2+final_layer', 'g', N, s4, DEC, K, s4, (1, 1, 1))]


def _pointwise_counts(N, H, cin, cout):
    """hrnet_conv2d_kxk with ks 1: its 8 x 16 pixel tiles and the dispatch rule of csrc/conv_kxk_body.h"""
    pad16 = lambda c: (c + 15) // 16 * 16
    ptiles, cop = N * ((H + 7) // 8) * ((H + 15) // 16), pad16(cout)
    if cop % 64 == 0 and ptiles * (cop // 64) >= 512:
        cb = 64
    elif ptiles * ((cop + 31) // 32) >= 256:
        cb = 32
    else:
        cb = 16
    return ptiles * 128 * -(-cop // cb) * cb * pad16(cin), N * H * H * cin * cout


def counts(B, V=4, C=CHANNELS, size=SIZE, K=JOINTS):
    """launches, FLOPs issued and useful, weight and activation bytes of one head forward, per stage and in total; and
    what the unfused decoder.2 -> final_layer pair would have cost"""
    from hipnet import ftl
    rows, total = {}, {'launches': 0, 'flops_issued': 0, 'flops_useful': 0, 'weight_bytes': 0, 'activation_bytes': 0}
    for name, kind, N, hin, cin, cout, hout, geo in stages(B, V, C, size, K):
        if kind == 'g':
            _, issued, useful = ftl.counts(N, hin, hin, cin, cout, hout, hout, *geo)
            wbytes = 4 * (cout * cin * 9 + cout)
        elif kind == 'p':
            issued, useful = _pointwise_counts(N, hin, cin, cout)
            wbytes = 4 * (cout * cin + cout)
        else:
            issued = useful = N * hin * hin * cin * 3          # 3 FMAs per output value, no MFMA
            wbytes = 4 * 12 * N
        n_in = B if name == 'ftl_scatter' else N
        row = {'launches': 1, 'flops_issued': 2 * issued, 'flops_useful': 2 * useful, 'weight_bytes': wbytes,
               'activation_bytes': 4 * (n_in * hin * hin * cin + (B if name == 'ftl_gather' else N) * hout * hout * cout *
                                        (V if name == 'ftl_gather' else 1))}
        rows[name] = row
        for key in total:
            total[key] += row[key]
    total['launches'] += 3                                      # layout in, layout out, softmax
    total['mfma_floor_us'] = 1e6 * total['flops_useful'] / F32_MFMA_FLOPS
    last = stages(B, V, C, size, K)[-1]
    unfused = 2 * last[2] * last[6] * last[6] * (DEC * DEC * 9 + DEC * K)
    return {'stages': rows, 'total': total, 'flops_of_unfused_last_two_layers': unfused}


def train_counts(B, V=4, C=CHANNELS, size=SIZE, K=JOINTS):
    """launches, useful FLOPs and bytes of the head's BACKWARD per stage (host arithmetic). A convolution layer's backward
    is a weight gradient (2 launches: partials, then their sum in split order) and, but for encoder_head.0, a data
    gradient (1 launch), each with the useful FLOPs of its forward; a BatchNorm backward is 1 launch over its map, read
    three times (gradient, input, output) and written once"""
    fwd = counts(B, V, C, size, K)['stages']
    rows, total = {}, {'launches': 0, 'flops_useful': 0, 'bytes': 0}
    for name, kind, N, hin, cin, cout, hout, geo in reversed(stages(B, V, C, size, K)):
        f = fwd[name]
        if kind == 't':
            row = {'launches': 1, 'flops_useful': f['flops_useful'], 'bytes': f['activation_bytes'] + f['weight_bytes']}
        else:
            want_dx = name != 'encoder_head.0'
            last = name == 'decoder.2+final_layer'
            row = {'launches': 2 + (1 if want_dx else 0) + (0 if last else 1),
                   'flops_useful': f['flops_useful'] * (2 if want_dx else 1),
                   'bytes': f['activation_bytes'] * (2 if want_dx else 1) + 2 * f['weight_bytes'] +
                   (0 if last else 4 * 4 * N * hout * hout * cout)}
        rows[name] = row
        for key in total:
            total[key] += row[key]
    total['launches'] += 2                                      # softmax backward, layout of the heat-map gradient
    total['mfma_floor_us'] = 1e6 * total['flops_useful'] / F32_MFMA_FLOPS
    return {'stages': rows, 'total': total}


def torch_train_head(model, feat, coef_g, coef_s, B, V):
    """the trainable head from torch ops on batch statistics, unfolded, on the model's own parameters"""
    import torch
    import torch.nn.functional as F

    def bn(seq, x):
        return F.relu(F.batch_norm(x, None, None, seq[1].weight, seq[1].bias, True, 0.1, seq[1].eps))

    e, f, d = model.encoder_head.layer_lst, model.fuse_after_FTL.layer_lst, model.decoder.layer_lst
    x = bn(e[0], F.conv2d(feat, e[0][0].weight, e[0][0].bias, stride=2, padding=2))
    x = bn(e[1], F.conv2d(x, e[1][0].weight, e[1][0].bias, stride=2, padding=2))
    C2, h2, w2 = x.shape[1:]
    trip = x.reshape(B, V, C2, h2 * w2 // 3, 3)
    Ag, cg = coef_g[..., :9].reshape(B, V, 1, 3, 3), coef_g[..., 9:].reshape(B, V, 1, 1, 3)
    cat = (torch.matmul(trip, Ag) + cg).reshape(B, V * C2, h2, w2)
    x = bn(f[0], F.conv2d(cat, f[0][0].weight, f[0][0].bias))
    x = bn(f[1], F.conv2d(x, f[1][0].weight, f[1][0].bias))
    As, cs = coef_s[..., :9].reshape(B, V, 1, 3, 3), coef_s[..., 9:].reshape(B, V, 1, 1, 3)
    x = (torch.matmul(x.reshape(B, 1, C2, h2 * w2 // 3, 3), As) + cs).reshape(B * V, C2, h2, w2)
    c = model.channel_expansion.layer_lst[0]
    x = bn(c, F.conv2d(x, c[0].weight, c[0].bias))
    x = bn(d[0], F.conv_transpose2d(x, d[0][0].weight, d[0][0].bias, stride=2, padding=2))
    x = bn(d[1], F.conv_transpose2d(x, d[1][0].weight, d[1][0].bias, stride=2, padding=2, output_padding=1))
    x = F.conv2d(x, d[2].weight, d[2].bias, padding=1)
    y = F.conv2d(x, model.final_layer.weight, model.final_layer.bias)
    return F.softmax(y.reshape(y.shape[0], y.shape[1], -1), 2).reshape(y.shape)


TRAIN_STAGES = ('encoder_head.0 wgrad', 'encoder_head.1 wgrad', 'decoder.0 wgrad', 'decoder.1 wgrad', 'encoder_head.1 dgrad',
                'decoder.0 dgrad', 'decoder.1 dgrad', 'transforms bwd')


def measure_train(B, V, repeats, warmup):
    import torch
    import torch.nn.functional as F
    from hipnet import ftl, ftl_train
    model = build_model(V, trainable=True).train()
    g = torch.Generator(device='cuda').manual_seed(2)
    feat = torch.randn(B * V, CHANNELS, SIZE, SIZE, device='cuda', generator=g).abs_()
    ext, K = unit_cameras(B, V, 'cuda')
    coef_g, coef_s = ftl.affines(ext, K)
    ghm = torch.randn(B * V, JOINTS, SIZE, SIZE, device='cuda', generator=g)
    params = model.head_parameters()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    table = {s[0]: s for s in stages(B, V)}

    def step_hip():
        model._head_train(feat, ext, K).backward(ghm)

    def step_torch():
        torch.autograd.grad(torch_train_head(model, feat, coef_g, coef_s, B, V), params, ghm)

    step_hip()
    mine = [p.grad.clone() for p in params]
    theirs = torch.autograd.grad(torch_train_head(model, feat, coef_g, coef_s, B, V), params, ghm)
    diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(mine, theirs) if a.ndim == 4)
    jobs = {'step_hip': step_hip, 'step_torch': step_torch}
    new = lambda *s: torch.randn(*s, device='cuda', generator=g)
    scratch = torch.empty(1 << 26, device='cuda')
    for name, transposed in (('encoder_head.0', False), ('encoder_head.1', False), ('decoder.0', True), ('decoder.1', True)):
        _, _, N, hin, cin, cout, hout, _ = table[name]
        x = new(N, cin, hin, hin).requires_grad_()
        w = (new(cin, cout, 3, 3) if transposed else new(cout, cin, 3, 3)).requires_grad_()
        if transposed:
            y = F.conv_transpose2d(x, w, stride=2, padding=2, output_padding=hout - (2 * hin - 3))
        else:
            y = F.conv2d(x, w, stride=2, padding=2)
        gy = new(*y.shape)
        xh, gh = x.detach().permute(0, 2, 3, 1).contiguous(), gy.permute(0, 2, 3, 1).contiguous()
        jobs[name + ' wgrad_torch'] = lambda y=y, w=w, gy=gy: torch.autograd.grad(y, w, gy, retain_graph=True)
        if transposed:
            dw = torch.empty(cin, cout, 3, 3, device='cuda')
            jobs[name + ' wgrad_hip'] = lambda xh=xh, gh=gh, dw=dw, cin=cin, cout=cout: \
                ftl_train.wgrad(gh, xh, scratch, dw, cout, cout, 0, cin, 0, 2, 2)
            packed = ftl_train.pack_dgrad_transpose(w.detach(), cout)
            dx = torch.empty(N, hin, hin, cin, device='cuda')
            jobs[name + ' dgrad_hip'] = lambda gh=gh, packed=packed, dx=dx, cin=cin, cout=cout: \
                ftl.conv(gh, packed, None, dx, cout, 0, cin, 0, 2, 2, 1, False)
        else:
            dw = torch.empty(cout, cin, 3, 3, device='cuda')
            jobs[name + ' wgrad_hip'] = lambda xh=xh, gh=gh, dw=dw, cin=cin, cout=cout: \
                ftl_train.wgrad(xh, gh, scratch, dw, cin, cin, 0, cout, 0, 2, 2)
            packed = ftl_train.pack_dgrad(w.detach(), cout)
            dx = torch.empty(N, hin, hin, cin, device='cuda')
            jobs[name + ' dgrad_hip'] = lambda gh=gh, packed=packed, dx=dx, cin=cin, cout=cout: \
                ftl.conv(gh, packed, None, dx, cout, 0, cin, 0, 1, 0, 2, False)
        jobs[name + ' dgrad_torch'] = lambda y=y, x=x, gy=gy: torch.autograd.grad(y, x, gy, retain_graph=True)
    for key in ('encoder_head.0 dgrad_hip', 'encoder_head.0 dgrad_torch'):
        del jobs[key]                                           # the features are frozen: no such pass in the step
    _, _, N, h2, C2, _, _, _ = table['ftl_gather']
    dcat, dsc = new(B, h2, h2, V * C2), new(N, h2, h2, C2)
    o1, o2 = torch.empty(N, h2, h2, C2, device='cuda'), torch.empty(B, h2, h2, C2, device='cuda')

    def transforms_hip():
        ftl_train.gather_bwd_raw(dcat, coef_g, o1, B, V, C2, 0, C2, 0)
        ftl_train.scatter_bwd_raw(dsc, coef_s, o2, B, V, C2, 0, 0)

    At = lambda coef: coef[..., :9].reshape(B, V, 1, 3, 3).transpose(-1, -2)
    tg, ts = dcat.permute(0, 3, 1, 2).reshape(B, V, C2, -1, 3), dsc.permute(0, 3, 1, 2).reshape(B, V, C2, -1, 3)
    jobs['transforms bwd_hip'] = transforms_hip
    jobs['transforms bwd_torch'] = lambda: (torch.matmul(tg, At(coef_g)), torch.matmul(ts, At(coef_s)).sum(1))
    times = {}
    for r in range(warmup + repeats):
        for label, fn in jobs.items():
            t = _time(fn, start, stop)
            if r >= warmup:
                times.setdefault(label, []).append(t)
    out = {k: {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)} for k, v in times.items()}
    out['relative_difference_of_the_weight_gradients'] = diff
    return out


def _time(fn, start, stop):
    import torch
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3          # us


def torch_plan(model):
    """the head's layers as torch wants them (NCHW OIHW weights), with the algebra of FTLMultiviewNet._head_plan: BatchNorm
    folded in (float64), decoder.2 and final_layer composed"""
    import torch
    from models.FTL_encoder_decoder import _fold

    def conv_bn(seq, transposed=False):
        scale, shift = _fold(seq[1])
        w = seq[0].weight.detach().double() * scale.reshape((1, -1, 1, 1) if transposed else (-1, 1, 1, 1))
        return w.float().contiguous(), (seq[0].bias.detach().double() * scale + shift).float().contiguous()

    last, fin = model.decoder.layer_lst[2], model.final_layer
    wf = fin.weight.detach().double().reshape(fin.out_channels, -1)
    return {'enc0': conv_bn(model.encoder_head.layer_lst[0]), 'enc1': conv_bn(model.encoder_head.layer_lst[1]),
            'fuse0': conv_bn(model.fuse_after_FTL.layer_lst[0]), 'fuse1': conv_bn(model.fuse_after_FTL.layer_lst[1]),
            'expand': conv_bn(model.channel_expansion.layer_lst[0]),
            'dec0': conv_bn(model.decoder.layer_lst[0], True), 'dec1': conv_bn(model.decoder.layer_lst[1], True),
            'out': (torch.einsum('km,mcrs->kcrs', wf, last.weight.detach().double()).float().contiguous(),
                    (wf @ last.bias.detach().double() + fin.bias.detach().double()).float().contiguous())}


def torch_head(T, feat, coef_g, coef_s, B, V):
    """features (B V, C, h, w) -> heat maps (B V, K, h, w) from torch ops, slot order b V + v"""
    import torch
    import torch.nn.functional as F
    x = F.relu(F.conv2d(feat, *T['enc0'], stride=2, padding=2))
    x = F.relu(F.conv2d(x, *T['enc1'], stride=2, padding=2))
    C2, h2, w2 = x.shape[1:]
    trip = x.reshape(B, V, C2, h2 * w2 // 3, 3)
    Ag, cg = coef_g[..., :9].reshape(B, V, 1, 3, 3), coef_g[..., 9:].reshape(B, V, 1, 1, 3)
    cat = (torch.matmul(trip, Ag) + cg).reshape(B, V * C2, h2, w2)
    x = F.relu(F.conv2d(cat, *T['fuse0']))
    x = F.relu(F.conv2d(x, *T['fuse1']))
    As, cs = coef_s[..., :9].reshape(B, V, 1, 3, 3), coef_s[..., 9:].reshape(B, V, 1, 1, 3)
    x = (torch.matmul(x.reshape(B, 1, C2, h2 * w2 // 3, 3), As) + cs).reshape(B * V, C2, h2, w2)
    x = F.relu(F.conv2d(x, *T['expand']))
    x = F.relu(F.conv_transpose2d(x, *T['dec0'], stride=2, padding=2))
    x = F.relu(F.conv_transpose2d(x, *T['dec1'], stride=2, padding=2, output_padding=1))
    y = F.conv2d(x, *T['out'], padding=1)
    return F.softmax(y.reshape(y.shape[0], y.shape[1], -1), 2).reshape(y.shape)


def build_model(V, C=CHANNELS, K=JOINTS, seed=0, trainable=False):
    """FTLMultiviewNet's HEAD with drawn weights and BatchNorm statistics, on the device, eval mode; no backbone is run"""
    import torch
    from config import cfg
    from models.FTL_encoder_decoder import FTLMultiviewNet
    c = cfg.clone()
    c.defrost()
    c.merge_from_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'experiments', 'MHP',
                                   'MHP_HRNet_w32_softmax_pose2dloss_FTL_v1.yaml'))
    c.DATASET.NUM_VIEWS, c.DATASET.NUM_JOINTS, c.MODEL.NUM_JOINTS = V, K, K
    if C != CHANNELS:
        c.MODEL.EXTRA.STAGE4.NUM_CHANNELS = [C // 8, C // 8, C // 4, C // 2]
    torch.manual_seed(seed)
    model = FTLMultiviewNet(c, trainable=True) if trainable else FTLMultiviewNet(c)
    with torch.no_grad():
        for name, m in model.named_modules():
            if name.startswith('backbone'):
                continue
            if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                fan = m.weight.shape[0] * 9 / 4.0 if isinstance(m, torch.nn.ConvTranspose2d) else m.weight[0].numel()
                m.weight.normal_(0.0, (2.0 / fan) ** 0.5)
                m.bias.normal_(0.0, 0.1)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.1)
                m.running_mean.normal_(0.0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    return model.cuda().eval()


def unit_cameras(B, V, device, seed=1):
    """unit-scale cameras: random rotations, |t| <= 1, K within 2x of the identity"""
    import torch
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(B, V, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1)).unsqueeze(-2)
    t = torch.randn(B, V, 3, 1, generator=g, dtype=torch.float64)
    t = t / t.norm(dim=2, keepdim=True) * (0.2 + 0.8 * torch.rand(B, V, 1, 1, generator=g, dtype=torch.float64))
    K = torch.tensor([[1.3, 0., 0.2], [0., 0.8, -0.3], [0., 0., 1.]], dtype=torch.float64)
    return torch.cat([q, t], -1).float().to(device), K.float().to(device)


def measure(B, V, repeats, warmup):
    import torch
    import torch.nn.functional as F
    from hipnet import ftl
    model = build_model(V)
    T = torch_plan(model)
    g = torch.Generator(device='cuda').manual_seed(2)
    feat = torch.randn(B * V, CHANNELS, SIZE, SIZE, device='cuda', generator=g).abs_()
    ext, K = unit_cameras(B, V, 'cuda')
    coef_g, coef_s = ftl.affines(ext, K)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    table = {s[0]: s for s in stages(B, V)}
    with torch.no_grad():
        hip = model.head_stages(feat, ext, K)['heatmaps']
        ref = torch_head(T, feat, coef_g, coef_s, B, V)
        diff = float((hip - ref).abs().max() / ref.abs().max())
        jobs = {'head_hip': lambda: model.head_stages(feat, ext, K), 'head_torch': lambda: torch_head(T, feat, coef_g, coef_s, B, V)}
        plan = model._head_plan()
        for name, key, tr in (('encoder_head.0', 'enc0', False), ('decoder.0', 'dec0', True), ('decoder.1', 'dec1', True)):
            _, _, N, hin, cin, cout, hout, (stride, pad_lo, z) = table[name]
            x_nchw = torch.randn(N, cin, hin, hin, device='cuda', generator=g)
            x_nhwc = x_nchw.permute(0, 2, 3, 1).contiguous()
            y = torch.empty(N, hout, hout, cout, device='cuda')
            w, b = plan[key]
            jobs[name + '_hip'] = lambda x=x_nhwc, w=w, b=b, y=y, cin=cin, cout=cout, geo=(stride, pad_lo, z): \
                ftl.conv(x, w, b, y, cin, 0, cout, 0, geo[0], geo[1], geo[2], True)
            if tr:
                op = hout - (2 * hin - 3)
                jobs[name + '_torch'] = lambda x=x_nchw, k=key, op=op: F.relu(F.conv_transpose2d(
                    x, *T[k], stride=2, padding=2, output_padding=op))
            else:
                jobs[name + '_torch'] = lambda x=x_nchw, k=key: F.relu(F.conv2d(x, *T[k], stride=2, padding=2))
        times = {}
        for r in range(warmup + repeats):
            for label, fn in jobs.items():
                t = _time(fn, start, stop)
                if r >= warmup:
                    times.setdefault(label, []).append(t)
    out = {k: {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)} for k, v in times.items()}
    c = counts(B, V)
    flops = dict({n: c['stages'][n]['flops_useful'] for n in DOMINANT}, head=c['total']['flops_useful'])
    for k, v in out.items():
        v['tflops'] = flops[k.rsplit('_', 1)[0]] / v['median_us'] / 1e6
    out['relative_difference_of_the_two_heads'] = diff
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--counts-only', action='store_true')
    ap.add_argument('--train', action='store_true', help='the training step of the head instead of its inference')
    args = ap.parse_args(argv)
    if not args.counts_only:
        import torch
        if not torch.cuda.is_available():
            sys.exit('bench_ftl: no HIP device: the timings need one (--counts-only prints the cost model)')
    lines = []
    if args.train:
        for B in args.batches:
            row = {'B': B, 'V': args.views, 'train_counts': train_counts(B, args.views)}
            if not args.counts_only:
                row['times'] = t = measure_train(B, args.views, args.repeats, args.warmup)
                for name in ('step',) + TRAIN_STAGES:
                    h, o = t[name + '_hip'], t[name + '_torch']
                    lines.append('--train B x V {} x {}  {:22s} hip {:.0f} ({:.0f} .. {:.0f}) us  torch {:.0f} ({:.0f} .. {:.0f}) '
                                 'us  torch / hip {:.2f}'.format(B, args.views, name, h['median_us'], h['min_us'], h['max_us'],
                                                                 o['median_us'], o['min_us'], o['max_us'],
                                                                 o['median_us'] / h['median_us']))
            print(json.dumps(row))
    for B in ([] if args.train else args.batches):
        row = {'B': B, 'V': args.views, 'counts': counts(B, args.views)}
        if not args.counts_only:
            row['times'] = t = measure(B, args.views, args.repeats, args.warmup)
            for name in ('head',) + DOMINANT:
                h, o = t[name + '_hip'], t[name + '_torch']
                row[name + '_ratio_torch_over_hip'] = o['median_us'] / h['median_us']
                lines.append('B x V {} x {}  {:16s} hip {:.0f} ({:.0f} .. {:.0f}) us {:.1f} TF ({:.0f} % of 155)  torch {:.0f} '
                             '({:.0f} .. {:.0f}) us {:.1f} TF  torch / hip {:.2f}'.format(
                                 B, args.views, name, h['median_us'], h['min_us'], h['max_us'], h['tflops'],
                                 100 * h['tflops'] / 155, o['median_us'], o['min_us'], o['max_us'], o['tflops'],
                                 o['median_us'] / h['median_us']))
        print(json.dumps(row))
    if lines:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), 'profiles',
                            'ftl_times.txt')
        with open(path, 'a') as f:
            f.write('bench_ftl.py: median (min .. max) of {} after {} warm-ups\n'.format(args.repeats, args.warmup) +
                    '\n'.join(lines) + '\n')
        print('\n'.join(lines))


if __name__ == '__main__':
    main()
