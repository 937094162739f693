#!/usr/bin/env python
"""bench.py - images/sec of the pose_hrnet_w32 256x256 training step (forward + heat-map loss +
backward + Adam) on N MI355X, batch 64 per GPU, bf16 MFMA with f32 accumulation/statistics.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One JSON line on rank 0 (contract in the task statement). A "step" = one pass of the hot path over
one synthetic RHD-shaped batch already resident in HBM: model forward, HeatmapLoss, backward,
gradient all-reduce (N > 1, RCCL, overlapped with backward), fused Adam update.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line; its figures beside the headline
are those computed from the timed steps alone (cpu_baseline is null; roofline is null but at --mode infer). --full adds
everything that takes runs of its own, after the timed region: the per-kernel roofline pass, the self-check against the
fp32 device path (exit code 3 on failure), the data-parallel-mode step, the fp32 and WITH_POSE2D_LOSS steps and the CPU
baselines (--no-roofline, --no-selfcheck, --no-extras and --no-cpu-baseline leave out parts of it); at --mode dcn, the
per-pass kernel timings.

roofline      per-kernel HIP-event timing of one instrumented step (after the timed region); the
              dominant MFMA kernel instantiation's algorithmic FLOP/launch over its mean launch time,
              against the dense MFMA peak of the dtype (MI355X_MICROARCH.md: bf16 2.5 PF, f32 157.3 TF).
cpu_baseline  the CPU oracle (oracle/hrnet_cpu.py, torch fp32 functional restatement of the
              reference path, pinned to reference-generated fixtures) timed on this box's host cores
              on a bounded sample (B=4 steps, about 10-30 s), rank 0 at N=1 only.
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(REPO, 'hrnet-hand-pose-estimation_amd')
for p in (REPO, os.path.join(PKG, 'lib')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GFLOP_PER_IMG = {'w32': 67.70, 'w48': 236.5}
# layer-wise roofline of SURVEY 8d: sum over the conv layers of max(FLOP / MFMA peak, conv in+out bytes / 8 TB/s) for
# bf16, forward 16.4 us per w32 image; the training step is taken as 3x that (dgrad and wgrad move the same tensors)
LAYERWISE_US_PER_IMG = {('w32', 'bf16'): 3 * 16.4}      # fwd+bwd conv FLOPs / image, BASELINE.md section 2
PEAK_TFLOPS = {'bf16': 2500.0, 'fp32': 157.3}
# self-check: share of (image, joint) maps whose bf16 arg-max lies within two heat-map pixels of the fp32 device path's
SELFCHECK_ARGMAX2 = 0.5


def build_model(dtype, yaml_name):
    from config import get_cfg_defaults
    from hipnet import synth
    from models import pose_hrnet
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(PKG, 'experiments', 'RHD', yaml_name))
    cfg.MODEL.COMPUTE_DTYPE = dtype
    model = pose_hrnet.get_pose_net(cfg, is_train=False)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.fill_state_dict(model.state_dict(), 0).items()}
    model.load_state_dict(sd)
    return model, cfg, sd


def conv_flops_table(plan):
    """algorithmic FLOPs and algorithmic HBM bytes of every MFMA op of the recorded programs + its kernel
    instantiation name. Bytes = every operand tensor once (no halo re-reads, no split-K slabs):
      conv / input gradient: input + output tensor (+ the two tensors of the fused backward-statistics epilogue);
      weight gradient: the two operand tensors; fused backward (3x3 and 1x1): dz, y, x in, dx out, + the residual
      addend and the next BatchNorm's raw input when the launch uses them."""
    from hipnet import _capi as C
    buf = ctypes.create_string_buffer(160)
    es = 4 if plan.dtid == 0 else 2

    def cbytes(op):
        i = op.i
        b = (i[1] * i[2] * i[3] * i[4] + i[1] * i[5] * i[6] * i[7]) * es
        if op.p[7]:
            b += i[1] * i[5] * i[6] * i[7] * es * (2 if op.p[8] else 1)     # bs_y (+ mask source)
        return float(b)

    def fbytes(op):
        i = op.i
        pix = i[1] * i[2] * i[3]
        # x, dx (+ addend, + the next BatchNorm's raw input when it is another tensor than x)
        cin_side = 2 + (1 if op.p[8] else 0) + (1 if (op.p[10] and op.p[10] != op.p[3]) else 0)
        return float(pix * es * (2 * i[5] + cin_side * i[4]))

    def flops(op, wgrad):
        i = op.i
        if wgrad:
            n, ho, wo, cout, cin, ks = i[1], i[5], i[6], i[7], i[4], i[8]
        else:
            n, ho, wo, cout, cin, ks = i[1], i[5], i[6], i[7], i[4], i[8]
            if i[10]:                      # zero-stuffed dgrad of a stride-2 conv: only 1/4 of the taps
                return 2.0 * n * i[2] * i[3] * cout * cin * ks * ks   # are algorithmic: count the forward's
        return 2.0 * n * ho * wo * cout * cin * ks * ks

    out = {}
    for pname, prog in (('fwd', plan.fwd), ('bwd', plan.bwd)):
        for idx, op in enumerate(prog.ops):
            if op.kind == C.OP_CONV:
                mode = C.call('hrnet_conv_mode', 1 if op.p[7] else 0, 1 if op.p[4] else 0, op.i[10], op.i[12],
                              1 if op.p[6] else 0, 1 if op.p[2] else 0, op.i[11])
                C.call('hrnet_conv_kernel_name', op.i[0], op.i[1], op.i[5], op.i[6], op.i[4], op.i[7], op.i[8],
                       op.i[9], op.i[10], mode, buf, 160)
                out[(pname, idx)] = (buf.value.decode(), flops(op, False), cbytes(op))
            elif op.kind == C.OP_CONV_SUM:
                # conv whose input is the residual sum formed in its prologue: x, x2 in; side, y out
                C.call('hrnet_conv_kernel_name', op.i[0], op.i[1], op.i[2], op.i[3], op.i[4], op.i[5], op.i[6], 1, 0, 5, buf, 160)
                out[(pname, idx)] = (buf.value.decode(), 2.0 * op.i[1] * op.i[2] * op.i[3] * op.i[4] * op.i[5] * op.i[6] * op.i[6],
                                     float(op.i[1] * op.i[2] * op.i[3] * (3 * op.i[4] + op.i[5]) * es))
            elif op.kind == C.OP_BWD_FUSED:
                # weight gradient + input gradient of one 3x3 conv in one launch: 2 x the forward conv's FLOPs
                C.call('hrnet_bwd_fused_kernel_name', op.i[0], op.i[4], op.i[5], buf, 160)
                out[(pname, idx)] = (buf.value.decode(), 2 * 2.0 * op.i[1] * op.i[2] * op.i[3] * op.i[4] * op.i[5] * 9, fbytes(op))
            elif op.kind == C.OP_BWD_PW:
                C.call('hrnet_bwd_pw_kernel_name', op.i[0], op.i[4], op.i[5], buf, 160)
                out[(pname, idx)] = (buf.value.decode(), 2 * 2.0 * op.i[1] * op.i[2] * op.i[3] * op.i[4] * op.i[5], fbytes(op))
            elif op.kind == C.OP_WGRAD:
                C.call('hrnet_wgrad_kernel_name', op.i[0], op.i[5], op.i[6], op.i[7], op.i[4], op.i[8], op.i[9], buf, 160)
                out[(pname, idx)] = (buf.value.decode(), flops(op, True),
                                     float((op.i[1] * op.i[2] * op.i[3] * op.i[4] + op.i[1] * op.i[5] * op.i[6] * op.i[7]) * es))
    return out


def traffic_of(kernel_name):
    """HBM bytes per launch of a kernel from the committed PMC summary (profiles/traffic_rNN.json:
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command, gfx950 correction applied by
    scratch/pmc_traffic.py); None if the table has no row for it."""
    import glob
    import re
    files = sorted(glob.glob(os.path.join(REPO, 'profiles', 'traffic_r*.json')))
    if not files:
        return None
    table = json.load(open(files[-1]))
    m = re.match(r'(conv_ring)_kernel<()(.*)>', kernel_name)
    if m:
        key = '|'.join(['conv_ring'] + [p.strip() for p in m.group(3).split(',')])
        row = table.get(key)
        return row['hbm_bytes_per_launch'] if row else None
    m = re.match(r'(conv_bs|conv_fwdb|conv_fwds|conv_fwd|conv_dg|conv|wgrad|bwd_fused)_kernel<[^,]+, (.*)>', kernel_name)
    if not m:
        m = re.match(r'(bwd_pw)_kernel<()(.*)>', kernel_name)
        if not m:
            return None
        key = '|'.join(['bwd_pw'] + [p.strip() for p in m.group(3).split(',')])
    else:
        key = '|'.join([m.group(1)] + [p.strip() for p in m.group(2).split(',')])
    row = table.get(key)
    return row['hbm_bytes_per_launch'] if row else None


def instrumented_step(model, x, gt, criterion):
    """run one step op by op with HIP events on the launch stream; returns {kernel: [n, ms, flops]}"""
    from hipnet import _capi as C
    net = model.hip()
    model.train()
    with torch.no_grad():
        net.pack_weights(for_backward=True)
    plan = net.plan(x.shape[0], x.shape[2], x.shape[3], True, True)
    table = conv_flops_table(plan)
    # run both recorded programs op by op on the current stream (same buffers as the timed steps)
    hm, inter = plan.run_forward(x)
    g_hm = torch.empty_like(hm)
    g_hm.copy_(hm - gt).mul_(2.0 / (hm.shape[0] * hm.shape[1]))
    stats = {}
    kinds = {}
    crit = {}
    net.prepare_grads()
    plan.bwd.set_ptr(plan.gout_op, 0, g_hm.data_ptr())
    for pname, prog in (('fwd', plan.fwd), ('bwd', plan.bwd)):
        evs = []
        for idx in range(len(prog)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            prog.run(idx, idx + 1)
            e1.record()
            evs.append((idx, e0, e1))
        torch.cuda.synchronize()
        # dependency-only critical path of this program: lanes advance independently, EVENT_RECORD /
        # STREAM_WAIT ops carry the time across (every kernel at its isolated duration, unlimited GPU)
        clock, evt, comp, evc = {}, {}, {}, {}
        for idx, e0, e1 in evs:
            op = prog.ops[idx]
            lane = int(op.i[C.LANE_SLOT])
            if int(op.kind) == C.OP_EVENT_RECORD:
                evt[op.p[0]] = clock.get(lane, 0.0)
                evc[op.p[0]] = dict(comp.get(lane, {}))
            elif int(op.kind) == C.OP_STREAM_WAIT:
                if evt.get(op.p[0], 0.0) > clock.get(lane, 0.0):
                    clock[lane] = evt[op.p[0]]
                    comp[lane] = dict(evc[op.p[0]])
            else:
                ms = e0.elapsed_time(e1)
                clock[lane] = clock.get(lane, 0.0) + ms
                c = comp.setdefault(lane, {})
                c[int(op.kind)] = c.get(int(op.kind), 0.0) + ms
        last = max(clock, key=lambda l: clock[l])
        crit[pname + '_by_kind'] = {str(k): round(v, 2) for k, v in sorted(comp[last].items())}
        crit[pname] = round(max(clock.values()), 3)
        for idx, e0, e1 in evs:
            ms = e0.elapsed_time(e1)
            key = (pname, idx)
            if key in table:
                name, fl, by = table[key]
                s = stats.setdefault(name, [0, 0.0, 0.0, 0.0])
                s[0] += 1; s[1] += ms; s[2] += fl; s[3] += by
            k = kinds.setdefault(int(prog.ops[idx].kind), [0, 0.0])
            k[0] += 1; k[1] += ms
    net.mark_weights_dirty()
    kinds['critical_path_ms'] = crit
    return stats, kinds


def cpu_baseline(sd, extra, budget_s=12.0, batch=4, threads=None, max_steps=60):
    from hipnet import synth
    from oracle import hrnet_cpu as O
    # the box's CPU share, not the host's core count (a one-GPU box gets 16 cores)
    cores = min(len(os.sched_getaffinity(0)), int(os.environ.get('HRNET_CPU_THREADS', '16')))
    if threads is not None:
        cores = min(cores, threads)
    torch.set_num_threads(cores)
    b = synth.rhd_batch(batch, seed=1234)
    x, gt = torch.from_numpy(b['imgs']), torch.from_numpy(b['heatmaps'])
    state = {k: v.clone() for k, v in sd.items()}
    params = [v.requires_grad_(True) for k, v in state.items()
              if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-4)

    def step():
        opt.zero_grad()
        hm, _, stats = O.hrnet_forward(state, extra, x, training=True)
        loss = O.heatmap_loss(hm, gt)
        loss.backward()
        opt.step()
        with torch.no_grad():
            for k, v in stats.items():
                state[k].copy_(v)
    step()                                    # warm-up (allocations, oneDNN primitive cache)
    t0 = time.perf_counter()
    n = 0
    while True:
        step()
        n += 1
        if time.perf_counter() - t0 >= budget_s or n >= max_steps:
            break
    dt = time.perf_counter() - t0
    return {'value': round(batch * n / dt, 3), 'unit': 'images/sec', 'cores': cores, 'kind': 'port',
            'sample': '{} optimiser steps of batch {} (256x256, fp32, fwd+HeatmapLoss+bwd+Adam, anomaly mode off) '
                      'after 1 warm-up, {:.1f} s'.format(n, batch, dt)}


def log(*a):
    print('[bench]', *a, file=sys.stderr, flush=True)


# --dump-outputs: at most this many bytes in all; an array is written whole up to `limit` elements, above that as the
# elements at a fixed, seeded set of positions of its flattened form (the same positions in every run)
DUMP_MAX_BYTES = 64 << 20


def dump_sample(t, limit):
    t = t.detach()
    if t.numel() <= limit:
        return t
    idx = np.sort(np.random.default_rng(0).choice(t.numel(), limit, replace=False))
    return t.reshape(-1)[torch.from_numpy(idx).to(t.device)]


def dump_outputs(out_dir, arrays):
    """write {name: tensor} as out_dir/<name>.npy: float64 stays float64, every other dtype becomes float32"""
    host = {}
    for name, t in arrays.items():
        t = t.detach().cpu()
        host[name] = t.double().numpy() if t.dtype == torch.float64 else t.float().numpy()
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_MAX_BYTES:
        raise RuntimeError('--dump-outputs: {} bytes exceed the {} byte budget'.format(total, DUMP_MAX_BYTES))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in host.items():
        np.save(os.path.join(out_dir, name + '.npy'), a)
    log('dumped {} arrays ({:.1f} MB) to {}'.format(len(host), total / 1e6, out_dir))


def infer_main(args, model, x, world, rank, dev):
    """config 2: eval-mode forward + decode of a resident batch (replicas only: no collective)"""
    from utils.heatmap_decoding import get_final_preds
    model.eval()

    def step(keep=None):
        with torch.no_grad():
            hm, _ = model(x)
            if keep is not None:
                keep['heatmaps'] = hm
            return get_final_preds(hm, use_softmax=False)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    keep = {} if args.dump_outputs else None
    t0 = time.perf_counter()
    for i in range(args.steps):
        preds = step(keep if i == args.steps - 1 else None)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {'preds': preds, 'heatmaps': dump_sample(keep['heatmaps'], 1 << 23)})
    if rank == 0:
        value = world * args.batch * args.steps / dt
        peak = PEAK_TFLOPS[args.dtype]
        ach = value * 22.584 / 1e3          # forward GFLOP / image, BASELINE.md section 2
        print(json.dumps({
            'metric': 'images/sec forward+decode pose_hrnet_w32 256x256 bs={}/GPU'.format(args.batch),
            'value': round(value, 2), 'unit': 'images/sec', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': round(dt / args.steps * 1e3, 3), 'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None, 'dtype': args.dtype, 'data': 'synthetic',
            'config': {'workload': 'pose_hrnet_w32 256x256 {} eval forward + arg-max decode, batch {}/GPU, synthetic '
                                   'RHD-shaped crops, random-init weights'.format(args.dtype, args.batch),
                       'global_batch': world * args.batch, 'parallelism': 'replicas{}'.format(world)},
            'roofline': {'bound': 'mfma', 'achieved': round(ach, 2), 'peak': peak, 'unit': 'TFLOP/s',
                         'frac': round(ach / peak, 5), 'traffic': None, 'kernel': 'whole forward pass'},
            'cpu_baseline': None, 'preds_checksum': float(preds.sum().item())}))
    if world > 1:
        dist.destroy_process_group()


def dcn_pass_roofline(case, B, dev):
    """--mode dcn --full: per-pass kernel times on the launch stream (events around the C-ABI calls themselves -
    autograd's graph walk and its accumulation of the 396 MB offset gradient into .grad stay out of the kernel figure),
    one dilation, against the HBM peak"""
    from hipnet import _capi as C
    dd, x, off, w, go = case
    xd, od, wd = x.detach(), off.detach(), w.detach()
    out = torch.empty(B, 21, 64, 64, device=dev)
    gx, goff, gw = torch.empty_like(xd), torch.empty_like(od), torch.empty_like(wd)
    blocks = C.call('hrnet_deform_conv_wgrad_blocks', B, 64, 64)
    scratch = torch.empty(blocks * 21 * 21 * 9, device=dev)

    def fwd_call():
        C.call('hrnet_deform_conv_forward', C.ptr(xd), C.ptr(od), C.ptr(wd), None, C.ptr(out), B, 21, 64, 64, 21, 3, 3,
               1, 1, dd, dd, dd, dd, 1, 21, C.stream_ptr())

    def bwd_call():
        C.call('hrnet_deform_conv_backward', C.ptr(xd), C.ptr(od), C.ptr(wd), C.ptr(go), C.ptr(gx), C.ptr(goff),
               C.ptr(gw), None, C.ptr(scratch), B, 21, 64, 64, 21, 3, 3, 1, 1, dd, dd, dd, dd, 1, 21, C.stream_ptr())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    n = 10
    fwd_call(); bwd_call()
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(n):
        fwd_call()
    ev[1].record()
    for _ in range(n):
        bwd_call()
    ev[2].record()
    torch.cuda.synchronize()
    tf, tb = ev[0].elapsed_time(ev[1]) / n, ev[1].elapsed_time(ev[2]) / n
    by_f = (off.numel() + x.numel() + out.numel()) * 4
    by_b = (2 * off.numel() + 2 * x.numel() + out.numel()) * 4          # offsets read + offset gradient written
    ach = by_b / (tb * 1e-3) / 1e9
    return {'bound': 'hbm', 'achieved': round(ach, 1), 'peak': 8000.0, 'unit': 'GB/s',
            'frac': round(ach / 8000.0, 4), 'traffic': None, 'kernel': 'dcn_bwd_fused_kernel (backward, dilation 12)',
            'avg_launch_us': round(tb * 1e3, 1), 'algorithmic_bytes_per_launch': by_b,
            'forward': {'achieved': round(by_f / (tf * 1e-3) / 1e9, 1), 'avg_launch_us': round(tf * 1e3, 1),
                        'algorithmic_bytes_per_launch': by_f}}


def dcn_main(args, world, rank, dev):
    """config 5 (BASELINE.json): the deformable-convolution branch of pose_hrnet_PoseAggr at its geometry
    (reference lib/models/pose_hrnet_PoseAggr.py:508-516,615-628): input (B,21,64,64), offsets (B,378,64,64),
    weight (21,21,3,3), stride 1, dilation = padding = d for d in (3,6,12,18,24), 21 deformable groups.
    One step = forward + backward (input, offset, weight gradients) of the five dilations on resident tensors.
    HBM-bound: algorithmic bytes = offsets read once per pass + offset gradient written + input/output maps."""
    from deformable_conv import DeformConvFunction
    B = args.batch
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + rank)
    cases = []
    for dd in (3, 6, 12, 18, 24):
        x = torch.randn(B, 21, 64, 64, device=dev, generator=g, requires_grad=True)
        off = (torch.randn(B, 21 * 18, 64, 64, device=dev, generator=g) * 2).requires_grad_(True)
        w = (torch.randn(21, 21, 3, 3, device=dev, generator=g) * 0.1).requires_grad_(True)
        go = torch.randn(B, 21, 64, 64, device=dev, generator=g)
        cases.append((dd, x, off, w, go))

    def step(keep=None):
        for dd, x, off, w, go in cases:
            x.grad = off.grad = w.grad = None
            y = DeformConvFunction.apply(x, off, w, None, 1, dd, dd, 1, 21, 64)
            y.backward(go)
            if keep is not None:
                keep[dd] = y.detach()
            del y
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    keep = {} if args.dump_outputs else None
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(keep if i == args.steps - 1 else None)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if rank == 0 and args.dump_outputs:
        outs = {}
        for dd, x, off, w, go in cases:
            outs.update({'d{}_output'.format(dd): dump_sample(keep[dd], 1 << 19),
                         'd{}_grad_input'.format(dd): dump_sample(x.grad, 1 << 19),
                         'd{}_grad_offset'.format(dd): dump_sample(off.grad, 1 << 19),
                         'd{}_grad_weight'.format(dd): w.grad})
        dump_outputs(args.dump_outputs, outs)
        del outs, keep
    roof = None
    if not args.no_roofline:
        roof = dcn_pass_roofline(cases[2], B, dev)
    if rank == 0:
        value = world * B * args.steps / dt
        print(json.dumps({
            'metric': 'images/sec fwd+bwd DCNv1 branch of pose_hrnet_PoseAggr (5 dilations) 21ch 64x64 bs={}/GPU'.format(B),
            'value': round(value, 2), 'unit': 'images/sec', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': round(dt / args.steps * 1e3, 3), 'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'config': {'workload': 'deformable conv v1 forward+backward, input (B,21,64,64), offsets (B,378,64,64), 3x3, '
                                   'dilations 3/6/12/18/24, 21 deformable groups, batch {}/GPU'.format(B),
                       'global_batch': world * B, 'parallelism': 'replicas{}'.format(world)},
            'roofline': roof, 'cpu_baseline': None}))
    if world > 1:
        dist.destroy_process_group()


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--arch', default='w32', choices=['w32', 'w48'],
                    help='w48 = BASELINE.json config 4: pose_hrnet_w48 384x288 (use --batch 32)')
    ap.add_argument('--mode', default='train', choices=['train', 'infer', 'dcn'],
                    help='train = the headline step (default); infer = BASELINE.json config 2: eval forward + '
                         'arg-max decode (use with --dtype fp32)')
    ap.add_argument('--full', action='store_true',
                    help='after the timed region, also measure and check what takes runs of its own: per-kernel '
                         'roofline pass, self-check against the fp32 device path, data-parallel-mode, fp32 and '
                         'WITH_POSE2D_LOSS steps, CPU baselines (a plain run prints the headline line alone)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baselines')
    ap.add_argument('--no-roofline', action='store_true', help='with --full: skip the per-kernel roofline pass')
    ap.add_argument('--pose2d-loss', action='store_true',
                    help='the WITH_POSE2D_LOSS form of the step (SURVEY 8d): decode + JointsMSELoss added through '
                         'core.function.AverageMeter.computeLosses, with its three .item() syncs per step as the reference has')
    ap.add_argument('--no-extras', action='store_true',
                    help='with --full: skip the extra (untimed, child-process) figures: fp32 training step, '
                         'WITH_POSE2D_LOSS step, CPU baseline at 1 thread and at batch 64')
    ap.add_argument('--no-selfcheck', action='store_true',
                    help='with --full: skip the (untimed) loss comparison with the fp32 device path, the '
                         'data-parallel-mode A/B and the extra figures')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step computed as DIR/<name>.npy (rank 0; '
                         'float32, float64 arrays as float64; at most 64 MB: large arrays as a fixed, seeded sample of '
                         'their elements). The inputs are the same in every run. Training mode: the steps sum BatchNorm '
                         'batch statistics in a fixed order (HRNET_DETERMINISTIC=1: per-BatchNorm finalize launches '
                         'instead of the default float-atomic sums, so ms_per_step is that of the slower ordered form), '
                         'and the last timed step starts from the seeded initial weights, BatchNorm buffers and '
                         'optimiser state (reset outside the clock; that step starts on an idle queue)')
    args = ap.parse_args(argv)
    if not args.full:
        # a plain run: nothing after the timed region but --dump-outputs and the result line
        args.no_cpu_baseline = args.no_roofline = args.no_extras = args.no_selfcheck = True
    return args


def main():
    args = parse_args()

    # --dump-outputs, training mode: BatchNorm batch sums in a fixed order (HRNET_DETERMINISTIC=1; weight gradients still
    # by float atomics, HRNET_WGRAD_ATOMIC=1), read when the step's plans are recorded. The default sums by float
    # atomics, and the chaotic forward pass turns their order into heat maps that differ from run to run by far more
    # than rounding; the ordered form repeats bit for bit and costs about 0.4 ms/step. Restored after the timed region.
    saved_env = None
    if args.dump_outputs and args.mode == 'train':
        saved_env = {k: os.environ.get(k) for k in ('HRNET_DETERMINISTIC', 'HRNET_WGRAD_ATOMIC')}
        os.environ['HRNET_DETERMINISTIC'] = '1'
        os.environ.setdefault('HRNET_WGRAD_ATOMIC', '1')

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    if world > 1:
        # the four lanes of the recorded programs plus RCCL's stream: give every stream a hardware queue of its own
        # (the HIP default is 4 per process; measured neutral at N=1, read before the runtime initialises)
        os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
    local = int(os.environ.get('LOCAL_RANK', '0'))
    # (rehearsal of the N>1 code path on a one-GPU box: HRNET_BENCH_REHEARSE=1 puts every rank on cuda:0 and carries the
    # exchange over gloo - it checks the path, its numbers mean nothing)
    rehearse = os.environ.get('HRNET_BENCH_REHEARSE', '0') == '1'
    if rehearse:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    if world > 1:
        import torch.distributed as dist
        if rehearse:
            dist.init_process_group('gloo')
        else:
            dist.init_process_group('nccl', device_id=dev)

    if args.mode == 'dcn':
        return dcn_main(args, world, rank, dev)

    from core.loss import HeatmapLoss
    from hipnet import synth
    from hipnet.optim import FlatAdam, GradSync

    yaml_name = 'RHD_HRNet_w32_max_hmloss_v1.yaml' if args.arch == 'w32' else 'RHD_HRNet_w48_softmax_hm-pose2dloss_v1.yaml'
    img_h, img_w = (256, 256) if args.arch == 'w32' else (384, 288)
    model, cfg, sd = build_model(args.dtype, yaml_name)
    model = model.to(dev).train()
    b = synth.rhd_batch(args.batch, seed=1234 + rank, img_h=img_h, img_w=img_w)
    x = torch.from_numpy(b['imgs']).to(dev)
    gt = torch.from_numpy(b['heatmaps']).to(dev)
    criterion = HeatmapLoss()
    opt = FlatAdam(model, lr=cfg.TRAIN.LR, weight_decay=cfg.TRAIN.WD)
    sync = None
    if world > 1:
        sync = GradSync(model, optimizer=opt)
    # --dump-outputs: the seeded state before any step (weights, BatchNorm buffers, optimiser moments), on the device
    init_state = None
    if args.dump_outputs and args.mode == 'train':
        init_state = ({k: v.detach().clone() for k, v in model.state_dict().items()},
                      {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()})

    if args.mode == 'infer':
        return infer_main(args, model, x, world, rank, dev)

    def step(keep=None):
        opt.zero_grad()
        hm, _ = model(x)
        loss = criterion(hm, gt)
        loss.backward()
        if sync is not None:
            sync.finish()
        opt.step()
        if keep is not None:
            keep['heatmaps'] = hm.detach()
        return loss

    if args.pose2d_loss:
        # reference lib/core/function.py:67-106 with LOSS.WITH_POSE2D_LOSS (yaml ...max_hmloss_v1.yaml:102-111 sets it
        # false; SURVEY 8d asks for the figure with it): decode (arg-max: MODEL.HEATMAP_SOFTMAX false) + JointsMSELoss
        from core.function import AverageMeter, _forward_and_losses
        from core.loss import JointsMSELoss
        cfg.defrost()
        cfg.LOSS.WITH_POSE2D_LOSS = True
        cfg.freeze()
        recorder = AverageMeter(cfg, {'heatmap_loss': criterion, 'pose2d_loss': JointsMSELoss()})
        ret = {'imgs': x, 'heatmaps': gt, 'pose2d': torch.from_numpy(b['pose2d']).to(dev),
               'visibility': torch.from_numpy(b['visibility']).to(dev)}

        def step(keep=None):      # noqa: F811  (the heat maps stay inside _forward_and_losses: not dumped)
            _imgs, loss_dict = _forward_and_losses(cfg, ret, model, recorder, dev)
            opt.zero_grad()
            loss_dict['total_loss'].backward()
            if sync is not None:
                sync.finish()
            opt.step()
            return loss_dict['total_loss']

    # (measurement, HRNET_MEASURE=1 HRNET_LANE0_PRIORITY=1: the step on a high-priority stream, i.e. lane 0 - the
    # critical chain - above the side lanes)
    prio_ctx = None
    if os.environ.get('HRNET_MEASURE') == '1' and os.environ.get('HRNET_LANE0_PRIORITY', '0') != '0':
        hp = torch.cuda.Stream(device=dev, priority=-1)
        hp.wait_stream(torch.cuda.current_stream())
        prio_ctx = torch.cuda.stream(hp)
        prio_ctx.__enter__()
    for _ in range(args.warmup):
        loss = step()
    torch.cuda.synchronize()
    # the weights the self-check below runs on: those at the start of the timed region, so that what it measures does
    # not depend on how long the run trains (the bf16 pass drifts from the fp32 one as the maps sharpen: loss 0.1-0.4 %
    # apart after 25 steps, 0.8 % after 120, 1.8 % after 320)
    snap = None
    if rank == 0 and world == 1 and not args.no_selfcheck:
        snap = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if rank == 0:
        log('warm-up done, timing {} steps'.format(args.steps))
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    keep = {} if args.dump_outputs else None
    paused = 0.0
    t0 = time.perf_counter()
    for i in range(args.steps):
        if keep is not None and i == args.steps - 1:
            # --dump-outputs: the dumped step starts from the seeded initial state, so that its inputs are the same in
            # every run (the steps before it sum by float atomics, and training amplifies that rounding from step to
            # step: the loss of the default run differs by several per cent after 25 steps). The reset is not timed.
            torch.cuda.synchronize()
            tp = time.perf_counter()
            model.load_state_dict(init_state[0])
            opt.load_state_dict(init_state[1])
            torch.cuda.synchronize()
            paused += time.perf_counter() - tp
        loss = step(keep if i == args.steps - 1 else None)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0 - paused
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    final_loss = float(loss.item())
    if saved_env is not None:
        for k, v in saved_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if prio_ctx is not None:
        prio_ctx.__exit__(None, None, None)
    if rank == 0 and args.dump_outputs:
        # the step's loss and heat maps, and the state it leaves behind: parameters after the Adam update, their
        # gradients, BatchNorm running statistics (parameters in module order, not the engine's flat order)
        params = list(model.parameters())
        flat_p = torch.cat([p.detach().reshape(-1) for p in params])
        flat_g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1) for p in params])
        outs = {'loss': loss.detach().reshape(1), 'params': dump_sample(flat_p, 1 << 20),
                'grads': dump_sample(flat_g, 1 << 20),
                'bn_running_stats': torch.cat([v.reshape(-1) for k, v in model.state_dict().items()
                                               if k.endswith(('running_mean', 'running_var'))])}
        if 'heatmaps' in keep:
            outs['heatmaps'] = dump_sample(keep['heatmaps'], 1 << 23)
        dump_outputs(args.dump_outputs, outs)
        del params, flat_p, flat_g, outs, keep

    roof = None
    extra_out = {}
    if rank == 0:
        log('timed region {:.3f} s{}'.format(dt, '' if args.no_roofline else '; instrumented per-kernel pass'))
    if rank == 0 and not args.no_roofline:
        stats, kinds = instrumented_step(model, x, gt, criterion)
        peak = PEAK_TFLOPS[args.dtype]
        # the dominant kernel: the largest share of the step's kernel time; instantiations within 3 % of the top (the two
        # fused-backward kernels take turns from box to box, 2.99 / 3.00 ms) are told apart by their algorithmic bytes per
        # step - the launch that moves more is the one the HBM roof is about - so that the named kernel does not flip
        # between runs
        top_ms = max(v[1] for v in stats.values())
        dom = max((kv for kv in stats.items() if kv[1][1] >= 0.97 * top_ms), key=lambda kv: kv[1][3])
        name, (n, ms, fl, by) = dom
        ach = fl / (ms * 1e-3) / 1e12
        ach_bw = by / (ms * 1e-3) / 1e9                      # GB/s of algorithmic bytes
        # the roof that binds this kernel: the larger of (FLOP / MFMA peak) and (algorithmic bytes / HBM peak)
        if by / 8000e9 > fl / (peak * 1e12):
            roof = {'bound': 'hbm', 'achieved': round(ach_bw, 1), 'peak': 8000.0, 'unit': 'GB/s',
                    'frac': round(ach_bw / 8000.0, 5)}
        else:
            roof = {'bound': 'mfma', 'achieved': round(ach, 2), 'peak': peak, 'unit': 'TFLOP/s',
                    'frac': round(ach / peak, 5)}
        # (the runner-up by time, when it is another instantiation of the same family: the two fused-backward kernels
        # take turns at the top from box to box)
        others = [kv for kv in sorted(stats.items(), key=lambda kv: -kv[1][1]) if kv[0] != name]
        second = others[0] if others else None
        if second is not None:
            n2, ms2, fl2, by2 = second[1]
            roof['runner_up'] = {'kernel': second[0], 'launches_per_step': n2, 'avg_launch_us': round(ms2 / n2 * 1e3, 2),
                                 'mfma_frac': round(fl2 / (ms2 * 1e-3) / 1e12 / peak, 5),
                                 'hbm_frac': round(by2 / (ms2 * 1e-3) / 8000e9, 5), 'traffic': traffic_of(second[0])}
        roof.update({'traffic': traffic_of(name), 'kernel': name, 'launches_per_step': n,
                     'avg_launch_us': round(ms / n * 1e3, 2), 'algorithmic_mb_per_launch': round(by / n / 1e6, 2),
                     'algorithmic_gflop_per_launch': round(fl / n / 1e9, 3), 'mfma_frac': round(ach / peak, 5),
                     'hbm_frac': round(ach_bw / 8000.0, 5)})
        mfma_ms = sum(v[1] for v in stats.values())
        mfma_fl = sum(v[2] for v in stats.values())
        mfma_by = sum(v[3] for v in stats.values())
        extra_out['mfma_kernels'] = {
            'ms_per_step': round(mfma_ms, 3), 'tflops': round(mfma_fl / (mfma_ms * 1e-3) / 1e12, 2),
            'frac_of_peak': round(mfma_fl / (mfma_ms * 1e-3) / 1e12 / peak, 5),
            'algorithmic_gflop_per_img': round(mfma_fl / args.batch / 1e9, 2),
            'algorithmic_gb_per_step': round(mfma_by / 1e9, 2),
            'hbm_frac_of_peak': round(mfma_by / (mfma_ms * 1e-3) / 8000e9, 5)}
        extra_out['kernel_ms'] = {k: [v[0], round(v[1], 3)] for k, v in
                                  sorted(stats.items(), key=lambda kv: -kv[1][1])}
        plan_ = model.hip().plan(x.shape[0], x.shape[2], x.shape[3], True, True)
        extra_out['launches_per_step'] = {'fwd': len(plan_.fwd), 'bwd': len(plan_.bwd),
                                          'fused_blocks': plan_.n_fused_blocks, 'deferred_wgrads': plan_.n_deferred_wgrads,
                                          'fused_sums': plan_.n_fused_sums, 'head_mix': plan_.n_head_mix,
                                          'batched_fwd_sums': plan_.n_batched_fwd_sums,
                                          'batched_bwd_jobs': plan_.n_batched_jobs}
        extra_out['wgrad_slab_mb_per_step'] = round(plan_.slab_bytes / 1e6, 1)
        extra_out['critical_path_ms'] = kinds.pop('critical_path_ms')
        extra_out['op_kind_ms'] = {str(k): [v[0], round(v[1], 3)] for k, v in sorted(kinds.items())}

    if rank == 0 and world == 1 and not args.no_selfcheck:
        # (1) parity self-check outside the timed region: the loss of one training-mode forward pass of THIS bf16 model
        # on THIS batch against the fp32 device path with the same weights (a broken kernel on the benchmark's exact
        # shapes - B=64, several tiles per workgroup - shows here; the tests run smaller batches)
        try:
            with torch.no_grad():
                if snap is not None:
                    model.load_state_dict(snap)
                hm16, _ = model(x)
                l16 = float(criterion(hm16, gt).item())
                m32, _, _ = build_model('fp32', yaml_name)
                m32.load_state_dict(model.state_dict())
                m32 = m32.to(dev).train()
                hm32, _ = m32(x)
                l32 = float(criterion(hm32, gt).item())
                rel = float(((hm16 - hm32).norm() / hm32.norm()).item())
                per_img = ((hm16 - hm32).flatten(1).norm(dim=1) / hm32.flatten(1).norm(dim=1))
                # per-joint arg-max agreement: the key point the reference's arg-max decode would report
                w_ = hm16.shape[3]
                i16, i32 = hm16.flatten(2).argmax(2), hm32.flatten(2).argmax(2)
                d = torch.maximum((i16 % w_ - i32 % w_).abs(), (i16 // w_ - i32 // w_).abs())
                agree, agree2 = float((d == 0).float().mean().item()), float((d <= 2).float().mean().item())
            loss_rel = abs(l16 - l32) / max(abs(l32), 1e-12)
            worst_img = float(per_img.max().item())
            # the limits: loss 1e-2 relative (on the weights at the start of the timed region: measured 2.5e-4 ... 6e-4
            # after 5 warm-up steps, 1.5e-3 after 20; a broken kernel is off by far more than 5e-2); no image further
            # from the fp32 path than 3x the batch's
            # rel-L2 (a broken tile walk hits single images or single tiles, not the whole batch alike); arg-max within
            # two heat-map pixels for at least SELFCHECK_ARGMAX2 of the (image, joint) maps (random-init maps are flat:
            # see DESIGN section 5 for the measured values)
            # (at random-init weights - fewer than 3 warm-up steps - the maps are flat and the arg-max is decided by
            # rounding: 0.46 within two pixels at --warmup 0, 0.66 at 1, 0.77-0.80 at 5; the bar is 0.3 there)
            amin = SELFCHECK_ARGMAX2 if args.warmup >= 3 else 0.3
            ok = (loss_rel <= 1e-2 and worst_img <= max(3.0 * rel, 0.05) and agree2 >= amin
                  and bool(torch.isfinite(hm16).all().item()))
            extra_out['selfcheck'] = {'loss_{}'.format(args.dtype): round(l16, 5), 'loss_fp32_device': round(l32, 5),
                                      'loss_rel_diff': round(loss_rel, 6), 'heatmap_rel_l2': round(rel, 5),
                                      'heatmap_rel_l2_worst_image': round(worst_img, 5),
                                      'argmax_agree': round(agree, 4), 'argmax_within_2px': round(agree2, 4)}
            extra_out['selfcheck_ok'] = ok
            del m32, hm32
            torch.cuda.empty_cache()
        except Exception as e:        # noqa: BLE001  (the line is still printed, marked failed, and the exit code says so)
            extra_out['selfcheck'] = {'error': repr(e)[:200]}
            extra_out['selfcheck_ok'] = False
        # (2) what the step costs in the form every rank of a data-parallel job runs (only the late region's weight
        # gradients deferred, none offloaded from lane 0: HRNET_DP_PLAN), on this one GPU: a SCALE record starts there
        # Measured in a child process of its own (a second plan built in THIS process after the first one's buffers were
        # freed ran 3 ms slower than the same plan in a fresh process: allocator state, not the plan).
        try:
            import subprocess
            env = dict(os.environ, HRNET_DP_PLAN='1')
            cmd = [sys.executable, os.path.abspath(__file__), '--steps', '10', '--warmup', '5', '--batch', str(args.batch),
                   '--dtype', args.dtype, '--arch', args.arch]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
            line = [l for l in r.stdout.splitlines() if l.startswith('{')][-1]
            extra_out['dp_mode_ms_per_step_1gpu'] = json.loads(line)['ms_per_step']
        except Exception as e:        # noqa: BLE001
            extra_out['dp_mode_ms_per_step_1gpu'] = None
            extra_out['dp_mode_error'] = repr(e)[:200]

    if rank == 0 and world == 1 and not args.no_selfcheck and not args.no_extras and args.arch == 'w32':
        # (3) figures SURVEY 8d asks for beside the headline, each in a child process of its own (bounded: ~15 s each):
        # the step in the reference's own arithmetic (fp32), and the WITH_POSE2D_LOSS form of the headline step (plain
        # runs, like the data-parallel-mode one above)
        import subprocess
        base = [sys.executable, os.path.abspath(__file__), '--steps', '8', '--warmup', '3', '--batch', str(args.batch),
                '--arch', args.arch]
        for key, extra_args in (('fp32_train_ms_per_step', ['--dtype', 'fp32']),
                                ('with_pose2d_loss_ms_per_step', ['--dtype', args.dtype, '--pose2d-loss'])):
            try:
                r = subprocess.run(base + extra_args, capture_output=True, text=True, timeout=240)
                line = [l for l in r.stdout.splitlines() if l.startswith('{')][-1]
                extra_out[key] = json.loads(line)['ms_per_step']
            except Exception as e:        # noqa: BLE001
                extra_out[key] = None
                extra_out[key + '_error'] = repr(e)[:200]
        if extra_out.get('fp32_train_ms_per_step'):
            v32 = args.batch / (extra_out['fp32_train_ms_per_step'] * 1e-3)
            extra_out['fp32_train_mfma_frac'] = round(v32 * GFLOP_PER_IMG[args.arch] / 1e3 / PEAK_TFLOPS['fp32'], 5)

    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        log('cpu baseline (oracle on host cores)')
        from oracle import hrnet_cpu as O    # the cpu_baseline leg is the only user of oracle/ here
        cpu = cpu_baseline(sd, O.W32_EXTRA)
        if not args.no_extras:
            # the same oracle step at one thread and at the benchmark's batch 64 (bounded samples)
            extra_out['cpu_baseline_1thread'] = cpu_baseline(sd, O.W32_EXTRA, budget_s=5.0, threads=1, max_steps=3)
            extra_out['cpu_baseline_b64'] = cpu_baseline(sd, O.W32_EXTRA, budget_s=5.0, batch=64, max_steps=2)

    if rank == 0:
        imgs = world * args.batch * args.steps
        value = imgs / dt
        out = {
            'metric': 'images/sec fwd+bwd pose_hrnet_{} {}x{} bs={}/GPU'.format(args.arch, img_h, img_w, args.batch),
            'value': round(value, 2), 'unit': 'images/sec', 'n_gpus': world, 'steps': args.steps,
            'warmup': args.warmup, 'ms_per_step': round(dt / args.steps * 1e3, 3), 'higher_is_better': True,
            'scaling': 'weak', 'vs_baseline': None, 'dtype': args.dtype, 'data': 'synthetic',
            'config': {'workload': 'pose_hrnet_{} {}x{} {} fwd+HeatmapLoss+bwd+Adam training step, batch {}/GPU, '
                                   'synthetic RHD-shaped crops, random-init weights'.format(
                                       args.arch, img_h, img_w, args.dtype, args.batch),
                       'global_batch': world * args.batch, 'parallelism': 'dp{}'.format(world)},
            'step_mfma_frac': round(value * GFLOP_PER_IMG[args.arch] / 1e3 / (world * PEAK_TFLOPS[args.dtype]), 5),
            'final_loss': final_loss,
            'layerwise_roofline_frac': (round(value * LAYERWISE_US_PER_IMG[(args.arch, args.dtype)] * 1e-6 / world, 5)
                                        if (args.arch, args.dtype) in LAYERWISE_US_PER_IMG else None),
            'roofline': roof, 'cpu_baseline': cpu,
        }
        out.update(extra_out)
        if sync is not None:
            out['dp_exchange'] = sync.describe()     # RCCL all-reduce buckets: where the backward program is cut
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()
    if rank == 0 and extra_out.get('selfcheck_ok') is False:
        log('SELF-CHECK FAILED: the timed {} program disagrees with the fp32 device path: {}'.format(
            args.dtype, extra_out.get('selfcheck')))
        sys.exit(3)


if __name__ == '__main__':
    main()
