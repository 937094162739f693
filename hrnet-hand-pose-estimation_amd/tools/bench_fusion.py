"""Timing of the cross-view fusion layer (csrc/view_fusion.hip) at the workload's size, against the same math in torch:

    python tools/bench_fusion.py [--batches 1 4] [--views 4] [--joints 21] [--size 64] [--repeats 20] [--warmup 3]
    python tools/bench_fusion.py --counts-only          (no device: the traffic model alone)
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_fusion.py --profile-pass --batches 1
                                                  (a run of its own for the per-kernel times; prints nothing else)

`traffic(B, V, K, P)` is the traffic model the share-of-floor figures come from: for each of the three kernels the bytes
that must cross HBM (every weight element read once by forward and dH, every dW element written once, the activations
read and written once) and the FLOPs (2 * M * P * P per pair), the floor max(bytes / 6.3 TB/s, FLOPs / 157 TFLOP/s)
and which of the two bounds it.

The baseline is the reference's composition (lib/models/multiview_pose_hrnet.py:57-71): twelve F.linear calls plus
scaled adds, and its autograd backward, in the same process on the same inputs, timed with device events after a
warm-up, alternating with the fused path; the figures are medians with the spread (min .. max) over the repeats.
Without a HIP device the timing modes fail: there is no fallback.
"""
import argparse
import json
import statistics
import sys

import _init_paths  # noqa: F401

HBM_BYTES_PER_S = 6.3e12          # achievable HBM rate of the MI355X
F32_MFMA_FLOPS = 157e12           # f32-input MFMA rate


def traffic(B, V, K, P):
    """{'forward' | 'dH' | 'dW': {'bytes', 'flops', 'floor_us', 'bound', 'launches'}} for one call"""
    M, pairs = B * K, V * (V - 1)
    weights = pairs * P * P * 4
    act = B * V * K * P * 4
    flops = 2 * M * P * P * pairs
    out = {}
    # forward: W once, H read, F written; dH: W once, dF read, dH written; dW: dW written once, dF and H read
    for name in ('forward', 'dH', 'dW'):
        nbytes = weights + 2 * act
        t_mem, t_cmp = nbytes / HBM_BYTES_PER_S, flops / F32_MFMA_FLOPS
        out[name] = {'bytes': nbytes, 'flops': flops, 'floor_us': 1e6 * max(t_mem, t_cmp),
                     'bound': 'bandwidth' if t_mem >= t_cmp else 'compute', 'launches': 1}
    return out


def torch_fusion(H, Ws, w_self=0.4, w_other=0.2):
    """the reference's composition on (B, V, K, P): one F.linear per ordered pair, then the weighted sum"""
    import torch
    import torch.nn.functional as F
    B, V, K, P = H.shape
    out, index = [], 0
    for i in range(V):
        acc = H[:, i] * w_self
        for j in range(V):
            if j != i:
                acc = acc + F.linear(H[:, j].reshape(B * K, P), Ws[index]).view(B, K, P) * w_other
                index += 1
        out.append(acc)
    return torch.stack(out, 1)


def _inputs(B, V, K, P, seed=0):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    H = torch.softmax(torch.randn(B, V, K, P, device='cuda', generator=g), -1)
    Ws = [(torch.rand(P, P, device='cuda', generator=g) * 2 - 1) / P ** 0.5 for _ in range(V * (V - 1))]
    dF = torch.randn(B, V, K, P, device='cuda', generator=g)
    return H, Ws, dF


def _time(fn, start, stop):
    import torch
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3          # us


def measure(B, V, K, P, repeats, warmup):
    import torch
    from models.multiview_pose_hrnet import view_fusion
    H, Ws, dF = _inputs(B, V, K, P)
    Hg = H.clone().requires_grad_(True)
    Wg = [w.requires_grad_(True) for w in Ws]
    params = [Hg] + Wg

    def fwd_hip():
        with torch.no_grad():
            view_fusion(H, Ws)

    def fwd_torch():
        with torch.no_grad():
            torch_fusion(H, Ws)

    state = {}

    def graph(fn, key):
        state[key] = fn(Hg, Wg)

    def bwd(key):
        torch.autograd.grad(state[key], params, dF)

    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in ('forward_hip', 'forward_torch', 'backward_hip', 'backward_torch')}
    for r in range(warmup + repeats):
        keep = r >= warmup
        # alternate the two paths; the graphs are rebuilt outside the timed region
        for path, ffn, gfn in (('hip', fwd_hip, view_fusion), ('torch', fwd_torch, torch_fusion)):
            t = _time(ffn, start, stop)
            if keep:
                times['forward_' + path].append(t)
            graph(gfn, path)
            torch.cuda.synchronize()
            t = _time(lambda: bwd(path), start, stop)
            if keep:
                times['backward_' + path].append(t)
            state.pop(path)
    return {k: {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)} for k, v in times.items()}


def profile_pass(B, V, K, P, repeats):
    """the fused path alone, for a kernel trace: forward, dH + dW"""
    import torch
    from models.multiview_pose_hrnet import view_fusion
    H, Ws, dF = _inputs(B, V, K, P)
    Hg = H.clone().requires_grad_(True)
    Wg = [w.requires_grad_(True) for w in Ws]
    for _ in range(repeats):
        F = view_fusion(Hg, Wg)
        torch.autograd.grad(F, [Hg] + Wg, dF)
    torch.cuda.synchronize()


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batches', type=int, nargs='+', default=[1, 4])
    p.add_argument('--views', type=int, default=4)
    p.add_argument('--joints', type=int, default=21)
    p.add_argument('--size', type=int, default=64, help='heat-map side: P = size * size')
    p.add_argument('--repeats', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--counts-only', action='store_true')
    p.add_argument('--profile-pass', action='store_true')
    args = p.parse_args(argv)
    V, K, P = args.views, args.joints, args.size * args.size
    if not args.counts_only:
        import torch
        if not torch.cuda.is_available():
            sys.exit('bench_fusion: no HIP device: the timings need one (--counts-only prints the traffic model)')
    for B in args.batches:
        if args.profile_pass:
            profile_pass(B, V, K, P, args.repeats)
            continue
        row = {'B': B, 'V': V, 'K': K, 'P': P, 'M': B * K, 'traffic': traffic(B, V, K, P)}
        if not args.counts_only:
            row['times'] = t = measure(B, V, K, P, args.repeats, args.warmup)
            floor_f = row['traffic']['forward']['floor_us']
            floor_b = row['traffic']['dH']['floor_us'] + row['traffic']['dW']['floor_us']
            row['forward_floor_share'] = floor_f / t['forward_hip']['median_us']
            row['backward_floor_share'] = floor_b / t['backward_hip']['median_us']
            row['forward_speedup_vs_torch'] = t['forward_torch']['median_us'] / t['forward_hip']['median_us']
            row['backward_speedup_vs_torch'] = t['backward_torch']['median_us'] / t['backward_hip']['median_us']
        print(json.dumps(row))


if __name__ == '__main__':
    main()
