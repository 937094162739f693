"""Timing of the PoseFormer head of pose_hrnet_transformer (csrc/transformer.hip through hipnet.transformer) at the yaml's
size, S = 4 sequences of F = 9 frames of J = 21 joints, against the same head built from torch modules on the device:

    python tools/bench_poseformer.py [--seqs 4] [--frames 9] [--joints 21] [--repeats 20] [--warmup 3]
    python tools/bench_poseformer.py --counts-only          (no device: launches and bytes alone)

`counts(S, F, J)` is the cost model: the launches of one forward and one backward of the head, the bytes of weights each
reads (forward once; backward once more, and the gradients written once) and of activations, and the floor those bytes
give at the achievable HBM rate. The head is bound by its launch boundaries, not by bytes or FLOPs (DESIGN, PoseFormer
section): the figures to watch are the launch counts.

The baseline is the reference's composition (lib/models/pose_hrnet_transformer.py:21-85, :195-237) from F.layer_norm,
F.linear, softmax and F.gelu with its autograd backward, in the same process on the same parameters and inputs (eval
mode: no stochastic depth), timed with device events after a warm-up, alternating with the HIP path; medians with the
spread (min .. max) over the repeats. Without a HIP device the timing mode fails: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import _init_paths  # noqa: F401

HBM_BYTES_PER_S = 6.3e12          # achievable HBM rate of the MI355X
EMBED, DEPTH, HEADS = 32, 4, 8
YAML = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'experiments', 'MHP',
                    'MHP_HRNet_w32_trainable_softmax_pose2dloss_PoseFormer_v1.yaml')


def counts(S, F, J):
    """launches, weight bytes and activation bytes of one forward and one backward of the head"""
    D = EMBED * J
    fwd = bwd = 0
    weights = acts = 0

    def linear(rows, cin, cout):
        nonlocal fwd, bwd, weights, acts
        fwd += 1
        bwd += 2                                     # dx; dW with db
        weights += (cin * cout + cout) * 4
        acts += rows * (cin + cout) * 4

    def norm(rows, c):
        nonlocal fwd, bwd, weights, acts
        fwd += 1
        bwd += 3                                     # dx; partial column sums; their sum
        weights += 2 * c * 4
        acts += 2 * rows * c * 4

    def block(rows, c):
        nonlocal fwd, bwd, acts
        norm(rows, c)
        linear(rows, c, 3 * c)
        fwd += 1                                     # attention
        bwd += 1
        acts += rows * 4 * c * 4
        linear(rows, c, c)
        norm(rows, c)
        linear(rows, c, 2 * c)
        linear(rows, 2 * c, c)

    linear(S * F * J, 2, EMBED)
    fwd += 1                                         # + Spatial_pos_embed
    bwd += 1
    weights += J * EMBED * 4
    for _ in range(DEPTH):
        block(S * F * J, EMBED)
    norm(S * F * J, EMBED)
    fwd += 1                                         # + Temporal_pos_embed
    bwd += 1
    weights += F * D * 4
    for _ in range(DEPTH):
        block(S * F, D)
    norm(S * F, D)
    fwd += 1                                         # weighted mean over the frames
    bwd += 1
    weights += (F + 1) * 4
    acts += S * (F + 1) * D * 4
    norm(S, D)
    linear(S, D, 2 * J)
    fwd_bytes, bwd_bytes = weights + acts, 2 * weights + 2 * acts
    return {'launches_forward': fwd, 'launches_backward': bwd, 'launches_per_block_forward': 7,
            'weight_bytes': weights, 'activation_bytes': acts,
            'forward_floor_us': 1e6 * fwd_bytes / HBM_BYTES_PER_S,
            'forward_backward_floor_us': 1e6 * (fwd_bytes + bwd_bytes) / HBM_BYTES_PER_S}


def torch_head(model, p):
    """the reference's head from torch ops on the model's own parameters (eval mode)"""
    import torch
    import torch.nn.functional as Fn
    S, F, J, _ = p.shape

    def block(x, blk):
        n, N, C = x.shape
        h = Fn.layer_norm(x, (C,), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
        qkv = Fn.linear(h, blk.attn.qkv.weight, blk.attn.qkv.bias).reshape(n, N, 3, HEADS, C // HEADS).permute(2, 0, 3, 1, 4)
        a = torch.softmax((qkv[0] @ qkv[1].transpose(-2, -1)) * blk.attn.scale, dim=-1)
        h = (a @ qkv[2]).transpose(1, 2).reshape(n, N, C)
        x = x + Fn.linear(h, blk.attn.proj.weight, blk.attn.proj.bias)
        h = Fn.layer_norm(x, (C,), blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
        h = Fn.gelu(Fn.linear(h, blk.mlp.fc1.weight, blk.mlp.fc1.bias))
        return x + Fn.linear(h, blk.mlp.fc2.weight, blk.mlp.fc2.bias)

    x = model.Spatial_patch_to_embedding(p.reshape(S * F, J, 2)) + model.Spatial_pos_embed
    for blk in model.Spatial_blocks:
        x = block(x, blk)
    x = model.Spatial_norm(x).reshape(S, F, -1) + model.Temporal_pos_embed
    for blk in model.blocks:
        x = block(x, blk)
    x = model.weighted_mean(model.Temporal_norm(x)).reshape(S, -1)
    return model.head(x).reshape(S, J, 2)


def _time(fn, start, stop):
    import torch
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3          # us


def measure(S, F, J, repeats, warmup):
    import torch
    from config import get_cfg_defaults
    from models import pose_hrnet_transformer
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(['MODEL.IMAGE_SIZE', '[64, 64]', 'MODEL.HEATMAP_SIZE', '[16, 16]', 'DATASET.NUM_JOINTS', str(J),
                         'MODEL.NUM_JOINTS', str(J), 'DATASET.SEQ_IDX', str(list(range(-(F // 2), F - F // 2)))])
    torch.manual_seed(0)
    model = pose_hrnet_transformer.get_pose_net(cfg, is_train=True).cuda().eval()
    head = [q for k, q in model.named_parameters() if not k.startswith('backbone.')]
    g = torch.Generator(device='cuda').manual_seed(1)
    p = (torch.rand(S, F, J, 2, device='cuda', generator=g) * 64).requires_grad_(True)
    dy = torch.randn(S, J, 2, device='cuda', generator=g)
    paths = {'hip': lambda: model.head_forward(p), 'torch': lambda: torch_head(model, p)}
    with torch.no_grad():
        diff = float((paths['hip']() - paths['torch']()).abs().max())
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in ('forward_hip', 'forward_torch', 'forward_backward_hip', 'forward_backward_torch')}

    def fwd(fn):
        with torch.no_grad():
            fn()

    def both(fn):
        torch.autograd.grad(fn(), [p] + head, dy)

    for r in range(warmup + repeats):
        for name, fn in paths.items():
            for key, run in (('forward_', fwd), ('forward_backward_', both)):
                t = _time(lambda: run(fn), start, stop)
                if r >= warmup:
                    times[key + name].append(t)
    out = {k: {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)} for k, v in times.items()}
    out['max_abs_difference_of_the_two_heads'] = diff
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--seqs', type=int, default=4)
    ap.add_argument('--frames', type=int, default=9)
    ap.add_argument('--joints', type=int, default=21)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--counts-only', action='store_true')
    args = ap.parse_args(argv)
    S, F, J = args.seqs, args.frames, args.joints
    row = {'S': S, 'F': F, 'J': J, 'counts': counts(S, F, J)}
    if not args.counts_only:
        import torch
        if not torch.cuda.is_available():
            sys.exit('bench_poseformer: no HIP device: the timings need one (--counts-only prints the cost model)')
        row['times'] = t = measure(S, F, J, args.repeats, args.warmup)
        row['forward_ratio_torch_over_hip'] = t['forward_torch']['median_us'] / t['forward_hip']['median_us']
        row['forward_backward_ratio_torch_over_hip'] = (t['forward_backward_torch']['median_us'] /
                                                        t['forward_backward_hip']['median_us'])
    print(json.dumps(row))


if __name__ == '__main__':
    main()
