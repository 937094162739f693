"""The PoseFormer head of models.pose_hrnet_transformer on the GPU against tests/golden/poseformer.npz (the reference's
own float64 run) and against the float64 restatement of tests/poseformer_ref.py: eval mode at the three fixture shapes,
training mode with explicit stochastic-depth flags, and bit-reproducibility.

err = max|dev - ref64| / max|ref64| must stay within 4 * e_ref + 2 * 2^-24, e_ref being the same measure of the
restatement run in float32 on the CPU. A parameter gradient is measured against the max of its own tensor;
weighted_mean.bias (exactly zero in exact arithmetic: a constant shift before the head's LayerNorm vanishes) against the
max of weighted_mean.weight's gradient. The k third of every qkv.bias gradient is exactly zero as well (a constant added
to all keys leaves the softmax unchanged); it is part of its tensor and measured with it.
"""
import functools
import os

import numpy as np
import pytest
import torch

import mhp_tree
import poseformer_ref as R

pytestmark = pytest.mark.gpu
YAML = os.path.join(mhp_tree.PKG, 'experiments', 'MHP', 'MHP_HRNet_w32_trainable_softmax_pose2dloss_PoseFormer_v1.yaml')
SMALL = ['MODEL.IMAGE_SIZE', '[64, 64]', 'MODEL.HEATMAP_SIZE', '[16, 16]']


def _cfg(F):
    from config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(SMALL + ['DATASET.SEQ_IDX', str(list(range(-(F // 2), F - F // 2)))])
    return cfg


@functools.lru_cache(maxsize=None)
def _model(F):
    from models import pose_hrnet_transformer
    torch.manual_seed(0)
    model = pose_hrnet_transformer.get_pose_net(_cfg(F), is_train=True)
    state = R.to_torch(R.fill_state_dict(R.head_keys(F, 21)), torch.float32)
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all(k.startswith('backbone.') for k in missing)
    return model.cuda()


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'poseformer.npz'))


def _device_run(model, p, g, drop_flags=None):
    for q in model.parameters():
        q.grad = None
    pt = torch.tensor(p, dtype=torch.float32, device='cuda', requires_grad=True)
    y = model.head_forward(pt, drop_flags)
    (y * torch.tensor(g, dtype=torch.float32, device='cuda')).sum().backward()
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    grads = {k: params[k].grad.detach().clone() for k in R.STORED}
    return y.detach().clone(), pt.grad.detach().clone(), grads


def _check(label, dev, r64, r32, denom=None, bad=None):
    dev = dev.double().cpu().numpy() if isinstance(dev, torch.Tensor) else dev
    assert dev.shape == np.shape(r64) and np.isfinite(dev).all(), label
    err, e_ref = R.rel(dev, r64, denom), R.rel(r32, r64, denom)
    print('{}: err {:.3g} e_ref {:.3g} bound {:.3g}'.format(label, err, e_ref, R.bound(e_ref)))
    if not err <= R.bound(e_ref):
        bad.append((label, err, e_ref, R.bound(e_ref)))


@pytest.mark.parametrize('S,F,J', R.SHAPES)
def test_head_against_the_fixture(S, F, J):
    """eval mode: forward, pose gradient and the stored parameter gradients against the reference's float64 run.
    MI355X, forward err / e_ref / bound: (4, 9, 21) 6.7e-07 / 7.8e-07 / 3.3e-06, (2, 5, 21) 4.9e-07 / 4.6e-07 / 1.9e-06,
    (1, 1, 21) 4.6e-07 / 6.1e-07 / 2.6e-06; the pose gradients and the stored parameter gradients stay below 0.5 of their
    bounds, the closest being weighted_mean.bias at (4, 9, 21), whose float32 restatement happens to give an exact 0 (e_ref
    2.5e-16, so the bound is 2 * 2^-24 = 1.19e-07 of weighted_mean.weight's gradient): err 7.3e-08. It was 8.6e-07 with
    f32 row sums in LayerNorm and 1.33e-07 with an f32 sum in the frame-mean backward; both are f64."""
    z, t = _golden(), R.tag(S, F, J)
    p, g = z[t + '/p'], z[t + '/g']
    state = R.fill_state_dict(R.head_keys(F, J), int(z['seed']))
    y32, dp32, g32 = R.run(p, g, state, torch.float32)
    model = _model(F).eval()
    y, dp, grads = _device_run(model, p, g)
    bad = []
    _check(t + ' y', y, z[t + '/y64'], y32, bad=bad)
    _check(t + ' dp', dp, z[t + '/dp64'], dp32, bad=bad)
    for k in R.STORED:
        denom = float(z[t + '/gmax/' + ('weighted_mean.weight' if k == 'weighted_mean.bias' else k)])
        _check(t + ' ' + k, R.sample(grads[k].double().cpu().numpy()), z[t + '/grad/' + k], R.sample(g32[k]), denom, bad)
    assert not bad, bad


def _flags(S, F):
    """everything kept, but: spatial block 1 drops both branches of frame-sequence 5, temporal block 2 drops both
    branches of sequence 1, temporal block 3 drops the attention branch of sequence 2. Sequence 0 keeps everything."""
    flags = [torch.ones(S * F) for _ in range(8)] + [torch.ones(S) for _ in range(8)]
    flags[2][F + 5 % F] = 0
    flags[3][F + 5 % F] = 0
    flags[8 + 4][1] = 0
    flags[8 + 5][1] = 0
    flags[8 + 6][2] = 0
    return flags


def test_head_training_mode_with_explicit_flags():
    """training mode, S = 4, F = 9: the same flags on the device and in the restatement; a dropped branch's parameters
    still get the other sequences' gradient. MI355X: forward err 5.5e-07, e_ref 7.1e-07, bound 3.0e-06; worst parameter
    gradient against its bound: Spatial_blocks.1.attn.qkv.bias, err 1.3e-06, e_ref 7.9e-07, bound 3.3e-06."""
    S, F, J = 4, 9, 21
    p, g = R.inputs(S, F, J, seed=7)
    state = R.fill_state_dict(R.head_keys(F, J))
    flags = _flags(S, F)
    y64, dp64, g64 = R.run(p, g, state, torch.float64, drop_flags=flags)
    y32, dp32, g32 = R.run(p, g, state, torch.float32, drop_flags=flags)
    kept64, _, _ = R.run(p, g, state, torch.float64)
    assert R.rel(kept64, y64) > 1e-3                      # the flags do change the result
    model = _model(F).train()
    y, dp, grads = _device_run(model, p, g, [f.cuda() for f in flags])
    bad = []
    _check('train y', y, y64, y32, bad=bad)
    _check('train dp', dp, dp64, dp32, bad=bad)
    for k in R.STORED:
        denom = np.abs(g64['weighted_mean.weight']).max() if k == 'weighted_mean.bias' else None
        _check('train ' + k, grads[k], g64[k], g32[k], denom, bad)
    assert not bad, bad
    assert float(grads['blocks.2.attn.proj.weight'].abs().max()) > 0 and np.abs(g64['blocks.2.attn.proj.weight']).max() > 0
    with pytest.raises(ValueError, match='drop_flags'):
        model.head_forward(torch.zeros(S, F, J, 2, device='cuda'), [f.cuda() for f in flags[:15]])
    # flags drawn by the model itself: 16 tensors of 0 / 1, block 0 (rate 0) keeps everything
    drawn = model.draw_drop_flags(S, 'cuda')
    assert [int(f.numel()) for f in drawn] == [S * F] * 8 + [S] * 8
    assert all(bool(((f == 0) | (f == 1)).all()) for f in drawn) and bool((drawn[0] == 1).all() and (drawn[8] == 1).all())


def test_head_is_bit_reproducible():
    """two runs of the head's forward + backward on the same inputs give identical bits (no float atomics)"""
    S, F, J = 4, 9, 21
    p, g = R.inputs(S, F, J, seed=11)
    model = _model(F).train()
    flags = [f.cuda() for f in _flags(S, F)]
    a = _device_run(model, p, g, flags)
    b = _device_run(model, p, g, flags)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    params = dict(model.named_parameters())
    for k in R.STORED:
        assert torch.equal(a[2][k], b[2][k]), k
    assert all(q.grad is not None for k, q in params.items() if not k.startswith('backbone.'))
