"""What the training of FTLMultiviewNet's head promises without a device: the float64 training reference
(tests/ftl_train_ref.py) against an independent per-layer restatement, the split plan of hrnet_conv2d_3x3g_wgrad and the
argument refusals of the new entries (all before any launch), the unchanged refusals of a model built without
trainable=True, tools/train_ftl.py's config checks and schedule, and the cost model of tools/bench_ftl.py --train."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ftl_ref as R
import ftl_train_ref as TR
import mhp_tree

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'hrnet-hand-pose-estimation_amd')
YAML = os.path.join(PKG, 'experiments', 'MHP', 'MHP_HRNet_w32_softmax_pose2dloss_FTL_v1.yaml')


def _cfg(opts=()):
    return mhp_tree.config('', list(opts), YAML)


def _tool(name):
    sys.path.insert(0, os.path.join(PKG, 'tools'))
    try:
        spec = importlib.util.spec_from_file_location('ftl_train_tool_' + name, os.path.join(PKG, 'tools', name + '.py'))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
    finally:
        sys.path.remove(os.path.join(PKG, 'tools'))
    return tool


# ---- the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['b', 'c', 'd'])
def test_reference_against_the_per_layer_restatement(case):
    """autograd through F.batch_norm(training=True), the two-step transforms and the two last layers, against autograd
    through hand-written batch statistics, the composed x A + c and the folded output convolution: the same function"""
    ref = TR.run(case, torch.float64)
    P, feat, ext, K, gt = TR.tensors(case, torch.float64)
    out = TR.forward_layers(P, feat, ext, K)
    loss = TR.loss_of(out['pose2d'], gt)
    loss.backward()
    assert abs(float(loss.detach()) - float(ref['loss'])) <= 1e-12 * float(ref['loss'])
    assert R.rel(out['heatmaps'].detach().numpy(), ref['heatmaps']) < 1e-11
    channels, V, B, (h, w), kind = R.CASES[case]
    assert ref['heatmaps'].shape == (B * V, R.K_JOINTS, h, w) and ref['pose2d'].shape == (B, V, R.K_JOINTS, 2)
    grads = [k[5:] for k in ref if k.startswith('grad/')]
    assert len(grads) == 32 and len([k for k in ref if k.startswith('stat/')]) == 21
    for name in grads:
        got = P[name].grad.numpy()
        assert np.isfinite(ref['grad/' + name]).all()
        if name in TR.ZERO_GRAD_BIASES:
            # sums that cancel: zero up to float64 residue on the scale of what is summed
            assert np.abs(ref['grad/' + name]).max() <= 1e-12 * ref['scale/' + name], name
            assert np.abs(got).max() <= 1e-12 * ref['scale/' + name], name
        else:
            assert np.abs(ref['grad/' + name]).max() > 0 and R.rel(got, ref['grad/' + name]) < 1e-9, name
    # the running statistics moved by momentum 0.1 towards the batch's, and the float32 run stays a usable yardstick
    state = R.fill_state_dict(channels, V, kind=kind)
    moved = [k for k in ref if k.startswith('stat/') and not k.endswith('num_batches_tracked')
             and not np.array_equal(ref[k], state[k[5:]])]
    assert len(moved) == 14
    ref32 = TR.run(case, torch.float32)
    assert max(R.rel(ref32['grad/' + n], ref['grad/' + n]) for n in grads if n not in TR.ZERO_GRAD_BIASES) <= 1e-3


# ---- the plan query and the refusals that need no device -----------------------------------------------------------------
def test_wgrad_plan_invariants():
    from hipnet import conv_kxk_train, ftl_train
    asked = 0
    for N in (1, 3, 16):
        for Ho, Wo in ((3, 5), (4, 3), (9, 9), (10, 18), (18, 18), (33, 33), (64, 64)):
            for cin in (4, 20, 56, 240, 480):
                for cout in (1, 16, 21, 256, 480):
                    nbytes, nsplit, per = ftl_train.wgrad_plan(N, Ho, Wo, cin, cout)
                    tiles = N * -(-Ho // 8) * -(-Wo // 16)
                    cot, cit = -(-cout // 16), -(-cin // 16)
                    assert 1 <= nsplit <= min(tiles, 128) and per >= 1
                    assert (nsplit - 1) * per < tiles <= nsplit * per            # the splits cover the tiles, none empty
                    assert nbytes == nsplit * (cot * cit * 9 * 256 + cot * 16) * 4
                    assert ftl_train.wgrad_plan(N, Ho, Wo, cin, cout) == (nbytes, nsplit, per)
                    if cin != 4:                                                 # the plan of the K x K weight gradient
                        assert conv_kxk_train.wgrad_plan(N, Ho, Wo, cin, cout, 3) == (nbytes, nsplit, per)
                    asked += 1
    assert asked == 3 * 7 * 5 * 5
    # the head's layers at full size, B x V = 1 x 4: encoder_head.1 (18 x 18 outputs) and decoder.1 (33 x 33 "outputs")
    assert ftl_train.wgrad_plan(4, 18, 18, 480, 240)[1:] == (3, 8)
    assert ftl_train.wgrad_plan(4, 33, 33, 256, 256)[1:] == (4, 15)
    with pytest.raises(RuntimeError, match='Cin = 6'):
        ftl_train.wgrad_plan(1, 3, 5, 6, 16)
    with pytest.raises(RuntimeError, match='Ho = 0'):
        ftl_train.wgrad_plan(1, 0, 5, 8, 16)
    with pytest.raises(RuntimeError, match='pixel tiles'):
        ftl_train.wgrad_plan(0x7fffffff, 0x7fffffff, 0x7fffffff, 8, 16)


def test_entries_refuse_before_any_launch():
    """every argument check of the new entries comes before the first launch: host buffers stand in for the maps, no call
    here reaches a kernel, and nothing is written"""
    from hipnet import _capi as C
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += -base % 16
    a, b, c, d = base, base + 4096, base + 8192, base + 12288
    F32 = C.HR_F32

    def refused(match, name, *args):
        with pytest.raises(RuntimeError, match=match):
            C.call(name, *args)

    w = 'hrnet_conv2d_3x3g_wgrad'
    room = 1 << 24
    #                      x  dy scr bytes dw N  H  W Cin real ldx xo Cout ldy yo Ho Wo s  p
    refused('only f32', w, 1, a, b, c, room, d, 1, 4, 8, 8, 8, 8, 0, 16, 16, 0, 3, 5, 2, 2, None)
    refused('null', w, F32, None, b, c, room, d, 1, 4, 8, 8, 8, 8, 0, 16, 16, 0, 3, 5, 2, 2, None)
    refused('stride = 3', w, F32, a, b, c, room, d, 1, 4, 8, 8, 8, 8, 0, 16, 16, 0, 3, 5, 3, 2, None)
    refused('pad_lo = 3', w, F32, a, b, c, room, d, 1, 4, 8, 8, 8, 8, 0, 16, 16, 0, 3, 5, 2, 3, None)
    refused('Ho x Wo = 4 x 5', w, F32, a, b, c, room, d, 1, 4, 8, 8, 8, 8, 0, 16, 16, 0, 4, 5, 2, 2, None)
    refused('Ho x Wo = 3 x 3', w, F32, a, b, c, room, d, 1, 4, 8, 8, 8, 8, 0, 16, 16, 0, 3, 3, 2, 2, None)
    refused('9 real', w, F32, a, b, c, room, d, 1, 4, 8, 8, 9, 8, 0, 16, 16, 0, 3, 5, 2, 2, None)
    refused('multiples of 4', w, F32, a, b, c, room, d, 1, 4, 8, 8, 8, 12, 2, 16, 16, 0, 3, 5, 2, 2, None)
    refused('16-byte', w, F32, a + 4, b, c, room, d, 1, 4, 8, 8, 8, 8, 0, 16, 16, 0, 3, 5, 2, 2, None)
    refused('outside ldx', w, F32, a, b, c, room, d, 1, 4, 8, 8, 8, 8, 4, 16, 16, 0, 3, 5, 2, 2, None)
    refused('outside ldy', w, F32, a, b, c, room, d, 1, 4, 8, 8, 8, 8, 0, 16, 16, 1, 3, 5, 2, 2, None)
    refused('scratch of', w, F32, a, b, c, (9 * 256 + 16) * 4 - 1, d, 1, 4, 8, 8, 8, 8, 0, 16, 16, 0, 3, 5, 2, 2, None)
    g, s = 'hrnet_ftl_gather_bwd', 'hrnet_ftl_scatter_bwd'
    #                     dcat coef dx B  V  H  W  C  ldd do slice ldx xo
    refused('null', g, None, b, c, 1, 3, 3, 4, 20, 60, 0, 20, 20, 0, None)
    refused('triplets', g, a, b, c, 1, 3, 4, 4, 20, 60, 0, 20, 20, 0, None)
    refused('slice = 16', g, a, b, c, 1, 3, 3, 4, 20, 60, 0, 16, 20, 0, None)
    refused('multiples of 4', g, a, b, c, 1, 3, 3, 4, 20, 64, 2, 20, 20, 0, None)
    refused('outside ld', g, a, b, c, 1, 3, 3, 4, 20, 56, 0, 20, 20, 0, None)
    refused('outside ld', g, a, b, c, 1, 3, 3, 4, 20, 60, 0, 20, 20, 4, None)
    refused('16-byte', g, a + 4, b, c, 1, 3, 3, 4, 20, 60, 0, 20, 20, 0, None)
    refused('aliased', g, a, b, a, 1, 3, 3, 4, 20, 60, 0, 20, 20, 0, None)
    refused('triplets', s, a, b, c, 1, 3, 2, 2, 20, 20, 0, 20, 0, None)
    refused('outside ld', s, a, b, c, 1, 3, 3, 4, 20, 20, 4, 20, 0, None)
    refused('V = 0', s, a, b, c, 1, 0, 3, 4, 20, 20, 0, 20, 0, None)
    assert not any(buf)
    # the checked wrappers refuse host tensors before anything else
    from hipnet import ftl_train
    z = torch.zeros
    for call in (lambda: ftl_train.gather_bwd(z(1, 3, 4, 60), z(1, 3, 12), 3, 20),
                 lambda: ftl_train.scatter_bwd(z(3, 3, 4, 20), z(1, 3, 12), 3),
                 lambda: ftl_train.conv3x3g_wgrad(z(1, 4, 8, 8), z(1, 3, 5, 16), 16, 2, 2),
                 lambda: ftl_train.pack_dgrad(z(16, 8, 3, 3)), lambda: ftl_train.pack_dgrad_transpose(z(8, 16, 3, 3))):
        with pytest.raises(ValueError, match='HIP-device'):
            call()


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_model_refusals_are_unchanged_without_trainable():
    from models import FTL_encoder_decoder as M
    cfg = _cfg(['MODEL.EXTRA.STAGE4.NUM_CHANNELS', str(list(R.NARROW)), 'DATASET.NUM_VIEWS', '3'])
    feat, ext, K = torch.zeros(3, 40, 4, 8), torch.zeros(1, 3, 3, 4), torch.eye(3)
    for model in (M.FTLMultiviewNet(cfg), M.get_pose_net(cfg, is_train=False, trainable=False)):
        assert model.trainable is False
        with pytest.raises(NotImplementedError, match='training of FTL is not built \\(the backward of the transforms'):
            model.train().head_forward(feat, ext, K)
        assert model.backbone.training                       # train() of such a model is nn.Module's own
        model.eval()
        with pytest.raises(NotImplementedError, match='eval mode with a gradient required is refused'):
            model.head_forward(feat, ext, K)
        with pytest.raises(NotImplementedError, match='build the model with trainable=True'):
            model.hip()
    model = M.get_pose_net(cfg, is_train=False, trainable=True)
    assert model.trainable and not model.train().backbone.training and model.encoder_head.training
    assert len(model.head_parameters()) == 32 and all(p.requires_grad for p in model.head_parameters())
    assert not any(p.requires_grad for p in model.backbone.parameters())
    for mode in (True, False):
        with pytest.raises(ValueError, match='HIP-device'):
            model.train(mode).head_forward(feat, ext, K)
    assert list(model.state_dict()) == list(M.FTLMultiviewNet(cfg).state_dict())


# ---- the tools ---------------------------------------------------------------------------------------------------------
def test_train_tool_config_and_schedule():
    tool = _tool('train_ftl')
    tool.check_config(_cfg())
    for name in ('pose_hrnet_softmax', 'CPM', 'vol', 'pose_hrnet_hamburger'):
        with pytest.raises(ValueError, match='trains FTLMultiviewNet'):
            tool.check_config(_cfg(['MODEL.NAME', name]))
    with pytest.raises(ValueError, match='BACKBONE_NAME'):
        tool.check_config(_cfg(['MODEL.BACKBONE_NAME', 'pose_hrnet']))
    with pytest.raises(ValueError, match='MHP_mv'):
        tool.check_config(_cfg(['DATASET.DATASET', "['RHD_kpt']"]))
    with pytest.raises(ValueError, match='FlatAdam'):
        tool.check_config(_cfg(['TRAIN.OPTIMIZER', 'sgd']))
    cfg = _cfg()
    assert [tool.lr_at(cfg, e) for e in (1, 7, 8, 16, 24, 30)] == [1e-3, 1e-3, 5e-4, 2.5e-4, 1.25e-4, 1.25e-4]
    assert tool.loss_factors(1) == tool.loss_factors(20) == (1.0, 0.0) and tool.loss_factors(21) == (0.1, 1.0)
    batch = tool.synthetic_batch(cfg, 2, 0)
    assert tuple(batch['imgs'].shape) == (8, 3, 256, 256) and tuple(batch['extrinsic_matrices'].shape) == (2, 4, 3, 4)
    assert tuple(batch['pose2d'].shape) == (8, 21, 2) and tuple(batch['pose3d'].shape) == (2, 21, 3)
    assert tuple(batch['hm_inverse'].shape) == (8, 2, 3) and tuple(batch['intrinsic_matrix'].shape) == (2, 3, 3)
    # the targets are the projections of the drawn joints, in heat-map pixels
    P = batch['intrinsic_matrix'][0].double() @ batch['extrinsic_matrices'][0, 1].double()
    X = torch.cat([batch['pose3d'][0].double(), torch.ones(21, 1, dtype=torch.float64)], 1) @ P.t()
    uv = X[:, :2] / X[:, 2:] / torch.tensor([10.0, 7.5], dtype=torch.float64)
    assert float((uv - batch['pose2d'][1].double()).abs().max()) < 1e-3
    # the other entry points keep refusing the model
    with pytest.raises(ValueError, match="MODEL.NAME 'FTL'"):
        _tool('train3D').check_config(_cfg())


def test_bench_train_counts_only():
    r = subprocess.run([sys.executable, os.path.join('tools', 'bench_ftl.py'), '--train', '--counts-only'], cwd=PKG,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(l) for l in r.stdout.strip().splitlines()]
    assert [(row['B'], row['V']) for row in rows] == [(1, 4), (4, 4)]
    assert all('times' not in row and 'counts' not in row for row in rows)
    c = rows[0]['train_counts']
    st = c['stages']
    assert list(st) == ['decoder.2+final_layer', 'decoder.1', 'decoder.0', 'channel_expansion.0', 'ftl_scatter', 'fuse_after_FTL.1',
                        'fuse_after_FTL.0', 'ftl_gather', 'encoder_head.1', 'encoder_head.0']
    assert all(set(v) == {'launches', 'flops_useful', 'bytes'} for v in st.values())
    # per convolution: weight gradient (2 launches) + data gradient (none for encoder_head.0) + BatchNorm backward (none for
    # the output layer); a transform's backward is one launch
    assert [v['launches'] for v in st.values()] == [3, 4, 4, 4, 1, 4, 4, 1, 4, 3]
    assert c['total']['launches'] == 32 + 2
    fwd = json.loads(subprocess.run([sys.executable, os.path.join('tools', 'bench_ftl.py'), '--counts-only'], cwd=PKG,
                                    capture_output=True, text=True, timeout=120).stdout.splitlines()[0])['counts']['stages']
    assert st['encoder_head.0']['flops_useful'] == fwd['encoder_head.0']['flops_useful']
    assert st['decoder.1']['flops_useful'] == 2 * fwd['decoder.1']['flops_useful']
    assert c['total']['flops_useful'] == sum(v['flops_useful'] for v in st.values())
