"""V2V training without a GPU: the opt-in flag, the refusals of a trainable model (all before any device call), the
state-dict surface, the exported symbols, the weight gradient's scratch and split query, and the training-mode
restatement (tests/v2v_train_ref.py) against torch.nn modules."""
import ctypes

import numpy as np
import pytest
import torch

import v2v_ref as R
import v2v_train_ref as TR

NEW = ('hrnet_bn3d_parts', 'hrnet_bn3d_stats', 'hrnet_bn3d_apply', 'hrnet_bn3d_bwd', 'hrnet_maxpool3d_bwd',
       'hrnet_pack_weights3d_dgrad', 'hrnet_deconv3d_k2s2_dgrad', 'hrnet_conv3d_wgrad_scratch', 'hrnet_conv3d_wgrad')


def test_trainable_defaults_to_false_and_keeps_the_state_dict():
    from models.v2v import V2VModel
    plain, trainable = V2VModel(2, 2), V2VModel(2, 2, trainable=True)
    assert plain.trainable is False and trainable.trainable is True
    assert V2VModel(2, 2, True).trainable is True                       # third positional argument
    a, b = plain.state_dict(), trainable.state_dict()
    assert list(a) == list(b) and [tuple(v.shape) for v in a.values()] == [tuple(v.shape) for v in b.values()]
    trainable.load_state_dict(a, strict=True)
    assert len(trainable._param_key()) == len(plain._param_key())


def test_refusals_of_a_trainable_model_come_before_any_device_call():
    from models.v2v import V2VModel
    model = V2VModel(2, 2, trainable=True)
    x = torch.zeros(2, 2, 32, 32, 32)
    assert model.training
    with pytest.raises(ValueError, match='HIP-device tensor'):            # training mode is accepted: the device check
        model(x)
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        model(x[:1])                                                      # B = 1 at 32^3: the bottom level is 1^3
    with torch.no_grad():
        with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
            model(x[:1])
    with pytest.raises(ValueError, match='HIP-device tensor'):
        model(torch.zeros(1, 2, 32, 32, 64))                              # two values per channel: allowed
    with pytest.raises(ValueError, match='multiples of 32'):
        model(torch.zeros(2, 2, 32, 48, 32))
    with pytest.raises(ValueError, match='input has 3 channels, the model takes 2'):
        model(torch.zeros(2, 3, 32, 32, 32))
    model.eval()
    with pytest.raises(NotImplementedError, match='eval mode with a gradient required is refused'):
        model(x)                                                          # the parameters require gradients
    with pytest.raises(NotImplementedError, match='backward through the running statistics is not built'):
        model(x)
    for p in model.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match='eval mode with a gradient required'):
        model(x.clone().requires_grad_(True))
    with torch.no_grad():
        with pytest.raises(ValueError, match='HIP-device tensor'):        # eval under no_grad: the inference path
            model(x[:1])
    assert model._packed is None and not model._plans and model._trainer is None
    # the default model keeps its refusals
    plain = V2VModel(2, 2)
    with pytest.raises(NotImplementedError, match='training-mode forward'):
        plain(x)


def test_new_symbols_are_exported_and_refuse_by_argument_check():
    from hipnet import _capi as C
    for name in NEW:
        assert name in C.EXPORTED and hasattr(C.lib(), name), name
    assert C.lib().hrnet_abi_version() == C.ABI_VERSION == 2
    nil = None
    for name, args, msg in (
            ('hrnet_bn3d_stats', (C.HR_BF16,) + (nil,) * 11 + (1, 2, 2, 2, 16, 16, 0.1, 1e-5), 'only f32'),
            ('hrnet_bn3d_stats', (C.HR_F32,) + (nil,) * 11 + (1, 1, 1, 1, 16, 16, 0.1, 1e-5), 'more than 1 value'),
            ('hrnet_bn3d_stats', (C.HR_F32,) + (nil,) * 11 + (1, 2, 2, 2, 24, 16, 0.1, 1e-5), 'C = 24'),
            ('hrnet_bn3d_apply', (C.HR_F32,) + (nil,) * 5 + (1, 2, 2, 2, 6, 1, 0), 'C = 6'),
            ('hrnet_bn3d_bwd', (C.HR_F32,) + (nil,) * 13 + (1, 2, 2, 2, 16, 17, 0, 0, 0), '17 are real'),
            ('hrnet_bn3d_bwd', (C.HR_F32,) + (nil,) * 13 + (1, 2, 2, 2, 16, 16, 0, 0, 0), 'null'),
            ('hrnet_maxpool3d_bwd', (C.HR_F32, 16, 32, 48, 1, 4, 3, 4, 32, 0), 'must be even'),
            ('hrnet_pack_weights3d_dgrad', (C.HR_F32, 16, 32, 16, 4, 3, 16, 4), 'Cin = 4 in 4'),
            ('hrnet_pack_weights3d_dgrad', (C.HR_F32, 16, 32, 16, 4, 2, 16, 16), 'ks = 2'),
            ('hrnet_deconv3d_k2s2_dgrad', (C.HR_F32, nil, nil, nil, 1, 2, 2, 2, 4, 16, 0), 'Cin = 4'),
            ('hrnet_conv3d_wgrad', (C.HR_F32, nil, nil, nil, 0, nil, 1, 2, 2, 2, 16, 16, 16, 16, 5, 0, 0), 'ks = 5'),
            ('hrnet_conv3d_wgrad', (C.HR_F32, 16, 32, 48, 8, 64, 1, 2, 2, 2, 16, 16, 16, 16, 3, 0, 0), 'scratch of 8'),
            ('hrnet_conv3d_wgrad', (C.HR_F32, 16, 32, 48, 1 << 30, 64, 1, 2, 2, 2, 16, 16, 17, 16, 3, 0, 0), '17 real')):
        with pytest.raises(RuntimeError, match=msg):
            C.call(name, *args, None)


def _query(C, N, D, H, W, cin, cout, ks, deconv=0, dtype=0):
    nbytes, nsplit, per = ctypes.c_int64(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
    C.call('hrnet_conv3d_wgrad_scratch', dtype, N, D, H, W, cin, cout, ks, deconv, ctypes.byref(nbytes),
           ctypes.byref(nsplit), ctypes.byref(per))
    # the splits of `per` voxels cover the volume, the last one is not empty
    assert (nsplit.value - 1) * per.value < N * D * H * W <= nsplit.value * per.value
    C.call('hrnet_conv3d_wgrad_scratch', dtype, N, D, H, W, cin, cout, ks, deconv, ctypes.byref(nbytes),
           ctypes.byref(nsplit), None)                                    # the split length is optional
    return nbytes.value, nsplit.value


def test_scratch_and_split_query():
    from hipnet import _capi as C
    # one split for a small volume; the scratch is splits * taps * Cout * Cin (rounded up to 16) floats
    assert _query(C, 1, 3, 5, 7, 32, 32, 3) == (27 * 32 * 32 * 4, 1)
    assert _query(C, 1, 3, 4, 9, 4, 16, 7) == (343 * 16 * 16 * 4, 1)
    assert _query(C, 1, 1, 1, 1, 128, 128, 2, 1) == (8 * 128 * 128 * 4, 1)
    nbytes, nsplit = _query(C, 1, 16, 16, 20, 16, 32, 3)
    assert nsplit >= 3 and nbytes == nsplit * 27 * 32 * 16 * 4
    # the workload: 64^3 at B = 2 and B = 8; never more than 256 splits, and the splits cover the voxels
    for B in (2, 8):
        nbytes, nsplit = _query(C, B, 64, 64, 64, 32, 32, 3)
        assert 1 <= nsplit <= 256 and nbytes == nsplit * 27 * 32 * 32 * 4
    # a voxel count and a scratch size beyond 32 bits
    nbytes, nsplit = _query(C, 64, 512, 512, 512, 128, 128, 3)           # 2^33 voxels
    assert nsplit == 256 and nbytes == 256 * 27 * 128 * 128 * 4
    nbytes, nsplit = _query(C, 4, 64, 64, 64, 4096, 4096, 7)
    assert nbytes == nsplit * 343 * 4096 * 4096 * 4 and nbytes > 2 ** 32
    for args, msg in (((1, 4, 4, 4, 32, 32, 5), 'ks = 5'), ((1, 4, 4, 4, 30, 32, 3), 'Cin = 30'),
                      ((1, 4, 4, 4, 32, 32, 3, 1), 'ks = 3'), ((0, 4, 4, 4, 32, 32, 3), 'N = 0'),
                      ((2 ** 31 - 1,) * 4 + (32, 32, 3), 'voxels'), ((1, 4, 4, 4, 32, 32, 3, 0, 1), 'only f32')):
        with pytest.raises(RuntimeError, match=msg):
            _query(C, *args)
    assert C.call('hrnet_bn3d_parts', 1) == 1 and C.call('hrnet_bn3d_parts', 257) == 2
    assert C.call('hrnet_bn3d_parts', 2 ** 40) == 256 and C.call('hrnet_bn3d_parts', 0) == 0


def test_training_restatement_matches_torch_modules():
    """tests/v2v_train_ref.py against the model's own nn.Conv3d / nn.BatchNorm3d / nn.ConvTranspose3d children called
    as ordinary torch modules on the CPU in float64: a Res3DBlock with a skip convolution and an Upsample3DBlock"""
    from models.v2v import Res3DBlock, Upsample3DBlock
    rng = np.random.default_rng(5)
    blk = Res3DBlock(4, 8).double()
    sd = TR.block_state(blk, rng)
    blk.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    x = rng.normal(0, 1, (2, 4, 2, 3, 4))
    g = rng.normal(0, 1, (2, 8, 2, 3, 4))
    got = TR.run({'b.' + k: v for k, v in sd.items()}, lambda net, t, a: net.res(t, 'b'), x, g)
    xt = torch.from_numpy(x).requires_grad_(True)
    y = torch.relu(blk.res_branch(xt) + blk.skip_con(xt))
    y.backward(torch.from_numpy(g))
    assert np.abs(got['y'] - y.detach().numpy()).max() < 1e-12
    assert np.abs(got['dx'] - xt.grad.numpy()).max() < 1e-12
    for k, p in blk.named_parameters():
        assert np.abs(got['grad:b.' + k] - p.grad.numpy()).max() < 1e-11, k
    for k, b in blk.named_buffers():
        assert np.abs(got['b.' + k] - b.numpy()).max() < 1e-12, k
    assert TR.bias_under_bn(set(sd)) == {'res_branch.0.bias', 'res_branch.3.bias', 'skip_con.0.bias'}
    up = Upsample3DBlock(8, 4, 2, 2).double()
    sd = TR.block_state(up, rng)
    up.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    x, add, g = rng.normal(0, 1, (2, 8, 1, 2, 3)), rng.normal(0, 1, (2, 4, 2, 4, 6)), rng.normal(0, 1, (2, 4, 2, 4, 6))
    got = TR.run({'b.' + k: v for k, v in sd.items()}, lambda net, t, a: net.upsample(t, 'b', a), x, g, add)
    xt, at = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(add).requires_grad_(True)
    (up.block(xt) + at).backward(torch.from_numpy(g))
    assert np.abs(got['dx'] - xt.grad.numpy()).max() < 1e-12 and np.array_equal(got['dadd'], g)
    assert np.abs(got['grad:b.block.0.weight'] - up.block[0].weight.grad.numpy()).max() < 1e-12
