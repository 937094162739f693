"""V2V without a GPU: the float64 restatement (tests/v2v_ref.py) against the reference's own output
(tests/golden/v2v.npz), the module's state-dict surface, its refusals, and the pure host query of csrc/conv3d.hip."""
import os

import numpy as np
import pytest
import torch

import v2v_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'v2v.npz')


def _fixture():
    z = np.load(GOLD)
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(z['shapes'], z['ndims'])]
    return z, [str(k) for k in z['keys']], shapes


def test_restatement_reproduces_the_reference():
    z, keys, shapes = _fixture()
    sd = R.fill_state_dict(zip(keys, shapes), int(z['seed']))
    y = R.forward(sd, z['x'])
    top = np.abs(z['y64']).max()
    err = np.abs(y - z['y64']).max() / top
    print('restatement against the reference, float64: {:.2e} of max|y| = {:.3f}'.format(err, top))
    assert y.shape == z['y64'].shape == (1, 2, 32, 32, 32) and y.dtype == np.float64
    assert err <= 1e-10
    assert 0.1 <= top <= 100.0
    # the fixture's own float32 run is a float32 run: close to y64, not equal
    e_ref = np.abs(z['y32'].astype(np.float64) - z['y64']).max() / top
    assert z['y32'].dtype == np.float32 and 0 < e_ref < 1e-4


def test_state_dict_has_the_reference_keys_and_shapes():
    from models.v2v import V2VModel
    z, keys, shapes = _fixture()
    model = V2VModel(2, 2)
    sd = model.state_dict()
    assert set(sd) == set(keys) and len(sd) == len(keys)
    assert [tuple(sd[k].shape) for k in keys] == shapes
    fill = R.fill_state_dict(zip(keys, shapes), int(z['seed']))
    loaded = {k: torch.from_numpy(np.asarray(fill[k])).to(sd[k].dtype) for k in keys}
    model.load_state_dict(loaded, strict=True)
    assert torch.equal(model.output_layer.weight.detach(), loaded['output_layer.weight'])
    # a checkpoint of the whole volumetric model carries the net under `volume_net.`
    ckpt = {'volume_net.' + k: v for k, v in loaded.items()}
    V2VModel(2, 2).load_state_dict({k[len('volume_net.'):]: v for k, v in ckpt.items()}, strict=True)
    # the workload's widths
    big = V2VModel(32, 21).state_dict()
    assert tuple(big['front_layers.0.block.0.weight'].shape) == (16, 32, 7, 7, 7)
    assert tuple(big['output_layer.weight'].shape) == (21, 32, 1, 1, 1)
    assert tuple(big['encoder_decoder.decoder_upsample2.block.0.weight'].shape) == (128, 64, 2, 2, 2)


def test_initialisation_is_xavier_normal_with_zero_bias():
    from models.v2v import V2VModel
    torch.manual_seed(3)
    model = V2VModel(2, 2)
    for m in model.modules():
        if isinstance(m, (torch.nn.Conv3d, torch.nn.ConvTranspose3d)):
            assert (m.bias == 0).all()
    w = model.encoder_decoder.mid_res.res_branch[0].weight            # 128 -> 128, 3^3: std = sqrt(2 / (2 * 128 * 27))
    want = (2.0 / (2 * 128 * 27)) ** 0.5
    assert abs(w.std().item() / want - 1.0) < 0.02 and abs(w.mean().item()) < 0.02 * want


def test_refusals_come_before_any_device_call():
    from models.v2v import V2VModel
    model = V2VModel(2, 2)
    x = torch.zeros(1, 2, 32, 32, 32)
    assert model.training
    with pytest.raises(NotImplementedError, match='training-mode forward'):
        model(x)
    model.eval()
    with pytest.raises(NotImplementedError, match='training forward and the backward are not built'):
        model(x)                                                      # the parameters require gradients
    with torch.no_grad():
        with pytest.raises(ValueError, match='HIP-device tensor'):
            model(x)
        with pytest.raises(ValueError, match='expected a .B, 2, D, H, W. tensor'):
            model(x[0])
        with pytest.raises(ValueError, match='input has 3 channels, the model takes 2'):
            model(torch.zeros(1, 3, 32, 32, 32))
        for shape in ((1, 2, 16, 32, 32), (1, 2, 32, 48, 32), (1, 2, 32, 32, 33)):
            with pytest.raises(ValueError, match='multiples of 32'):
                model(torch.zeros(shape))
    for p in model.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match='requires a gradient'):
        model(x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='HIP-device tensor'):         # nothing asks for a gradient: the device check
        model(x)
    assert model._packed is None and not model._plans


def test_host_query_answers_for_what_v2v_uses():
    from hipnet import _capi as C
    used = {(4, 16, 7), (32, 16, 7), (16, 32, 3), (16, 32, 1), (32, 32, 3), (32, 64, 3), (32, 64, 1), (64, 64, 3),
            (64, 128, 3), (64, 128, 1), (128, 128, 3), (32, 32, 1)}
    for cin, cout, ks in sorted(used):
        assert C.call('hrnet_conv3d_supported', C.HR_F32, cin, cout, ks) == 1, (cin, cout, ks)
        assert C.call('hrnet_conv3d_supported', C.HR_BF16, cin, cout, ks) == 0, (cin, cout, ks)
    for cin, cout, ks in ((2, 16, 7), (32, 21, 1), (32, 32, 5), (32, 32, 2), (0, 16, 1)):
        assert C.call('hrnet_conv3d_supported', C.HR_F32, cin, cout, ks) == 0, (cin, cout, ks)
    # the compute entries refuse by argument check alone (no device call is reached)
    for name, args in (('hrnet_conv3d', (C.HR_BF16, None, None, None, None, None, None, 1, 4, 4, 4, 32, 32, 3, 0)),
                       ('hrnet_conv3d', (C.HR_F32, None, None, None, None, None, None, 1, 4, 4, 4, 32, 32, 5, 0)),
                       ('hrnet_conv3d', (C.HR_F32, None, None, None, None, None, None, 1, 4, 4, 4, 30, 32, 3, 0)),
                       ('hrnet_maxpool3d', (C.HR_F32, 16, 32, 1, 4, 3, 4, 32)),
                       ('hrnet_maxpool3d', (C.HR_BF16, 16, 32, 1, 4, 4, 4, 32)),
                       ('hrnet_deconv3d_k2s2', (C.HR_BF16, None, None, None, None, None, None, 1, 2, 2, 2, 32, 32, 1)),
                       ('hrnet_pack_weights3d', (C.HR_BF16, None, None, 16, 4, 3, 16, 4, 0))):
        with pytest.raises(RuntimeError, match=name[len('hrnet_'):]):
            C.call(name, *args, None)
