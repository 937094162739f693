"""The SwinPose head of models.swin_transformer on the GPU against tests/golden/swin.npz (the reference's own float64 run)
and, at full size, against the float64 restatement of tests/swin_ref.py run inside the test.

err = max|dev - ref64| / max|ref64| must stay within swin_ref.bound(e_ref) = 4 * e_ref + 2 * 2^-24, e_ref being the same
measure of the restatement run in float32 on the CPU (the rule of tests/test_poseformer_head_gpu.py)."""
import functools
import os

import numpy as np
import pytest
import torch

import swin_ref as R

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hrnet-hand-pose-estimation_amd')
YAML = os.path.join(PKG, 'experiments', 'RHD', 'RHD_HRNet_w32_SwinTransformer_v3.yaml')


def _cfg(case, backbone, opts=()):
    from config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(['MODEL.BACKBONE_NAME', 'pose_hrnet_softmax' if backbone else '', 'MODEL.PATCH_SIZE',
                         str(case['patch']), 'MODEL.EMB_DIM', '[{}]'.format(case['emb']), 'MODEL.DEPTHS',
                         str(list(case['depths']))] + list(opts))
    return cfg


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'swin.npz'))


def _load(model, case, seed, prefix=''):
    state = R.to_torch(R.fill_state_dict(R.head_keys(case), seed), torch.float32)
    state = {k: v for k, v in state.items() if k.startswith(prefix)}
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected, unexpected
    return missing


def _report(label, dev, r64, r32):
    dev = dev.double().cpu().numpy()
    assert dev.shape == r64.shape and np.isfinite(dev).all(), label
    err, e_ref = R.rel(dev, r64), R.rel(r32, r64)
    print('{}: err {:.3g} e_ref {:.3g} bound {:.3g}'.format(label, err, e_ref, R.bound(e_ref)))
    return err, R.bound(e_ref)


def test_head_against_the_fixture_case_a():
    """head_forward (swinTransformer, decoder, softmax) on 480-channel 16x16 features, EMB_DIM 48, B = 2, against the
    reference's float64 heat maps. MI355X: err 3.86e-07, e_ref 5.26e-07, bound 2.22e-06."""
    from models import swin_transformer
    z, case = _golden(), R.CASE_A
    model = swin_transformer.get_pose_net(_cfg(case, True, ['MODEL.IMAGE_SIZE', '[64, 64]', 'MODEL.HEATMAP_SIZE', '[16, 16]']),
                                          is_train=False)
    missing = _load(model, case, int(z['seed']))
    assert all(k.startswith('backbone.') for k in missing)
    model = model.cuda().eval()
    x = torch.tensor(z['a/x'].astype(np.float32)).cuda()
    with torch.no_grad():
        y = model.head_forward(x)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (2, 21, 16, 16)
    err, bound = _report('case a', y, z['a/y64'], R.run(case, torch.float32, int(z['seed'])))
    assert err <= bound, (err, bound)
    assert abs(float(y.double().sum(dim=(2, 3)).sub(1).abs().max())) < 1e-5


def test_swin_transformer_against_the_fixture_case_b():
    """swinTransformer alone on a 3-channel 41x25 image, PATCH_SIZE 4, EMB_DIM 96: patch-embed padding, an 11x7 token map,
    odd merges; the last stage's normalised tokens against the reference's float64 run. MI355X: err 8.69e-07,
    e_ref 9.49e-07, bound 3.92e-06."""
    from models import swin_transformer
    z, case = _golden(), R.CASE_B
    model = swin_transformer.get_pose_net(_cfg(case, False), is_train=False)
    missing = _load(model, case, int(z['seed']), prefix='swinTransformer.')
    assert all(k.startswith('decoder.') or k == 'trainable_temp' for k in missing)
    model = model.cuda().eval()
    x = torch.tensor(z['b/x'].astype(np.float32)).cuda()
    with torch.no_grad():
        t, H, W = model.swinTransformer.run(x)
    torch.cuda.synchronize()
    assert (H, W) == (2, 1) and tuple(t.shape) == (1, 2, 768)
    err, bound = _report('case b', t, z['b/y64'], R.run(case, torch.float32, int(z['seed'])))
    assert err <= bound, (err, bound)


def test_full_size_head_once_and_bit_reproducible():
    """the v3 yaml's head (EMB_DIM 96, DEPTHS 2 / 2 / 18 / 2, 64x64 features) at B = 1 against the restatement run in
    float64 on the CPU; two device runs give the same bits. MI355X: err 1.16e-06, e_ref 6.91e-07, bound 2.88e-06 (24
    blocks deep; 0.40 of the bound)."""
    from models import swin_transformer
    case, seed = R.FULL, 7
    model = swin_transformer.get_pose_net(_cfg(case, True), is_train=False)
    state = R.fill_state_dict(R.head_keys(case), seed)
    P32 = R.to_torch(state, torch.float32)
    missing, unexpected = model.load_state_dict(P32, strict=False)
    assert not unexpected and all(k.startswith('backbone.') for k in missing)
    x = R.inputs(case, seed)
    with torch.no_grad():
        r32 = R.head(torch.tensor(x, dtype=torch.float32), P32, case).double().numpy()
        del P32
        r64 = R.head(torch.tensor(x), R.to_torch(state, torch.float64), case).numpy()
    del state
    model = model.cuda().eval()
    xd = torch.tensor(x, dtype=torch.float32).cuda()
    with torch.no_grad():
        a = model.head_forward(xd)
        b = model.head_forward(xd)
    torch.cuda.synchronize()
    assert tuple(a.shape) == (1, 21, 64, 64) and torch.equal(a, b)
    err, bound = _report('full size', a, r64, r32)
    assert err <= bound, (err, bound)
