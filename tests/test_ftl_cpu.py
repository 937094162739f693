"""FTL without a GPU: the float64 restatement (tests/ftl_ref.py) against the fixture recorded from the reference's own
forward (tests/golden/ftl.npz), the state dict of models.FTL_encoder_decoder, the model's and the tools' refusals, the
yaml, the cost model of tools/bench_ftl.py and the new C entries' declarations."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ftl_ref as R
import mhp_tree

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'hrnet-hand-pose-estimation_amd')
YAML = os.path.join(PKG, 'experiments', 'MHP', 'MHP_HRNet_w32_softmax_pose2dloss_FTL_v1.yaml')
NPZ = os.path.join(REPO, 'tests', 'golden', 'ftl.npz')


@pytest.fixture(scope='module')
def golden():
    return np.load(NPZ)


def _cfg(opts=(), root=''):
    return mhp_tree.config(root, list(opts), YAML)


def _small(channels=R.WIDE, V=4):
    return _cfg(['MODEL.EXTRA.STAGE4.NUM_CHANNELS', str(list(channels)), 'DATASET.NUM_VIEWS', str(V)])


def _tool(name):
    sys.path.insert(0, os.path.join(PKG, 'tools'))
    try:
        spec = importlib.util.spec_from_file_location('ftl_tool_' + name, os.path.join(PKG, 'tools', name + '.py'))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
    finally:
        sys.path.remove(os.path.join(PKG, 'tools'))
    return tool


# ---- the restatement and the fixture ---------------------------------------------------------------------------------
def test_restatement_against_the_fixture(golden):
    assert int(golden['seed']) == R.SEED and os.path.getsize(NPZ) < 700000
    sizes = set()
    for case, (channels, V, B, (h, w), kind) in R.CASES.items():
        feat, ext, K = R.inputs(case)
        assert np.array_equal(feat, golden[case + '/feat'].astype(np.float64))
        assert np.array_equal(ext, golden[case + '/ext']) and np.array_equal(K, golden[case + '/K'])
        mine = R.run(case, torch.float64)
        C, h2, w2 = sum(channels), R.enc_size(R.enc_size(h)), R.enc_size(R.enc_size(w))
        assert (h2 * w2) % 3 == 0
        sizes.add((h2, w2))
        assert mine['encoder_head'].shape == (B * V, C // 2, h2, w2) and mine['fuse_after_FTL'].shape == (B, C // 2, h2, w2)
        assert mine['channel_expansion'].shape == (B * V, C, h2, w2) and mine['decoder'].shape == (B * V, R.DEC, h, w)
        assert mine['heatmaps'].shape == (B * V, R.K_JOINTS, h, w) and mine['pose2d'].shape == (B, V, R.K_JOINTS, 2)
        for s in R.STAGES:
            assert R.rel(R.kept(s, mine[s]), golden[case + '/' + s]) < 1e-12, (case, s)
        assert R.rel(mine['pose2d'], golden[case + '/pose2d']) < 1e-12
        e32 = golden[case + '/e32']
        assert e32.shape == (5,) and e32.min() > 5e-8
        assert kind != 'unit' or e32.max() < 1e-5
        # the float32 restatement is as far from float64 as the reference's float32 run was
        mine32 = R.run(case, torch.float32)
        assert R.rel(mine32['heatmaps'], golden[case + '/heatmaps']) < 4 * e32[4] + 1e-7
    assert sizes == {(3, 4), (4, 3), (6, 6)}                       # triplets across rows, an odd 5 x 3 on the way, 9 x 9
    assert {(c[0], c[1]) for c in R.CASES.values()} == {(R.WIDE, 4), (R.WIDE, 3), (R.NARROW, 4), (R.NARROW, 3)}
    assert {c[2] for c in R.CASES.values()} == {1, 2} and {c[4] for c in R.CASES.values()} == {'unit', 'mhp'}


def test_composed_affines_are_the_two_step_transform():
    rng = np.random.RandomState(3)
    for kind in ('unit', 'mhp'):
        ext, K = R.cameras(kind, 2, 3, rng)
        ext, K = torch.tensor(ext), torch.tensor(K)
        g, s = R.affines(ext, K)
        x = torch.tensor(rng.standard_normal((2, 3, 5, 7, 3)))
        Rt, tt, Kt = ext[..., :3].transpose(2, 3), ext[..., 3:].transpose(2, 3), K.t()
        for v in range(3):
            want = (x[:, v] @ torch.inverse(Kt) - tt[:, v:v + 1]) @ torch.inverse(Rt[:, v:v + 1])
            got = x[:, v] @ g[:, v, :9].reshape(2, 1, 3, 3) + g[:, v, 9:].reshape(2, 1, 1, 3)
            assert R.rel(got, want) < 1e-12
            want = (x[:, v] @ Rt[:, v:v + 1] + tt[:, v:v + 1]) @ Kt
            got = x[:, v] @ s[:, v, :9].reshape(2, 1, 3, 3) + s[:, v, 9:].reshape(2, 1, 1, 3)
            assert R.rel(got, want) < 1e-12
        # hipnet.ftl.affines: the same coefficients, float64 on the host, handed over as float32
        from hipnet import ftl
        hg, hs = ftl.affines(ext, K.expand(2, 3, 3))
        assert hg.dtype == torch.float32 and tuple(hg.shape) == (2, 3, 12) == tuple(hs.shape)
        assert torch.equal(hg, g.float()) and torch.equal(hs, s.float())
    with pytest.raises(ValueError, match='differ'):
        ftl.affines(ext, torch.stack([K, K * 2]))
    with pytest.raises(ValueError, match=r'\(B, V, 3, 4\)'):
        ftl.affines(ext[0], K)
    with pytest.raises(ValueError, match='intrinsic'):
        ftl.affines(ext, K[:2])


def test_state_dict_is_the_references(golden):
    from models import FTL_encoder_decoder as M
    for channels, V in ((R.WIDE, 3), (R.NARROW, 4)):
        model = M.get_pose_net(_small(channels, V), is_train=False)
        assert isinstance(model, M.FTLMultiviewNet) and model.num_views == V and model.in_channel == sum(channels)
        head = [(k, v) for k, v in model.state_dict().items() if not k.startswith('backbone.')]
        tag = '{}_{}'.format(sum(channels), V)
        assert [k for k, _ in head] == list(golden[tag + '/keys']) and len(head) == 53
        assert [list(v.shape) + [0] * (4 - v.ndim) for _, v in head] == golden[tag + '/shapes'].tolist()
        assert [(k, tuple(v.shape)) for k, v in head] == R.keys_and_shapes(channels, V)
        state = dict(model.state_dict())
        state.update(R.to_torch(R.fill_state_dict(channels, V, seed=1), torch.float32))
        model.load_state_dict(state, strict=True)
        assert not any(p.requires_grad for p in model.backbone.parameters())
    assert any(k.startswith('backbone.') for k in model.state_dict())
    # the full width: the reference's 240 is C // 2
    full = dict(R.keys_and_shapes((32, 64, 128, 256), 4))
    assert full['encoder_head.layer_lst.1.0.weight'] == (240, 480, 3, 3)
    assert full['fuse_after_FTL.layer_lst.0.0.weight'] == (240, 960, 1, 1) and full['decoder.layer_lst.0.0.weight'] == (480, 256, 3, 3)


def test_model_refusals():
    from models import FTL_encoder_decoder as M
    with pytest.raises(ValueError, match='BACKBONE_NAME'):
        M.FTLMultiviewNet(_cfg(['MODEL.BACKBONE_NAME', 'pose_hrnet']))
    with pytest.raises(ValueError, match='COMPUTE_DTYPE'):
        M.FTLMultiviewNet(_cfg(['MODEL.COMPUTE_DTYPE', 'bf16']))
    with pytest.raises(ValueError, match='multiple of 8'):
        M.FTLMultiviewNet(_cfg(['MODEL.EXTRA.STAGE4.NUM_CHANNELS', '[4, 8, 12, 18]']))
    model = M.FTLMultiviewNet(_small(R.NARROW, 3))
    feat, ext, K = torch.zeros(3, 40, 4, 8), torch.zeros(1, 3, 3, 4), torch.eye(3)
    img = torch.zeros(1, 3, 3, 32, 32)
    with pytest.raises(NotImplementedError, match='training of FTL is not built'):
        model.train().head_forward(feat, ext, K)
    with pytest.raises(NotImplementedError, match='training of FTL is not built'):
        model.train()(img, ext, K)
    model.eval()
    with pytest.raises(NotImplementedError, match='training of FTL is not built'):
        model.head_forward(feat, ext, K)                      # eval mode, a gradient required
    with torch.no_grad():
        with pytest.raises(ValueError, match='HIP-device'):
            model.head_forward(feat, ext, K)
        with pytest.raises(ValueError, match='HIP-device'):
            model(img, ext, K)
    for m in (model.encoder_head, model.decoder):
        with pytest.raises(NotImplementedError, match='holds parameters'):
            m(feat)
    assert model.encoded_size(64, 64) == (18, 18) and model.encoded_size(4, 8) == (3, 4)
    from hipnet import ftl
    z = torch.zeros
    for call in (lambda: ftl.gather(z(3, 3, 4, 20), z(1, 3, 12), 3), lambda: ftl.scatter(z(1, 3, 4, 20), z(1, 3, 12), 3),
                 lambda: ftl.conv3x3g(z(1, 4, 8, 8), z(16 * 9 * 8), 16, 2, 2)):
        with pytest.raises(ValueError, match='HIP-device'):
            call()
    assert ftl.out_size(64, 2, 2) == 33 and ftl.out_size(33, 2, 2) == 18 and ftl.out_size(18, 1, 0, 2, 0) == 33
    assert ftl.out_size(33, 1, 0, 2, 1) == 64 and ftl.size_range(33, 2, 2) == (17, 18) and ftl.size_range(18, 1, 0, 2) == (33, 35)


# ---- yaml and tools ----------------------------------------------------------------------------------------------------
def test_yaml_values():
    cfg = _cfg()
    assert cfg.MODEL.NAME == 'FTL' and cfg.MODEL.BACKBONE_NAME == 'pose_hrnet_softmax'
    assert cfg.EXP_NAME == 'MHP_HRNet_w32_softmax_pose2dloss_FTL_v1'
    assert list(cfg.MODEL.IMAGE_SIZE) == [256, 256] and list(cfg.MODEL.HEATMAP_SIZE) == [64, 64]
    assert list(cfg.DATASET.DATASET) == ['MHP_mv'] == list(cfg.DATASET.TEST_DATASET)
    assert cfg.DATASET.NUM_JOINTS == 21 and cfg.DATASET.NUM_VIEWS == 4 and cfg.DATASET.SIGMA == 2
    assert cfg.DATASET.FLIP is True and cfg.DATASET.ROT_FACTOR == 45 and cfg.DATASET.SCALE_FACTOR == 0.35
    assert cfg.MODEL.HEATMAP_SOFTMAX is True and cfg.MODEL.TRAINABLE_SOFTMAX is False
    assert list(cfg.MODEL.EXTRA.STAGE4.NUM_CHANNELS) == [32, 64, 128, 256]
    assert cfg.LOSS.WITH_POSE2D_LOSS and cfg.LOSS.WITH_POSE3D_LOSS and not cfg.LOSS.WITH_HEATMAP_LOSS
    assert cfg.TRAIN.IMAGES_PER_GPU == 1 and cfg.TEST.IMAGES_PER_GPU == 2 and cfg.TRAIN.LR == 0.001
    assert list(cfg.TRAIN.LR_STEP) == [8, 16, 24] and cfg.TRAIN.LR_FACTOR == 0.5 and cfg.TRAIN.END_EPOCH == 31


def test_tools_refuse(tmp_path):
    tool = _tool('evaluate_ftl')
    tool.check_config(_cfg(), (1, 2, 3, 4))
    with pytest.raises(ValueError, match='evaluates FTLMultiviewNet'):
        tool.check_config(_cfg(['MODEL.NAME', 'vol']))
    with pytest.raises(ValueError, match='DATASET.NUM_VIEWS = 4'):
        tool.check_config(_cfg(), (1, 2, 3))
    with pytest.raises(ValueError, match='BACKBONE_NAME'):
        tool.check_config(_cfg(['MODEL.BACKBONE_NAME', 'pose_hrnet']))
    with pytest.raises(ValueError, match='never random weights'):
        tool.main(['--cfg', YAML, '--model_path', str(tmp_path / 'none.pth.tar')])
    # the triangulating tool and the 3-D trainer keep refusing the model
    e3d = _tool('evaluate_3D')
    assert 'FTL' in e3d.NOT_BUILT
    with pytest.raises(ValueError, match="MODEL.NAME 'FTL' is not built"):
        e3d.build_model('FTL')
    with pytest.raises(ValueError, match="MODEL.NAME 'FTL'"):
        _tool('train3D').check_config(_cfg())


def test_bench_counts_only():
    r = subprocess.run([sys.executable, os.path.join('tools', 'bench_ftl.py'), '--counts-only'], cwd=PKG,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(l) for l in r.stdout.strip().splitlines()]
    assert [(row['B'], row['V']) for row in rows] == [(1, 4), (4, 4)] and all('times' not in row for row in rows)
    c = rows[0]['counts']
    st = c['stages']
    assert list(st) == ['encoder_head.0', 'encoder_head.1', 'ftl_gather', 'fuse_after_FTL.0', 'fuse_after_FTL.1', 'ftl_scatter',
                        'channel_expansion.0', 'decoder.0', 'decoder.1', 'decoder.2+final_layer']
    assert c['total']['launches'] == 10 + 3

    def real(n_out, n_in, stride, pad_lo, z):                 # taps of n_out outputs that meet a real input, by hand
        return sum(1 for o in range(n_out) for r in range(3)
                   if (o * stride + r - pad_lo) % z == 0 and 0 <= (o * stride + r - pad_lo) // z < n_in)

    N = 4
    assert st['encoder_head.0']['flops_useful'] == 2 * N * real(33, 64, 2, 2, 1) ** 2 * 480 * 480
    assert st['encoder_head.1']['flops_useful'] == 2 * N * real(18, 33, 2, 2, 1) ** 2 * 480 * 240
    assert st['decoder.0']['flops_useful'] == 2 * N * real(33, 18, 1, 0, 2) ** 2 * 480 * 256
    assert st['decoder.1']['flops_useful'] == 2 * N * real(64, 33, 1, 0, 2) ** 2 * 256 * 256
    assert st['decoder.2+final_layer']['flops_useful'] == 2 * N * real(64, 64, 1, 1, 1) ** 2 * 256 * 21
    assert st['fuse_after_FTL.0']['flops_useful'] == 2 * 1 * 18 * 18 * 960 * 240
    # a transposed layer issues the live taps only: 9 / 4 per output on average, 128-pixel tiles per parity class
    # decoder.1: 33 -> 64, classes of 32 x 32 outputs = 4 x 2 tiles of 8 x 16, (4 + 2 + 2 + 1) live taps over the classes
    assert st['decoder.1']['flops_issued'] == 2 * N * 8 * 128 * 9 * 256 * 256
    # decoder.0: 18 -> 33, classes of up to 17 x 17 = 289 outputs: 3 strips of 128 pixels in place of 3 x 2 tiles
    assert st['decoder.0']['flops_issued'] == 2 * N * 3 * 128 * 9 * 480 * 256
    # the stride-2 encoder, all nine taps: 33 x 33 = 1089 outputs in 9 strips (5 x 3 tiles), 18 x 18 = 324 in 3 (3 x 2)
    assert st['encoder_head.0']['flops_issued'] == 2 * N * 9 * 128 * 9 * 480 * 480
    assert st['encoder_head.1']['flops_issued'] == 2 * N * 3 * 128 * 9 * 480 * 240
    from hipnet import ftl
    assert ftl.counts(1, 64, 64, 256, 21, 64, 64, 1, 1, 1)[0] == (32, 2)          # 64 x 64: the 8 x 16 grid fits, no strips
    assert ftl.counts(1, 256, 256, 16, 16, 129, 129, 2, 2, 1)[0][0] == 17 * 9     # too wide for a strip's window
    for row in st.values():
        assert row['flops_issued'] >= row['flops_useful'] > 0 and row['launches'] == 1
    assert c['total']['flops_useful'] == sum(r['flops_useful'] for r in st.values())
    assert rows[1]['counts']['total']['flops_useful'] == 4 * c['total']['flops_useful']
    assert abs(c['total']['mfma_floor_us'] - 1e6 * c['total']['flops_useful'] / 155e12) < 1e-6
    # composing decoder.2 with final_layer: 4.8 GFLOP per image less
    saved = c['flops_of_unfused_last_two_layers'] - st['decoder.2+final_layer']['flops_useful']
    assert 4.3e9 < saved / N < 4.9e9


def test_entries_are_declared_as_status_launchers():
    from hipnet import _capi as C
    from hipnet import _header
    from hipnet import conv_kxk
    H = _header.load(os.path.join(REPO, 'include', 'hrnet_hip.h'))
    for name, nargs in (('hrnet_ftl_gather', 14), ('hrnet_ftl_scatter', 13), ('hrnet_conv2d_3x3g', 21)):
        p = H.protos[name]
        assert p.status and len(p.params) == nargs and name in C.EXPORTED, name
    names = [n for n, _ in H.protos['hrnet_conv2d_3x3g'].params]
    assert names == ['dtype', 'x', 'w', 'bias', 'y', 'N', 'H', 'W', 'Cin', 'ldx', 'x_off', 'Cout', 'ldy', 'y_off', 'Ho', 'Wo',
                     'stride', 'pad_lo', 'z', 'relu', 'stream']
    assert C.VALUES['HR_ABI_VERSION'] == 2 and "'ftl.hip'" in open(os.path.join(PKG, 'build.py')).read()
    lib = C.lib()
    assert all(hasattr(lib, n) for n in ('hrnet_ftl_gather', 'hrnet_ftl_scatter', 'hrnet_conv2d_3x3g'))
    assert conv_kxk.tile()[:3] == (8, 16, 16)              # the tile that hipnet.ftl.counts assumes
    # the argument checks need no device: they refuse before any launch
    E, p = C.VALUES['HR_E_BADARG'], 4096
    conv = lambda *a: lib.hrnet_conv2d_3x3g(*a)
    ok = [C.HR_F32, p, p, None, p, 1, 4, 8, 8, 8, 0, 16, 16, 0, 3, 5, 2, 2, 1, 0, None]

    def bad(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return conv(*a) == E

    assert bad(dtype=C.HR_BF16) and bad(Ho=4) and bad(Ho=1) and bad(Wo=6) and bad(Wo=3)      # 4 x 8 at s2 p2: 2 .. 3 x 4 .. 5
    assert bad(stride=3) and bad(pad_lo=3) and bad(z=2) and bad(z=3)                  # z 2 goes with stride 1
    assert bad(Cin=6) and bad(x_off=4) and bad(y_off=4) and bad(x=p + 4) and bad(relu=2)
    g = lambda *a: lib.hrnet_ftl_gather(*a)
    assert g(p, p, p, 1, 3, 4, 4, 20, 20, 0, 60, 0, 20, None) == E                    # 16 pixels: no triplets
    assert g(p, p, p, 1, 3, 3, 4, 20, 20, 0, 56, 0, 20, None) == E                    # the last slice leaves its row
    assert g(p, p, p, 1, 3, 3, 4, 18, 20, 0, 60, 0, 20, None) == E                    # C no multiple of 4
    assert g(p, p, p, 1, 3, 3, 4, 20, 20, 0, 60, 0, 18, None) == E                    # a slice narrower than C
    assert g(p + 8, p, p, 1, 3, 3, 4, 20, 20, 0, 60, 0, 20, None) == E                # alignment
    s = lambda *a: lib.hrnet_ftl_scatter(*a)
    assert s(p, p, p, 1, 3, 4, 4, 20, 20, 0, 20, 0, None) == E
    assert s(p, p, p, 1, 3, 3, 4, 20, 20, 4, 20, 0, None) == E
    assert s(p, p, p, 1, 3, 3, 4, 20, 20, 0, 20, 4, None) == E
