"""PredRNN without a GPU: the float64 restatement (tests/predrnn_ref.py) against the fixture recorded from the reference's own
modules (tests/golden/predrnn.npz), the state dict of models.predrnn against the reference's table, every refusal of a
config and of a call, the yaml, tools/train.py's and tools/evaluate_predrnn.py's checks, pack_ln, the cost model of
tools/bench_predrnn.py and the new C entries' declarations."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import mhp_tree
import predrnn_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'hrnet-hand-pose-estimation_amd')
YAML = os.path.join(PKG, 'experiments', 'Pred_RNN', 'PredRNN_8frames_256x256_adam_lr1e-3.yaml')
NPZ = os.path.join(REPO, 'tests', 'golden', 'predrnn.npz')
SMALL = ['MODEL.N_HIDDEN', [8, 8], 'MODEL.HEATMAP_SIZE', [8, 8], 'MODEL.IMAGE_SIZE', [32, 32]]


@pytest.fixture(scope='module')
def golden():
    return np.load(NPZ)


def _cfg(opts=()):
    return mhp_tree.config('', list(opts), YAML)


def _tool(name):
    tools = os.path.join(PKG, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    spec = importlib.util.spec_from_file_location('predrnn_tool_' + name, os.path.join(tools, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the restatement and the fixture ---------------------------------------------------------------------------------
def test_restatement_against_the_fixture(golden):
    seed = int(golden['seed'])
    assert seed == R.SEED and os.path.getsize(NPZ) < 600000
    for name, case in R.CASES.items():
        x = R.frames(name, seed)
        assert np.array_equal(x, golden[name + '/frames'].astype(np.float64))
        y64, p64 = golden[name + '/rnn64'], golden[name + '/pose64']
        assert y64.shape == (case['B'], case['L'], 53, case['size'], case['size']) and p64.shape == (case['B'], 63)
        state = R.fill_state_dict(case, seed)
        mine_y, mine_p = R.run(name, torch.float64, seed, state)
        assert R.rel(mine_y, y64) <= 1e-10 and R.rel(mine_p, p64) <= 1e-10
        assert np.array_equal(R.last_frame(y64), golden[name + '/last'].astype(np.float64))
        for key in ('rnn', 'pose'):
            e32 = float(golden[name + '/' + key + '_e32'])
            assert abs(R.rel(golden[name + '/' + key + '32'], golden[name + '/' + key + '64']) - e32) < 1e-12
            assert 5e-8 < e32 < 3e-6
        # the recorder's condition: the final ReLU leaves at least a third of every sample's outputs well above the bound
        need = 100 * R.bound(float(golden[name + '/pose_e32'])) * np.abs(p64).max()
        assert ((p64 > need).mean(1) >= 1.0 / 3.0).all()


def test_state_dict_is_the_references(golden):
    from models import predrnn
    model = predrnn.get_pose_net(_cfg(), is_train=False)
    table = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    want = [(str(k), tuple(int(d) for d in s[:int((s != 0).sum())])) for k, s in zip(golden['keys'], golden['shapes'])]
    assert len(want) == 1940 and table == want
    head = [t for t in table if not t[0].startswith('HRNet.')]
    assert head == R.head_keys_and_shapes(R.FULL)
    assert dict(table)['resnet.fc1.weight'] == (1024, 53 * 32 * 32)
    assert dict(table)['PredRNN.cell_list.0.conv_x.1.weight'] == (448, 64, 64)


# ---- refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('opts, match', [
    (['MODEL.STRIDE', 2], 'MODEL.STRIDE 2'),
    (['MODEL.FILTER_SIZE', 4], 'MODEL.FILTER_SIZE 4'),
    (['MODEL.FILTER_SIZE', 13], 'MODEL.FILTER_SIZE 13'),
    (['MODEL.N_HIDDEN', [8, 16]], 'MODEL.N_HIDDEN'),
    (['MODEL.N_HIDDEN', [6, 6]], 'multiples of 4'),
    (['MODEL.N_HIDDEN', []], 'MODEL.N_HIDDEN'),
    (['MODEL.HEATMAP_SIZE', [64, 48]], 'square'),
    (['MODEL.HEATMAP_SIZE', [63, 63]], 'even'),
    (['MODEL.NUM_JOINTS', 20], 'MODEL.NUM_JOINTS 20'),
])
def test_config_refusals_before_anything_is_built(opts, match):
    from models import predrnn
    with pytest.raises(ValueError, match=match):
        predrnn.check_predrnn_config(_cfg(opts))
    with pytest.raises(ValueError, match=match):
        predrnn.get_pose_net(_cfg(opts), is_train=False)


def test_layer_norm_flag_is_accepted_and_ignored():
    from models import predrnn
    a = predrnn.get_pose_net(_cfg(SMALL + ['MODEL.LAYER_NORM', 0]), is_train=False)
    b = predrnn.get_pose_net(_cfg(SMALL + ['MODEL.LAYER_NORM', 1]), is_train=False)
    assert [k for k in a.state_dict()] == [k for k in b.state_dict()]
    assert 'PredRNN.cell_list.1.conv_o.1.bias' in a.state_dict()


def test_call_refusals_without_a_device():
    from models import predrnn
    model = predrnn.get_pose_net(_cfg(SMALL), is_train=False)
    frames = torch.zeros((1, 2, 3, 32, 32))
    assert model.training
    for call in (lambda: model(frames), lambda: model.rnn_forward(torch.zeros((1, 2, 53, 8, 8))),
                 lambda: model.pose_forward(torch.zeros((1, 53, 8, 8)))):
        with pytest.raises(NotImplementedError, match='training of PredRNN is not built'):
            call()
    model.eval()
    with pytest.raises(NotImplementedError, match='eval mode with a gradient required'):
        model(frames)
    with torch.no_grad():
        with pytest.raises(ValueError, match='HIP-device'):
            model(frames)
        with pytest.raises(ValueError, match='HIP-device'):
            model.rnn_forward(torch.zeros((1, 2, 53, 8, 8)))
        with pytest.raises(ValueError, match='expected'):
            model.pose_forward(torch.zeros((1, 53, 8, 6)))
        with pytest.raises(ValueError, match='expected'):
            model(torch.zeros((1, 2, 4, 32, 32)))


def test_ops_refuse_cpu_tensors():
    from hipnet import predrnn as P
    x = torch.zeros((1, 2, 2, 28))
    with pytest.raises(ValueError, match='HIP-device'):
        P.sample_stats([x])
    with pytest.raises(ValueError, match='HIP-device'):
        P.maxpool2x2(x)
    with pytest.raises(ValueError, match='HIP-device'):
        P.stlstm_out(x, x, x, x, x, x)


def test_pack_ln_round_trip():
    from hipnet import predrnn as P
    t = torch.arange(4 * 3 * 5, dtype=torch.float64).reshape(4, 3, 5)
    p = P.pack_ln(t)
    assert tuple(p.shape) == (3, 5, 4) and p.is_contiguous() and p.dtype == torch.float32
    assert float(p[2, 4, 3]) == float(t[3, 2, 4])
    assert torch.equal(P.unpack_ln(p), t.float())
    with pytest.raises(ValueError, match='pack_ln'):
        P.pack_ln(torch.zeros((3, 5)))


# ---- yaml and tools ----------------------------------------------------------------------------------------------------
def test_yaml_and_tool_checks():
    cfg = _cfg()
    assert cfg.MODEL.NAME == 'predrnn' and list(cfg.MODEL.N_HIDDEN) == [64, 64, 64, 64] and cfg.MODEL.FILTER_SIZE == 3
    assert len(cfg.DATASET.SEQ_IDX) == 8 and list(cfg.DATASET.TEST_DATASET) == ['MHP_seq'] and cfg.DATASET.SEQ_IDX[-1] == 0
    train = _tool('train')
    with pytest.raises(ValueError, match='MODEL.NAME predrnn: training of PredRNN is not built'):
        train.check_config(cfg)
    ev = _tool('evaluate_predrnn')
    ev.check_config(cfg)
    with pytest.raises(ValueError, match='MODEL.NAME \'pose_hrnet\''):
        ev.check_config(_cfg(['MODEL.NAME', 'pose_hrnet']))
    # the loader's frame-major slots -> one sequence per (window, view)
    from dataset import mhp
    B, F, V = 2, 3, 4
    imgs = torch.zeros((F * B * V, 1, 1, 1))
    order = mhp.slot_order(B, F, V)
    for b in range(B):
        for j in range(F):
            for v in range(V):
                imgs[order[b, j * V + v]] = 100 * b + 10 * j + v
    seq = ev.sequences(imgs, F, V)
    assert tuple(seq.shape) == (B * V, F, 1, 1, 1)
    for b in range(B):
        for v in range(V):
            assert [int(t) for t in seq[b * V + v].flatten()] == [100 * b + 10 * j + v for j in range(F)]


def test_counts_only(capsys):
    bench = _tool('bench_predrnn')
    assert bench.main(['--counts-only', '--shapes', '1x8', '4x8']) == 0
    rows = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    assert [(r['B'], r['L']) for r in rows] == [(1, 8), (4, 8)]
    one = rows[0]
    # a cell: five convolutions, two statistic entries of two kernels each, the two gate kernels
    assert one['launches_per_cell'] == {'conv_kxk': 5, 'sample_stats': 2, 'sample_stats kernels': 4, 'stlstm_gates': 1,
                                        'stlstm_out': 1, 'kernels': 11}
    assert one['cell']['launches'] == 11 and sum(s['launches'] for s in one['cell_stages']) == 11
    assert one['rnn']['launches'] == 8 * 4 * 11 - 7
    hw, nh = 64 * 64, 64
    assert one['cell']['flops'] == 2 * hw * nh * nh * (9 * (7 + 4 + 3 + 2) + 2)
    gates = [s for s in one['cell_stages'] if s['stage'] == 'stlstm_gates'][0]
    assert gates['ln_bytes'] == 4 * hw * 28 * nh and gates['activation_bytes'] == 4 * hw * 19 * nh
    assert rows[1]['cell']['activation_bytes'] == 4 * one['cell']['activation_bytes']
    assert rows[1]['cell']['ln_bytes'] == one['cell']['ln_bytes']               # the parameters do not grow with the batch


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_exported():
    from hipnet import _capi as C
    I, F, D, I64, VP = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_int64, ctypes.c_void_p
    names = ('hrnet_sample_stats_scratch', 'hrnet_sample_stats', 'hrnet_stlstm_gates', 'hrnet_stlstm_out',
             'hrnet_maxpool2d_2x2')
    for n in names:
        p = C.HEADER.protos[n]
        assert p.status and p.restype is I and n in C.EXPORTED and hasattr(C.lib(), n)
    assert C.ABI_VERSION == 2
    assert C._SIGS['hrnet_sample_stats_scratch'] == [I, I64, I64, I64, ctypes.POINTER(I64)]
    assert C._SIGS['hrnet_sample_stats'] == [VP, VP, VP, I64, I64, I64, I, D, VP, I64, VP, VP]
    assert C._SIGS['hrnet_stlstm_gates'] == [VP] * 11 + [I, I, VP, I, I, VP, I, VP, I, I, I, I, VP]
    assert C._SIGS['hrnet_stlstm_out'] == [VP] * 7 + [I, I, I, I, VP]
    assert C._SIGS['hrnet_maxpool2d_2x2'] == [VP, VP] + [I] * 8 + [VP]
    from hipnet import predrnn as P
    assert P.stats_scratch_bytes(4, [1835008, 1048576, 786432]) == 4 * (224 + 128 + 96) * 16
    with pytest.raises(RuntimeError, match='multiples of 4'):
        P.stats_scratch_bytes(1, [6])
