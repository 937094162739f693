"""CPM training without a GPU: the restatement with explicit decisions (tests/cpm_train_ref.py) against cpm_ref and against
itself, the new C entries' declarations and host-side refusals, the trainable flag of models.CPM, tools/train_cpm.py's
config check and the split rule's source of truth."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import cpm_ref as R
import cpm_train_ref as TR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'hrnet-hand-pose-estimation_amd')
YAML = os.path.join(PKG, 'experiments', 'MHP', 'MHP_CPM_v1.yaml')


def test_fixed_decisions_reproduce_the_free_path():
    """free run = cpm_ref.forward; the same run fed its own float64 decisions reproduces loss and gradients to 1e-12"""
    state = R.fill_state_dict(R.K_JOINTS, R.SEED)
    img, cm, tgt = TR.inputs('q')
    P = R.to_torch(state, torch.float64)
    with torch.no_grad():
        free = TR.forward(P, torch.tensor(img), torch.tensor(cm))
        ref = R.forward(P, torch.tensor(img), torch.tensor(cm))
    for a, b in zip(free, ref):
        assert torch.equal(a, b)
    for weights in (TR.LAST_STAGE, TR.ALL_STAGES):
        rec = {}
        l0, g0 = TR.loss_and_grads(state, img, cm, tgt, weights, torch.float64, None, rec)
        assert len(rec) == 6 + 3 + 5 * 5 + 6 and len(g0) == 80
        l1, g1 = TR.loss_and_grads(state, img, cm, tgt, weights, torch.float64, rec)
        assert abs(l1 - l0) <= 1e-12 * abs(l0)
        for k in g0:
            assert R.rel(g1[k], g0[k]) <= 1e-12, k
        # plain autograd of cpm_ref.forward is the same function
        Q = {k: torch.tensor(v).requires_grad_(True) for k, v in state.items()}
        TR.loss_of(R.forward(Q, torch.tensor(img), torch.tensor(cm)), torch.tensor(tgt), weights).backward()
        for k in g0:
            assert R.rel(Q[k].grad.numpy(), g0[k]) <= 1e-12, k
    assert np.array_equal(img, img.astype(np.float16).astype(np.float64)) and tgt.shape == (1, 22, 1, 2)


def test_new_entries_are_declared_and_refuse_without_a_device():
    import ctypes
    from hipnet import _capi as C
    from hipnet import _header
    H = _header.load(os.path.join(REPO, 'include', 'hrnet_hip.h'))
    for name, nargs in (('hrnet_conv2d_kxk_wgrad_scratch', 10), ('hrnet_conv2d_kxk_wgrad', 19), ('hrnet_conv2d_kxk_dgrad', 19),
                        ('hrnet_maxpool2d_3x3s2_bwd', 15)):
        p = H.protos[name]
        assert p.status and len(p.params) == nargs and name in C.EXPORTED, name
    assert C.VALUES['HR_ABI_VERSION'] == 2
    build = open(os.path.join(PKG, 'build.py')).read()
    assert "'conv_kxk_train.hip'" in build and 'conv_kxk_body.h' in build and 'conv_kxk_split.h' in build
    lib, E, p = C.lib(), C.VALUES['HR_E_BADARG'], 4096
    b, ns, per = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)
    q = lambda *a: lib.hrnet_conv2d_kxk_wgrad_scratch(*a, ctypes.byref(b), ctypes.byref(ns), ctypes.byref(per))
    assert q(C.HR_F32, 16, 32, 32, 128, 128, 11) == 0 and (b.value, ns.value, per.value) == (16 * (64 * 121 * 256 + 128) * 4, 16, 8)
    assert q(C.HR_F32, 1, 32, 32, 128, 128, 11) == 0 and (ns.value, per.value) == (8, 1)
    assert q(C.HR_F32, 1, 256, 256, 4, 128, 9) == 0 and b.value == ns.value * (8 * 27 * 256 + 128) * 4   # four-tap units
    assert q(C.HR_BF16, 1, 4, 4, 8, 16, 3) == E and q(C.HR_F32, 1, 4, 4, 8, 16, 4) == E and q(C.HR_F32, 1, 4, 4, 6, 16, 3) == E
    assert lib.hrnet_conv2d_kxk_wgrad(C.HR_F32, p, p, p, 1 << 20, p, None, 1, 4, 4, 8, 8, 8, 0, 16, 16, 0, 13, None) == E
    assert lib.hrnet_conv2d_kxk_wgrad(C.HR_F32, p, p, p, 16, p, None, 1, 4, 4, 8, 8, 8, 0, 16, 16, 0, 3, None) == E
    assert b'scratch of' in lib.hrnet_last_error_string()
    assert lib.hrnet_conv2d_kxk_wgrad(C.HR_F32, p, p, p, 1 << 20, p, None, 1, 4, 4, 8, 9, 8, 0, 16, 16, 0, 3, None) == E
    assert lib.hrnet_conv2d_kxk_dgrad(C.HR_F32, p, p, 2 * p, None, 1, 4, 4, 22, 24, 0, 8, 8, 0, 0, 0, 3, 0, None) == E
    assert lib.hrnet_conv2d_kxk_dgrad(C.HR_F32, p, p, p, None, 1, 4, 4, 24, 24, 0, 8, 8, 0, 0, 0, 3, 0, None) == E    # dx is dy
    assert lib.hrnet_conv2d_kxk_dgrad(C.HR_F32, p, p, 2 * p, None, 1, 4, 4, 24, 24, 0, 8, 8, 4, 0, 0, 3, 0, None) == E
    assert lib.hrnet_maxpool2d_3x3s2_bwd(p, p, p, 1, 4, 4, 8, 8, 0, 8, 0, 8, 0, 0, None) == E
    assert lib.hrnet_maxpool2d_3x3s2_bwd(p, 2 * p, 3 * p, 1, 4, 4, 8, 8, 4, 8, 0, 8, 0, 0, None) == E
    from hipnet import conv_kxk_train as T
    for call in (lambda: T.conv_kxk_wgrad(torch.zeros(1, 2, 2, 8), torch.zeros(1, 2, 2, 16), 16, 3),
                 lambda: T.conv_kxk_dgrad(torch.zeros(1, 2, 2, 16), torch.zeros(16 * 9 * 16), 8, 3),
                 lambda: T.maxpool3x3s2_bwd(torch.zeros(1, 2, 2, 8), torch.zeros(1, 1, 1, 8)),
                 lambda: T.pack_dgrad(torch.zeros(16, 8, 3, 3))):
        with pytest.raises(ValueError, match='HIP-device'):
            call()


def test_trainable_flag():
    from models import CPM
    img, cm = torch.zeros(1, 3, 16, 16), torch.zeros(1, 1, 16, 16)
    with pytest.raises(NotImplementedError, match='training of CPM is not built'):
        CPM.CPM(21).train()(img, cm)
    with pytest.raises(NotImplementedError, match='trainable=True'):
        CPM.CPM(21).hip()
    model = CPM.CPM(21, trainable=True)
    assert model.trainable and [k for k, _ in model.state_dict().items()] == [k for k, _ in R.keys_and_shapes()]
    with pytest.raises(ValueError, match='HIP-device'):
        model.train()(img, cm)                           # the flag lifts the refusal of training, not the device check
    with pytest.raises(NotImplementedError, match='training of CPM is not built'):
        model.eval()(img, cm)                            # eval mode with a gradient required stays refused
    with pytest.raises(ValueError, match='six'):
        CPM.cpm_loss([img] * 5, img)
    with pytest.raises(ValueError, match='zero'):
        CPM.cpm_loss([img] * 6, img, (0,) * 6)


def test_train_tool_config_check():
    import mhp_tree
    sys.path.insert(0, os.path.join(PKG, 'tools'))
    try:
        spec = importlib.util.spec_from_file_location('cpm_train_cpm_tool', os.path.join(PKG, 'tools', 'train_cpm.py'))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
    finally:
        sys.path.remove(os.path.join(PKG, 'tools'))
    cfg = lambda *opts: mhp_tree.config('', list(opts), YAML)
    assert tool.check_config(cfg()) == (0, 0, 0, 0, 0, 1)
    assert tool.check_config(cfg('TRAIN.CPM_STAGE_WEIGHTS', '[1, 1, 1, 1, 1, 1]')) == (1,) * 6
    with pytest.raises(ValueError, match='trains CPM'):
        tool.check_config(cfg('MODEL.NAME', 'pose_hrnet_softmax'))
    with pytest.raises(ValueError, match='six non-negative'):
        tool.check_config(cfg('TRAIN.CPM_STAGE_WEIGHTS', '[0, 0, 0]'))
    with pytest.raises(ValueError, match='FlatAdam'):
        tool.check_config(cfg('TRAIN.OPTIMIZER', 'sgd'))
    assert cfg().TRAIN.LR == 1e-4 and 'is_train=False' in tool.__doc__ and 'DEVIATION' in tool.__doc__
    from dataset import mhp
    with pytest.raises(ValueError, match='evaluation only'):            # the random transforms stay unbuilt
        mhp.MHP_CPM_kpt(cfg(), 'training', is_train=True)


def test_bench_train_cost_model():
    """three times the forward's FLOPs, minus the data gradient of the two image layers"""
    import json
    import subprocess
    r = subprocess.run([sys.executable, os.path.join('tools', 'bench_cpm.py'), '--train', '--counts-only'], cwd=PKG,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(l) for l in r.stdout.strip().splitlines()]
    assert [row['B'] for row in rows] == [1, 16] and all('times' not in row for row in rows)
    c = rows[0]['train_counts']
    forward = sum(2 * side * side * co * ci * ks * ks for (name, ci, co, ks), side in
                  ((row, {'1': 256, '2': 128, '3': 64}[row[0][4]] if row[0][:4] == 'conv' and row[0][4] in '123' and
                    row[0][-1] in '12' else 32) for row in R.conv_table()))
    image = 2 * 2 * 256 * 256 * 128 * 3 * 81
    assert c['total']['forward'] == c['total']['wgrad'] == forward and c['total']['dgrad'] == forward - image
    assert c['total']['flops'] == 3 * forward - image and c['total']['flops'] == 504625889280
    assert c['layers']['conv1_stage1']['dgrad'] == 0 == c['layers']['conv1_stage2']['dgrad']
    assert c['layers']['Mconv2_stage2'] == {'forward': 2 * 1024 * 128 * 128 * 121, 'wgrad': 2 * 1024 * 128 * 128 * 121,
                                            'dgrad': 2 * 1024 * 128 * 128 * 121}
    assert rows[1]['train_counts']['total']['flops'] == 16 * c['total']['flops']


def test_restatement_against_the_fixture():
    """tests/golden/cpm_train.npz holds the reference module's own float64 autograd: losses, max |g| and 1 024 sampled
    gradient values per tensor; the restatement (own decisions) matches them to 1e-10"""
    path = os.path.join(REPO, 'tests', 'golden', 'cpm_train.npz')
    G = np.load(path)
    assert os.path.getsize(path) < 1000000 and int(G['seed']) == R.SEED and float(G['lr']) == 1e-4
    keys = [k for k, _ in R.keys_and_shapes()]
    assert list(G['keys']) == keys
    state = R.fill_state_dict(R.K_JOINTS, R.SEED)
    for case in sorted(TR.CASES):
        img, cm, tgt = TR.inputs(case)
        for a, name in ((img, 'img'), (cm, 'center'), (tgt, 'target')):
            assert np.array_equal(a, G[case + '/' + name].astype(np.float64)), name
        index = TR.sample_index(case, [state[k].size for k in keys])
        assert G[case + '/gsamples'].shape == (2, 80, 1024) and index.shape == (80, 1024)
        for wi, weights in enumerate((TR.LAST_STAGE, TR.ALL_STAGES)):
            loss, grads = TR.loss_and_grads(state, img, cm, tgt, weights, torch.float64)
            assert abs(loss - G[case + '/loss'][wi]) <= 1e-10 * abs(loss)
            for i, k in enumerate(keys):
                gmax = G[case + '/gmax'][wi, i]
                assert gmax > 0 and abs(np.abs(grads[k]).max() - gmax) <= 1e-10 * gmax, k
                assert np.abs(grads[k].reshape(-1)[index[i]] - G[case + '/gsamples'][wi, i]).max() <= 1e-10 * gmax, k
    traj = G['p/trajectory']
    assert traj.shape == (6,) and abs(traj[0] - G['p/loss'][0]) <= 1e-12 * traj[0] and traj[-1] < 0.8 * traj[0]
