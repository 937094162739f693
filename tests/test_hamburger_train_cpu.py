"""Training of pose_hrnet_hamburger, what needs no GPU: the training-mode restatement against the reference's fixture,
the closed-form ham gradient against autograd, the warm-up schedule, the ABI names and the refusals."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hamburger_ref as R
import hamburger_train_ref as T

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hrnet-hand-pose-estimation_amd')
YAML = os.path.join(PKG, 'experiments', 'RHD', 'RHD_HRNet_w32_Hamburger_v2.yaml')
SMALL = ['MODEL.IMAGE_SIZE', '[64, 64]', 'MODEL.HEATMAP_SIZE', '[16, 16]', 'MODEL.EMB_DIM', '[32]', 'MODEL.R', '16']
NAMES = ['hrnet_burger_mix', 'hrnet_burger_mix_scratch', 'hrnet_burger_mix_bwd', 'hrnet_dropout2d']


def _cfg(opts=()):
    from config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(list(opts))
    return cfg


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'hamburger_train.npz'))


def fixture_inputs(golden, tag):
    case = R.CASES[tag]
    bases = [golden['{}/bases{}'.format(tag, i)] for i in range(len(R.ham_list(case)))]
    return case, bases, golden[tag + '/keep'], golden[tag + '/targets']


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_restatement_against_the_fixture(golden, tag):
    """float64, 1e-10: the loss, sum and sum of squares of every gradient, the stored gradients in full, channels 0-7 of the
    feature gradient and the running statistics after the step, against the reference's own training step"""
    case, bases, keep, targets = fixture_inputs(golden, tag)
    assert int(golden['seed']) == T.SEED
    assert np.array_equal(keep, T.draw_keep(case)) and np.array_equal(targets, T.draw_targets(case))
    assert set(np.unique(keep)) <= {np.float32(0), np.float32(1 / 0.9)} and (keep == 0).any()
    r = T.run_train(case, torch.float64, bases, keep, targets)
    names = [str(n) for n in golden[tag + '/names']]
    assert names == ['features'] + T.param_keys(case)
    assert abs(r['loss'] - float(golden[tag + '/loss'])) <= 1e-10 * abs(float(golden[tag + '/loss']))
    sums = golden[tag + '/sums']
    scale = max(np.sqrt(s[1]) for n, s in zip(names, sums) if n != 'fc.1.bias')
    full = 0
    for n, (s1, s2) in zip(names, sums):
        g = r['grads'][n]
        if n == 'fc.1.bias':                   # zero by the softmax's shift invariance: rounding noise on both sides
            assert np.abs(g).max() <= 1e-10 * scale
            continue
        assert abs((g ** 2).sum() - s2) <= 1e-10 * s2, n
        assert abs(g.sum() - s1) <= 1e-10 * np.sqrt(s2 * g.size), n
        key = '{}/grad/{}'.format(tag, n)
        if key in golden.files:
            want = golden[key]
            assert R.rel(g[:, :8] if n == 'features' else g, want) <= 1e-10, n
            full += 1
        else:
            assert g.size > 4096, n
    assert full >= 10
    for prefix in T.BN_PREFIXES:
        for leaf in ('running_mean', 'running_var'):
            assert R.rel(r['running'][prefix + leaf], golden['{}/running/{}'.format(tag, prefix + leaf)]) <= 1e-10


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_num_batches_tracked_is_unchanged_in_the_fixture(golden, tag):
    """the reference's SyncBN calls F.batch_norm directly: the counters stay 0 after a training forward"""
    assert golden[tag + '/tracked'].tolist() == [0, 0, 0]


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_float32_restatement_error_keeps_the_rule_tight(golden, tag):
    names = [str(n) for n in golden[tag + '/names']] + ['loss']
    e32 = dict(zip(names, golden[tag + '/e32']))
    assert e32['loss'] <= 1e-7
    assert all(e <= 1e-4 for n, e in e32.items() if n != 'fc.1.bias'), e32


@pytest.mark.parametrize('spatial,S,D,N,Rr,steps', [(True, 1, 12, 35, 8, 6), (False, 1, 35, 12, 8, 6), (True, 2, 6, 35, 8, 6),
                                                   (False, 2, 35, 6, 8, 6), (True, 1, 12, 35, 40, 6),
                                                   (False, 1, 35, 12, 40, 6), (True, 1, 12, 35, 8, 0),
                                                   (False, 2, 35, 6, 40, 0)])
def test_closed_form_ham_gradient_against_autograd(spatial, S, D, N, Rr, steps):
    """float64, 1e-12 of max|dX|: spatial and channel hams, S = 2, R > D, steps = 0 - through the (B, C, H, W) grouping of
    NMF2D, so that the per-image views of a channel ham with S > 1 are covered"""
    rng = np.random.RandomState(3)
    B, H, W = 2, 5, 7
    C = S * (D if spatial else N)
    assert (D if spatial else N) * S == C and (N if spatial else D) == H * W
    x = torch.tensor(np.abs(rng.normal(size=(B, C, H, W))), requires_grad=True)
    bases = R.normalise(torch.tensor(rng.uniform(size=(B * S, D, Rr))))
    dY = torch.tensor(rng.normal(size=(B, C, H, W)))
    y = T.nmf2d_train(x, bases, steps, spatial, S)
    want, = torch.autograd.grad(y, x, dY)
    got = T.ungroup(T.ham_grad(T.group(x.detach(), spatial, S), bases, steps, T.group(dY, spatial, S)), x.shape, spatial)
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-12
    # the steps carry no gradient: differentiating through them gives something else
    if steps:
        X = T.group(x, spatial, S)
        through, = torch.autograd.grad(T.ungroup(R.factorise(X, bases, steps), x.shape, spatial), x, dY)
        assert float((through - want).abs().max() / want.abs().max()) > 1e-6


def _tool(name):
    sys.path.insert(0, os.path.join(PKG, 'tools'))
    try:
        spec = importlib.util.spec_from_file_location('ham_' + name, os.path.join(PKG, 'tools', name + '.py'))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
    finally:
        sys.path.remove(os.path.join(PKG, 'tools'))
    return tool


def test_warmup_factor_by_hand():
    f = _tool('train_hamburger').warmup_factor
    assert f(0, 10, 5) == 0.0 and f(1, 10, 5) == 0.1 and f(5, 10, 5) == 0.5 and f(10, 10, 5) == 1.0
    assert f(3, 2, 10) == 7.0 / 8.0 and f(9, 2, 10) == 1.0 / 8.0
    assert f(10, 2, 10) == 0.5 / 8.0 and f(12, 2, 10) == 0.5 / 8.0          # the floor of 0.5 is on the numerator
    assert f(0, 0, 4) == 0.0 and f(1, 0, 4) == 3.0 / 4.0                    # max(1, warmup)
    assert f(11, 10, 10) == 0.5                                             # max(1, total - warmup)


def test_tool_and_yaml():
    tool = _tool('train_hamburger')
    cfg = _cfg()
    tool.check_config(cfg)
    Tr = cfg.TRAIN
    assert Tr.OPTIMIZER == 'sgd' and Tr.LR == 0.009 and Tr.LR_SCHEDULE == 'warmup' and Tr.WARMUP_EPOCHS == 10
    assert Tr.MOMENTUM == 0.9 and Tr.NESTEROV is False and Tr.WD == 0.0001 and Tr.END_EPOCH == 5
    assert abs(tool.lr_at(cfg, 0) - 0.0009) < 1e-12 and abs(tool.lr_at(cfg, 4) - 0.0045) < 1e-12
    multi = _cfg(['TRAIN.LR_SCHEDULE', 'multi_step', 'TRAIN.LR_STEP', '[1, 3]', 'TRAIN.LR_FACTOR', '0.1'])
    assert [round(tool.lr_at(multi, e) / 0.009, 6) for e in range(4)] == [1.0, 0.1, 0.1, 0.01]
    with pytest.raises(ValueError, match='LR_SCHEDULE'):
        tool.check_config(_cfg(['TRAIN.LR_SCHEDULE', 'cosine']))
    with pytest.raises(ValueError, match='trains pose_hrnet_hamburger'):
        tool.check_config(_cfg(['MODEL.NAME', 'pose_hrnet_softmax']))
    with pytest.raises(ValueError, match='is not built'):
        _tool('train').check_config(cfg)                                     # tools/train.py still refuses the model


def test_abi_names_are_declared_exported_and_refuse_by_argument_check():
    from hipnet import _capi as C
    lib = C.lib()
    for name in NAMES:
        assert name in C.EXPORTED and hasattr(lib, name), name
    assert "'burger_train.hip'" in open(os.path.join(PKG, 'build.py')).read()
    scratch = lambda *a: C.call('hrnet_burger_mix_scratch', *a)
    assert scratch(1, 16) == 2 and scratch(4099, 48) > 2 and scratch(4 * 4096, 512) == 1024
    assert scratch(0, 16) == 0 and scratch(8, 24) == 0 and scratch(8, 0) == 0 and scratch(1 << 40, 16) == 0
    p = 4096                                                           # never dereferenced: every call below is refused
    mix = lambda **k: C.call('hrnet_burger_mix', k.get('u', p), k.get('s', 2 * p), 3 * p, 4 * p, k.get('out', 5 * p),
                             k.get('rows', 8), k.get('C', 16), None)
    for kw, match in ((dict(C=24), 'C = 24'), (dict(rows=0), 'rows = 0'), (dict(u=None), 'null pointer'),
                      (dict(out=2 * p), 'aliases s')):
        with pytest.raises(RuntimeError, match=match):
            mix(**kw)
    bwd = lambda **k: C.call('hrnet_burger_mix_bwd', p, 2 * p, 3 * p, 4 * p, 5 * p, 6 * p, k.get('du', 7 * p),
                             k.get('ds', 8 * p), k.get('dcoef', 9 * p), k.get('scratch', 10 * p), k.get('n', 2),
                             k.get('rows', 8), k.get('C', 16), None)
    for kw, match in ((dict(C=24), 'C = 24'), (dict(n=1), 'scratch of 1 doubles'), (dict(scratch=None), 'scratch'),
                      (dict(du=None, ds=None, dcoef=None), 'nothing to compute'), (dict(du=2 * p), 'du aliases'),
                      (dict(ds=p), 'ds aliases'), (dict(rows=-1), 'rows = -1')):
        with pytest.raises(RuntimeError, match=match):
            bwd(**kw)
    drop = lambda **k: C.call('hrnet_dropout2d', p, k.get('keep', 2 * p), k.get('y', 3 * p), k.get('B', 2), k.get('P', 35),
                              k.get('C', 48), None)
    for kw, match in ((dict(C=24), 'C = 24'), (dict(B=0), 'B = 0'), (dict(P=0), 'P = 0'), (dict(keep=None), 'null pointer'),
                      (dict(y=2 * p), 'aliases keep')):
        with pytest.raises(RuntimeError, match=match):
            drop(**kw)


def test_refusals_without_a_device(monkeypatch):
    from hipnet import burger_train as BT
    from hipnet import nhwc
    from hipnet import nmf_train as NT
    from models import pose_hrnet_hamburger as M
    plain = M.get_pose_net(_cfg(SMALL), is_train=False)
    assert plain.trainable is False and M.HamNet.autograd_grads is True
    with pytest.raises(NotImplementedError, match='training of pose_hrnet_hamburger is not built'):
        plain.train()(torch.zeros(1, 3, 64, 64))
    model = M.get_pose_net(_cfg(SMALL), is_train=False, trainable=True).train()
    assert model.trainable and model.train_steps == 6
    assert not any(p.requires_grad for p in model.backbone.parameters())
    with pytest.raises(ValueError, match='HIP-device'):
        model(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match='HIP-device'):
        model.head_forward(torch.zeros(1, 480, 16, 16))
    model.eval()
    with pytest.raises(NotImplementedError, match='eval mode with a gradient required'):
        model(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match='TRAIN_STEPS'):
        M.get_pose_net(_cfg(SMALL + ['MODEL.TRAIN_STEPS', '-1']), is_train=False, trainable=True)
    M.get_pose_net(_cfg(SMALL + ['MODEL.TRAIN_STEPS', '-1']), is_train=False)           # read by a trainable model only
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='WORLD_SIZE'):
        M.get_pose_net(_cfg(SMALL), is_train=False, trainable=True)
    M.get_pose_net(_cfg(SMALL), is_train=False)
    keep = M.HamNet.draw_drop_keep(plain, 3, 'cpu')
    assert tuple(keep.shape) == (3, 256) and bool(((keep == 0) | ((keep - 1 / 0.9).abs() < 1e-6)).all())
    assert 0 < int((keep == 0).sum()) < 3 * 256 // 4
    x, c = torch.zeros(2, 5, 7, 48), torch.ones(1)
    conv, bn = torch.nn.Conv2d(48, 16, 1, bias=False), torch.nn.BatchNorm2d(16)
    for call in (lambda: BT.burger_mix(x, x, c, c), lambda: BT.dropout2d(x, torch.ones(2, 48)),
                 lambda: BT.conv_bn_relu_train(x, conv, bn, 1), lambda: nhwc.conv1x1_train(x, conv),
                 lambda: nhwc.to_nhwc(torch.zeros(2, 3, 5, 7), 16),
                 lambda: NT.hams_train(x, [(True, 0, 48, 1)], [torch.zeros(2, 48, 8)], 6)):
        with pytest.raises(ValueError, match='HIP-device'):
            call()


def test_bench_counts_only_train():
    r = subprocess.run([sys.executable, os.path.join('tools', 'bench_hamburger.py'), '--counts-only', '--train'], cwd=PKG,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(l) for l in r.stdout.strip().splitlines()]
    assert [row['B'] for row in rows] == [1, 4] and all(row['train'] and 'times' not in row for row in rows)
    st = rows[0]['counts']['stages']
    assert list(st) == ['layout', 'squeeze', 'lower_bread', 'ham_spatial', 'ham_channel', 'cheese', 'upper_bread', 'mix',
                        'align', 'dropout', 'fc']
    # by hand for the v2 yaml at B = 1. mix: one launch forward, the pass and its reduce backward, no products
    assert st['mix']['launches'] == 3 and st['mix']['flops'] == 0 and st['dropout']['launches'] == 2
    assert st['mix']['activation_bytes'] == 4 * 4096 * 512 * 9
    # squeeze: pack + 9 taps, BatchNorm 4 + 3, weight gradient 2; forward and weight-gradient products, no input gradient
    assert st['squeeze']['launches'] == 10 + 7 + 2 and st['squeeze']['flops'] == 2 * (2 * 4096 * 480 * 512 * 9)
    # align: the same with the nine-tap input gradient and its pack; three products
    assert st['align']['launches'] == 10 + 7 + 2 + 10 and st['align']['flops'] == 3 * (2 * 4096 * 512 * 256 * 9)
    # a ham's backward adds one update and one reconstruction to the 42 launches of its forward
    assert st['ham_spatial']['launches'] == st['ham_channel']['launches'] == 42 + 2
    D, N, Rr = 512, 4096, 512
    fwd = 2 * N * D * Rr + 6 * (2 * N * Rr * (D + Rr) + 2 * D * Rr * (N + Rr) + 2 * D * Rr * Rr + 2 * N * Rr * Rr) \
        + 2 * N * Rr * (D + Rr) + 2 * D * Rr * Rr + 2 * D * N * Rr
    assert st['ham_spatial']['flops'] == fwd + 2 * N * Rr * (D + Rr) + 2 * D * N * Rr
    assert 6.3e9 < st['ham_spatial']['flops'] - fwd < 6.6e9                 # "about 6 GFLOP of products"
    tot = rows[0]['counts']['total']
    assert tot['launches'] == sum(s['launches'] for s in st.values())
    assert rows[1]['counts']['total']['flops'] == 4 * tot['flops']
