"""The transformer kernels of csrc/transformer.hip (hipnet.transformer) at edge shapes, forward and backward, every
gradient output checked against the float64 restatement of tests/poseformer_ref.py on the CPU.

err = max|dev - ref64| / max|ref64| must stay within 4 * e_ref + 2 * 2^-24, e_ref being the same measure of the
restatement run in float32 on the CPU on the same inputs (the convention of tests/test_v2v_gpu.py). Each test prints
err, e_ref and the bound of every output.

Achieved on an MI355X: the worst err against its bound over the cases of each test is in the test's docstring.
"""
import numpy as np
import pytest
import torch

import poseformer_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _t(a, dtype, grad=True, dev='cpu'):
    return None if a is None else torch.tensor(a, dtype=dtype, device=dev).requires_grad_(grad)


def _run(fn, arrays, g, dtype, dev, nograd=()):
    """fn(*tensors) -> y; returns [y, d/d(array) of sum(y * g) for every array that takes a gradient] as float64 numpy"""
    ts = [_t(a, dtype, grad=(i not in nograd), dev=dev) for i, a in enumerate(arrays)]
    y = fn(*ts)
    (y * torch.tensor(g, dtype=dtype, device=dev)).sum().backward()
    out = [y.detach().double().cpu().numpy()]
    for i, t in enumerate(ts):
        if t is not None and i not in nograd:
            assert t.grad is not None, 'no gradient for input {}'.format(i)
            out.append(t.grad.double().cpu().numpy())
    return out


def _compare(label, fn_dev, fn_ref, arrays, g, names, nograd=()):
    ref64 = _run(fn_ref, arrays, g, torch.float64, 'cpu', nograd)
    ref32 = _run(fn_ref, arrays, g, torch.float32, 'cpu', nograd)
    dev = _run(fn_dev, arrays, g, torch.float32, DEV, nograd)
    assert len(dev) == len(ref64) == len(names) + 1
    bad = []
    for name, d, r64, r32 in zip(['y'] + list(names), dev, ref64, ref32):
        assert d.shape == r64.shape and np.isfinite(d).all(), (label, name)
        err, e_ref = R.rel(d, r64), R.rel(r32, r64)
        print('{} {}: err {:.3g} e_ref {:.3g} bound {:.3g}'.format(label, name, err, e_ref, R.bound(e_ref)))
        if not err <= R.bound(e_ref):
            bad.append((name, err, e_ref, R.bound(e_ref)))
    assert not bad, (label, bad)


LN_CASES = [(1, 32, 1e-6, False), (756, 32, 1e-6, True), (5, 672, 1e-5, False), (37, 672, 1e-6, False),
            (37, 672, 1e-5, False)]


@pytest.mark.parametrize('rows,C,eps,const_row', LN_CASES)
def test_layer_norm(rows, C, eps, const_row):
    """forward, dx, dgamma, dbeta; (756, 32) holds a row of constants (variance 0, rstd = 1 / sqrt(eps)).
    MI355X: worst against its bound: dgamma of (37, 672, 1e-6), err 1.9e-07, e_ref 1.3e-07, bound 6.6e-07."""
    from hipnet import transformer as T
    rng = np.random.default_rng((1, rows, C))
    x = rng.normal(0.3, 2.0, (rows, C))
    if const_row:
        x[min(3, rows - 1)] = 0.5
    w, b, g = rng.uniform(0.5, 1.5, C), rng.normal(0, 0.2, C), rng.normal(0, 1, (rows, C))
    _compare('layer_norm({}, {}, eps {})'.format(rows, C, eps), lambda x, w, b: T.layer_norm(x, w, b, eps),
             lambda x, w, b: R.layer_norm(x, w, b, eps), [x, w, b], g, ['dx', 'dgamma', 'dbeta'])


#              rows  Cin   Cout  act     res    scale  bias
LIN_CASES = [(756, 2, 32, None, False, False, True),
             (756, 32, 96, None, False, False, True),
             (757, 32, 64, 'gelu', False, False, True),
             (756, 64, 32, None, True, True, True),
             (36, 672, 2016, None, False, False, True),
             (37, 672, 1344, 'gelu', False, False, True),
             (36, 1344, 672, None, True, True, True),
             (4, 672, 42, None, False, False, True),
             (1, 672, 42, None, False, False, True),
             (37, 672, 96, None, False, False, False)]


@pytest.mark.parametrize('rows,Cin,Cout,act,res,scale,bias', LIN_CASES)
def test_linear(rows, Cin, Cout, act, res, scale, bias):
    """forward, dx, dW, db and the residual's pass-through gradient; the row scale holds 0 rows (a dropped branch) and
    1 / (1 - r) rows. MI355X: worst against its bound: dW of (756, 64, 32),
    err 9.2e-07, e_ref 2.7e-07, bound 1.2e-06."""
    from hipnet import transformer as T
    rng = np.random.default_rng((2, rows, Cin, Cout))
    x = rng.normal(0, 1, (rows, Cin))
    w = rng.normal(0, 1 / np.sqrt(Cin), (Cout, Cin))
    b = rng.normal(0, 0.1, Cout) if bias else None
    r = rng.normal(0, 1, (rows, Cout)) if res else None
    s = None
    if scale:
        s = np.where(rng.uniform(size=rows) < 0.3, 0.0, 1.0 / 0.8)
        s[0], s[-1] = 0.0, 1.0 / 0.8
    g = rng.normal(0, 1, (rows, Cout))
    names = ['dx', 'dW'] + (['db'] if bias else []) + (['dres'] if res else [])
    _compare('linear({}, {}, {}, {})'.format(rows, Cin, Cout, act),
             lambda x, w, b, r, s: T.linear(x, w, b, act=act, residual=r, row_scale=s),
             lambda x, w, b, r, s: R.linear(x, w, b, act=act, residual=r, row_scale=s), [x, w, b, r, s], g, names,
             nograd=(4,))


ATT_CASES = [(36, 21, 8, 4, 1.0), (4, 9, 8, 84, 1.0), (3, 5, 8, 84, 1.0), (1, 1, 8, 84, 1.0), (2, 64, 8, 4, 1.0),
             (2, 21, 8, 4, 30.0)]


@pytest.mark.parametrize('S,N,heads,hd,big', ATT_CASES)
def test_attention(S, N, heads, hd, big):
    """forward and dqkv; N = 1 is a softmax of one element (out = v); `big` scales q so that the scores reach +-30 and
    the max subtraction matters. MI355X: worst against its bound: dqkv of (4, 9, 8, 84), err 3.0e-07, e_ref 2.4e-07,
    bound 1.1e-06."""
    from hipnet import transformer as T
    rng = np.random.default_rng((3, S, N, hd, int(big)))
    qkv = rng.normal(0, 1, (S, N, 3, heads, hd))
    scale = hd ** -0.5
    if big > 1:
        # unit keys, q along a key's direction: the score of that pair is +-big
        qkv[:, :, 1] /= np.linalg.norm(qkv[:, :, 1], axis=-1, keepdims=True)
        sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)[None, :, None, None]
        qkv[:, :, 0] = qkv[:, :, 1] * sign * big / scale
    qkv = qkv.reshape(S, N, 3 * heads * hd)
    g = rng.normal(0, 1, (S, N, heads * hd))
    _compare('attention({}, {}, {}, {})'.format(S, N, heads, hd), lambda q: T.attention(q, heads, scale),
             lambda q: R.attention(q, heads, scale), [qkv], g, ['dqkv'])
    if big > 1:
        s = np.einsum('snhd,smhd->shnm', qkv.reshape(S, N, 3, heads, hd)[:, :, 0], qkv.reshape(S, N, 3, heads, hd)[:, :, 1])
        assert np.abs(s * scale).max() >= 29.9


@pytest.mark.parametrize('N,hd', [(65, 4), (9, 129)])
def test_attention_refuses_what_it_has_no_kernel_for(N, hd):
    from hipnet import _capi as C
    from hipnet import transformer as T
    calls = []
    real = C.call
    C.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        with pytest.raises(ValueError, match='no kernel'):
            T.attention(torch.zeros(1, N, 3 * 2 * hd, device=DEV), 2, 1.0)
    finally:
        C.call = real
    assert calls == ['hrnet_tf_supported']           # nothing was launched


@pytest.mark.parametrize('S', [1, 4])
@pytest.mark.parametrize('F', [1, 5, 9])
def test_frame_mean(S, F):
    """forward, dx, dw, db at D = 672, with the Conv1d's own (1, F, 1) weight shape.
    MI355X: worst against its bound: db of (1, 9), err 3.2e-07, e_ref 1.2e-07, bound 6.1e-07."""
    from hipnet import transformer as T
    rng = np.random.default_rng((4, S, F))
    x, w, b, g = rng.normal(0, 1, (S, F, 672)), rng.normal(0, 0.5, (1, F, 1)), rng.normal(0, 0.1, 1), \
        rng.normal(0, 1, (S, 672))
    _compare('frame_mean({}, {})'.format(S, F), T.frame_mean, R.frame_mean, [x, w, b], g, ['dx', 'dw', 'db'])


def test_add_rows_and_refusals():
    """the position-embedding add (forward, dx, dpos) and the CPU-tensor refusals of every op"""
    from hipnet import transformer as T
    rng = np.random.default_rng(5)
    x, pos, g = rng.normal(0, 1, (36, 672)), rng.normal(0, 0.5, (9, 672)), rng.normal(0, 1, (36, 672))
    _compare('add_rows', T.add_rows, lambda x, p: (x.reshape(4, 9, 672) + p).reshape(36, 672), [x, pos], g,
             ['dx', 'dpos'])
    c = torch.zeros(4, 32)
    for call in (lambda: T.layer_norm(c, c[0], c[0], 1e-6), lambda: T.linear(c, torch.zeros(8, 32)),
                 lambda: T.attention(torch.zeros(1, 4, 96), 8, 1.0), lambda: T.frame_mean(torch.zeros(2, 4, 8), c[0, :4]),
                 lambda: T.add_rows(c, c[:2])):
        with pytest.raises(ValueError, match='HIP-device'):
            call()


def test_backward_computes_only_what_is_asked():
    """needs_input_grad: a linear layer whose input needs no gradient launches no dx kernel work (dx stays None), and
    without any gradient required the autograd Function is bypassed"""
    from hipnet import transformer as T
    x = torch.randn(5, 32, device=DEV)
    w = torch.randn(8, 32, device=DEV, requires_grad=True)
    y = T.linear(x, w)
    assert y.grad_fn is not None
    y.sum().backward()
    assert w.grad is not None and x.grad is None
    assert T.linear(x, w.detach()).grad_fn is None
    with torch.no_grad():
        assert T.linear(x, w).grad_fn is None
