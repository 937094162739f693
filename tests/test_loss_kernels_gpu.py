"""The small kernels of csrc/loss.hip over the shapes at which they can go wrong: more than one pass of every
grid-stride and block-stride loop, sizes next to 64, 256 and the grid caps, non-square maps, NaN / inf / ties in the
arg-max, temperatures and logits that overflow exp, upstream gradients other than 1, frozen parameters behind `n`.

Each kernel is called through the C ABI and compared with the float64 reference of tests/loss_refs.py under the bounds
stated there (max(2 * dev32, floor), never looser than tests/test_kernels_gpu.py); tests/test_loss_refs_cpu.py pins those
references and the planted elements of every reduction input on the CPU. Integer results compare exactly. Every output
lies inside a larger buffer of sentinels, at least 64 elements on each side, which must come back bit-unchanged; every
reduction runs twice and must give the same bits (the file header of loss.hip promises a fixed order). Every case
prints its measured error next to its bound. Each test runs in a spawned child (tests/spawned.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import loss_refs as R
from spawned import spawned

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PAD = 64
SENTINEL = 0x7FC5C3E1                 # the int32 bits of a quiet NaN with a payload no kernel produces


def _C():
    from hipnet import _capi as C
    return C


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded(object):
    """n float32 inside PAD sentinels on each side; `init` fills the payload (an in/out argument)"""

    def __init__(self, n, init=None):
        self.n = int(n)
        self.raw = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.t = self.raw.view(torch.float32)[PAD:PAD + self.n]
        if init is not None:
            self.t.copy_(torch.as_tensor(init, dtype=torch.float32).reshape(-1))

    def ptr(self):
        return self.t.data_ptr()

    def get(self, what):
        """the payload as numpy, after checking that it was written completely (no sentinel left) and the guards not"""
        torch.cuda.synchronize()
        raw = self.raw.cpu().numpy()
        assert (raw[:PAD] == SENTINEL).all() and (raw[PAD + self.n:] == SENTINEL).all(), what + ': write outside the output'
        assert not (raw[PAD:PAD + self.n] == SENTINEL).any(), what + ': an output element was not written'
        return raw[PAD:PAD + self.n].view(np.float32).copy()


def _twice(what, run):
    """run() -> tuple of numpy arrays, on fresh outputs each time: bit-identical both times"""
    a, b = run(), run()
    for x, y in zip(a, b):
        assert R.same_bits(x, y), what + ': two runs differ'
    return a


# ---- heat-map loss ----------------------------------------------------------------------------------------------------

@spawned
def test_heatmap_loss_forward_over_map_shapes_and_batch_sizes():
    C = _C()
    for h, w in R.PER_MAP_SHAPES:
        for bk in R.PER_MAP_BK + ((255, 256, 336) if (h, w) in ((8, 8), (5, 13)) else ()):       # mean_kernel strides
            pred, gt, _ = R.heatmap_case(bk, h * w)
            pd, gd = _dev(pred), _dev(gt)
            for mode in (0, 1):
                name = 'heatmap_fwd {}x{} BK {} mode {}'.format(h, w, bk, mode)

                def run():
                    part, loss = Guarded(bk), Guarded(1)
                    C.call('hrnet_heatmap_loss_fwd', pd.data_ptr(), gd.data_ptr(), part.ptr(), loss.ptr(), bk, h * w, mode,
                           C.stream_ptr())
                    return part.get(name), loss.get(name)
                part, loss = _twice(name, run)
                e = R.heatmap_expected(pred, gt, mode)
                R.check_sums(name + ' per map', part, *e['partial'])
                R.check_sums(name + ' loss', loss, *e['loss'])


@spawned
def test_heatmap_loss_backward_past_the_grid_cap_and_through_the_module():
    C = _C()
    from core.loss import HeatmapLoss
    for bk, hw in ((1, 1048577), (336, 4096)):           # one element into the second grid-stride pass; a training batch
        pred, gt, zeros = R.heatmap_case(bk, hw, seed=1)
        pd, gd = _dev(pred), _dev(gt)
        p64, g64 = torch.from_numpy(pred).double(), torch.from_numpy(gt).double()
        p32, g32 = torch.from_numpy(pred), torch.from_numpy(gt)
        for mode in (0, 1):
            unit64, unit32 = R.heatmap_loss_grad(p64, g64, mode, 1.0), R.heatmap_loss_grad(p32, g32, mode, 1.0)
            for gout in (1.0, 0.37, -3.0):
                name = 'heatmap_bwd {}x{} mode {} gout {}'.format(bk, hw, mode, gout)
                out, go = Guarded(bk * hw), _dev(np.array([gout], np.float32))
                C.call('hrnet_heatmap_loss_bwd', pd.data_ptr(), gd.data_ptr(), go.data_ptr(), out.ptr(), bk, hw, mode,
                       C.stream_ptr())
                got = out.get(name).reshape(bk, hw)
                # the gradient is linear in gout: the float32 autograd run is scaled in float32, as autograd would
                ref32 = unit32 * torch.tensor(R.f32(gout))
                R.check(name, got, unit64 * R.f32(gout), ref32, cap=1e-6 * float(unit64.abs().max()) * abs(gout))
                assert not got[:, zeros].any(), name + ': pred == gt must give gradient 0'
                assert got[bk - 1, hw - 1] != 0 and got[0, 0] != 0
    # core.loss.HeatmapLoss: a 3-D input, a non-contiguous input, an upstream gradient of 0.37
    for mode, mname in ((0, 'l2'), (1, 'l1')):
        pred, gt, zeros = R.heatmap_case(6, 13 * 10, seed=2)
        wide = torch.from_numpy(np.concatenate([pred.reshape(6, 13, 10), gt.reshape(6, 13, 10)], 2))     # [6, 13, 20]
        for shape in ((6, 13, 10), (2, 3, 13, 10)):
            view = wide.to(DEV)[:, :, :10]               # [6, 13, 10], not contiguous, and neither is its 4-D reshape
            p = (view if len(shape) == 3 else view.reshape(shape)).detach().requires_grad_(True)
            assert not p.is_contiguous()
            loss = HeatmapLoss(mname)(p, _dev(gt).reshape(shape))
            (loss * 0.37).backward()
            e = R.heatmap_expected(pred, gt, mode)
            name = 'HeatmapLoss {} {}'.format(mname, shape)
            R.check_sums(name + ' loss', loss.detach().cpu().numpy(), *e['loss'])
            p64, g64 = torch.from_numpy(pred).double(), torch.from_numpy(gt).double()
            ref32 = R.heatmap_loss_grad(torch.from_numpy(pred), torch.from_numpy(gt), mode, R.f32(0.37))
            ref64 = R.heatmap_loss_grad(p64, g64, mode, R.f32(0.37))
            got = p.grad.cpu().numpy().reshape(6, -1)
            R.check(name + ' grad', got, ref64, ref32, cap=1e-6 * float(ref64.abs().max()))
            assert not got[:, zeros].any()


# ---- key-point loss ---------------------------------------------------------------------------------------------------

@spawned
def test_joints_loss_forward_and_backward_over_point_counts_and_weights():
    C = _C()
    for b, k in R.JOINTS_SHAPES:
        for vis_mode in R.JOINTS_VIS:
            pred, gt, vis, zeros = R.joints_case(b, k, vis_mode)
            pd, gd, vd = _dev(pred), _dev(gt), (None if vis is None else _dev(vis))
            name = 'joints {}x{} vis {}'.format(b, k, vis_mode)

            def run():
                loss = Guarded(1)
                C.call('hrnet_joints_loss_fwd', pd.data_ptr(), gd.data_ptr(), C.ptr(vd), loss.ptr(), b, k, C.stream_ptr())
                return (loss.get(name),)
            loss, = _twice(name, run)
            e = R.joints_expected(pred, gt, vis)
            R.check_sums(name + ' loss', loss, *e['loss'])
            if vis_mode == 'zero':
                assert loss[0] == 0.0
            a64 = [None if a is None else torch.from_numpy(a).double() for a in (pred, gt, vis)]
            a32 = [None if a is None else torch.from_numpy(a) for a in (pred, gt, vis)]
            for gout in (1.0, 0.75, -2.0):
                ref64, ref32 = R.joints_loss_grad(*a64, gout), R.joints_loss_grad(*a32, gout)

                def run_bwd():
                    out, go = Guarded(b * k * 2), _dev(np.array([gout], np.float32))
                    C.call('hrnet_joints_loss_bwd', pd.data_ptr(), gd.data_ptr(), C.ptr(vd), go.data_ptr(), out.ptr(), b, k,
                           C.stream_ptr())
                    return (out.get(name),)
                got, = _twice(name + ' bwd', run_bwd)           # (its sum of the weights is a reduction too)
                got = got.reshape(b, k, 2)
                R.check('{} bwd gout {}'.format(name, gout), got, ref64, ref32, cap=1e-6)
                assert not got.reshape(-1, 2)[zeros].any(), name + ': pred == gt must give gradient 0'
                if vis_mode == 'zero':
                    assert not got.any()


# ---- arg-max decode ---------------------------------------------------------------------------------------------------

@spawned
def test_decode_argmax_nan_inf_ties_and_both_styles():
    C = _C()
    for h, w in R.PER_MAP_SHAPES:
        hm_all, names = R.argmax_case(257, h, w)
        for bk in R.PER_MAP_BK:
            hm = hm_all[257 - bk:] if bk == 3 else hm_all[:bk]       # (BK = 3: three of the later scenarios)
            hd = _dev(hm)
            for style in (0, 1):
                want_p, want_m = R.decode_argmax(hm, style)
                for with_max in (True, False):
                    name = 'argmax {}x{} BK {} style {} maxvals {}'.format(h, w, bk, style, with_max)

                    def run():
                        preds, mx = Guarded(bk * 2), Guarded(bk)
                        C.call('hrnet_decode_argmax', hd.data_ptr(), preds.ptr(), mx.ptr() if with_max else None, bk, h, w,
                               style, C.stream_ptr())
                        torch.cuda.synchronize()
                        if not with_max:           # nothing may be written there
                            assert (mx.raw.cpu().numpy() == SENTINEL).all(), name
                        return (preds.get(name), mx.get(name) if with_max else np.zeros(0, np.float32))
                    preds, mx = _twice(name, run)
                    bad = np.flatnonzero((preds.reshape(bk, 2) != want_p).any(1))
                    assert bad.size == 0, (name, [(int(i), names[(257 - bk + i) if bk == 3 else i]) for i in bad[:5]],
                                           preds.reshape(bk, 2)[bad[:5]], want_p[bad[:5]])
                    if with_max:
                        assert R.same_bits(mx, want_m), name
        print('argmax {}x{}: 257 + 3 + 1 maps, both styles, exact'.format(h, w))


# ---- spatial softmax --------------------------------------------------------------------------------------------------

@spawned
def test_spatial_softmax_forward_backward_over_temperatures_and_extreme_logits():
    C = _C()
    for si, (h, w) in enumerate(R.PER_MAP_SHAPES):
        hw = h * w
        for bk in R.PER_MAP_BK:
            for temp in R.SOFTMAX_TEMPS:
                x, g, kinds = R.softmax_case(bk, hw, temp, si)
                xd, gd, td = _dev(x), _dev(g), _dev(np.array([temp], np.float32))
                name = 'softmax {}x{} BK {} t {}'.format(h, w, bk, temp)

                def run():
                    out, dx, dt = Guarded(bk * hw), Guarded(bk * hw), Guarded(bk)
                    C.call('hrnet_spatial_softmax_fwd', xd.data_ptr(), td.data_ptr(), out.ptr(), bk, hw, C.stream_ptr())
                    C.call('hrnet_spatial_softmax_bwd', xd.data_ptr(), out.ptr(), gd.data_ptr(), td.data_ptr(), dx.ptr(),
                           dt.ptr(), bk, hw, C.stream_ptr())
                    return out.get(name), dx.get(name), dt.get(name)
                out, dx, dt = _twice(name, run)
                e = R.softmax_expected(x, g, temp)
                out = out.reshape(bk, hw)
                R.check(name + ' out', out, *e['out'])
                R.check_sums(name + ' row sums', out.astype(np.float64).sum(1), *e['rowsum'])
                R.check(name + ' dx', dx.reshape(bk, hw), *e['dx'])
                allowed, dev32 = R.elementwise_allowed(*e['dx_plain'])
                print('{:58s} abs err {:.3e} against max|dx| * max(2 dev32, 4u) = {:.3e} (dev32 {:.2e}; not asserted, see '
                      'loss_refs.softmax_expected)'.format(name + ' dx', float(np.abs(dx.reshape(bk, hw) - e['dx'][0].numpy()).max()),
                                                           allowed, dev32))
                R.check_sums(name + ' dtemp per map', dt, *e['dtemp'])
                eq = kinds == R.ROW_EQUAL
                if eq.any():                     # all-equal rows: every output the same
                    assert (out[eq] == out[eq][:, :1]).all(), name


# ---- expectation decode -----------------------------------------------------------------------------------------------

@spawned
def test_decode_expectation_forward_and_backward_with_accumulate():
    C = _C()
    for h, w in R.PER_MAP_SHAPES:
        for bk in R.PER_MAP_BK:
            hm = R.expectation_case(bk, h, w)
            hd = _dev(hm)
            name = 'expectation {}x{} BK {}'.format(h, w, bk)

            def run():
                preds = Guarded(bk * 2)
                C.call('hrnet_decode_expectation', hd.data_ptr(), preds.ptr(), bk, h, w, C.stream_ptr())
                return (preds.get(name),)
            preds, = _twice(name, run)
            R.check_sums(name, preds, *R.expectation_expected(hm)['preds'])
            # backward: gradients that tell x from y (and so H from W), accumulate 0 and 1
            rng = np.random.default_rng([9, bk, h, w])
            gp = rng.standard_normal((bk, 2)).astype(np.float32)
            gp[:, 1] *= 3.0
            prev = rng.standard_normal((bk, h, w)).astype(np.float32)
            g64 = R.decode_expectation_grad(torch.from_numpy(gp).double(), h, w)
            g32 = R.decode_expectation_grad(torch.from_numpy(gp), h, w)
            gpd = _dev(gp)
            for acc in (0, 1):
                out = Guarded(bk * h * w, init=prev)
                C.call('hrnet_decode_expectation_bwd', gpd.data_ptr(), out.ptr(), bk, h, w, acc, C.stream_ptr())
                got = out.get(name).reshape(bk, h, w)
                ref64 = g64 + torch.from_numpy(prev).double() if acc else g64
                ref32 = g32 + torch.from_numpy(prev) if acc else g32
                R.check('{} bwd accumulate {}'.format(name, acc), got, ref64, ref32,
                        cap=1e-6 * float(ref64.abs().max()) if not acc else None)


# ---- Gaussian targets -------------------------------------------------------------------------------------------------

def _targets(C, pose, vis, bk, h, w, sigma, name):
    out = Guarded(bk * h * w)
    pd, vd = _dev(pose), (None if vis is None else _dev(vis))
    C.call('hrnet_gaussian_targets', pd.data_ptr(), C.ptr(vd), out.ptr(), bk, h, w, float(sigma), C.stream_ptr())
    return out.get(name).reshape(bk, h, w)


@spawned
def test_gaussian_targets_edge_coordinates_sigmas_and_visibility():
    """against hipnet.synth.gaussian_heatmaps (pinned to the reference's generator, float32 itself): 1e-7 absolute as
    the older test, and the zero pattern exactly"""
    C = _C()
    from hipnet import synth
    cases = [(h, w, bk, s) for (h, w) in ((64, 64), (48, 40), (40, 48)) for bk in (1, 257) for s in (1, 2, 3)]
    cases += [(h, w, bk, 1) for (h, w) in R.PER_MAP_SHAPES for bk in R.PER_MAP_BK]
    for h, w, bk, sigma in cases:
        worst = 0.0
        for seed in ((0, 4, 9, 11) if bk == 1 else (0,)):            # BK = 1: a corner, (-0.7, .), (w - 0.01, .), far out
            pose, vis = R.targets_case(bk, h, w, seed)
            for v in (None, vis):
                name = 'targets {}x{} BK {} sigma {} vis {}'.format(h, w, bk, sigma, 'NULL' if v is None else 'given')
                got = _targets(C, pose, v, bk, h, w, sigma, name)
                want = synth.gaussian_heatmaps(pose.reshape(1, bk, 2), None if v is None else v.reshape(1, bk, 1), h, w,
                                               sigma)[0]
                err = float(np.abs(got - want).max())
                assert np.array_equal(got == 0, want == 0), name + ': zero pattern'
                assert err <= 1e-7, (name, err)
                worst = max(worst, err)
        print('targets {}x{} BK {} sigma {}: max abs err {:.3e} bound 1.000e-07, zero pattern exact'.format(
            h, w, bk, sigma, worst))


# ---- u8 normalise -----------------------------------------------------------------------------------------------------

@spawned
def test_normalize_u8_every_byte_value_past_the_grid_cap():
    C = _C()
    for n, h, w in R.U8_CASES:
        img = R.u8_case(n, h, w)
        imd = _dev(img)
        for mean, std in R.U8_CONSTANTS:
            name = 'normalize_u8 {}x{}x{} mean {}'.format(n, h, w, mean[0])
            out = Guarded(n * 3 * h * w)
            m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
            C.call('hrnet_normalize_u8', imd.data_ptr(), out.ptr(), n, h, w, m, s, C.stream_ptr())
            got = out.get(name).reshape(n, 3, h, w)
            mean32, std32 = [R.f32(v) for v in mean], [R.f32(v) for v in std]
            t = torch.from_numpy(img)
            R.check(name, got, R.normalize_u8(t, mean32, std32, torch.float64), R.normalize_u8(t, mean32, std32, torch.float32),
                    cap=1e-6)


# ---- Adam -------------------------------------------------------------------------------------------------------------

def _adam_call(C, p, g, m, v, n, step, gscale, wd, lr, name):
    """the step over the first n elements of buffers that hold `frozen` more: those and the guards must stay"""
    bufs = [Guarded(len(a), init=a) for a in (p, m, v)]
    gd = _dev(g)
    C.call('hrnet_adam_step', bufs[0].ptr(), gd.data_ptr(), bufs[1].ptr(), bufs[2].ptr(), n, lr, 0.9, 0.999, 1e-8, wd, step,
           gscale, C.stream_ptr())
    return [b.get(name) for b in bufs]


@spawned
def test_adam_step_past_the_grid_cap_with_gradient_scale_and_frozen_tail():
    C = _C()
    big = 2097152
    late = ((0.125, 1e-4, 1e-3), (1.0 / 3.0, 0.0, 3e-4))
    configs = []
    for n in (1, 255, 257):
        for gscale in (1.0, 0.125, 1.0 / 3.0):
            for wd in (0.0, 1e-4):
                configs += [(n, step, gscale, wd, lr) for step, lr in ((1, 1e-3), (2, 3e-4))]
        configs += [(n, 1000, gs, wd, lr) for gs, wd, lr in late] + [(n, 100000,) + late[0]]
    # past the cap of 8192 blocks of 256: one element into the second pass, and five into the fourth
    configs += [(big + 1, 100000) + late[0], (big + 1, 1, 1.0 / 3.0, 0.0, 3e-4), (3 * big + 5, 2, 0.125, 1e-4, 1e-3)]
    frozen = 100
    for n, step, gscale, wd, lr in configs:
        p, g, m, v, z = R.adam_case(n, step, gscale, wd, lr)
        name = 'adam n {} step {} gscale {:.3f} wd {} lr {}'.format(n, step, gscale, wd, lr)
        tail = np.random.default_rng(n).standard_normal(frozen).astype(np.float32)
        full = [np.concatenate([a, tail * c]) for a, c in ((p, 1.0), (m, 0.5), (v, 0.25))]
        gfull = np.concatenate([g, tail])                  # a gradient behind n must not be applied
        got = _adam_call(C, full[0], gfull, full[1], full[2], n, step, gscale, wd, lr, name)
        for a, b in zip(got, full):
            assert R.same_bits(a[n:], b[n:]), name + ': the frozen tail was touched'
        e = R.adam_expected(p, g, m, v, step, gscale, wd, lr)
        for key, a in zip('pmv', got):
            R.check('{} {}'.format(name, key), a[:n], *e[key])
        if wd == 0.0 and len(z):
            assert R.same_bits(got[0][z], p[z]) and not got[1][z].any() and not got[2][z].any(), name + ': 0 / eps'
        assert got[0][n - 1] != p[n - 1] and got[0][0] != p[0]
    # hipnet.optim.FlatAdam over a stand-in for the flat buffers: three steps, gradient scale 1/8, a frozen tail
    from hipnet.optim import FlatAdam

    class Net(object):
        params = []
        dirty = 0

        def mark_weights_dirty(self):
            self.dirty += 1

    class Model(object):
        def hip(self):
            return net
    n = 2 * 256 + 3
    net = Net()
    p0 = np.random.default_rng(21).standard_normal(n + frozen).astype(np.float32)
    net.flat_p, net.flat_g, net.trainable_count = _dev(p0), torch.zeros(n + frozen, device=DEV), n
    opt = FlatAdam(Model(), lr=1e-3, weight_decay=1e-4)
    opt.grad_scale = 0.125
    p64, m64, v64 = torch.from_numpy(p0[:n]).double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p32, m32, v32 = torch.from_numpy(p0[:n]), torch.zeros(n), torch.zeros(n)
    h = R.ADAM_HYPER
    for step in range(1, 4):
        g = np.random.default_rng(30 + step).standard_normal(n + frozen).astype(np.float32)
        net.flat_g.copy_(torch.from_numpy(g))
        opt.step()
        args = (step, R.f32(1e-3), h['b1'], h['b2'], h['eps'], R.f32(1e-4), 0.125)
        p64, m64, v64 = R.adam_step(p64, torch.from_numpy(g[:n]).double(), m64, v64, *args)
        p32, m32, v32 = R.adam_step(p32, torch.from_numpy(g[:n]), m32, v32, *args)
    torch.cuda.synchronize()
    assert net.dirty == 3 and opt.step_count == 3
    # three steps: three times the error of one
    for key, ours, r64, r32 in (('p', net.flat_p, p64, p32), ('m', opt.exp_avg, m64, m32), ('v', opt.exp_avg_sq, v64, v32)):
        a = ours.cpu().numpy()
        R.check('FlatAdam 3 steps ' + key, a[:n], r64, r32, floor=3 * R.FLOOR, cap=1e-6 if key == 'p' else None)
        assert R.same_bits(a[n:], p0[n:] if key == 'p' else np.zeros(frozen, np.float32)), 'FlatAdam: frozen tail ' + key


# ---- structure losses and the 3-D key-point loss past their caps ------------------------------------------------------

def _structure(C, pred, gt, b, normalize, name):
    outs = [Guarded(1), Guarded(1), Guarded(b * 42), Guarded(b * 42)]
    pd, gd = _dev(pred[:b]), _dev(gt[:b])
    C.call('hrnet_structure_loss', pd.data_ptr(), gd.data_ptr(), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), outs[3].ptr(),
           b, 21, normalize, 3, C.stream_ptr())
    return [o.get(name) for o in outs]


@spawned
def test_structure_loss_batches_past_256_and_joints3d_backward_past_its_cap():
    C = _C()
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'structure_loss.npz'))
    for case in ('b70', 'raw'):
        normalize = int(bool(z[case + '_normalize']))
        for b in (256, 257, 300):
            rng = np.random.default_rng([13, b, normalize])
            reps = -(-b // z[case + '_pred'].shape[0])
            base = z[case + '_pred']               # perturbed by 1 % of the smallest hand (wrist to joint 9) in the fixture
            scale = 0.01 * np.sqrt(((base[:, 9] - base[:, 0]) ** 2).sum(-1)).min()
            pred = np.tile(z[case + '_pred'], (reps, 1, 1))[:b] + (rng.standard_normal((b, 21, 2)) * scale).astype(np.float32)
            gt = np.tile(z[case + '_gt'][:, :, :2], (reps, 1, 1))[:b] + (rng.standard_normal((b, 21, 2)) * scale).astype(np.float32)
            pred, gt = pred.astype(np.float32), gt.astype(np.float32)
            name = 'structure {} B {}'.format(case, b)
            full = _twice(name, lambda: _structure(C, pred, gt, b, normalize, name))
            head = _structure(C, pred, gt, 256, normalize, name)
            parts = [head] + ([_structure(C, pred[256:], gt[256:], b - 256, normalize, name)] if b > 256 else [])
            for q, i in (('dbone', 2), ('dangle', 3)):
                assert np.isfinite(full[i]).all() and full[i].any()
                assert R.same_bits(full[i], np.concatenate([p[i] for p in parts])), '{} {}: per-sample gradients'.format(name, q)
            for q, i in (('bone', 0), ('angle', 1)):
                want = sum(float(p[i][0]) for p in parts)
                err = abs(float(full[i][0]) - want) / want
                # each call rounds its float64 sum to float32 once: three roundings between the two sides
                print('{} {:5s} rel err {:.3e} bound {:.3e} (against the float64 sum of the two calls)'.format(
                    name, q, err, R.FLOOR))
                assert want > 0 and err <= R.FLOOR
    # hrnet_joints3d_loss_bwd: B * K = 262,145, one point past 1024 blocks of 256
    b, k = 52429, 5
    rng = np.random.default_rng(3)
    pred = rng.normal(0, 80, (b, k, 3)).astype(np.float32)
    gt = rng.normal(0, 80, (b, k, 3)).astype(np.float32)
    gt[0, 0] = pred[0, 0]
    p64 = torch.from_numpy(pred).double().requires_grad_(True)
    ref = torch.norm(torch.from_numpy(gt).double() - p64, dim=2).sum() / k
    (ref * 0.75).backward()
    pd, gd, go = _dev(pred), _dev(gt), _dev(np.array([0.75], np.float32))
    name = 'joints3d B*K 262145'

    def run():
        loss, out = Guarded(1), Guarded(b * k * 3)
        C.call('hrnet_joints3d_loss_fwd', pd.data_ptr(), gd.data_ptr(), loss.ptr(), b, k, C.stream_ptr())
        C.call('hrnet_joints3d_loss_bwd', pd.data_ptr(), gd.data_ptr(), go.data_ptr(), out.ptr(), b, k, C.stream_ptr())
        return loss.get(name), out.get(name)
    loss, got = _twice(name, run)
    gref = p64.grad.numpy()
    err = np.abs(got.reshape(b, k, 3) - gref).max() / np.abs(gref).max()
    lerr = abs(float(loss[0]) - ref.item()) / abs(ref.item())
    print('{} loss rel err {:.3e} bound 1.000e-06, grad rel err {:.3e} bound 1.000e-06'.format(name, lerr, err))
    assert lerr <= 1e-6 and err <= 1e-6
    assert not got[:3].any() and got.reshape(-1, 3)[-1].any()


# ---- argument checks --------------------------------------------------------------------------------------------------

@spawned
def test_bad_arguments_raise_and_write_nothing():
    C = _C()
    buf = Guarded(4096)
    untouched = buf.raw.clone()
    a, s = buf.ptr(), C.stream_ptr()
    u8 = torch.zeros(64, dtype=torch.uint8, device=DEV)
    ok3, zero_std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.5, 0.0, 0.5)
    bad = [
        ('hrnet_heatmap_loss_fwd', (None, a, a, a, 1, 4, 0, s)), ('hrnet_heatmap_loss_fwd', (a, a, None, a, 1, 4, 0, s)),
        ('hrnet_heatmap_loss_fwd', (a, a, a, None, 1, 4, 0, s)), ('hrnet_heatmap_loss_fwd', (a, a, a, a, 0, 4, 0, s)),
        ('hrnet_heatmap_loss_fwd', (a, a, a, a, 1, 0, 0, s)), ('hrnet_heatmap_loss_fwd', (a, a, a, a, 1, 4, 2, s)),
        ('hrnet_heatmap_loss_bwd', (a, None, a, a, 1, 4, 0, s)), ('hrnet_heatmap_loss_bwd', (a, a, None, a, 1, 4, 0, s)),
        ('hrnet_heatmap_loss_bwd', (a, a, a, None, 1, 4, 0, s)), ('hrnet_heatmap_loss_bwd', (a, a, a, a, 0, 4, 0, s)),
        ('hrnet_heatmap_loss_bwd', (a, a, a, a, 1, 4, 2, s)), ('hrnet_heatmap_loss_bwd', (a, a, a, a, 1, 4, -1, s)),
        ('hrnet_gaussian_targets', (None, None, a, 1, 4, 4, 2.0, s)), ('hrnet_gaussian_targets', (a, None, None, 1, 4, 4, 2.0, s)),
        ('hrnet_gaussian_targets', (a, None, a, 0, 4, 4, 2.0, s)), ('hrnet_gaussian_targets', (a, None, a, 1, 4, 4, 0.0, s)),
        ('hrnet_gaussian_targets', (a, None, a, 1, 4, 4, -1.0, s)), ('hrnet_gaussian_targets', (a, None, a, 1, 0, 4, 2.0, s)),
        ('hrnet_normalize_u8', (None, a, 1, 2, 2, ok3, ok3, s)), ('hrnet_normalize_u8', (u8.data_ptr(), None, 1, 2, 2, ok3, ok3, s)),
        ('hrnet_normalize_u8', (u8.data_ptr(), a, 1, 2, 2, None, ok3, s)), ('hrnet_normalize_u8', (u8.data_ptr(), a, 0, 2, 2, ok3, ok3, s)),
        ('hrnet_normalize_u8', (u8.data_ptr(), a, 1, 2, 2, ok3, zero_std, s)),
        ('hrnet_spatial_softmax_fwd', (a, None, a, 1, 4, s)), ('hrnet_spatial_softmax_fwd', (a, a, a, 0, 4, s)),
        ('hrnet_spatial_softmax_bwd', (a, a, a, a, a, None, 1, 4, s)), ('hrnet_spatial_softmax_bwd', (a, a, a, a, a, a, 0, 4, s)),
        ('hrnet_decode_expectation', (a, None, 1, 4, 4, s)), ('hrnet_decode_expectation', (a, a, 0, 4, 4, s)),
        ('hrnet_decode_expectation_bwd', (None, a, 1, 4, 4, 0, s)), ('hrnet_decode_expectation_bwd', (a, a, 0, 4, 4, 0, s)),
        ('hrnet_decode_expectation_bwd', (a, a, 1, 0, 4, 0, s)),
        ('hrnet_decode_argmax', (a, None, None, 1, 4, 4, 0, s)), ('hrnet_decode_argmax', (a, a, None, 0, 4, 4, 0, s)),
        ('hrnet_joints_loss_fwd', (a, None, None, a, 1, 4, s)), ('hrnet_joints_loss_fwd', (a, a, None, None, 1, 4, s)),
        ('hrnet_joints_loss_fwd', (a, a, None, a, 0, 4, s)), ('hrnet_joints_loss_bwd', (a, a, None, None, a, 1, 4, s)),
        ('hrnet_joints_loss_bwd', (a, a, None, a, a, 1, 0, s)),
        ('hrnet_joints3d_loss_fwd', (a, a, None, 1, 4, s)), ('hrnet_joints3d_loss_bwd', (a, a, a, a, 0, 4, s)),
        ('hrnet_structure_loss', (a, a, a, a, a, a, 2, 20, 1, 3, s)), ('hrnet_structure_loss', (a, a, a, a, a, a, 2, 22, 0, 3, s)),
        ('hrnet_structure_loss', (None, a, a, a, a, a, 2, 21, 1, 3, s)), ('hrnet_structure_loss', (a, a, a, a, a, a, 0, 21, 1, 3, s)),
        ('hrnet_structure_loss', (a, None, a, a, a, a, 2, 21, 1, 1, s)), ('hrnet_structure_loss', (a, a, a, a, a, a, 2, 21, 1, 0, s)),
        ('hrnet_structure_loss_bwd', (a, a, a, a, a, 2, 20, s)),
        ('hrnet_adam_step', (a, a, a, a, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, s)),
        ('hrnet_adam_step', (a, a, a, a, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, s)),
        ('hrnet_adam_step', (None, a, a, a, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, s)),
        ('hrnet_adam_step', (a, a, a, None, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, s)),
    ]
    for fn, args in bad:
        with pytest.raises(RuntimeError, match=fn):
            C.call(fn, *args)
    torch.cuda.synchronize()
    assert torch.equal(buf.raw, untouched), 'a refused call launched something'
    # the same entry points still work afterwards
    loss = Guarded(1)
    one = _dev(np.ones(8, np.float32))
    zero = _dev(np.zeros(8, np.float32))
    part = Guarded(2)
    C.call('hrnet_heatmap_loss_fwd', one.data_ptr(), zero.data_ptr(), part.ptr(), loss.ptr(), 2, 4, 1, s)
    assert loss.get('after')[0] == 4.0 and part.get('after').tolist() == [4.0, 4.0]
    print('bad arguments: {} calls refused with RuntimeError, nothing written'.format(len(bad)))
