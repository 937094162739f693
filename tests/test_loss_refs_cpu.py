"""tests/loss_refs.py on the CPU: its float64 references against what the project already trusts (the reference's own
results in tests/golden/micro.npz, decode_crosscheck.npz and inference_preds.npz, oracle.hrnet_cpu, torch.optim.Adam in
float64), and the planted-element condition of every reduction input that tests/test_loss_kernels_gpu.py feeds to a
kernel: under the reference, losing or doubling a planted element moves the result by at least 100 bounds."""
import os

import numpy as np
import pytest
import torch

import loss_refs as R
from hipnet import synth
from oracle import hrnet_cpu as O

F64 = torch.float64


def _z(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def test_heatmap_loss_reference_matches_fixture_and_oracle(golden_dir):
    z = _z(golden_dir, 'micro.npz')
    p, g = _t(z['hl_pred']), _t(z['hl_gt'])
    bk = p.shape[0] * p.shape[1]
    for mode, key, name in ((0, 'hl_l2', 'l2'), (1, 'hl_l1', 'l1')):
        part, loss = R.heatmap_loss(p.reshape(bk, -1), g.reshape(bk, -1), mode)
        assert abs(loss.item() - float(z[key])) <= 1e-6 * float(z[key])          # the fixture is a float32 run
        assert abs(loss.item() - O.heatmap_loss(p, g, name).item()) <= 1e-14 * loss.item()
        pr = p.clone().requires_grad_(True)
        (O.heatmap_loss(pr, g, name) * 0.37).backward()
        got = R.heatmap_loss_grad(p.reshape(bk, -1), g.reshape(bk, -1), mode, 0.37).reshape(p.shape)
        assert (got - pr.grad).abs().max().item() <= 1e-15
    # sign(0) = 0 under L1, and a zero L2 gradient too
    d = torch.tensor([[0.5, 0.0, -2.0]], dtype=F64)
    assert R.heatmap_loss_grad(d, torch.zeros_like(d), 1, -3.0).tolist() == [[-3.0, 0.0, 3.0]]
    assert R.heatmap_loss_grad(d, torch.zeros_like(d), 0, 1.0).tolist() == [[1.0, 0.0, -4.0]]


def test_joints_loss_reference_matches_fixture_and_oracle(golden_dir):
    z = _z(golden_dir, 'micro.npz')
    p, g, vis = _t(z['jm_pred']), _t(z['jm_gt']), _t(z['jm_vis'])
    for v, key in ((vis, 'jm_vis_loss'), (None, 'jm_novis_loss'), (torch.zeros_like(vis), 'jm_allinvis_loss')):
        loss = R.joints_loss(p, g, v)
        assert abs(loss.item() - float(z[key])) <= 1e-6 * max(float(z[key]), 1.0)
        assert abs(loss.item() - O.joints_mse_loss(p, g, v).item()) <= 1e-14 * max(loss.item(), 1.0)
        pr = p.clone().requires_grad_(True)
        (O.joints_mse_loss(pr, g, v) * -2.0).backward()
        assert (R.joints_loss_grad(p, g, v, -2.0) - pr.grad).abs().max().item() <= 1e-15
    # fractional weights below 1 in sum: the denominator is max(1, sum vis) = 1; a zero difference has no gradient
    w = torch.tensor([[0.25, 0.5]], dtype=F64)
    a, b = torch.tensor([[[3.0, 4.0], [1.0, 1.0]]], dtype=F64), torch.tensor([[[0.0, 0.0], [1.0, 1.0]]], dtype=F64)
    assert R.joints_loss(a, b, w).item() == 1.25 and R.joints_denominator(a, w) == 1.0
    assert R.joints_loss_grad(a, b, w, 1.0).tolist() == [[[0.25 * 0.6, 0.25 * 0.8], [0.0, 0.0]]]
    assert R.joints_loss(a, b, None).item() == 2.5


def test_argmax_reference_matches_fixtures_oracle_and_torch(golden_dir):
    z, inf = _z(golden_dir, 'micro.npz'), _z(golden_dir, 'inference_preds.npz')
    hm = z['am_hm']
    preds, _ = R.decode_argmax(hm.reshape(-1, *hm.shape[2:]), 0)
    assert np.array_equal(preds.reshape(z['am_pred'].shape), z['am_pred'])
    for tag in ('sq', 'rect'):
        hm = inf['hm_' + tag]
        preds, mx = R.decode_argmax(hm.reshape(-1, *hm.shape[2:]), 1)
        assert np.array_equal(preds.reshape(inf['preds_' + tag].shape), inf['preds_' + tag])
        assert np.array_equal(mx.reshape(inf['maxvals_' + tag].shape), inf['maxvals_' + tag])
    ns = np.random.default_rng(0).standard_normal((2, 3, 4, 6)).astype(np.float32)
    preds, _ = R.decode_argmax(ns.reshape(6, 4, 6), 0)
    assert np.array_equal(preds.reshape(2, 3, 2), O.get_final_preds(torch.from_numpy(ns), use_softmax=False).numpy())
    preds, mx = R.decode_argmax(ns.reshape(6, 4, 6), 1)
    rp, rm = O.get_max_preds(ns)
    assert np.array_equal(preds.reshape(2, 3, 2), rp) and np.array_equal(mx.reshape(2, 3, 1), rm)
    # every scenario of the GPU test: the first maximal index, a NaN maximal, as torch.argmax has it
    for h, w in R.PER_MAP_SHAPES:
        hm, names = R.argmax_case(257, h, w)
        flat = torch.from_numpy(hm.reshape(257, -1))
        idx = torch.argmax(flat, dim=1).numpy()
        for style, d in ((0, h), (1, w)):
            preds, mx = R.decode_argmax(hm, style)
            want = np.stack((idx % d, idx // d), 1).astype(np.float32)
            if style:
                want[~(mx > 0)] = 0
            assert np.array_equal(preds, want), (h, w, style)
        if h * w >= 3:
            assert set(names) >= {'one_nan', 'two_nans', 'all_nan', 'all_neg_inf', 'pos_inf', 'all_equal', 'tie_next'}
        if h * w > 460:
            assert set(names) == set(R.ARGMAX_SCENARIOS)
        for k, s in enumerate(names):
            m = hm[k].ravel()
            if s in ('all_nan', 'all_neg_inf', 'all_equal', 'all_zero'):
                assert idx[k] == 0
            if s in ('one_nan', 'two_nans', 'nan_other_stripe'):
                assert np.isnan(m[idx[k]]) and not np.isnan(m[:idx[k]]).any()
            if s == 'nan_other_stripe':
                q = int(np.nanargmax(m))
                assert q < idx[k] and (idx[k] - q) % 256 != 0
            if s.startswith('tie_'):
                assert (m == m[idx[k]]).sum() == 2 and idx[k] > 0
            if s == 'tie_cross':
                other = int(np.flatnonzero(m == m[idx[k]])[1])
                assert idx[k] % 256 > other % 256                         # the winner sits in the higher thread


def test_expectation_and_softmax_references_match_fixture_and_oracle(golden_dir):
    z = _z(golden_dir, 'decode_crosscheck.npz')
    pos, raw = _t(z['pos']), _t(z['raw'])
    b, k, h, w = pos.shape
    got = R.decode_expectation(pos.reshape(b * k, h, w)).reshape(b, k, 2)
    assert np.abs(got.numpy() - z['coords_normalised']).max() <= 2e-5
    assert (got - O.get_final_preds(pos, True)).abs().max().item() <= 1e-11
    soft = R.softmax(raw.reshape(b * k, -1), torch.tensor(1.0, dtype=F64))
    assert np.abs(soft.numpy().reshape(z['softmax_maps'].shape) - z['softmax_maps']).max() <= 1e-7
    got = R.decode_expectation(soft.reshape(b * k, h, w)).reshape(b, k, 2)
    assert np.abs(got.numpy() - z['coords_softmax']).max() <= 2e-5
    # gradients: autograd through the oracle's decode, and through torch's softmax with ONE temperature
    gp = torch.from_numpy(np.random.default_rng(1).standard_normal((b * k, 2)))
    pr = pos.clone().requires_grad_(True)
    (O.get_final_preds(pr, True).reshape(b * k, 2) * gp).sum().backward()
    assert (R.decode_expectation_grad(gp, h, w) - pr.grad.reshape(b * k, h, w)).abs().max().item() <= 1e-12
    gout = torch.from_numpy(np.random.default_rng(2).standard_normal((b * k, h * w)))
    x = raw.reshape(b * k, -1).clone().requires_grad_(True)
    t = torch.tensor(1.7, dtype=F64, requires_grad=True)
    torch.softmax(x * t, dim=-1).backward(gout)
    out, dx, dtemp = R.softmax_grads(raw.reshape(b * k, -1), t.detach(), gout)
    assert (dx - x.grad).abs().max().item() <= 1e-15
    assert abs(dtemp.sum().item() - t.grad.item()) <= 1e-12 * R.softmax_dtemp_abs_terms(x.detach(), out, gout).sum().item()
    assert dtemp.shape == (b * k,)


def test_adam_reference_matches_torch_adam_in_float64():
    rng = np.random.default_rng(5)
    for wd, gscale, lr in ((1e-4, 1.0, 1e-3), (0.0, 1.0 / 3.0, 3e-4), (1e-4, 0.125, 1e-3)):
        p0 = torch.from_numpy(rng.standard_normal(300))
        p_ref = p0.clone().requires_grad_(True)
        opt = torch.optim.Adam([p_ref], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for step in range(1, 5):
            g = torch.from_numpy(rng.standard_normal(300))
            g[::7] = 0.0
            p_ref.grad = g * gscale
            opt.step()
            p, m, v = R.adam_step(p, g, m, v, step, lr, 0.9, 0.999, 1e-8, wd, gscale)
            assert (p - p_ref.detach()).abs().max().item() <= 1e-14
            st = opt.state[p_ref]
            assert (m - st['exp_avg']).abs().max().item() <= 1e-15 and (v - st['exp_avg_sq']).abs().max().item() <= 1e-15
    # numpy arrays step the same way (the late-step states are walked in numpy)
    pn, mn, vn = R.adam_step(p0.numpy(), g.numpy(), m.numpy(), v.numpy(), 7, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 0.125)
    pt, mt, vt = R.adam_step(p0, g, m, v, 7, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 0.125)
    assert np.abs(pn - pt.numpy()).max() <= 1e-15 and np.array_equal(mn, mt.numpy()) and np.array_equal(vn, vt.numpy())
    # the walk: step 1 is the start, step 2 one reference step on, and late states are reached and finite
    p1, m1, v1 = R.adam_pool_state(1, 0.125, 1e-4, 1e-3)
    p2, m2, v2 = R.adam_pool_state(2, 0.125, 1e-4, 1e-3)
    assert not m1.any() and not v1.any() and m2.any() and (v2 > 0).all() and np.abs(p2 - p1).max() <= 1.01e-3
    pk, mk, vk = R.adam_pool_state(1000, 0.125, 1e-4, 1e-3)
    assert np.isfinite(pk).all() and (vk > 0).all() and np.abs(pk - p1).max() > 1e-3
    # the gradient table has no net pull, so p stays where float32 resolves the older test's 1e-6 (half an ulp below 8)
    pl, ml, vl = R.adam_pool_state(100000, 0.125, 1e-4, 1e-3)
    assert np.abs(pl).max() < 8 and np.abs(pl - pk).max() > 1e-3 and ml.any() and (vl > 0).all()


def test_normalize_and_targets_references():
    rng = np.random.default_rng(11)
    u8 = torch.from_numpy(rng.integers(0, 256, (3, 32, 24, 3), dtype=np.uint8))
    ref = (u8.float() / 255.0 - torch.tensor(synth.IMAGENET_MEAN)) / torch.tensor(synth.IMAGENET_STD)
    got = R.normalize_u8(u8, R.U8_CONSTANTS[0][0], R.U8_CONSTANTS[0][1], F64)
    assert (got - ref.permute(0, 3, 1, 2).double()).abs().max().item() <= 1e-6
    for n, h, w in R.U8_CASES[:4]:
        img = R.u8_case(n, h, w)
        assert img.shape == (n, h, w, 3)
    img = R.u8_case(3, 16, 16)
    assert all(len(np.unique(img[..., c])) == 256 for c in range(3)) and not np.array_equal(img[..., 0], img[..., 1])
    # Gaussian targets: no visibility draws every joint; a joint is drawn where its visibility is > 0
    pose, vis = R.targets_case(257, 48, 40)
    pose, vis = pose.reshape(1, 257, 2), vis.reshape(1, 257, 1)
    every = synth.gaussian_heatmaps(pose, None, 48, 40, 2)
    assert np.array_equal(every, synth.gaussian_heatmaps(pose, np.ones_like(vis), 48, 40, 2))
    some = synth.gaussian_heatmaps(pose, vis, 48, 40, 2)
    drawn = vis[0, :, 0] > 0
    assert np.array_equal(some[0, drawn], every[0, drawn]) and not some[0, ~drawn].any() and (~drawn).sum() > 50
    assert np.array_equal(some, synth.gaussian_heatmaps(pose, vis > 0, 48, 40, 2))
    # the edge coordinates: (-1, 0) truncates onto the map, exactly W or H is off it, W - 0.01 is on it
    on = every[0].reshape(257, -1).max(1) == 1.0
    for k, (x, y) in enumerate(pose[0][:20]):
        assert on[k] == (int(x) >= 0 and int(y) >= 0 and int(x) < 40 and int(y) < 48), (k, x, y)
    assert on[4] and on[5] and on[6] and not on[7] and not on[8] and on[9] and not on[11] and not on[17]
    assert every[0, 9, 47, 39] == 1.0 and every[0, 4, 3, 0] == 1.0


# ---- the planted elements ---------------------------------------------------------------------------------------------

def _rel(allowed, s):
    """the allowed error of one reduced scalar as a fraction of its sum |terms|"""
    return float(np.asarray(allowed, dtype=np.float64).ravel()[0]) / float(s)


def test_planted_elements_of_the_heatmap_loss_inputs():
    for (h, w) in R.PER_MAP_SHAPES:
        for bk in R.PER_MAP_BK + ((255, 256, 336) if (h, w) in ((8, 8), (5, 13)) else ()):
            pred, gt, zeros = R.heatmap_case(bk, h * w)
            assert (pred[:, zeros] == gt[:, zeros]).all()
            for mode in (0, 1):
                e = R.heatmap_expected(pred, gt, mode)
                ref64, ref32, s, floor = e['partial']
                allowed = R.sums_allowed(ref64, ref32, s, floor)
                pi = R.planted_indices(h * w)
                for k in (0, bk - 1):
                    R.assert_planted(e['terms'][k], pi, allowed[k] / float(s[k]), ('heatmap map', h, w, bk, mode))
                ref64, ref32, s, floor, cap = e['loss']
                rel = _rel(R.sums_allowed(ref64, ref32, s, floor, cap), s)
                R.assert_planted(e['terms'].sum(1), R.planted_indices(bk), rel, ('heatmap loss', h, w, bk, mode))


def test_planted_elements_of_the_joints_loss_inputs():
    for b, k in R.JOINTS_SHAPES:
        for vis_mode in R.JOINTS_VIS:
            pred, gt, vis, zeros = R.joints_case(b, k, vis_mode)
            assert (pred.reshape(-1, 2)[zeros] == gt.reshape(-1, 2)[zeros]).all()
            e = R.joints_expected(pred, gt, vis)
            ref64, ref32, s, floor, cap = e['loss']
            if vis_mode == 'zero':                       # the edge case itself: every term is 0 and so is the loss
                assert float(ref64) == 0.0 and float(s) == 0.0
                continue
            rel = _rel(R.sums_allowed(ref64, ref32, s, floor, cap), s)
            pi = R.planted_indices(b * k)
            R.assert_planted(e['terms'], pi, rel, ('joints loss', b, k, vis_mode))
            if vis is not None and e['denominator'] > 1.0:
                # the denominator's own reduction: a lost or doubled weight moves the loss by that share of it
                R.assert_planted(vis.ravel(), pi, rel, ('joints weights', b, k, vis_mode))


def test_planted_elements_of_the_expectation_and_softmax_inputs():
    for si, (h, w) in enumerate(R.PER_MAP_SHAPES):
        pi = R.planted_indices(h * w)
        for bk in R.PER_MAP_BK:
            if h * w > 1:
                hm = R.expectation_case(bk, h, w)
                ref64, ref32, s, floor, cap = R.expectation_expected(hm)['preds']
                allowed = R.sums_allowed(ref64, ref32, s, floor, cap).reshape(bk, 2)
                xs, ys = np.arange(h * w) % w, np.arange(h * w) // w
                for k in (0, bk - 1):
                    for c, coord in ((0, xs), (1, ys)):
                        if s[k, c] > 0:                  # (a 1-wide or 1-high map has one coordinate identically 0)
                            live = pi[coord[pi] > 0]
                            R.assert_planted(hm[k].ravel() * coord, live, allowed[k, c] / float(s[k, c]),
                                             ('expectation', h, w, bk, c))
            for temp in R.SOFTMAX_TEMPS:
                x, g, kinds = R.softmax_case(bk, h * w, temp, si)
                assert kinds[0] == R.ROW_PLAIN
                e = R.softmax_expected(x, g, temp)
                # out: a lost element i rescales the row by 1 / (1 - mass_i): the largest output moves by more than
                # mass_i * max(out); dx and dtemp: the terms of their two reductions
                out_allowed, _ = R.elementwise_allowed(*e['out'])
                mass = e['mass'][0]
                assert (mass[pi] * mass.max()).min() >= 100 * out_allowed[0] or h * w == 1, (h, w, bk, temp)
                ref64, ref32, s, floor = e['dtemp']
                allowed = R.sums_allowed(ref64, ref32, s, floor)
                if h * w > 1:
                    R.assert_planted(e['dtemp_terms'][0], pi, allowed[0] / float(s[0]), ('dtemp', h, w, bk, temp))
                    dot = e['dot_terms'][0]
                    R.assert_planted(dot, pi, R.sum_floor(h * w, 1), ('softmax dot', h, w, bk, temp))
        if len(R.PER_MAP_SHAPES) > si:
            kinds = R.softmax_row_kinds(3, si)
            assert len(set(kinds)) == 3 or R.ROW_PLAIN in kinds[1:]
    seen = set()
    for si in range(len(R.PER_MAP_SHAPES)):
        seen |= set(R.softmax_row_kinds(3, si))
    assert seen == {R.ROW_PLAIN, R.ROW_SHIFTED, R.ROW_EQUAL, R.ROW_ONE_HOT}
    x, _, kinds = R.softmax_case(257, 64, 1.7, 0)
    z = x.astype(np.float64) * R.f32(1.7)
    assert z[kinds == R.ROW_SHIFTED].max() >= 1e4 and z[kinds == R.ROW_SHIFTED].min() <= -1e4
    assert (np.ptp(z[kinds == R.ROW_EQUAL], axis=1) == 0).all()


def test_adam_inputs_have_zero_gradient_points_and_late_states():
    p, g, m, v, z = R.adam_case(257, 1000, 0.125, 1e-4, 1e-3)
    assert len(z) > 30 and not g[z].any() and not m[z].any() and not v[z].any()
    assert g[0] != 0 and g[-1] != 0 and (v[np.setdiff1d(np.arange(257), z)] > 0).all()
    e = R.adam_expected(p, g, m, v, 1000, 0.125, 0.0, 1e-3)
    assert np.array_equal(e['p'][0].numpy()[z], p[z].astype(np.float64))       # 0 / eps: the parameter stays
    # every element moves by far more than its bound: an element that is skipped is seen
    moved = np.abs(e['p'][0].numpy() - p)[np.setdiff1d(np.arange(257), z)]
    assert moved.min() >= 0 and np.median(moved) >= 100 * R.elementwise_allowed(*e['p'])[0]
