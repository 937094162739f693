"""The fuse-sum and BatchNorm-backward passes of csrc/eltwise.hip at the shapes where they can go wrong: one channel
vector, 12 vectors (48 / 96 channels: 256 / 12 leaves four idle threads), odd extents, more than one grid-stride turn,
workgroups with an empty pixel range, mask values of +-0 and a denormal, pre-activations of exactly 0.

Case group -> kernels:
    test_sum_terms_*                        sum_terms_kernel<T, false> (plain, and bnref with sums_mode = 0)
    test_sum_terms_from_batch_sums          sum_terms_kernel<T, true> (sums_mode masks, SUM_MAXC, the variance clamp);
                                            its _sum_tables: sum_terms_table_kernel<T, false> and <T, true> (eps in
                                            SUM_EPS_BITS)
    test_grad_term_on_the_lattice_*         grad_term_kernel (compute_dz at shifts 0..4, both destinations, dst == g)
    test_grad_term_real_values_*            grad_term_kernel over grid-stride turns; its _grad_table: grad_term_table_kernel
    test_grad_term_at_the_rows_boundary     grad_term_rows_kernel against grad_term_kernel one pixel short
    test_bn_bwd_reduce_*                    bn_bwd_reduce_kernel (with / without the dz store); its _reduce_table:
                                            bn_bwd_reduce_table_kernel
    test_pool_reduce_*                      pool_reduce_kernel / pool_reduce_table_kernel, pool_reduce_block<T, 1|2|3>
    test_bn_bwd_finalize_*                  bn_bwd_finalize_kernel / bn_bwd_finalize_table_kernel (partial_sums)
    test_reduce_finalize_apply_*            the three passes chained, as launches and as three table launches

Every kernel is reached as a launch of its own - through its C entry point where it has one and through
hrnet_program_run with an op built by hipnet.ops.make - and as a job of an OP_EW_TABLE launch built the way
engine._add_ew_table builds it; a table launch must give the bits of the per-job launches. A job is only placed in a
table after it has been accepted and run as a launch of its own in the same test (the host validates only the table
header), and the refusal cases are those HR_REQUIRE rejects before any launch. The conventions are those of
tests/test_glue_kernels_gpu.py: every output inside 64 sentinels on each side that come back unchanged, the payload
fully written, every launch twice with the same bits, every test in a spawned child. References, bounds and inputs:
tests/fuse_refs.py (pinned on the CPU by tests/test_fuse_refs_cpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

import fuse_refs as R
import glue_refs as G
from spawned import spawned
from test_glue_kernels_gpu import DEV, DT, DTYPE_IDS, Guarded, _dev, _ip, _pp, _twice

pytestmark = pytest.mark.gpu

F32 = torch.float32


def _C():
    from hipnet import _capi as C
    from hipnet import ops
    return C, ops


def _run_op(C, op):
    C.call('hrnet_program_run', ctypes.byref(op), 1, C.stream_ptr())


def _p(t):
    return None if t is None else t.data_ptr()


class Job(object):
    """one op of an element-wise kind: `fields` are its inputs (ops.make names; device tensors are kept alive in
    `keep`), `outs` its outputs as (field, member index or None, elements, dtype, initial payload or None); `alias`
    maps an input field to the output it shares memory with; `dims`: the (N, H, W, C) that size its table blocks"""

    def __init__(self, kind, fields, outs, dims, keep, alias=None, capi=None):
        self.kind, self.fields, self.outs, self.dims, self.keep = kind, fields, outs, dims, keep
        self.alias, self.capi = alias or {}, capi

    def guards(self):
        return [Guarded(n, dtype, init) for _, _, n, dtype, init in self.outs]

    def op(self, ops, gs):
        f = dict(self.fields)
        for (field, k, _, _, _), g in zip(self.outs, gs):
            if k is None:
                f[field] = g.ptr()
            else:
                f.setdefault(field, [None, None, None])[k] = g.ptr()
        for field, k in self.alias.items():
            f[field] = gs[k].ptr()
        return ops.make(self.kind, **f)


def _alone(C, ops, job, name, capi=False):
    """the job as a launch of its own (capi: through its C entry point), twice -> the values of its outputs"""
    def run():
        gs = job.guards()
        if capi:
            job.capi(gs)
        else:
            _run_op(C, job.op(ops, gs))
        return [g.get(name) for g in gs]
    return _twice(name, run)


def _both_ways(C, ops, job, name):
    """through hrnet_program_run and through the C entry point: the same bits"""
    a = _alone(C, ops, job, name + ' (op)')
    b = _alone(C, ops, job, name + ' (C entry)', capi=True)
    for x, y in zip(a, b):
        assert G.same_bits(x, y), name + ': the C entry point and the op differ'
    return a


def _refused(C, ops, job, name):
    gs = job.guards()
    with pytest.raises(RuntimeError):
        _run_op(C, job.op(ops, gs))
    assert all(g.untouched() for g in gs), name + ': a refused op wrote'
    if job.capi is not None:
        with pytest.raises(RuntimeError):
            job.capi(gs)
        assert all(g.untouched() for g in gs), name + ': a refused call wrote'


def _table(C, ops, dtype, jobs, alone, name, **fields):
    """`jobs` (each already run alone, outputs `alone`) as ONE table launch: the bits of the per-job launches"""
    kind, dtid = jobs[0].kind, C.dtype_id(dtype)
    assert 3 <= len(jobs) <= 5 and len(alone) == len(jobs)
    counts = []

    def run():
        gss = [j.guards() for j in jobs]
        recs = [j.op(ops, gs) for j, gs in zip(jobs, gss)]
        block = 0
        del counts[:]
        for j, rec in zip(jobs, recs):
            nb = C.call('hrnet_ew_table_blocks', kind, dtid, *j.dims)
            ops.set_job_blocks(rec, block, nb)
            counts.append(nb)
            block += nb
        arr = (C.HrOp * len(recs))(*recs)
        raw = bytes(ctypes.string_at(ctypes.addressof(arr), ctypes.sizeof(arr)))
        table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
        _run_op(C, ops.make(C.OP_EW_TABLE, jobs=len(recs), blocks=block, kind=kind, dtype=dtid, table=table.data_ptr(),
                            **fields))
        out = [g.get(name) for gs in gss for g in gs]          # (get synchronises: the table is alive until here)
        del table
        return out
    got = _twice(name, run)
    assert 1 in counts, name + ': no one-block job'
    want = [v for vs in alone for v in vs]
    assert len(got) == len(want)
    for k, (x, y) in enumerate(zip(got, want)):
        assert G.same_bits(x, y), '{}: output {} differs from the job\'s own launch'.format(name, k)
    print('{}: {} jobs of {} blocks, the bits of their own launches'.format(name, len(jobs), counts))


# ---- sum_terms ----------------------------------------------------------------------------------------------------------

def _sum_job(C, dt, shape, terms, relu_out, sums_mode=0, eps=1e-5, bnref=False):
    """terms: dicts src, sh, relu, and scale / shift [C] or None - or, for a bit of sums_mode, sums [8][2][C], gamma,
    beta and inv_count"""
    dtype, (N, H, W, cv) = DT[dt], shape
    Cc = cv * R.VEC[dt]
    src = [_dev(t['src'], dtype) for t in terms]
    sc = [None if t.get('scale') is None else _dev(t['sums'] if 'sums' in t else t['scale']) for t in terms]
    sf = [None if t.get('scale') is None else
          _dev(np.concatenate([t['gamma'], t['beta']]) if 'sums' in t else t['shift']) for t in terms]
    inv = [float(t.get('inv_count', 0.0)) for t in terms]
    shs, relus = [t['sh'] for t in terms], [1 if t.get('relu') else 0 for t in terms]
    fields = dict(dtype=C.dtype_id(dtype), n=N, h=H, w=W, c=Cc, nterms=len(terms), relu_out=relu_out, sh=shs,
                  relu=relus, src=[_p(t) for t in src], scale=[_p(t) for t in sc], shift=[_p(t) for t in sf])
    if sums_mode or bnref:
        from hipnet import ops
        fields.update(sums_mode=sums_mode, inv_count=inv, eps_bits=ops.f32_bits(eps))

    def capi(gs):
        head = (C.dtype_id(dtype), gs[0].ptr(), N, H, W, Cc, len(terms), _pp([_p(t) for t in src]),
                _pp([_p(t) for t in sc]), _pp([_p(t) for t in sf]), _ip(shs), _ip(relus), relu_out)
        if sums_mode or bnref:
            C.call('hrnet_sum_terms_bnref', *(head + (sums_mode, (ctypes.c_float * 4)(*(inv + [0.0] * 4)[:4]), eps,
                                                      C.stream_ptr())))
        else:
            C.call('hrnet_sum_terms', *(head + (C.stream_ptr(),)))
    return Job(C.OP_SUM_TERMS, fields, [('out', None, N * H * W * Cc, dtype, None)], (N, H, W, Cc), [src, sc, sf],
               capi=capi)


def _real_terms(shape, dt, specs, *key):
    N, H, W, cv = shape
    Cc = cv * R.VEC[dt]
    terms = []
    for k, (sh, affine, relu) in enumerate(specs):
        t = dict(src=R.real((N, H >> sh, W >> sh, Cc), dt, *key, k), sh=sh, scale=None, shift=None, relu=relu)
        if affine:
            t.update(scale=G.real((Cc,), *key, k, 1), shift=G.real((Cc,), *key, k, 2))
        terms.append(t)
    return terms


@pytest.mark.parametrize('dt', DTYPE_IDS)
@spawned
def test_sum_terms_on_the_lattice_is_bit_equal(dt):
    """one vector, 12 vectors with four terms of shifts 0..3 (identity term in every slot, ReLUs both ways, scale given
    and NULL) and odd extents, as the plain call, as the bnref call with sums_mode = 0 and as an op: the bits of the
    float64 reference, pre-activations of exactly 0 included. A shift on an odd extent is refused."""
    C, ops = _C()
    cases = R.sum_lattice_cases()
    for ci, (shape, specs, relu_out) in enumerate(cases):
        terms = R.lattice_terms(shape, dt, specs, 11, ci)
        ref, tot, _ = R.sum_terms(terms, relu_out)
        assert R.lattice_exact(tot)
        want = R.stored_bits(ref, dt).reshape(-1)
        name = 'sum_terms lattice {} {} case {}'.format(dt, shape, ci)
        got = _both_ways(C, ops, _sum_job(C, dt, shape, terms, relu_out), name)[0]
        assert G.same_bits(got, want), name
        if all(t['scale'] is not None for t in terms) or ci % 3 == 0:
            # the entry point of the batch-sum form with no bit set: the plain instantiation, the same bits
            got = _both_ways(C, ops, _sum_job(C, dt, shape, terms, relu_out, bnref=True), name + ' bnref')[0]
            assert G.same_bits(got, want), name + ' bnref'
    terms = R.lattice_terms((3, 8, 8, 8), dt, [(0, False, False), (1, True, False)], 12)
    _refused(C, ops, _sum_job(C, dt, R.ODD, terms, 0), 'sum_terms shift 1 on 5 x 7')
    print('sum_terms {}: {} lattice cases bit-equal'.format(dt, len(cases)))


@pytest.mark.parametrize('dt', DTYPE_IDS)
@spawned
def test_sum_terms_real_values_over_widths_and_grid_stride_turns(dt):
    """one vector, 12 vectors with terms at shifts 0..3 in two orders, odd extents, and 2 x 128 x 128 x 160 / 320 with
    a shift-3 term (1.31 M vectors against the 4096 x 256 grid cap), each as the plain call and as an op.
    Worst error / bound: 0.638 (f32), 0.996 (bf16) on an MI355X"""
    C, ops = _C()
    key = 'sum_terms real ' + dt
    cases = [(R.ONE_VECTOR, [(0, True, True), (2, True, False)], 0),
             (R.W48, [(0, False, False), (1, True, True), (2, True, False), (3, True, True)], 1),
             (R.W48, [(3, True, False), (0, True, True), (1, False, False)], 0),
             (R.ODD, [(0, True, True), (0, False, False)], 1),
             (R.BIG, [(0, False, False), (3, True, True)], 1)]
    for ci, (shape, specs, relu_out) in enumerate(cases):
        terms = _real_terms(shape, dt, specs, 13, ci)
        ref, tot, n = R.sum_terms(terms, relu_out)
        name = 'sum_terms real {} {} case {}'.format(dt, shape, ci)
        got = _both_ways(C, ops, _sum_job(C, dt, shape, terms, relu_out), name)[0]
        R.check_elem(key, name, got.reshape(ref.shape), ref, tot, n, dt == 'bf16')
    R.report(key)


def _sums_terms(shape, dt, mask, *key):
    """four terms of shifts (0, 1, 0, 2): bit t of `mask` makes term t a batch-sum term; of the others term 1 and 3
    are plain-affine terms and term 0 and 2 bare ones -> (terms for the device, terms for the reference, extra
    allowance per element, e_ref values)"""
    N, H, W, cv = shape
    Cc = cv * R.VEC[dt]
    dev, ref, extra, e_refs = [], [], 0.0, []
    for t, sh in enumerate((0, 1, 0, 2)):
        src = R.real((N, H >> sh, W >> sh, Cc), dt, *key, t)
        term = dict(src=src, sh=sh, scale=None, shift=None, relu=t % 2 == 1)
        rterm = dict(term)
        if (mask >> t) & 1:
            sums, gamma, beta, inv, eps, _ = R.sums_case(Cc, *key, t, 5)
            sc, sf, dsc, dsf, e_sc, e_sf = R.sums_allowance(sums, inv, eps, gamma, beta)
            term.update(sums=sums, gamma=gamma, beta=beta, inv_count=inv, scale=True)
            rterm.update(scale=sc, shift=sf)
            extra = extra + np.abs(R.up(src.astype(np.float64), sh)) * dsc + dsf
            e_refs += [e_sc, e_sf]
        elif t in (1, 3):
            term.update(scale=G.real((Cc,), *key, t, 1), shift=G.real((Cc,), *key, t, 2))
            rterm.update(scale=term['scale'], shift=term['shift'])
        dev.append(term)
        ref.append(rterm)
    return dev, ref, extra, e_refs


SUMS_EPS = 1e-3


def _sum_tables(C, ops, dt):
    """a plain table of plain jobs (sum_terms_table_kernel<T, false>) and a sums = 1 table that mixes a batch-sum job
    with plain ones (<T, true>); eps is not the default, so a job reading it from the wrong slot differs"""
    dtype = DT[dt]
    plain = [_sum_job(C, dt, R.ODD, _real_terms(R.ODD, dt, [(0, True, True), (0, False, False)], 21), 1),
             _sum_job(C, dt, R.ONE_VECTOR, _real_terms(R.ONE_VECTOR, dt, [(0, True, False), (3, True, True)], 22), 0),
             _sum_job(C, dt, R.W48, _real_terms(R.W48, dt, [(0, False, False), (1, True, True), (2, True, False),
                                                            (3, True, True)], 23), 1),
             _sum_job(C, dt, (1, 2, 2, 1), _real_terms((1, 2, 2, 1), dt, [(1, True, True)], 24), 0)]
    alone = [_alone(C, ops, j, 'sum_terms job {}'.format(k)) for k, j in enumerate(plain)]
    _table(C, ops, dtype, plain, alone, 'sum_terms table {} plain'.format(dt), sums=0)
    mixed = [plain[0],
             _sum_job(C, dt, R.W48, _sums_terms(R.W48, dt, 0b101, 25)[0], 1, sums_mode=0b101, eps=SUMS_EPS),
             plain[3],
             _sum_job(C, dt, (1, 4, 4, 2), _sums_terms((1, 4, 4, 2), dt, 0b010, 26)[0], 0, sums_mode=0b010,
                      eps=SUMS_EPS)]
    # (a plain job of a sums = 1 launch carries sums_mode = 0 and runs through the instantiation with the table)
    alone = [alone[0], _alone(C, ops, mixed[1], 'sum_terms sums job'), alone[3],
             _alone(C, ops, mixed[3], 'sum_terms small sums job')]
    _table(C, ops, dtype, mixed, alone, 'sum_terms table {} sums'.format(dt), sums=1)


@pytest.mark.parametrize('dt', DTYPE_IDS)
@spawned
def test_sum_terms_from_batch_sums(dt):
    """sums_mode 0b001, 0b010, 0b101 and 0b1111 over four terms (a batch-sum term beside a plain-affine and a bare
    one), 384 channels served, one vector more refused with a bit set and served without, every eighth channel a
    constant whose sums leave a negative variance; then the table launches (_sum_tables).
    Worst error / bound: 0.505 (f32), 0.996 (bf16) on an MI355X"""
    C, ops = _C()
    key = 'sum_terms sums_mode ' + dt
    vec = R.VEC[dt]
    for shape in ((2, 8, 24, 12), (1, 4, 4, R.SUM_MAXC // vec)):
        for mask in (0b001, 0b010, 0b101, 0b1111):
            dev, ref, extra, e_refs = _sums_terms(shape, dt, mask, 17, shape[3], mask)
            r, tot, n = R.sum_terms(ref, 1)
            name = 'sum_terms sums_mode {:04b} {} {} (e_ref {:.1e})'.format(mask, dt, shape, max(e_refs))
            got = _both_ways(C, ops, _sum_job(C, dt, shape, dev, 1, sums_mode=mask, eps=SUMS_EPS), name)[0]
            R.check_elem(key, name, got.reshape(r.shape), r, tot, n, dt == 'bf16', extra=extra)
    wide = (1, 4, 4, R.SUM_MAXC // vec + 1)              # 388 / 392 channels
    dev, ref, _, _ = _sums_terms(wide, dt, 0b001, 18)
    _refused(C, ops, _sum_job(C, dt, wide, dev, 1, sums_mode=1, eps=SUMS_EPS), 'sum_terms sums_mode beyond SUM_MAXC')
    plain = _real_terms(wide, dt, [(0, True, True), (1, False, False)], 19)
    r, tot, n = R.sum_terms(plain, 1)
    got = _both_ways(C, ops, _sum_job(C, dt, wide, plain, 1, bnref=True), 'sum_terms wide, no bit set')[0]
    R.check_elem(key, 'sum_terms {} {} sums_mode 0'.format(dt, wide), got.reshape(r.shape), r, tot, n, dt == 'bf16')
    _sum_tables(C, ops, dt)
    R.report(key)


# ---- grad_term ------------------------------------------------------------------------------------------------------------

def _grad_job(C, dt, shape, sh, inp, coef, acc, inner_relu, dst2=None, alias_g=False):
    """inp: dict g, mask, y, scale, shift (numpy, a device tensor that is used as it is, or None); coef [3][C] or None;
    acc: None or the old dst; dst2: None, or (old dst2 or None): the second destination"""
    dtype, (N, H, W, cv) = DT[dt], shape
    Cc = cv * R.VEC[dt]
    t = {k: (inp.get(k) if inp.get(k) is None or isinstance(inp[k], torch.Tensor) else
             _dev(inp[k], dtype if k in ('g', 'mask', 'y') else F32)) for k in ('g', 'mask', 'y', 'scale', 'shift')}
    t['coef'] = None if coef is None else _dev(coef)
    n = N * H * W * Cc
    fields = dict(dtype=C.dtype_id(dtype), n=N, h=H, w=W, c=Cc, sh=sh, inner_relu=inner_relu,
                  accumulate=0 if acc is None else 1, accumulate2=1 if dst2 is not None and dst2[0] is not None else 0,
                  **{k: _p(v) for k, v in t.items()})
    outs = [('dst', None, n, dtype, inp['g'] if alias_g else acc)]
    if dst2 is not None:
        outs.append(('dst2', None, n, dtype, dst2[0]))

    def capi(gs):
        gp = gs[0].ptr() if alias_g else _p(t['g'])
        tail = (gp, _p(t['mask']), _p(t['y']), _p(t['scale']), _p(t['shift']), _p(t['coef']), N, H, W, Cc)
        if dst2 is not None:
            C.call('hrnet_grad_term2', C.dtype_id(dtype), gs[0].ptr(), gs[1].ptr(), *(tail + (
                fields['accumulate'], fields['accumulate2'], C.stream_ptr())))
        else:
            C.call('hrnet_grad_term', C.dtype_id(dtype), gs[0].ptr(), *(tail + (sh, inner_relu, fields['accumulate'],
                                                                               C.stream_ptr())))
    return Job(C.OP_GRAD_TERM, fields, outs, (N, H, W, Cc), [t], alias={'g': 0} if alias_g else None, capi=capi)


def _grad_ref(inp, sh, inner_relu, coef, acc):
    d, a, near = R.dz(inp['g'], inp['mask'], inp['y'], inp['scale'], inp['shift'], sh, inner_relu)
    ref, tot = R.grad_term(d, a, inp['y'], coef, acc)
    return ref, tot, near, d, a


def _grad_cases(C, ops, dt, lattice, key):
    n_cases = 0
    for ci, (sh, shape, with_mask, inner_relu, with_scale, with_coef, accumulate) in enumerate(R.grad_configs()):
        Cc = shape[3] * R.VEC[dt]
        inp = R.grad_inputs(shape, sh, dt, lattice, with_mask, inner_relu, with_scale, 31, ci, int(lattice))
        lo = inp['y'].shape
        coef = (R.lattice_coef(Cc, 32, ci) if lattice else G.real((3, Cc), 32, ci)) if with_coef else None
        acc = (R.lattice(lo, 33, ci) if lattice else R.real(lo, dt, 33, ci)) if accumulate else None
        ref, tot, near, _, _ = _grad_ref(inp, sh, inner_relu, coef, acc)
        name = 'grad_term {} {} sh {} mask {} relu {} scale {} coef {} acc {}'.format(
            dt, 'lattice' if lattice else 'real', sh, int(with_mask), inner_relu, int(with_scale), int(with_coef),
            int(accumulate))
        got = _both_ways(C, ops, _grad_job(C, dt, shape, sh, inp, coef, acc, inner_relu), name)[0]
        if lattice:
            assert R.lattice_exact(tot)
            assert G.same_bits(got, R.stored_bits(ref, dt).reshape(-1)), name
        else:
            R.check_elem(key, name, got.reshape(ref.shape), ref, tot, R.grad_adds(sh, with_coef, accumulate),
                         dt == 'bf16', skip=near)
        n_cases += 1
    return n_cases


@pytest.mark.parametrize('dt', DTYPE_IDS)
@spawned
def test_grad_term_on_the_lattice_is_bit_equal(dt):
    """shifts 0 to 4, inner ReLU with and without scale (pre-activations of exactly 0), coef given and NULL,
    accumulate 0 and 1, masks of +-0 and a denormal; dst == g at shift 0 (how the engine applies onto a kept dz);
    the second destination; what fill_grad_args refuses"""
    C, ops = _C()
    n = _grad_cases(C, ops, dt, True, None)
    shape, Cc = R.GRAD_SHAPE, R.GRAD_SHAPE[3] * R.VEC[dt]
    inp = R.grad_inputs(shape, 0, dt, True, False, 0, False, 34)
    coef = R.lattice_coef(Cc, 35)
    ref, tot, _, d, a = _grad_ref(inp, 0, 0, coef, None)
    got = _both_ways(C, ops, _grad_job(C, dt, shape, 0, inp, coef, None, 0, alias_g=True), 'grad_term dst == g')[0]
    assert G.same_bits(got, R.stored_bits(ref, dt).reshape(-1)), 'grad_term dst == g'
    inp = R.grad_inputs(shape, 0, dt, True, True, 0, False, 36)
    ref, tot, _, d, a = _grad_ref(inp, 0, 0, coef, None)
    for old2 in (None, R.lattice(inp['y'].shape, 37)):
        got = _both_ways(C, ops, _grad_job(C, dt, shape, 0, inp, coef, None, 0, dst2=(old2,)), 'grad_term2')
        assert G.same_bits(got[0], R.stored_bits(ref, dt).reshape(-1)), 'grad_term2 dst'
        assert G.same_bits(got[1], R.stored_bits(d + (0.0 if old2 is None else old2), dt).reshape(-1)), 'grad_term2 dst2'
    # refused before any launch: a second destination with a shift or an inner ReLU, shift 5, coef without y, a
    # channel count that is no multiple of the vector
    up1 = R.grad_inputs(shape, 1, dt, True, True, 1, True, 38)
    job = _grad_job(C, dt, shape, 1, up1, coef, None, 0, dst2=(None,))
    job.capi = None                                      # (hrnet_grad_term2 has neither a shift nor an inner_relu argument)
    _refused(C, ops, job, 'dst2 with shift 1')
    job = _grad_job(C, dt, shape, 0, R.grad_inputs(shape, 0, dt, True, True, 1, True, 39), coef, None, 1, dst2=(None,))
    job.capi = None
    _refused(C, ops, job, 'dst2 with an inner ReLU')
    _refused(C, ops, _grad_job(C, dt, shape, 5, up1, coef, None, 0), 'shift 5')
    no_y = dict(inp, y=None)
    _refused(C, ops, _grad_job(C, dt, shape, 0, no_y, coef, None, 0), 'coef without y')
    odd_c = _grad_job(C, dt, shape, 0, inp, None, None, 0)
    odd_c.fields['c'] = Cc = R.VEC[dt] * 3 // 2          # 6 / 12 channels
    odd_c.capi = None
    _refused(C, ops, odd_c, 'C = {}'.format(Cc))
    print('grad_term {}: {} lattice cases bit-equal'.format(dt, n + 3))


def _grad_table(C, ops, dt):
    """five jobs of different shapes, shifts and forms (one of one block) as one launch of grad_term_table_kernel"""
    jobs = []
    for k, (shape, sh, relu, with_coef, accumulate, two) in enumerate((
            (R.GRAD_SHAPE, 2, 1, True, True, False), ((1, 2, 2, 1), 4, 0, False, False, False),
            ((3, 5, 7, 12), 0, 0, True, False, True), ((2, 32, 32, 12), 1, 1, True, True, False),
            ((1, 2, 2, 12), 3, 1, False, True, False))):
        Cc = shape[3] * R.VEC[dt]
        inp = R.grad_inputs(shape, sh, dt, False, k % 2 == 0, relu, True, 51, k)
        coef = G.real((3, Cc), 52, k) if with_coef else None
        acc = R.real(inp['y'].shape, dt, 53, k) if accumulate else None
        jobs.append(_grad_job(C, dt, shape, sh, inp, coef, acc, relu,
                              dst2=(R.real(inp['y'].shape, dt, 54, k),) if two else None))
    alone = [_alone(C, ops, j, 'grad_term job {}'.format(k)) for k, j in enumerate(jobs)]
    _table(C, ops, DT[dt], jobs, alone, 'grad_term table {}'.format(dt))


@pytest.mark.parametrize('dt', DTYPE_IDS)
@spawned
def test_grad_term_real_values_and_grid_stride_turns(dt):
    """the same configurations on real values, and 2 x 128 x 128 x 160 / 320 at shift 1 (1.31 M vectors: more than
    one turn); then five jobs as one table launch.
    Worst error / bound: 0.420 (f32), 0.996 (bf16) on an MI355X"""
    C, ops = _C()
    key = 'grad_term real ' + dt
    _grad_cases(C, ops, dt, False, key)
    shape, Cc = R.BIG, R.BIG[3] * R.VEC[dt]
    inp = R.grad_inputs(shape, 1, dt, False, True, 1, True, 41)
    coef, acc = G.real((3, Cc), 42), R.real(inp['y'].shape, dt, 43)
    ref, tot, near, _, _ = _grad_ref(inp, 1, 1, coef, acc)
    name = 'grad_term real {} {} sh 1'.format(dt, shape)
    got = _both_ways(C, ops, _grad_job(C, dt, shape, 1, inp, coef, acc, 1), name)[0]
    R.check_elem(key, name, got.reshape(ref.shape), ref, tot, R.grad_adds(1, True, True), dt == 'bf16', skip=near)
    _grad_table(C, ops, dt)
    R.report(key)


@pytest.mark.parametrize('dt,cv', [('f32', 12), ('bf16', 12), ('f32', 2)])
@spawned
def test_grad_term_at_the_rows_boundary(dt, cv):
    """the smallest tensor grad_term hands to grad_term_rows_kernel (4 * 4096 * 256 vectors) and the same data one
    pixel short, which grad_term_kernel takes: both the bits of one float64 reference on the lattice, with coef, mask,
    inner ReLU and accumulate (as an op), and as the two-destination form (through hrnet_grad_term2). The tensors are
    64 MiB each, so a case runs the two-destination form once per side: accumulate2 = 1 on the rows kernel and 0 on
    the plain one in the f32 cases, the other way round in the bf16 case - over the three cases either kernel sees
    both"""
    C, ops = _C()
    dtype = DT[dt]
    npix = R.rows_boundary_pixels(cv)
    assert (npix - 1) * cv < R.ROWS_KERNEL_VECTORS <= npix * cv
    Cc = cv * R.VEC[dt]
    # the data repeat with a period of BOUNDARY_PERIOD pixels (a prime: no stride of either kernel divides it), so the
    # float64 reference is formed on one period and laid out the same way
    period = R.BOUNDARY_PERIOD
    tile = R.reduce_inputs((1, 1, period, cv), 0, dt, True, True, True, 45, cv)
    coef = R.lattice_coef(Cc, 46)
    acc_t, old2_t = R.lattice((1, 1, period, Cc), 47), R.lattice((1, 1, period, Cc), 48)
    ref, tot, _, _, _ = _grad_ref(tile, 0, 1, coef, acc_t)
    assert R.lattice_exact(tot)
    ref2, tot2, _, d2, _ = _grad_ref(dict(tile, scale=None, shift=None), 0, 0, coef, None)

    def lay(a):
        return np.ascontiguousarray(np.tile(a, (1, 1, -(-npix // period), 1))[:, :, :npix])
    inp = dict(tile, **{k: lay(tile[k]) for k in ('g', 'mask', 'y')})
    acc, old2 = lay(acc_t), lay(old2_t)
    want, want2 = lay(R.stored_bits(ref, dt)), lay(R.stored_bits(ref2, dt))
    want_d = [lay(R.stored_bits(d2, dt)), lay(R.stored_bits(d2 + old2_t, dt))]
    # one upload: the shorter tensor is the first npix - 1 pixels of the same memory
    dev = dict(inp, **{k: _dev(inp[k], dtype) for k in ('g', 'mask', 'y')})
    dev2 = dict(dev, scale=None, shift=None)
    for side, pixels in enumerate((npix, npix - 1)):
        shape = (1, 1, pixels, cv)
        name = 'grad_term {} cv {} at {} pixels'.format(dt, cv, pixels)
        got = _alone(C, ops, _grad_job(C, dt, shape, 0, dev, coef, acc[:, :, :pixels], 1), name)[0]
        assert G.same_bits(got, want[:, :, :pixels].reshape(-1)), name
        k = (1 - side) if dt == 'f32' else side          # accumulate2 of this side
        o2 = old2[:, :, :pixels] if k else None
        got = _alone(C, ops, _grad_job(C, dt, shape, 0, dev2, coef, None, 0, dst2=(o2,)), name + ' two dst', capi=True)
        assert G.same_bits(got[0], want2[:, :, :pixels].reshape(-1)), name + ' dst'
        assert G.same_bits(got[1], want_d[k][:, :, :pixels].reshape(-1)), name + ' dst2'
        print('{}: bit-equal (accumulate2 {})'.format(name, k))


# ---- bn_bwd_reduce ----------------------------------------------------------------------------------------------------------

def _reduce_job(C, dt, shape, sh, inp, inner_relu, store):
    dtype, (N, H, W, cv) = DT[dt], shape
    Cc = cv * R.VEC[dt]
    t = {k: (None if inp.get(k) is None else _dev(inp[k], dtype if k in ('g', 'mask', 'y') else F32))
         for k in ('g', 'mask', 'y', 'scale', 'shift')}
    blocks = C.call('hrnet_reduce_blocks', N, H, W, Cc)
    assert blocks == R.reduce_blocks(N * H * W)
    fields = dict(dtype=C.dtype_id(dtype), n=N, h=H, w=W, c=Cc, sh=sh, inner_relu=inner_relu,
                  **{k: _p(v) for k, v in t.items()})
    outs = [('partials', None, blocks * 2 * Cc, F32, None)]
    if store:
        outs.append(('dz', None, N * H * W * Cc, dtype, None))

    def capi(gs):
        C.call('hrnet_bn_bwd_reduce', C.dtype_id(dtype), gs[0].ptr(), _p(t['g']), _p(t['mask']), _p(t['y']),
               _p(t['scale']), _p(t['shift']), N, H, W, Cc, sh, inner_relu, C.stream_ptr())
    return Job(C.OP_BN_BWD_REDUCE, fields, outs, (N, H, W, Cc), [t], capi=None if store else capi)


def _check_reduce(C, ops, dt, shape, sh, inp, inner_relu, lattice, key, name):
    """both forms (with and without the dz store), the stored dz against grad_term with coef NULL bit for bit, the
    partial rows against the float64 sums -> (job without store, job with store, outputs of both)"""
    N, H, W, cv = shape
    Cc, vec, npix = cv * R.VEC[dt], R.VEC[dt], N * H * W
    blocks, rows = R.reduce_geometry(npix, Cc, vec)
    D = R.reduce_D(npix, Cc, vec, sh)
    d, a, near = R.dz(inp['g'], inp['mask'], inp['y'], inp['scale'], inp['shift'], sh, inner_relu)
    plain = _reduce_job(C, dt, shape, sh, inp, inner_relu, False)
    keep = _reduce_job(C, dt, shape, sh, inp, inner_relu, True)
    out_plain = _both_ways(C, ops, plain, name)
    out_keep = _alone(C, ops, keep, name + ' dz')
    rows_plain, rows_keep = out_plain[0].reshape(blocks, 2, Cc), out_keep[0].reshape(blocks, 2, Cc)
    got_dz = out_keep[1].reshape(d.shape)
    apply_ = _alone(C, ops, _grad_job(C, dt, shape, sh, inp, None, None, inner_relu), name + ' grad_term', capi=True)
    assert G.same_bits(out_keep[1], apply_[0]), name + ': the stored dz is not what grad_term computes'
    if blocks * rows >= npix + rows:                     # a workgroup with no pixel stores zeros
        assert not rows_plain[-1].any() and not rows_keep[-1].any(), name + ': rows of an empty workgroup'
    y = inp['y']
    if lattice:
        s, sa = R.row_sums(d, y)
        assert R.lattice_exact(sa, 2.0 ** -8) and R.lattice_exact(a)
        assert G.same_bits(got_dz, R.stored_bits(d, dt)), name + ' dz'
        assert (rows_plain.astype(np.float64).sum(axis=0) == s).all(), name + ' rows'
        s, _ = R.row_sums(R.stored_bits(d, dt), y)       # (the sums of the stored, once-rounded values)
        assert (rows_keep.astype(np.float64).sum(axis=0) == s).all(), name + ' rows of the stored dz'
    else:
        assert near is None or not near.any(), name      # (one-sign data: no decision near 0)
        R.check_elem(key, name + ' dz', got_dz, d, a, (1 << sh) ** 2, dt == 'bf16')
        s, sa = R.row_sums(d, y)
        live = np.abs(inp['g']).min()
        assert R.share_ok(D, sa, [[live], [live * np.abs(y).min()]]), name + ': the bound does not see one pixel'
        R.check_rows(key, name + ' rows', rows_plain, s, sa, D)
        s, sa = R.row_sums(got_dz, y)
        R.check_rows(key, name + ' rows of the stored dz', rows_keep, s, sa, D)
    return plain, keep, out_plain, out_keep


def _reduce_table(C, ops, dt):
    """five jobs (with and without the dz store, one of one block) as one launch of bn_bwd_reduce_table_kernel"""
    jobs, alone = [], []
    for k, (shape, sh, with_mask, inner_relu, store) in enumerate((
            ((3, 5, 7, 12), 1, True, 1, True), ((1, 1, 1, 1), 3, True, 0, False), ((1, 8, 16, 1), 0, False, 1, True),
            ((2, 8, 8, 256), 0, True, 0, True), ((2, 16, 24, 12), 1, True, 1, False))):
        inp = R.reduce_inputs(shape, sh, dt, False, with_mask, inner_relu, 63, k)
        jobs.append(_reduce_job(C, dt, shape, sh, inp, inner_relu, store))
        alone.append(_alone(C, ops, jobs[-1], 'bn_bwd_reduce job {}'.format(k)))
    _table(C, ops, DT[dt], jobs, alone, 'bn_bwd_reduce table {}'.format(dt))


@pytest.mark.parametrize('dt', DTYPE_IDS)
@spawned
def test_bn_bwd_reduce_over_shapes_shifts_masks_and_the_dz_store(dt):
    """one pixel, a second workgroup with an empty range (its rows are zeros), 5 x 7 at 12 vectors, 256 vectors
    (rows = 1); shifts 0, 1, 3; inner ReLU and mask both ways; lattice (bits) and one-sign real values (bounds); one
    vector more than 256 refused; then five jobs as one table launch.
    Worst error / bound: 0.387 (f32), 0.996 (bf16) on an MI355X"""
    C, ops = _C()
    key = 'bn_bwd_reduce ' + dt
    for ci, (shape, sh, with_mask, inner_relu) in enumerate(R.reduce_configs()):
        for lattice in (True, False):
            if lattice and shape[3] == 256 and sh > 0:
                continue
            inp = R.reduce_inputs(shape, sh, dt, lattice, with_mask, inner_relu, 61, ci)
            name = 'bn_bwd_reduce {} {} {} sh {} mask {} relu {}'.format(dt, 'lattice' if lattice else 'real', shape, sh,
                                                                      int(with_mask), inner_relu)
            _check_reduce(C, ops, dt, shape, sh, inp, inner_relu, lattice, key, name)
    wide = (1, 2, 2, 257)                                # 1028 / 2056 channels
    inp = R.reduce_inputs(wide, 0, dt, True, False, 0, 62)
    _refused(C, ops, _reduce_job(C, dt, wide, 0, inp, 0, False), 'bn_bwd_reduce 257 vectors')
    _refused(C, ops, _reduce_job(C, dt, wide, 0, inp, 0, True), 'bn_bwd_reduce 257 vectors, dz store')
    _reduce_table(C, ops, dt)
    R.report(key)


# ---- pool_reduce --------------------------------------------------------------------------------------------------------------

def _pool_job(C, dt, shape, nlev, inp, null_level=None):
    dtype, (N, H, W, cv) = DT[dt], shape
    Cc = cv * R.VEC[dt]
    g, mask = _dev(inp['g'], dtype), None if inp['mask'] is None else _dev(inp['mask'], dtype)
    ys = [_dev(y, dtype) for y in inp['ys']]
    blocks = C.call('hrnet_reduce_blocks', N, H >> 1, W >> 1, Cc)
    fields = dict(dtype=C.dtype_id(dtype), n=N, h=H, w=W, c=Cc, nlev=nlev, g=_p(g), mask=_p(mask),
                  y=[None if l == null_level else _p(y) for l, y in enumerate(ys)])
    outs = []
    for l in range(nlev):
        outs.append(('dz', l, N * (H >> (l + 1)) * (W >> (l + 1)) * Cc, dtype, None))
        outs.append(('partials', l, blocks * 2 * Cc, F32, None))
    return Job(C.OP_POOL_REDUCE, fields, outs, (N, H >> 1, W >> 1, Cc), [g, mask, ys])


@pytest.mark.parametrize('dt', DTYPE_IDS)
@spawned
def test_pool_reduce_every_level_against_pooling_and_bn_bwd_reduce(dt):
    """nlev 1, 2, 3 at 8 and 12 vectors (rows 32 / 21, 20, 16) and 16 vectors with nlev 3 (one coarsest block per
    step), with and without a mask: every level's dz and rows against the float64 pooling of the masked gradient, and
    on the lattice against bn_bwd_reduce at sh = level bit for bit; then the jobs as one table launch. Worst error /
    bound: 0.391 (f32), 0.996 (bf16) on an MI355X"""
    C, ops = _C()
    key = 'pool_reduce ' + dt
    vec = R.VEC[dt]
    jobs, alone = [], []
    for ci, (shape, levels) in enumerate(R.POOL_CASES):
        N, H, W, cv = shape
        Cc = cv * vec
        n1 = N * (H >> 1) * (W >> 1)
        for nlev in levels:
            for lattice, with_mask in ((True, True), (False, True), (False, False)):
                inp = R.pool_inputs(shape, nlev, dt, lattice, with_mask, 71, ci, nlev)
                name = 'pool_reduce {} {} {} nlev {} mask {}'.format(dt, 'lattice' if lattice else 'real', shape, nlev,
                                                                    int(with_mask))
                job = _pool_job(C, dt, shape, nlev, inp)
                out = _alone(C, ops, job, name)
                blocks, _ = R.pool_geometry(n1, Cc, vec, nlev)
                for l in range(1, nlev + 1):
                    y = inp['ys'][l - 1]
                    d, a, _ = R.dz(inp['g'], inp['mask'], None, None, None, l, 0)
                    got_dz, rows = out[2 * l - 2].reshape(d.shape), out[2 * l - 1].reshape(blocks, 2, Cc)
                    D = R.pool_D(n1, Cc, vec, nlev, l)
                    if lattice:
                        assert R.lattice_exact(a) and R.lattice_exact(R.row_sums(d, y)[1], 2.0 ** -8)
                        assert G.same_bits(got_dz, R.stored_bits(d, dt)), '{} level {} dz'.format(name, l)
                        s, _ = R.row_sums(R.stored_bits(d, dt), y)
                        assert (rows.astype(np.float64).sum(axis=0) == s).all(), '{} level {} rows'.format(name, l)
                        low = (N, H >> l, W >> l, cv)
                        ref_job = _reduce_job(C, dt, low, l, dict(g=inp['g'], mask=inp['mask'], y=y), 0, True)
                        ref_out = _alone(C, ops, ref_job, name + ' bn_bwd_reduce')
                        assert G.same_bits(out[2 * l - 2], ref_out[1]), '{} level {}: dz of bn_bwd_reduce'.format(name, l)
                        rb = ref_out[0].reshape(-1, 2, Cc).astype(np.float64).sum(axis=0)
                        assert (rows.astype(np.float64).sum(axis=0) == rb).all(), name + ': rows of bn_bwd_reduce'
                    else:
                        R.check_elem(key, '{} level {} dz'.format(name, l), got_dz, d, a, 4 ** l, dt == 'bf16')
                        s, sa = R.row_sums(got_dz, y)
                        share = np.abs(inp['g']).min()
                        assert R.share_ok(D, sa, [[share], [share * np.abs(y).min()]]), name
                        R.check_rows(key, '{} level {} rows'.format(name, l), rows, s, sa, D)
                if not lattice and with_mask and (ci, nlev) in ((0, 1), (1, 2), (2, 3), (3, 3), (0, 3)):
                    jobs.append(job)
                    alone.append(out)
    _table(C, ops, DT[dt], jobs, alone, 'pool_reduce table {}'.format(dt))
    # refused before any launch: an extent that is no multiple of 2^nlev, 64 vectors with three levels, a level
    # without its pointers
    for shape, nlev, null_level in (((1, 8, 12, 8), 3, None), ((1, 6, 8, 8), 2, None), ((1, 8, 8, 64), 3, None),
                                    ((1, 8, 8, 8), 2, 1)):
        inp = R.pool_inputs((1, 8, 8, shape[3]), nlev, dt, True, True, 72)
        _refused(C, ops, _pool_job(C, dt, shape, nlev, inp, null_level), 'pool_reduce {} nlev {}'.format(shape, nlev))
    R.report(key)


# ---- bn_bwd_finalize ------------------------------------------------------------------------------------------------------------

def _finalize_job(C, blocks, Cc, accumulate, case):
    rows, gamma, mean, invstd, count, old = case
    rows_g = Guarded(rows.size, F32, rows)               # (NaN on both sides: a read beyond the rows would show)
    t = [_dev(v) for v in (gamma, mean, invstd)]
    fields = dict(blocks=blocks, c=Cc, accumulate=accumulate, count=count, partials=rows_g.ptr(), gamma=_p(t[0]),
                  save_mean=_p(t[1]), save_invstd=_p(t[2]))
    outs = [('dgamma', None, Cc, F32, old[0] if accumulate else None),
            ('dbeta', None, Cc, F32, old[1] if accumulate else None), ('coef', None, 3 * Cc, F32, None)]

    def capi(gs):
        C.call('hrnet_bn_bwd_finalize', rows_g.ptr(), blocks, Cc, count, _p(t[0]), _p(t[1]), _p(t[2]), gs[0].ptr(),
               gs[1].ptr(), gs[2].ptr(), accumulate, C.stream_ptr())
    return Job(C.OP_BN_BWD_FINALIZE, fields, outs, (1, 1, 1, Cc), [rows_g, t], capi=capi)


def _check_finalize(key, name, out, case, accumulate):
    rows, gamma, mean, invstd, count, old = case
    dg, db, coef = R.finalize(rows, count, gamma, mean, invstd)
    for k, (got, ref) in enumerate(((out[0], dg), (out[1], db))):
        if accumulate:
            R.check_rel(key, name + ' d' + 'gb'[k], got, ref + old[k], np.abs(ref) + np.abs(old[k]), 2 * R.U)
        else:
            R.check_rel(key, name + ' d' + 'gb'[k], got, ref, np.abs(ref), 2 * R.U)
    R.check_rel(key, name + ' coef', out[2].reshape(coef.shape), coef, np.abs(coef), 2 * R.U)


@pytest.mark.parametrize('accumulate', [0, 1])
@spawned
def test_bn_bwd_finalize_at_the_ends_of_its_loops(accumulate):
    """synthetic rows of 1, 31, 32, 33, 63, 64, 65 and 2048 blocks (the ends of the unrolled 32-lane loop of
    partial_sums) by 1, 32, 33, 48 and 480 channels: every output finite and the f32 rounding of the float64 formula,
    the rows unchanged, and the sentinels behind dgamma, dbeta and each third of coef - the elements a thread of a
    channel >= C would own (C = 1, 33, 48 and 480 leave such threads in the last workgroup) - untouched. The rows lie
    between NaN sentinels, so a read past the last row would show in an output of the last channels; a read of a
    channel >= C inside the rows is valid memory and cannot show, since only a thread of a channel < C stores. Then
    five of the cases as one table launch. Worst error / bound: 0.498 (accumulate 0), 0.882 (accumulate 1) on an
    MI355X"""
    C, ops = _C()
    key = 'bn_bwd_finalize accumulate {}'.format(accumulate)
    jobs, alone = [], []
    for blocks in R.FIN_BLOCKS:
        for Cc in R.FIN_C:
            case = R.finalize_case(blocks, Cc, accumulate)
            job = _finalize_job(C, blocks, Cc, accumulate, case)
            name = 'bn_bwd_finalize blocks {} C {} accumulate {}'.format(blocks, Cc, accumulate)
            out = _both_ways(C, ops, job, name)
            assert G.same_bits(job.keep[0].t.cpu().numpy(), case[0].reshape(-1)), name + ': the rows were written'
            _check_finalize(key, name, out, case, accumulate)
            if (blocks, Cc) in ((1, 1), (33, 48), (65, 33), (2048, 480), (31, 32)):
                jobs.append(job)
                alone.append(out)
    _table(C, ops, F32, jobs, alone, 'bn_bwd_finalize table accumulate {}'.format(accumulate))
    gs = _finalize_job(C, 4, 8, 0, R.finalize_case(4, 8, 9))
    gs.fields['gamma'] = None
    gs.capi = None
    _refused(C, ops, gs, 'bn_bwd_finalize without gamma')
    R.report(key)


# ---- reduce, finalize, apply ---------------------------------------------------------------------------------------------------

def _autograd(ident, y, gamma, beta, gout, sh, eps):
    """float64 autograd of relu(ident + up(bn(y))) in NCHW -> (out, dy, dgamma, dbeta, mean, invstd) as NHWC / [C]"""
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    nchw = lambda a: t(a).permute(0, 3, 1, 2).contiguous()
    yt, gt, bt = nchw(y).requires_grad_(True), t(gamma).requires_grad_(True), t(beta).requires_grad_(True)
    z = F.batch_norm(yt, None, None, gt, bt, True, 0.0, eps)
    if sh:
        z = F.interpolate(z, scale_factor=1 << sh, mode='nearest')
    out = torch.relu(nchw(ident) + z)
    out.backward(nchw(gout))
    mean = yt.detach().mean(dim=(0, 2, 3))
    var = yt.detach().var(dim=(0, 2, 3), unbiased=False)
    nhwc = lambda a: a.detach().permute(0, 2, 3, 1).contiguous().numpy()
    return nhwc(out), nhwc(yt.grad), gt.grad.numpy(), bt.grad.numpy(), mean.numpy(), (1.0 / torch.sqrt(var + eps)).numpy()


@pytest.mark.parametrize('dt', DTYPE_IDS)
@spawned
def test_reduce_finalize_apply_against_float64_autograd(dt):
    """dy, dgamma and dbeta of relu(ident + up(bn(y))) at 3 x 5 x 7 and 2 x 8 x 24 (shift 0 and 3) with 12 vectors and
    at 1 x 2 x 2 with one vector (shift 1: the one-block job of each of the three tables),
    as three launches and as three table launches (the bits of the launches), against float64 autograd under the
    bounds of the three passes composed (below). Worst error / bound: 0.055 (f32), 0.602 (bf16) on an MI355X"""
    C, ops = _C()
    key = 'reduce, finalize, apply ' + dt
    dtype, vec, bf16, eps, u = DT[dt], R.VEC[dt], dt == 'bf16', 1e-5, R.U
    chains = []
    for ci, (shape, sh) in enumerate(R.E2E_CASES):
        N, H, W, cv = shape
        Cc, npix, f2 = cv * vec, N * H * W, (1 << sh) ** 2
        y = R.one_sign((N, H, W, Cc), dt, 81, ci) + R.real((N, H, W, Cc), dt, 82, ci) * np.float32(0.25)
        y = R.np_dtype_round(y, dt)
        gamma, beta = (0.5 + G.rng(83, ci).random_sample(Cc)).astype(np.float32), G.real((Cc,), 84, ci)
        hi = (N, H << sh, W << sh, Cc)
        ident, gout = R.real(hi, dt, 85, ci), R.one_sign(hi, dt, 86, ci)
        out64, dy, dgam, dbet, mean, invstd = _autograd(ident, y, gamma, beta, gout, sh, eps)
        out = R.np_dtype_round(out64.astype(np.float32), dt)             # the mask as the forward pass stored it
        assert ((out > 0) == (out64 > 0)).all()
        mean32, invstd32 = mean.astype(np.float32), invstd.astype(np.float32)
        inp = dict(g=gout, mask=out, y=y, scale=None, shift=None)
        blocks = R.reduce_blocks(npix)
        reduce_ = _reduce_job(C, dt, shape, sh, inp, 0, True)
        r_out = _alone(C, ops, reduce_, 'chain reduce')
        rows, dz_dev = r_out[0].reshape(blocks, 2, Cc), r_out[1].reshape(N, H, W, Cc)
        case = (rows, gamma, mean32, invstd32, float(npix), np.zeros((2, Cc), np.float32))
        fin = _finalize_job(C, blocks, Cc, 0, case)
        f_out = _alone(C, ops, fin, 'chain finalize')
        coef_dev = f_out[2].reshape(3, Cc)
        app = _grad_job(C, dt, shape, 0, dict(g=dz_dev, mask=None, y=y), coef_dev, None, 0)
        a_out = _alone(C, ops, app, 'chain apply')
        chains.append((reduce_, fin, app, r_out, f_out, a_out))
        # ---- the bounds composed. dz: (f2 + 1) u sum |g| per element, then its rounding to storage (ddz)
        d, a, _ = R.dz(gout, out, None, None, None, sh, 0)
        ddz = (f2 + 1) * u * a
        if bf16:
            ddz = G.rounding_allowance(d, ddz)
        s, sa = R.row_sums(d, y)
        D = R.reduce_D(npix, Cc, vec, sh)
        # the two sums: what dz is off by, and the f32 summation of the rows
        b1 = ddz.reshape(-1, Cc).sum(axis=0) + R.rows_bound(D, sa[0] + ddz.reshape(-1, Cc).sum(axis=0))
        dzy = (ddz * np.abs(y)).reshape(-1, Cc).sum(axis=0)
        b2 = dzy + R.rows_bound(D, sa[1] + dzy)
        r, mu, g_ = invstd, mean, gamma.astype(np.float64)
        # dgamma = r (s2 - mu s1): the sums' bounds, u on mu and r as the device is given them, 2 u for the result
        mag = r * (np.abs(s[1]) + np.abs(mu * s[0]))
        t_dg = r * (b2 + np.abs(mu) * b1) + 4 * u * mag
        t_db = b1 + 2 * u * np.abs(s[0])
        R.check_rel(key, 'chain {} {} sh {} dgamma'.format(dt, shape, sh), f_out[0], dgam, t_dg, 1.0)
        R.check_rel(key, 'chain {} {} sh {} dbeta'.format(dt, shape, sh), f_out[1], dbet, t_db, 1.0)
        # dy = A dz + B y + Cc with A = g r, B = -g r^2 dgamma / n, Cc = -g r dbeta / n + g r^2 mu dgamma / n
        A = g_ * r
        B = -g_ * r * r * dgam / npix
        c1, c2 = g_ * r * dbet / npix, g_ * r * r * mu * dgam / npix
        dA = 3 * u * np.abs(A)
        dB = g_ * r * r * t_dg / npix + 4 * u * np.abs(B)
        dC = g_ * r * t_db / npix + g_ * r * r * np.abs(mu) * t_dg / npix + 6 * u * (np.abs(c1) + np.abs(c2))
        tot = np.abs(A) * np.abs(d) + np.abs(B * y) + np.abs(c2 - c1)
        b32 = 4 * u * tot + np.abs(A) * ddz + dA * np.abs(d) + dB * np.abs(y) + dC
        allow = G.rounding_allowance(dy, b32) if bf16 else b32
        R.check_rel(key, 'chain {} {} sh {} dy'.format(dt, shape, sh), a_out[0].reshape(dy.shape), dy, allow, 1.0)
    for k, what in enumerate(('reduce', 'finalize', 'apply')):
        _table(C, ops, F32 if k == 1 else dtype, [c[k] for c in chains], [c[3 + k] for c in chains],
               'chain {} table {}'.format(what, dt))
    R.report(key)
