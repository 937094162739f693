"""tests/plan_fingerprint.py on hand-made programs over CPU tensors: the digest follows what a program does and
nothing else. No library call, no GPU."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import plan_fingerprint as F
from hipnet import _capi as C
from hipnet import ops

_alive = []      # every fake plan stays allocated, so that the next one gets other addresses


def _u8(n):
    return torch.zeros(n, dtype=torch.uint8)


def _plan(anon_order=(0, 1), edit=None, stray=None):
    """a two-op forward program and a five-op backward program over two activations, one conv, one BatchNorm, two
    anonymous buffers and a job table. edit(names) may change the ops before the table is uploaded."""
    module = torch.nn.Sequential(torch.nn.Conv2d(8, 8, 1, bias=False), torch.nn.BatchNorm2d(8))
    grads = {id(p): torch.zeros_like(p) for p in module.parameters()}
    net = SimpleNamespace(module=module, grad_of=lambda p: grads[id(p)],
                          convs={'0': SimpleNamespace(wf=_u8(128), wd=_u8(128))})
    acts = [SimpleNamespace(t=_u8(512), g=_u8(512)) for _ in range(2)]
    bn = SimpleNamespace(sums=None, **{k: torch.zeros(8) for k in ('scale', 'shift', 'mean', 'invstd', 'coef')})
    anon = [None, None]
    for k in anon_order:                      # allocation order = list order of plan.keep
        anon[k] = torch.zeros(64 + 32 * k)
    keep = [anon[k] for k in anon_order]
    gamma, beta = module[1].weight, module[1].bias
    ref = C.HrBnBwdRef()
    ref.rows, ref.gamma, ref.dgamma, ref.dbeta = C.ptr(anon[1]), C.ptr(gamma), C.ptr(grads[id(gamma)]), C.ptr(grads[id(beta)])
    ref.save_mean, ref.save_invstd, ref.count, ref.nrows, ref.accumulate = C.ptr(bn.mean), C.ptr(bn.invstd), 64.0, 3, 1
    n = dict(
        conv=ops.make(C.OP_CONV, dtype=1, n=2, h=4, w=4, cin=8, ho=4, wo=4, cout=8, ks=1, stride=1, x=C.ptr(acts[0].t),
                      wgt=C.ptr(net.convs['0'].wf), y=C.ptr(acts[1].t), stats=C.ptr(anon[0])),
        job0=ops.make(C.OP_GRAD_TERM, dtype=1, n=2, h=4, w=4, c=8, dst=C.ptr(acts[0].g), g=C.ptr(acts[1].g)),
        job1=ops.make(C.OP_GRAD_TERM, dtype=1, n=2, h=4, w=4, c=8, dst=C.ptr(acts[1].g), g=C.ptr(acts[0].g),
                      mask=C.ptr(acts[1].t)),
        term=ops.make(C.OP_GRAD_TERM, dtype=1, n=2, h=4, w=4, c=8, dst=C.ptr(acts[0].g), g=C.ptr(acts[1].g),
                      scale=C.ptr(bn.scale), shift=C.ptr(bn.shift)),
        fin=ops.make(C.OP_BN_BWD_FINALIZE, blocks=3, c=8, accumulate=1, count=32.0, partials=C.ptr(anon[1]) + 16,
                     gamma=C.ptr(gamma), save_mean=C.ptr(bn.mean), save_invstd=C.ptr(bn.invstd),
                     dgamma=C.ptr(grads[id(gamma)]), dbeta=C.ptr(grads[id(beta)]), coef=C.ptr(bn.coef)),
        rec=ops.make(C.OP_EVENT_RECORD, event=0x7f0000001000 + 64 * len(_alive)),
        fused=ops.make(C.OP_BWD_FUSED, dtype=1, n=2, h=4, w=4, cin=8, cout=8, dz=C.ptr(acts[1].g), y=C.ptr(acts[1].t),
                       x=C.ptr(acts[0].t), wt=C.ptr(net.convs['0'].wd), dx=C.ptr(acts[0].g),
                       slabs=C.ptr(grads[id(module[0].weight)]), bnref=ctypes.addressof(ref)),
    )
    if stray is not None:
        n['term'].p[ops.slot(C.OP_GRAD_TERM, 'p', 'mask')] = C.ptr(stray)
    if edit is not None:
        edit(n, acts)
    for k, job in enumerate((n['job0'], n['job1'])):
        ops.set_job_blocks(job, 2 * k, 2)
    arr = (C.HrOp * 2)(n['job0'], n['job1'])
    table = torch.frombuffer(bytearray(ctypes.string_at(ctypes.addressof(arr), ctypes.sizeof(arr))), dtype=torch.uint8)
    keep.append(table)
    n['table'] = ops.make(C.OP_EW_TABLE, jobs=2, blocks=4, kind=C.OP_GRAD_TERM, dtype=1, table=C.ptr(table))
    n['fin'].i[C.LANE_SLOT] = 1
    plan = SimpleNamespace(net=net, acts=acts, keep=keep, bns={'1': bn}, _bnrefs=[ref], bucket_marks=[(2, '0')],
                           fwd=SimpleNamespace(ops=[n['conv'], n['table']], tags={0: '0'}),
                           bwd=SimpleNamespace(ops=[n['term'], n['fin'], n['rec'], n['fused'], n['table']], tags={}),
                           n_jobs=2)
    _alive.append(plan)
    return plan


def _digests(plan):
    fp = F.fingerprint(plan)
    return fp['fwd']['sha256'], fp['bwd']['sha256']


@pytest.fixture(scope='module')
def base():
    return _digests(_plan())


def test_text_names_what_every_pointer_points_at():
    fp = F.fingerprint(_plan())
    fwd, bwd = fp['fwd']['text'], fp['bwd']['text']
    assert 'act0.t+0 wf:0+0' in fwd and 'anon0:256+0' in fwd and 'tag=0' in fwd
    assert fwd.count('\n  job kind={}'.format(C.OP_GRAD_TERM)) == 2 and 'act1.g+0 act0.g+0 act1.t+0' in fwd
    assert 'anon1:384+16 param:1.weight+0 bn:1.mean+0 bn:1.invstd+0 grad:1.weight+0 grad:1.bias+0 bn:1.coef+0' in bwd
    assert 'op lane=1 kind={}'.format(C.OP_BN_BWD_FINALIZE) in bwd and ' p=ev0 0 ' in bwd
    assert 'bnref{rows=anon1:384+0 gamma=param:1.weight+0' in bwd and 'nrows=3 accumulate=1' in bwd
    assert 'wd:0+0' in bwd and 'grad:0.weight+0' in bwd
    assert fp['fwd']['ops'] == 2 and fp['fwd']['kinds'] == {str(C.OP_CONV): 1, str(C.OP_EW_TABLE): 1}
    assert fp['side']['bucket_marks'] == [[2, '0']] and fp['side']['counters'] == {'n_jobs': 2}


def test_digest_ignores_addresses_and_allocation_order(base):
    assert _digests(_plan()) == base                          # every tensor at another address
    assert _digests(_plan(anon_order=(1, 0))) == base         # the anonymous buffers allocated the other way round


def _swap_named(n, acts):
    g = ops.slot(C.OP_GRAD_TERM, 'p', 'g')
    n['term'].p[g], n['conv'].p[ops.slot(C.OP_CONV, 'p', 'x')] = C.ptr(acts[0].t), C.ptr(acts[1].g)


def _int_slot(n, acts):
    n['term'].i[ops.slot(C.OP_GRAD_TERM, 'i', 'accumulate')] = 1


def _lane(n, acts):
    n['term'].i[C.LANE_SLOT] = 2


def _offset(n, acts):
    n['term'].p[ops.slot(C.OP_GRAD_TERM, 'p', 'dst')] += 64


def _float_slot(n, acts):
    n['fin'].f[ops.slot(C.OP_BN_BWD_FINALIZE, 'f', 'count')] = 32.000004


def _job(n, acts):
    n['job1'].p[ops.slot(C.OP_GRAD_TERM, 'p', 'mask')] = C.ptr(acts[0].t)


def _job_int(n, acts):
    n['job0'].i[ops.slot(C.OP_GRAD_TERM, 'i', 'sh')] = 1


@pytest.mark.parametrize('edit,progs', [(_swap_named, 'fb'), (_int_slot, 'b'), (_lane, 'b'), (_offset, 'b'),
                                        (_float_slot, 'b'), (_job, 'fb'), (_job_int, 'fb')])
def test_digest_follows_a_changed_slot(base, edit, progs):
    got = _digests(_plan(edit=edit))
    assert (got[0] != base[0]) == ('f' in progs) and (got[1] != base[1]) == ('b' in progs)


def test_bnref_contents_are_part_of_the_digest(base):
    plan = _plan()
    plan._bnrefs[0].nrows = 4
    assert _digests(plan)[1] != base[1] and _digests(plan)[0] == base[0]


def test_unresolved_pointer_raises():
    with pytest.raises(F.Unresolved):
        F.fingerprint(_plan(stray=torch.zeros(16)))           # a live tensor the plan does not hold
    plan = _plan()
    plan._bnrefs = []
    with pytest.raises(F.Unresolved):
        F.fingerprint(plan)
