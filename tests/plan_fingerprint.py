"""Fingerprint of a recorded hipnet.engine.Plan: its two programs as canonical text, and that text's digest.

A recorded program is a list of HrOp whose pointer slots hold device addresses; two recordings of the same plan
differ in every address and in nothing else. canonical text replaces each pointer by WHAT it points at:

  act<k>.t / act<k>.g              storage / gradient of plan.acts[k]
  param:<name> / grad:<name>       a parameter of the module (state_dict name) / its slice of the flat gradient
  bn:<prefix>.<field>              scale, shift, mean, invstd, coef, sums of the plan's BatchNorm record
  run:<name>                       a buffer of the module (running_mean, running_var, num_batches_tracked)
  wf:<prefix> / wd:<prefix>        packed forward / dgrad weights of a convolution
  biaspad:<prefix>, headwf:<j>     the net's padded biases and the head's packed column slices
  anon<k>:<bytes>                  any other tensor of plan.keep (scratch, rows, slabs), numbered by first appearance
                                   in the walk - forward program, then backward, op by op, slot by slot
  ev<k>                            an event handle, numbered the same way

each followed by `+<byte offset>`. Device tables (the jobs of OP_EW_TABLE, the rows of OP_BN_FINALIZE_TABLE and
OP_WGRAD_REDUCE_TABLE) and the host HrBnBwdRef behind a `bnref` slot are decoded and written out the same way. A
non-null pointer that is none of these raises Unresolved.

It reads the programs, plan.acts / keep / bns / _bnrefs, the side data (marks, cuts, counters, tags) and the net's
parameters, buffers and packed weights - never the tape the programs were recorded from.

The second half records the configurations tests/test_plan_fingerprint_gpu.py holds against
tests/plan_fingerprints.json. `python tests/plan_fingerprint.py OUT.json` records them (two child processes) and
writes such a file: run it on the commit whose programs are the reference.
"""
import bisect
import ctypes
import hashlib
import json
import os
import struct
import sys

_TESTS = os.path.dirname(os.path.abspath(__file__))
for _p in (_TESTS, os.path.dirname(_TESTS), os.path.join(os.path.dirname(_TESTS), 'hrnet-hand-pose-estimation_amd', 'lib')):
    if _p not in sys.path:
        sys.path.insert(0, _p)          # (run as a script; under pytest tests/conftest.py has done this)

from hipnet import _capi as C           # noqa: E402
from hipnet import ops             # noqa: E402


class Unresolved(LookupError):
    """a recorded pointer that is no tensor the plan or its net knows"""


def _nbytes(t):
    return t.numel() * t.element_size()


def _f32_hex(v):
    return '%08x' % struct.unpack('I', struct.pack('f', v))[0]


class _Ranges(object):
    """disjoint [lo, hi) address ranges -> payload"""

    def __init__(self, items):
        items = sorted((t.data_ptr(), t.data_ptr() + _nbytes(t), what) for t, what in items if _nbytes(t))
        self.los = [lo for lo, _, _ in items]
        self.items = items

    def find(self, p):
        k = bisect.bisect_right(self.los, p) - 1
        if k >= 0 and p < self.items[k][1]:
            return self.items[k]
        return None


def named_tensors(plan):
    """[(tensor, label)] of every tensor of `plan` and its net that has a name"""
    net = plan.net
    out = []
    for k, a in enumerate(plan.acts):
        out.append((a.t, 'act{}.t'.format(k)))
        if a.g is not None:
            out.append((a.g, 'act{}.g'.format(k)))
    for name, p in net.module.named_parameters():
        out.append((p, 'param:' + name))
        out.append((net.grad_of(p), 'grad:' + name))
    for name, b in net.module.named_buffers():
        out.append((b, 'run:' + name))
    for prefix, b in plan.bns.items():
        for field in ('scale', 'shift', 'mean', 'invstd', 'coef', 'sums'):
            t = getattr(b, field)
            if t is not None:
                out.append((t, 'bn:{}.{}'.format(prefix, field)))
    for prefix, r in net.convs.items():
        for field in ('wf', 'wd'):
            if getattr(r, field) is not None:
                out.append((getattr(r, field), '{}:{}'.format(field, prefix)))
    for prefix, t in getattr(net, 'bias_pad', {}).items():
        out.append((t, 'biaspad:' + prefix))
    for j, t in enumerate(getattr(net, '_head_wf', [])):
        out.append((t, 'headwf:{}'.format(j)))
    return out


_TABLE_ROWS = {C.OP_EW_TABLE: C.HrOp, C.OP_BN_FINALIZE_TABLE: C.HrBnEnt, C.OP_WGRAD_REDUCE_TABLE: C.HrWredEnt}


class Canon(object):
    """the labels of one plan; anonymous tensors and events are numbered as text() meets them"""

    def __init__(self, plan):
        self.named = _Ranges(named_tensors(plan))
        self.keep = _Ranges([(t, t) for t in plan.keep])
        self.bnrefs = {ctypes.addressof(r): r for r in getattr(plan, '_bnrefs', [])}
        self.anon, self.events, self._raw = {}, {}, {}

    def label(self, p):
        if not p:
            return '0'
        hit = self.named.find(p)
        if hit is not None:
            return '{}+{}'.format(hit[2], p - hit[0])
        hit = self.keep.find(p)
        if hit is None:
            raise Unresolved('pointer {:#x} is no tensor of the plan'.format(p))
        k = self.anon.setdefault(hit[0], len(self.anon))
        return 'anon{}:{}+{}'.format(k, hit[1] - hit[0], p - hit[0])

    def _struct(self, s):
        out = []
        for name, ty in s._fields_:
            v = getattr(s, name)
            if ty is ctypes.c_void_p:
                out.append('{}={}'.format(name, self.label(v)))
            elif ty is ctypes.c_float:
                out.append('{}={}'.format(name, _f32_hex(v)))
            else:
                out.append('{}={}'.format(name, int(v)))
        return ' '.join(out)

    def _rows(self, p, n, row_type):
        """`n` structs of `row_type` at device address `p`, inside one of the plan's kept tensors"""
        hit = self.keep.find(p)
        if hit is None:
            raise Unresolved('table pointer {:#x} is no tensor of the plan'.format(p))
        lo, hi, t = hit
        if lo not in self._raw:
            self._raw[lo] = bytes(t.cpu().numpy().tobytes())
        size = n * ctypes.sizeof(row_type)
        if p + size > hi:
            raise Unresolved('table at {:#x}: {} rows run past its tensor'.format(p, n))
        return list((row_type * n).from_buffer_copy(self._raw[lo][p - lo:p - lo + size]))

    def op_lines(self, op, tag=None, job=False):
        kind = int(op.kind)
        slots = ops.SLOTS[kind]['p']
        ptrs, extra = [], []
        for k, v in enumerate(op.p):
            if not v:
                ptrs.append('0')
            elif kind in (C.OP_EVENT_RECORD, C.OP_STREAM_WAIT) and k == slots['EVENT']:
                ptrs.append('ev{}'.format(self.events.setdefault(v, len(self.events))))
            elif kind in _TABLE_ROWS and k == slots['TABLE']:
                ptrs.append('table')
                for row in self._rows(v, int(op.i[0]), _TABLE_ROWS[kind]):
                    extra += (self.op_lines(row, job=True) if kind == C.OP_EW_TABLE else ['  row ' + self._struct(row)])
            elif k == slots.get('BNREF'):
                if v not in self.bnrefs:
                    raise Unresolved('bnref {:#x} is none of the plan\'s host structs'.format(v))
                ptrs.append('bnref{' + self._struct(self.bnrefs[v]) + '}')
            else:
                ptrs.append(self.label(v))
        head = '  job' if job else 'op lane={}'.format(int(op.i[C.LANE_SLOT]))
        line = '{} kind={} i={} f={} p={}'.format(head, kind, ','.join(str(int(v)) for v in op.i),
                                                 ','.join(_f32_hex(v) for v in op.f), ' '.join(ptrs))
        if tag is not None:
            line += ' tag=' + tag
        return [line] + extra

    def text(self, prog):
        lines = []
        for k, op in enumerate(prog.ops):
            lines += self.op_lines(op, tag=prog.tags.get(k))
        return '\n'.join(lines) + '\n'


def fingerprint(plan):
    """{'fwd' | 'bwd': {'text', 'sha256', 'ops', 'kinds'}, 'side': {...}} of a recorded plan"""
    canon = Canon(plan)
    out = {}
    for name in ('fwd', 'bwd'):         # (this order: it numbers the anonymous tensors)
        prog = getattr(plan, name)
        text = canon.text(prog)
        kinds = {}
        for op in prog.ops:
            kinds[str(int(op.kind))] = kinds.get(str(int(op.kind)), 0) + 1
        out[name] = {'text': text, 'sha256': hashlib.sha256(text.encode()).hexdigest(), 'ops': len(prog.ops),
                     'kinds': dict(sorted(kinds.items(), key=lambda kv: int(kv[0])))}
    out['side'] = {
        'bucket_marks': [[int(i), str(p)] for i, p in plan.bucket_marks],
        'late_cuts': [[int(v) for v in cut] for cut in getattr(plan, 'late_cuts', [])],
        'gout_op': getattr(plan, 'gout_op', None), 'inter_gop': getattr(plan, 'inter_gop', None),
        'slab_bytes': getattr(plan, 'slab_bytes', None),
        'counters': {k: int(v) for k, v in sorted(vars(plan).items()) if k.startswith('n_')},
    }
    return out


def summary(fp):
    """what the fixture keeps of a fingerprint: everything but the texts"""
    return {'fwd': {k: v for k, v in fp['fwd'].items() if k != 'text'},
            'bwd': {k: v for k, v in fp['bwd'].items() if k != 'text'}, 'side': fp['side']}


# ---- the recorded configurations -------------------------------------------------------------------------------------
# (name, model, training, environment). Every plan is plan(2, 64, 64, ...): the smallest shape at which all four
# branches exist and N > 1. The order within a process is part of the fixture.
W32 = 'w32_bf16'
CONFIGS = {
    # product switches only: no HRNET_MEASURE
    'product': [
        ('w32_bf16_train', W32, True, {}),
        ('w32_fp32_train', 'w32_fp32', True, {}),
        ('w48_bf16_train', 'w48_bf16', True, {}),
        ('softmax_bf16_train', 'softmax_bf16', True, {}),
        ('w32_bf16_eval', W32, False, {}),
        ('deterministic', W32, True, {'HRNET_DETERMINISTIC': '1'}),
        ('deterministic_wgrad_atomic', W32, True, {'HRNET_DETERMINISTIC': '1', 'HRNET_WGRAD_ATOMIC': '1'}),
        ('dp_plan', W32, True, {'HRNET_DP_PLAN': '1'}),
        ('lanes_0', W32, True, {'HRNET_LANES': '0'}),
    ],
    # HRNET_MEASURE=1 from the start of the process, one measurement switch per plan
    'measure': [(name, W32, True, env) for name, env in [
        ('fused_bwd_0', {'HRNET_FUSED_BWD': '0'}),
        ('fused_pw_0', {'HRNET_FUSED_PW': '0'}),
        ('fused_maxc_32', {'HRNET_FUSED_MAXC': '32'}),
        ('fuse_sum_0', {'HRNET_FUSE_SUM': '0'}),
        ('batch_sumbwd_0', {'HRNET_BATCH_SUMBWD': '0'}),
        ('batch_sumfwd_0', {'HRNET_BATCH_SUMFWD': '0'}),
        ('batch_wred_0', {'HRNET_BATCH_WRED': '0'}),
        ('fuse_bwdstats_0', {'HRNET_FUSE_BWDSTATS': '0'}),
        ('keep_dz_0', {'HRNET_KEEP_DZ': '0'}),
        ('pool_reduce_0', {'HRNET_POOL_REDUCE': '0'}),
        ('head_mix_0', {'HRNET_HEAD_MIX': '0'}),
        ('head_bwd_0', {'HRNET_HEAD_BWD': '0'}),
        ('defer_wgrad_0', {'HRNET_DEFER_WGRAD': '0'}),
        ('offload_wgrad_0', {'HRNET_OFFLOAD_WGRAD': '0'}),
        ('defer_branch_0', {'HRNET_DEFER_BRANCH': '0'}),
        ('bnbwd_inline_0', {'HRNET_BNBWD_INLINE': '0'}),
        ('bs_store_masked_0', {'HRNET_BS_STORE_MASKED': '0'}),
        ('wlane_1', {'HRNET_WLANE': '1'}),
        ('wlane_2', {'HRNET_WLANE': '2'}),
        ('dp_plan_late_groups_0', {'HRNET_DP_PLAN': '1', 'HRNET_LATE_GROUPS': '0'}),
    ]],
}
# the configurations a fixture may lack (with the error the reference commit raised for them, under 'not_recorded')
OPTIONAL = {'lanes_0'} | {c[0] for c in CONFIGS['measure'][6:]}


def _build_model(key):
    import numpy as np
    import torch
    import test_bench_path_gpu as B
    if key == 'w32_bf16':
        return B._model('bf16')[0]
    if key == 'w32_fp32':
        return B._model('fp32')[0]
    if key == 'w48_bf16':
        return B._model('bf16', yaml=B.YAML48)[0]
    # pose_hrnet_softmax (inter_feat = the concat, align_corners head), built the way B._model builds pose_hrnet
    from config import get_cfg_defaults
    from hipnet import synth
    from models import pose_hrnet_softmax
    cfg = get_cfg_defaults()
    cfg.merge_from_file(os.path.join(B.EXP, 'RHD_HRNet_w32_trainable_softmax_pose2dloss_v1.yaml'))
    cfg.MODEL.COMPUTE_DTYPE = 'bf16'
    model = pose_hrnet_softmax.get_pose_net(cfg, is_train=False)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.fill_state_dict(model.state_dict(), 0).items()}
    model.load_state_dict(sd, strict=True)
    return model.cuda()


def record(which, only=None):
    """record the configurations of process `which` in THIS process, in order -> [(name, fingerprint | {'error': ..})].
    Call it first thing in a fresh process: it sets the HRNET_* environment before the library loads."""
    for k in [k for k in os.environ if k.startswith('HRNET_') and k != 'HRNET_HIP_LIB']:
        del os.environ[k]
    if which == 'measure':
        os.environ['HRNET_MEASURE'] = '1'
    models, out = {}, []
    for name, key, training, env in CONFIGS[which]:
        if only is not None and name not in only:
            continue
        if key not in models:
            models[key] = _build_model(key)
        model = models[key]
        net = (model.train() if training else model.eval()).hip()
        net.plans.clear()
        os.environ.update(env)
        try:
            out.append((name, fingerprint(net.plan(2, 64, 64, training, training))))    # recorded, never run
        except Exception as e:                  # noqa: B902 - the reference commit's own error goes into the fixture
            if name not in OPTIONAL:
                raise
            out.append((name, {'error': '{}: {}'.format(type(e).__name__, e)}))
        finally:
            for k in env:
                del os.environ[k]
            net.plans.clear()
    return out


def _record_child(which, queue):
    try:
        queue.put([(name, fp if 'error' in fp else summary(fp)) for name, fp in record(which)])
    except BaseException:                       # noqa: B902 - the parent re-raises it
        import traceback
        queue.put(traceback.format_exc())


def main(path):
    import multiprocessing
    ctx = multiprocessing.get_context('spawn')
    fixture = {'configs': {}, 'not_recorded': {}}
    for which in ('product', 'measure'):
        queue = ctx.SimpleQueue()
        p = ctx.Process(target=_record_child, args=(which, queue))
        p.start()
        got = queue.get()
        p.join()
        if isinstance(got, str):
            raise RuntimeError(got)
        fixture['configs'][which] = [[name, fp] for name, fp in got if 'error' not in fp]
        fixture['not_recorded'].update({name: fp['error'] for name, fp in got if 'error' in fp})
    with open(path, 'w') as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main(sys.argv[1])
