"""Plan builder + executor for the HRNet hot path on MI355X.

The model module (models/pose_hrnet.py) owns PyTorch parameters with the reference's
state_dict names; this file turns (parameters, input shape, mode) into two recorded programs
of C-ABI ops (forward, backward) over NHWC device buffers and runs each with ONE host call
(hrnet_program_run). PyTorch is only the allocator / stream / autograd anchor.

Dataflow conventions
  Act   a device tensor [N,H,W,C] in the compute dtype. A conv output followed by BatchNorm is
        stored RAW (pre-BN); its consumers apply scale/shift(+ReLU) while loading, so the
        normalised tensor never makes an HBM round trip (reference: 7 separate kernels per
        BasicBlock, lib/models/pose_hrnet.py:41-57).
  Val   (act, bn, relu): the logical value relu?(bn?(act)) a consumer reads.
  Grad  every Act has a gradient buffer. For a raw+BN act it first accumulates the gradient
        w.r.t. the post-activation value, then BatchNorm backward rewrites it in place into the
        gradient w.r.t. the raw conv output (two-stage deterministic reductions).

Scheduling
  Lanes  ops carry a lane (HIP stream); EVENT_RECORD / STREAM_WAIT ops order them. The branches of a
         HighResolutionModule run on their own lanes, and the fuse-layer convs stay on the lane of the
         branch they read; only the sums wait for all lanes (HRNET_LANES=0: one stream).
  Fused BatchNorm-backward sums  the input-gradient conv that writes the LAST contribution to an
         activation gradient gathers (sum dz, sum dz*y) in its epilogue (hrnet_conv2d_bwdstats), which
         replaces the separate reduction pass for ~80 % of the BatchNorms (HRNET_FUSE_BWDSTATS=0: off).
  Fused block backward  the two 3x3 convs of a BasicBlock whose widths fit (hrnet_bwd_fused_supported) run their
         whole backward - BatchNorm-backward apply, weight gradient, input gradient, residual add, ReLU mask, the
         next BatchNorm's sums - as ONE launch each (hrnet_conv3x3_bwd_fused) instead of grad_term + wgrad +
         conv_bs (HRNET_FUSED_BWD=0: off).
  Batched slab sums  every layer keeps its own weight-gradient slab region; one table-driven launch per
         lane segment sums them (HRNET_BATCH_WRED=0: per-layer launches on shared scratch).
  Bucket marks  op indices at which every gradient above a flat offset is final (module boundaries and
         every ~16 MB on lane 0): hipnet.optim.GradSync issues its all-reduces there.
"""
import ctypes
import os
from collections import namedtuple

import torch

from . import _capi as C
from . import ops


def _round_up(x, m):
    return (x + m - 1) // m * m


# Environment switches. PRODUCT switches are read whenever a plan is recorded (INTEGRATION.md lists them). Every other
# HRNET_* variable this file knows is a MEASUREMENT switch - it changes which ops a recorded program holds (fusion on /
# off, lanes, deferral sizes ...) and exists for A/B runs and for the tests that compare a fused path with its unfused
# form - and is honoured only together with HRNET_MEASURE=1; without it the defaults below are what runs, and a
# variable that is set but ignored is reported once.
PRODUCT_ENV = ('HRNET_DETERMINISTIC', 'HRNET_WGRAD_ATOMIC', 'HRNET_DP_PLAN', 'HRNET_LANES')
_ignored = set()


def _knob(name, default):
    if name in PRODUCT_ENV or os.environ.get('HRNET_MEASURE', '0') == '1':
        return os.environ.get(name, default)
    if name in os.environ and name not in _ignored:
        _ignored.add(name)
        import warnings
        warnings.warn('{}={} is a measurement switch and is ignored without HRNET_MEASURE=1'.format(
            name, os.environ[name]))
    return default


class Act(object):
    __slots__ = ('name', 'N', 'H', 'W', 'C', 't', 'g', 'ginit', 'bn', 'bn_done', 'nuse', 'bwd_rows', 'gmasked')

    def __init__(self, name, N, H, W, Cc):
        self.name, self.N, self.H, self.W, self.C = name, N, H, W, Cc
        self.t = None       # torch tensor (storage)
        self.g = None       # gradient tensor
        self.ginit = False  # gradient buffer written yet (while recording the backward)
        self.bn = None      # BNRec if this is a raw conv output followed by BatchNorm
        self.bn_done = False
        self.nuse = 0       # number of consumers of the logical value
        self.bwd_rows = None  # (rows tensor, nrows): BN-backward sums gathered by a dgrad epilogue
        self.gmasked = False  # the gradient buffer already carries the ReLU mask of this activation (fused backward)

    @property
    def pixels(self):
        return self.N * self.H * self.W


class Val(object):
    __slots__ = ('act', 'bn', 'relu')

    def __init__(self, act, bn=None, relu=False):
        self.act, self.bn, self.relu = act, bn, relu


# The tape: one record per forward step; the backward pass walks it in reverse. `lane`: the lane the backward of the
# entry works on (the forward lane, but for the batched fuse sums: _hr_module).
ConvEntry = namedtuple('ConvEntry', 'lane xin crec stride y bnrec')
SumEntry = namedtuple('SumEntry', 'lane terms shifts relu_out out')
CatEntry = namedtuple('CatEntry', 'lane vals cat align')
HeadMixEntry = namedtuple('HeadMixEntry', 'lane vals crec y bnrec ts offs align')
# a fork (or join) of the side `lanes` from lane 0; sums: the pair around the fuse sums of a HighResolutionModule
LaneMark = namedtuple('LaneMark', 'lane fork lanes sums')


class BNRec(object):
    def __init__(self, prefix, mod, dev):
        self.prefix = prefix
        self.mod = mod
        c = mod.num_features
        self.C = c
        f = dict(dtype=torch.float32, device=dev)
        self.scale = torch.empty(c, **f)
        self.shift = torch.empty(c, **f)
        self.mean = torch.empty(c, **f)
        self.invstd = torch.empty(c, **f)
        self.coef = torch.empty(3 * c, **f)
        self.sums = None        # [8][2][C] batch sums (consumer-side BatchNorm; a slice of the plan's arena)
        self.count = 0.0        # elements per channel the sums cover


class ConvRec(object):
    def __init__(self, prefix, mod, stem=False):
        self.prefix, self.mod, self.stem = prefix, mod, stem
        w = mod.weight
        self.Cout, self.Cin, self.ks = w.shape[0], w.shape[1], w.shape[2]
        self.Cout_pad = _round_up(self.Cout, 16)
        self.Cin_pad = 32 if stem else _round_up(self.Cin, 8)
        self.wf = None   # packed forward weights
        self.wd = None   # packed dgrad weights


class Program(object):
    """A recorded list of HrOp, run with ONE C call. Every op carries a lane (= stream index);
    EVENT_RECORD / STREAM_WAIT ops express the dependencies between lanes: the branches of a
    HighResolutionModule are independent chains, and weight-gradient work is off the backward
    critical path, so the latency-bound kernels of one lane fill the gaps of another. On a single
    stream (no side streams given) the same list runs in order and the event ops are skipped."""

    def __init__(self):
        self.ops = []
        self.lane = 0
        self.events = []
        self._arr = None
        self.tags = {}          # op index -> layer name (measurement scripts only)
        self.before_add = None  # called before every op is appended (the plan flushes a held-back sum there)

    def add(self, op, lane=None):
        """append a built op (ops.make) on `lane` (None: the current lane); returns its index"""
        if self.before_add is not None:
            self.before_add(self.lane if lane is None else lane)
        op.i[C.LANE_SLOT] = self.lane if lane is None else lane
        self.ops.append(op)
        self._arr = None
        return len(self.ops) - 1

    def lane_of(self, idx):
        return self.ops[idx].i[C.LANE_SLOT]

    def sync(self, src, dst):
        """everything enqueued so far on lane `src` happens before what follows on lane `dst`"""
        ev = C.lib().hrnet_event_create()
        if not ev:
            raise RuntimeError('hrnet_event_create failed')
        self.events.append(ev)
        self.add(ops.make(C.OP_EVENT_RECORD, event=ev), lane=src)
        self.add(ops.make(C.OP_STREAM_WAIT, event=ev), lane=dst)

    def fork(self, lanes):
        for l in lanes:
            self.sync(0, l)

    def join(self, lanes):
        for l in lanes:
            self.sync(l, 0)

    def finalize(self):
        self._arr = (C.HrOp * len(self.ops))(*self.ops) if self.ops else None
        return self

    def set_ptr(self, op_index, slot, value):
        self._arr[op_index].p[slot] = value

    def set_int(self, op_index, slot, value):
        self._arr[op_index].i[slot] = value

    def run(self, lo=0, hi=None, streams=None):
        if self._arr is None:
            self.finalize()
        hi = len(self.ops) if hi is None else hi
        if hi <= lo:
            return
        base = ctypes.cast(ctypes.byref(self._arr, lo * ctypes.sizeof(C.HrOp)), ctypes.POINTER(C.HrOp))
        if streams is None:
            C.call('hrnet_program_run', base, hi - lo, C.stream_ptr())
        else:
            handles = (ctypes.c_void_p * len(streams))(
                *[C.stream_ptr() if st is None else st.cuda_stream for st in streams])
            C.call('hrnet_program_run_streams', base, hi - lo, handles, len(streams))

    def __del__(self):
        try:
            for ev in self.events:
                C.lib().hrnet_event_destroy(ev)
        except Exception:
            pass

    def __len__(self):
        return len(self.ops)


class PlanTicket(object):
    """held by the autograd node of one training forward: marks the plan busy until the backward has run or the
    graph is dropped (then the node, and with it this ticket, is garbage-collected)"""

    def __init__(self, plan):
        self.plan, self.gen = plan, plan.gen
        plan.busy = True

    def valid(self):
        return self.plan.gen == self.gen

    def release(self):
        if self.plan is not None and self.plan.gen == self.gen:
            self.plan.busy = False
        self.plan = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Plan(object):
    """Forward (+ backward) programs of one (batch, height, width, mode) instance."""

    def __init__(self, net, N, H, W, training, need_grad):
        self.net = net
        self.N, self.H, self.W = N, H, W
        self.training, self.need_grad = training, need_grad
        self.dev = net.device
        self.dt = net.compute_dtype
        self.dtid = C.dtype_id(self.dt)
        self.esize = 4 if self.dt == torch.float32 else 2
        self.fwd = Program()
        self.bwd = Program()
        self.pack_f = Program()   # master f32 OIHW -> packed forward weights
        self.pack_d = Program()   # -> packed dgrad weights
        self.keep = []            # tensors kept alive
        self.tape = []
        self.acts = []
        self.max_stats = 0
        self.max_slab = 0
        self.max_bwd_part = 0
        self.pending = []         # (program, op_index, slot, kind) scratch pointers to patch
        self.bucket_marks = []    # backward op indices after which a gradient bucket is complete
        self.nlanes = 4 if _knob('HRNET_LANES', '1') != '0' else 1   # module branches
        # weight-gradient lane (off by default): '2' = only the weight gradients of lane 0 (the high-resolution
        # branch, whose HBM-bound elementwise passes make it the critical chain) move to their own lane; '1' =
        # all of them. Measured on MI355X: '2' shortens the dependency-only critical path of the backward
        # program from 14.4 to 12.3 ms but the step stays at 24.4 ms - the step is throughput-bound, not
        # dependency-bound - and '1' is slower.
        wl = _knob('HRNET_WLANE', '0')
        self.wlane = 4 if (self.nlanes > 1 and wl in ('1', '2')) else 0
        self.defer_lanes = int(_knob('HRNET_DEFER_LANES', '3'))      # side lanes the deferred weight gradients use
        self.wlane_all = wl == '1'
        self.streams = None
        self.gen = 0              # bumped by every forward run: a backward must see the generation it recorded
        self.busy = False         # a training forward ran and its backward has not (PlanTicket)
        self._build()

    # ---- allocation helpers -----------------------------------------------------------
    def _act(self, name, N, H, W, Cc, grad=True):
        a = Act(name, N, H, W, Cc)
        a.t = torch.empty(N * H * W * Cc * self.esize, dtype=torch.uint8, device=self.dev)
        if self.need_grad and grad:
            a.g = torch.empty(N * H * W * Cc * self.esize, dtype=torch.uint8, device=self.dev)
        self.acts.append(a)
        return a

    def _f32(self, n, zero=False):
        t = (torch.zeros if zero else torch.empty)(n, dtype=torch.float32, device=self.dev)
        self.keep.append(t)
        return t

    def _scratch(self, prog, idx, slot, kind):
        self.pending.append((prog, idx, slot, kind))

    def _device_table(self, arr):
        """a ctypes struct array as a device table that lives as long as the plan"""
        raw = bytes(ctypes.string_at(ctypes.addressof(arr), ctypes.sizeof(arr)))
        table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.dev)
        self.keep.append(table)
        return table

    # ---- forward recording -------------------------------------------------------------
    def conv(self, xin, crec, stride=1, bnrec=None, relu=False, name=None):
        """conv (+bias) [+ BatchNorm statistics]; returns the Val consumers read."""
        x = xin.act
        ks = 1 if crec.stem else crec.ks
        Ho = (x.H + 2 * (ks // 2) - ks) // stride + 1
        Wo = (x.W + 2 * (ks // 2) - ks) // stride + 1
        y = self._act(name or crec.prefix, x.N, Ho, Wo, crec.Cout_pad)
        cin = x.C
        assert cin == crec.Cin_pad, (crec.prefix, cin, crec.Cin_pad)
        want_stats = bnrec is not None and self.training
        tiles = C.call('hrnet_conv_tiles', x.N, Ho, Wo, crec.Cout_pad, ks, stride)
        bias = crec.mod.bias
        sums_in = self.bn_sums and xin.bn is not None       # the input's BatchNorm from its batch sums, on the fly
        m_in = xin.bn.mod if xin.bn is not None else None
        ps = self._pending_sum.get(self.fwd.lane)
        # (the wide layers' fat LDS-ring launches take one input tensor: their residual sums stay separate launches)
        fat = (ks == 3 and stride == 1 and cin >= 96 and (self.bn_sums or not want_stats)
               and C.call('hrnet_conv_ring_supported', self.dtid, x.N, x.H, x.W, cin, crec.Cout_pad) >= 3)
        if (ps is not None and ps['out'] is x and xin.bn is None and not xin.relu and stride == 1 and not crec.stem
                and bias is None and ps['lane'] == self.fwd.lane and not fat):
            # the residual sum that produced x has not been emitted: this conv forms it in its prologue and writes
            # it out on the side (hrnet_conv2d_sum) - one launch and one tensor read less per block
            del self._pending_sum[self.fwd.lane]
            bt, it = ps['bn_term'], ps['id_term']
            sm = self.bn_sums
            mb = bt.bn.mod
            bn_in = (dict(in_inv_count=1.0 / bt.bn.count, in_eps=mb.eps, in_sums=C.ptr(bt.bn.sums),
                          in_gamma=C.ptr(mb.weight), in_beta=C.ptr(mb.bias)) if sm
                     else dict(in_scale=C.ptr(bt.bn.scale), in_shift=C.ptr(bt.bn.shift)))
            kind = C.OP_CONV_SUM
            i = self.fwd.add(ops.make(kind, dtype=self.dtid, n=x.N, h=x.H, w=x.W, cin=cin, cout=crec.Cout_pad, ks=ks,
                                      stats_atomic=1 if (want_stats and sm) else 0, x=C.ptr(bt.act.t),
                                      wgt=C.ptr(crec.wf), y=C.ptr(y.t),
                                      stats=C.ptr(bnrec.sums) if (want_stats and sm) else None,
                                      x2=C.ptr(it.act.t), side=C.ptr(x.t), **bn_in))
            self.n_fused_sums += 1
        else:
            bn_in = {}
            if sums_in:
                bn_in = dict(in_inv_count=1.0 / xin.bn.count, in_eps=m_in.eps, in_sums=C.ptr(xin.bn.sums),
                             in_gamma=C.ptr(m_in.weight), in_beta=C.ptr(m_in.bias))
            elif xin.bn:
                bn_in = dict(in_scale=C.ptr(xin.bn.scale), in_shift=C.ptr(xin.bn.shift))
            kind = C.OP_CONV
            i = self.fwd.add(ops.make(kind, dtype=self.dtid, n=x.N, h=x.H, w=x.W, cin=cin, ho=Ho, wo=Wo,
                                      cout=crec.Cout_pad, ks=ks, stride=stride, in_relu=1 if xin.relu else 0,
                                      stats_atomic=1 if (want_stats and self.bn_sums) else 0, x=C.ptr(x.t),
                                      wgt=C.ptr(crec.wf),
                                      bias=C.ptr(self.net.bias_pad[crec.prefix]) if bias is not None else None,
                                      y=C.ptr(y.t), stats=C.ptr(bnrec.sums) if (want_stats and self.bn_sums) else None,
                                      **bn_in))
        self.fwd.tags[i] = crec.prefix
        if want_stats and not self.bn_sums:
            self.max_stats = max(self.max_stats, tiles * 2 * crec.Cout_pad)
            self._scratch(self.fwd, i, ops.slot(kind, 'p', 'stats'), 'stats')
        x.nuse += 1
        if bnrec is not None:
            y.bn = bnrec
            bnrec.count = float(y.pixels)
            if self.training and self.bn_sums:
                self.bn_finalize_list.append(bnrec)      # one table-driven launch at the end of the pass
            elif self.training:
                self._bn_finalize(bnrec, tiles, y.pixels)
        self.tape.append(ConvEntry(self.fwd.lane, xin, crec, stride, y, bnrec))
        return Val(y, bnrec, relu)

    def _bn_finalize(self, bnrec, rows, count):
        """OP_BN_FINALIZE of a BatchNorm in training mode from `rows` statistic rows in the lane's scratch"""
        m = bnrec.mod
        j = self.fwd.add(ops.make(C.OP_BN_FINALIZE, tiles=rows, c=bnrec.C, training=1, count=count,
                                  momentum=m.momentum if m.momentum is not None else 0.1, eps=m.eps,
                                  gamma=C.ptr(m.weight), beta=C.ptr(m.bias), running_mean=C.ptr(m.running_mean),
                                  running_var=C.ptr(m.running_var), num_batches_tracked=C.ptr(m.num_batches_tracked),
                                  scale=C.ptr(bnrec.scale), shift=C.ptr(bnrec.shift), save_mean=C.ptr(bnrec.mean),
                                  save_invstd=C.ptr(bnrec.invstd)))
        self._scratch(self.fwd, j, ops.slot(C.OP_BN_FINALIZE, 'p', 'stats'), 'stats')

    def sum(self, terms, shifts, relu_out, name, batch=None, lane=None):
        """batch: a list - the op is appended to it as a job of a table-driven launch (HR_OP_EW_TABLE) instead of
        being emitted as a launch of its own; lane: the lane the backward pass works this sum on (None: the current one)"""
        t0 = terms[0].act
        sh0 = shifts[0]
        out = self._act(name, t0.N, t0.H << sh0, t0.W << sh0, t0.C)
        # relu(bn(y) + identity) that closes a block: held back - if the very next op of this lane is the stride-1
        # conv that reads it, that conv forms the sum itself (hrnet_conv2d_sum); any other op emits it first
        bn_terms = [t for t in terms if t.bn is not None]
        hold = (self.fuse_sums and len(terms) == 2 and list(shifts) == [0, 0] and relu_out and len(bn_terms) == 1
                and not bn_terms[0].relu and all(t.bn is not None or not t.relu for t in terms)
                and (not self.bn_sums or t0.C <= 768) and batch is None)
        if self.bn_sums and any(t.bn for t in terms):
            bn = dict(sums_mode=sum(1 << k for k, t in enumerate(terms) if t.bn),
                      eps_bits=ops.f32_bits(next(t.bn.mod.eps for t in terms if t.bn)),
                      scale=[C.ptr(t.bn.sums) if t.bn else None for t in terms],
                      shift=[C.ptr(t.bn.mod.weight) if t.bn else None for t in terms],
                      inv_count=[1.0 / t.bn.count if t.bn else 0.0 for t in terms])
        else:
            bn = dict(scale=[C.ptr(t.bn.scale) if t.bn else None for t in terms],
                      shift=[C.ptr(t.bn.shift) if t.bn else None for t in terms])
        op = ops.make(C.OP_SUM_TERMS, dtype=self.dtid, n=out.N, h=out.H, w=out.W, c=out.C, nterms=len(terms),
                      relu_out=1 if relu_out else 0, sh=shifts, relu=[1 if t.relu else 0 for t in terms],
                      out=C.ptr(out.t), src=[C.ptr(t.act.t) for t in terms], **bn)
        if hold:
            self._flush_pending_sum(self.fwd.lane)
            self._pending_sum[self.fwd.lane] = dict(out=out, lane=self.fwd.lane, op=op, bn_term=bn_terms[0],
                                                    id_term=next(t for t in terms if t.bn is None))
        elif batch is not None:
            batch.append(op)
        else:
            self.fwd.add(op)
        for t in terms:
            t.act.nuse += 1
        self.tape.append(SumEntry(self.fwd.lane if lane is None else lane, list(terms), list(shifts), relu_out, out))
        return Val(out)

    def _flush_pending_sum(self, lane=None):
        """emit the held-back residual sum of `lane` (None: of every lane) as its own launch (its consumer was not a
        fusable conv). One slot per lane: the lanes of a module may be recorded interleaved."""
        for l in ([lane] if lane is not None else sorted(self._pending_sum)):
            ps = self._pending_sum.pop(l, None)
            if ps is not None:
                self.fwd.add(ps['op'], lane=ps['lane'])

    def bilinear_cat(self, vals, name, align=False):
        a0 = vals[0].act
        ctot = sum(v.act.C for v in vals)
        cat = self._act(name, a0.N, a0.H, a0.W, ctot)
        self.fwd.add(ops.make(C.OP_BILINEAR_CAT, dtype=self.dtid, nbr=len(vals), n=a0.N, h=a0.H, w=a0.W,
                              hs=[v.act.H for v in vals], ws=[v.act.W for v in vals], cs=[v.act.C for v in vals],
                              align=1.0 if align else 0.0, cat=C.ptr(cat.t), x=[C.ptr(v.act.t) for v in vals]))
        for v in vals:
            assert v.bn is None and not v.relu
            v.act.nuse += 1
        self.tape.append(CatEntry(self.fwd.lane, list(vals), cat, align))
        return Val(cat)

    def head_mix(self, vals, crec, bnrec, align=False):
        """last_layer[0] over cat(x0, up(x1), ...) WITHOUT the concat (pose_hrnet.py:560-566; csrc/gemm_pw.hip):
        t_j = W_j x_j at branch j's resolution, then y = W0 x0 + bias + sum_j up(t_j) with its batch statistics."""
        net = self.net
        x0 = vals[0].act
        widths = [v.act.C for v in vals]
        offs = [0]
        for c in widths:
            offs.append(offs[-1] + c)
        wfs = net.head_slices(crec, widths)
        y = self._act(crec.prefix, x0.N, x0.H, x0.W, crec.Cout_pad)
        ts = []
        for j in range(1, len(vals)):
            xa = vals[j].act
            t = self._act('{}.t{}'.format(crec.prefix, j), xa.N, xa.H, xa.W, crec.Cout_pad)
            i = self.fwd.add(ops.make(C.OP_CONV, dtype=self.dtid, n=xa.N, h=xa.H, w=xa.W, cin=xa.C, ho=xa.H, wo=xa.W,
                                      cout=crec.Cout_pad, ks=1, stride=1, x=C.ptr(xa.t), wgt=C.ptr(wfs[j]), y=C.ptr(t.t)))
            self.fwd.tags[i] = '{}.t{}'.format(crec.prefix, j)
            ts.append(t)
        want_stats = bnrec is not None and self.training
        rows_mode = 0 if self.bn_sums else 1
        bias = crec.mod.bias
        i = self.fwd.add(ops.make(C.OP_HEAD_MIX, dtype=self.dtid, n=x0.N, h=x0.H, w=x0.W, c0=x0.C, cout=crec.Cout_pad,
                                  nup=len(ts), align=1 if align else 0, up_h=[t.H for t in ts], up_w=[t.W for t in ts],
                                  rows_mode=rows_mode, x0=C.ptr(x0.t), w0=C.ptr(wfs[0]),
                                  bias=C.ptr(net.bias_pad[crec.prefix]) if bias is not None else None, y=C.ptr(y.t),
                                  stats=C.ptr(bnrec.sums) if (want_stats and self.bn_sums) else None,
                                  t=[C.ptr(t.t) for t in ts]))
        self.fwd.tags[i] = crec.prefix
        rows = C.call('hrnet_head_mix_rows', x0.N, x0.H, x0.W)
        if want_stats and not self.bn_sums:
            self.max_stats = max(self.max_stats, rows * 2 * crec.Cout_pad)
            self._scratch(self.fwd, i, ops.slot(C.OP_HEAD_MIX, 'p', 'stats'), 'stats')
        for v in vals:
            assert v.bn is None and not v.relu
            v.act.nuse += 1
        if bnrec is not None:
            y.bn = bnrec
            bnrec.count = float(y.pixels)
            if self.training and self.bn_sums:
                self.bn_finalize_list.append(bnrec)
            elif self.training:
                self._bn_finalize(bnrec, rows, y.pixels)
        self.tape.append(HeadMixEntry(self.fwd.lane, list(vals), crec, y, bnrec, ts, offs, align))
        self.n_head_mix = 1
        self._head_y = y
        return Val(y, bnrec, True)

    # ---- network walk (reference: PoseHighResolutionNet.forward, pose_hrnet.py:511-568) ----
    def _build(self):
        net = self.net
        N, H, W = self.N, self.H, self.W
        # BatchNorm coefficient buffers (scale/shift/mean/invstd/coef) belong to the PLAN: two plans of one net
        # can be in flight at once (hipnet.net.HipNet.plan), and each backward needs its own forward's statistics
        self.bns = {name: BNRec(name, rec.mod, self.dev) for name, rec in net.bns.items()}
        # residual sums fused into the conv that reads them (hrnet_conv2d_sum): HRNET_FUSE_SUM=0 turns it off.
        # Training only: 18.75 vs 18.92 ms/step; an eval pass is faster with the separate sum kernels (5.25 vs
        # 5.36 ms: the two-tensor prologue re-reads two halos and lengthens the latency-bound conv launches)
        self.fuse_sums = self.training and _knob('HRNET_FUSE_SUM', '1') != '0'
        self._pending_sum = {}        # lane -> held-back residual sum
        self.n_fused_sums = 0
        self.n_batched_fwd_sums = 0
        self.fwd.before_add = self._flush_pending_sum
        self._setup_batch_sums()
        cv, bn = net.convs, self.bns
        if not self.training:
            # eval mode: every BatchNorm's affine from its running statistics, ONE table launch (306 launches of
            # 12 us each before: a third of the isolated kernel time of an eval forward pass)
            self.bn_finalize_list = list(self.bns.values())
            self._add_bn_finalize_table(eval_mode=True)
            self.bn_finalize_list = []
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        cols = self._act('stem.cols', N, Ho, Wo, 32, grad=False)
        self.in_op = self.fwd.add(ops.make(C.OP_IM2COL_STEM, dtype=self.dtid, n=N, c=3, h=H, w=W, ho=Ho, wo=Wo, kpad=32,
                                           cols=C.ptr(cols.t)))
        v = self.conv(Val(cols), cv['conv1'], 1, bn['bn1'], relu=True)
        v = self.conv(v, cv['conv2'], 2, bn['bn2'], relu=True)
        for k in range(4):
            p = 'layer1.{}'.format(k)
            a = self.conv(v, cv[p + '.conv1'], 1, bn[p + '.bn1'], relu=True)
            b = self.conv(a, cv[p + '.conv2'], 1, bn[p + '.bn2'], relu=True)
            c = self.conv(b, cv[p + '.conv3'], 1, bn[p + '.bn3'], relu=False)
            if (p + '.downsample.0') in cv:
                res = self.conv(v, cv[p + '.downsample.0'], 1, bn[p + '.downsample.1'], relu=False)
            else:
                res = v
            v = self.sum([c, res], [0, 0], True, p + '.out')
        ys = [v]
        inter = None
        for s in (2, 3, 4):
            sc = net.stage_cfg[s]
            nbr = sc['NUM_BRANCHES']
            tp = 'transition{}'.format(s - 1)
            xs = []
            for i in range(nbr):
                if i < len(ys):
                    key = '{}.{}.0'.format(tp, i)
                    xs.append(self.conv(ys[i], cv[key], 1, bn['{}.{}.1'.format(tp, i)], relu=True)
                              if key in cv else ys[i])
                else:
                    t = ys[-1]
                    for j in range(i + 1 - len(ys)):
                        q = '{}.{}.{}'.format(tp, i, j)
                        t = self.conv(t, cv[q + '.0'], 2, bn[q + '.1'], relu=True)
                    xs.append(t)
            for m in range(sc['NUM_MODULES']):
                xs = self._hr_module(xs, 'stage{}.{}'.format(s, m), sc['NUM_BLOCKS'])
            ys = xs
            if s == 3:
                inter = ys[0]
        self._record_head(ys, inter)
        if self.bn_sums and self.bn_finalize_list:
            self._add_bn_finalize_table()
        self._flush_pending_sum()
        self.fwd.before_add = None
        if self.need_grad:
            self._build_backward()
            if self.wlane:
                self.bwd.sync(self.wlane, 0)     # all weight gradients done before the optimiser
        self._resolve_scratch()
        self.fwd.finalize()
        self.bwd.finalize()

    def _setup_batch_sums(self):
        # Consumer-side BatchNorm (training): producers add their batch sums into 8 partial copies per BatchNorm with
        # float atomics, forward consumers build scale/shift from them on the fly, and ONE table-driven launch at the
        # end of the pass fills the arrays the backward pass reads and updates the running statistics - instead of a
        # finalize launch after each of the 306 convs. HRNET_DETERMINISTIC=1: per-workgroup rows + a finalize launch
        # per BatchNorm (bit-reproducible statistics).
        contiguous = all(b.mod.bias.data_ptr() == b.mod.weight.data_ptr() + 4 * b.C for b in self.bns.values())
        # capacity of the on-the-fly coefficient tables: 768 channels in the conv prologues (HR_CONV_MAXC: the head's
        # 480 / 720), 384 in hrnet_sum_terms (SUM_MAXC: the widest BatchNorm that reaches a sum is a branch width -
        # the head's BatchNorm is read by a conv); wider nets fall back to per-BatchNorm finalize launches
        sum_w = max([b.C for n, b in self.bns.items() if not n.startswith('last_layer')] or [0])
        self.bn_sums = (self.training and contiguous and _knob('HRNET_DETERMINISTIC', '0') != '1'
                        and max(b.C for b in self.bns.values()) <= 768 and sum_w <= 384)
        self.bn_finalize_list = []
        if self.bn_sums:
            total = sum(16 * b.C for b in self.bns.values())
            self.bn_arena = self._f32(total, zero=True)
            off = 0
            for b in self.bns.values():
                b.sums = self.bn_arena[off:off + 16 * b.C]
                off += 16 * b.C
            nbytes = total * 4
            self.fwd.add(ops.make(C.OP_FILL, bytes_lo=ops.u32_bits(nbytes & 0xffffffff), bytes_hi=nbytes >> 32,
                                  dst=C.ptr(self.bn_arena)))

    def _record_head(self, ys, inter):
        net, cv, bn, N = self.net, self.net.convs, self.bns, self.N
        # pose_hrnet_softmax (lib/models/pose_hrnet_softmax.py:499-506): align_corners=True, inter_feat = the concat
        # The head: last_layer[0] commutes with the bilinear upsampling, so (bf16, widths the mix launch takes) the
        # 480-channel concat and its gradient are never formed - head_mix(). HRNET_HEAD_MIX=0, the fp32 device path
        # and pose_hrnet_softmax (whose inter_feat IS the concat) keep the concat form.
        align = bool(getattr(net.module, 'head_align_corners', False))
        c0 = cv['last_layer.0']
        self.n_head_mix = 0
        self._head_y = None
        self._head_bwd = None
        mix = (_knob('HRNET_HEAD_MIX', '1') != '0' and not getattr(net.module, 'inter_from_cat', False)
               and 2 <= len(ys) <= 4 and all(v.bn is None and not v.relu for v in ys)
               and sum(v.act.C for v in ys) == c0.Cin and c0.Cin_pad == c0.Cin and c0.Cout_pad == c0.Cout
               and C.call('hrnet_head_mix_supported', self.dtid, ys[0].act.C, c0.Cout_pad) == 1)
        if mix:
            h = self.head_mix(ys, c0, bn['last_layer.1'], align=align)
        else:
            cat = self.bilinear_cat(ys, 'head.cat', align=align)
            if getattr(net.module, 'inter_from_cat', False):
                inter = cat
            h = self.conv(cat, c0, 1, bn['last_layer.1'], relu=True)
        out = self.conv(h, cv['last_layer.3'], 1, None, relu=False)
        self.out_act, self.inter_act = out.act, inter.act
        self.nj = cv['last_layer.3'].Cout
        self.out_op = self.fwd.add(ops.make(C.OP_NHWC_TO_NCHW, dtype=self.dtid, n=N, h=out.act.H, w=out.act.W,
                                            cp=out.act.C, c=self.nj, src=C.ptr(out.act.t)))
        self.inter_op = self.fwd.add(ops.make(C.OP_NHWC_TO_NCHW, dtype=self.dtid, n=N, h=inter.act.H, w=inter.act.W,
                                              cp=inter.act.C, c=inter.act.C, src=C.ptr(inter.act.t)))

    def _add_bn_finalize_table(self, eval_mode=False):
        ents = (C.HrBnEnt * len(self.bn_finalize_list))()
        block = 0
        for e, b in zip(ents, self.bn_finalize_list):
            m = b.mod
            e.sums, e.gamma, e.beta = (None if eval_mode else C.ptr(b.sums)), C.ptr(m.weight), C.ptr(m.bias)
            e.running_mean, e.running_var = C.ptr(m.running_mean), C.ptr(m.running_var)
            e.num_batches_tracked = None if eval_mode else C.ptr(m.num_batches_tracked)
            e.scale, e.shift, e.mean, e.invstd = C.ptr(b.scale), C.ptr(b.shift), C.ptr(b.mean), C.ptr(b.invstd)
            e.count = 1.0 if eval_mode else b.count
            e.momentum, e.eps = (m.momentum if m.momentum is not None else 0.1), m.eps
            e.C, e.block0 = b.C, block
            block += (b.C + 255) // 256
        self.fwd.lane = 0
        self.fwd.add(ops.make(C.OP_BN_FINALIZE_TABLE, n=len(self.bn_finalize_list), blocks=block,
                              table=C.ptr(self._device_table(ents))))

    def _hr_module(self, xs, pre, num_blocks):
        """HighResolutionModule.forward, pose_hrnet.py:247-266."""
        cv, bn = self.net.convs, self.bns
        nb = len(xs)
        xs = list(xs)
        side = [i for i in range(1, nb) if i < self.nlanes]
        if side:
            self.fwd.fork(side)
            self.tape.append(LaneMark(self.fwd.lane, fork=True, lanes=side, sums=False))
        # recording order of the branches: lane by lane (every block of branch 0, then branch 1 ...), or - HRNET_INTERLEAVE=1,
        # measurement - block by block across the branches, so that the host hands every lane its first launches at once
        # (the programs are enqueued in recording order at ~3.5 us per op)
        interleave = _knob('HRNET_INTERLEAVE', '0') == '1' and len(side) > 0
        order = ([(i, k) for k in range(max(num_blocks[:nb])) for i in range(nb) if k < num_blocks[i]] if interleave
                 else [(i, k) for i in range(nb) for k in range(num_blocks[i])])
        for i, k in order:
            self.fwd.lane = i if i in side else 0
            b = '{}.branches.{}.{}'.format(pre, i, k)
            a = self.conv(xs[i], cv[b + '.conv1'], 1, bn[b + '.bn1'], relu=True)
            c = self.conv(a, cv[b + '.conv2'], 1, bn[b + '.bn2'], relu=False)
            xs[i] = self.sum([c, xs[i]], [0, 0], True, b + '.out')
        # fuse-layer convolutions stay on the lane of the branch they READ (source-major): they start as
        # soon as that branch is done, and in the backward pass every accumulation into a branch
        # output's gradient is ordered on one lane. The sums wait for all lanes.
        fuse_lanes = _knob('HRNET_FUSE_LANES', '1') != '0'
        if side and not fuse_lanes:
            self.fwd.lane = 0
            self.fwd.join(side)
            self.tape.append(LaneMark(self.fwd.lane, fork=False, lanes=side, sums=False))
        term_of = {}
        for j in range(nb):
            if fuse_lanes:
                self.fwd.lane = j if j in side else 0
            for i in range(nb):
                if j == i:
                    term_of[(i, j)] = (xs[j], 0)
                elif j > i:
                    f = '{}.fuse_layers.{}.{}'.format(pre, i, j)
                    term_of[(i, j)] = (self.conv(xs[j], cv[f + '.0'], 1, bn[f + '.1'], relu=False), j - i)
                else:
                    t = xs[j]
                    for k in range(i - j):
                        f = '{}.fuse_layers.{}.{}.{}'.format(pre, i, j, k)
                        t = self.conv(t, cv[f + '.0'], 2, bn[f + '.1'], relu=(k != i - j - 1))
                    term_of[(i, j)] = (t, 0)
        self.fwd.lane = 0
        if side and fuse_lanes:
            self.fwd.join(side)
            self.tape.append(LaneMark(self.fwd.lane, fork=False, lanes=side, sums=False))
        # the sums of the module outputs run on the lane of their output branch (a second fork/join): in the
        # backward pass that spreads a module's 16 sum-term passes over the lanes, and every consumer of a
        # branch gradient sits on that branch's lane
        sum_lanes = side and fuse_lanes and _knob('HRNET_SUM_LANES', '1') != '0'
        # ... or, forward (HRNET_BATCH_SUMFWD, default on): the nb sums as ONE table-driven launch on lane 0 - they are
        # 10-30 us each, and the fork / join around them cost more than running them side by side saved. The tape
        # keeps the fork / join marks (sums=True): the backward pass batches its side of them the same way.
        batch = [] if (sum_lanes and _knob('HRNET_BATCH_SUMFWD', '1') != '0') else None
        if sum_lanes:
            if batch is None:
                self.fwd.fork(side)
            self.tape.append(LaneMark(self.fwd.lane, fork=True, lanes=side, sums=True))
        outs = []
        for i in range(nb):
            if sum_lanes and batch is None:
                self.fwd.lane = i if i in side else 0
            terms = [term_of[(i, j)][0] for j in range(nb)]
            shifts = [term_of[(i, j)][1] for j in range(nb)]
            # the output-resolution term first (sum_terms sizes the output from term 0)
            order = sorted(range(nb), key=lambda q: shifts[q])
            # (batched: recorded on lane 0, but the backward pass works this branch on its own lane)
            outs.append(self.sum([terms[q] for q in order], [shifts[q] for q in order], True,
                                 '{}.fuse.{}'.format(pre, i), batch=batch,
                                 lane=None if batch is None else (i if i in side else 0)))
        self.fwd.lane = 0
        if batch:
            sums = any(op.i[ops.slot(C.OP_SUM_TERMS, 'i', 'sums_mode')] for op in batch)
            self._add_ew_table(self.fwd, C.OP_SUM_TERMS, batch, sums=1 if sums else 0)
            self.n_batched_fwd_sums += len(batch)
        if sum_lanes:
            if batch is None:
                self.fwd.join(side)
            self.tape.append(LaneMark(self.fwd.lane, fork=False, lanes=side, sums=True))
        return outs

    def _add_ew_table(self, prog, kind, jobs, **fields):
        """`jobs` (ops of one kind) as ONE OP_EW_TABLE launch of `prog`: every job gets its block range, the jobs go to
        the device as the launch's table"""
        dims = ops.SLOTS[kind]['i']
        block = 0
        for op in jobs:
            if kind == C.OP_BN_BWD_FINALIZE:
                nb = C.call('hrnet_ew_table_blocks', kind, self.dtid, 1, 1, 1, op.i[dims['C']])
            else:
                # (a pooled reduction is sized by its first level, H / 2 x W / 2)
                sh = 1 if kind == C.OP_POOL_REDUCE else 0
                nb = C.call('hrnet_ew_table_blocks', kind, self.dtid, op.i[dims['N']], op.i[dims['H']] >> sh,
                            op.i[dims['W']] >> sh, op.i[dims['C']])
            ops.set_job_blocks(op, block, nb)
            block += nb
        table = self._device_table((C.HrOp * len(jobs))(*jobs))
        prog.add(ops.make(C.OP_EW_TABLE, jobs=len(jobs), blocks=block, kind=kind, dtype=self.dtid, table=C.ptr(table),
                          **fields))

    # ---- backward recording ---------------------------------------------------------------
    def _bn_backward(self, y, g_src, mask, sh, inner_relu, extra=None, pooled=None):
        """BatchNorm backward for raw act y: reads the upstream gradient from g_src (pooled over
        2^sh blocks, masked by mask>0 and the BN's own ReLU), writes d(raw) into y.g. `extra`: an
        identity term of the same sum whose gradient (the same dz) is written by the same pass."""
        b = y.bn
        blocks = C.call('hrnet_reduce_blocks', y.N, y.H, y.W, y.C)
        self.max_bwd_part = max(self.max_bwd_part, blocks * 2 * y.C)
        # a reduction pass (no sums gathered by a producer) pools and masks the upstream gradient: it keeps that dz in
        # y.g, and the apply pass reads it from there instead of pooling and masking the full-resolution tensors
        # again (an up-sampled fuse term of branch 0 re-read 2 x 16.8 MB per term). HRNET_KEEP_DZ=0: both passes pool.
        keep_dz = None
        if y.bwd_rows is None and g_src != C.ptr(y.g) and _knob('HRNET_KEEP_DZ', '1') != '0':
            keep_dz = C.ptr(y.g)
        shape = dict(dtype=self.dtid, n=y.N, h=y.H, w=y.W, c=y.C)
        reduce_ = dict(shape, sh=sh, inner_relu=1 if inner_relu else 0, g=g_src, mask=mask, y=C.ptr(y.t),
                       scale=C.ptr(b.scale), shift=C.ptr(b.shift), dz=keep_dz)
        if pooled is not None:
            # the reduction ran as one level of a HR_OP_POOL_REDUCE job (its dz is in y.g, its partial rows in `pooled`)
            part, pblocks = pooled
            keep_dz = C.ptr(y.g)
            self._emit(self._bn_bwd_finalize_op(y, pblocks, C.ptr(part)))
        elif y.bwd_rows is not None:
            # the dgrad conv that finished g_src already gathered (sum dz, sum dz*y) in its epilogue
            rows, blocks = y.bwd_rows
            assert sh == 0
            self._emit(self._bn_bwd_finalize_op(y, blocks, C.ptr(rows)))
        elif self._batch is not None:
            part = self._f32(blocks * 2 * y.C)          # (a job of a batched launch: partial rows of its own)
            self._emit(ops.make(C.OP_BN_BWD_REDUCE, partials=C.ptr(part), **reduce_))
            self._emit(self._bn_bwd_finalize_op(y, blocks, C.ptr(part)))
        else:
            i = self.bwd.add(ops.make(C.OP_BN_BWD_REDUCE, **reduce_))
            self._scratch(self.bwd, i, ops.slot(C.OP_BN_BWD_REDUCE, 'p', 'partials'), 'bwdpart')
            j = self.bwd.add(self._bn_bwd_finalize_op(y, blocks, None))
            self._scratch(self.bwd, j, ops.slot(C.OP_BN_BWD_FINALIZE, 'p', 'partials'), 'bwdpart')
        term = dict(shape, dst=C.ptr(y.g), y=C.ptr(y.t), scale=C.ptr(b.scale), shift=C.ptr(b.shift), coef=C.ptr(b.coef))
        if keep_dz is not None:
            term.update(g=keep_dz)                    # dz as the reduction stored it: pooled and masked already
        else:
            term.update(sh=sh, inner_relu=1 if inner_relu else 0, g=g_src, mask=mask)
        if extra is not None:
            assert sh == 0 and not inner_relu
            term.update(accumulate2=1 if extra.ginit else 0, dst2=C.ptr(extra.g))
            extra.ginit = True
        self._emit(ops.make(C.OP_GRAD_TERM, **term))
        y.bn_done = True
        y.ginit = True

    def _bn_bwd_finalize_op(self, y, blocks, partials):
        """OP_BN_BWD_FINALIZE of y's BatchNorm: `blocks` partial rows -> its coefficients, dgamma / dbeta added to"""
        b, m = y.bn, y.bn.mod
        return ops.make(C.OP_BN_BWD_FINALIZE, blocks=blocks, c=y.C, accumulate=1, count=y.pixels, partials=partials,
                        gamma=C.ptr(m.weight), save_mean=C.ptr(b.mean), save_invstd=C.ptr(b.invstd),
                        dgamma=C.ptr(self.net.grad_of(m.weight)), dbeta=C.ptr(self.net.grad_of(m.bias)),
                        coef=C.ptr(b.coef))

    # ---- batched element-wise jobs (the backward of a HighResolutionModule's fuse sums) ----
    def _emit(self, op):
        """an HR_OP_GRAD_TERM / HR_OP_BN_BWD_REDUCE / HR_OP_BN_BWD_FINALIZE / HR_OP_POOL_REDUCE op: its own launch, or -
        while a batch is open - a job of the batched launch of its kind (HR_OP_EW_TABLE)"""
        if self._batch is None:
            return self.bwd.add(op)
        self._batch[op.kind].append(op)
        return None

    def _flush_batch(self):
        """the open batch as (at most) three launches on lane 0: every reduction, every finalize, every apply job"""
        batch, self._batch = self._batch, None
        if batch is None:
            return
        self.bwd.lane = 0
        for kind in (C.OP_POOL_REDUCE, C.OP_BN_BWD_REDUCE, C.OP_BN_BWD_FINALIZE, C.OP_GRAD_TERM):
            jobs = batch[kind]
            if jobs:
                self._add_ew_table(self.bwd, kind, jobs)
                self.n_batched_jobs += len(jobs)

    def _build_backward(self):
        """the backward program: the tape in reverse, one method per entry kind"""
        # d(heatmaps) NCHW f32 -> NHWC grad of the final conv; d(inter_feat) likewise (optional)
        oa = self.out_act
        self.gout_op = self.bwd.add(ops.make(C.OP_NCHW_TO_NHWC, dtype=self.dtid, n=oa.N, h=oa.H, w=oa.W, cp=oa.C,
                                             c=self.nj, dst=C.ptr(oa.g)))
        oa.ginit = True
        self._backward_settings()
        self._scan_tape()
        self._in_region = False        # between the backward fork and join of a module's lanes
        self._first_fork = next((i for i, e in enumerate(self.tape) if isinstance(e, LaneMark) and e.fork), None)
        fused_at, fused_skip = self._find_fused_blocks(), set()
        self.n_fused_blocks = len(fused_at)
        self._fused_out_ids = {id(self.tape[ti].out) for ti in fused_at}     # block outputs a fused launch consumes
        for ti in reversed(range(len(self.tape))):
            e = self.tape[ti]
            self.bwd.lane = e.lane
            if ti in fused_skip:
                continue
            if ti in fused_at:
                self._inter_grad_joins_at(e.out)
                if fused_at[ti] == 'basic':
                    self._fused_block_backward(ti)
                else:
                    self._fused_bottleneck_backward(ti, downsample=fused_at[ti] == 'bottleneck_ds')
                fused_skip.update(range(ti - self.FUSED_CONVS[fused_at[ti]], ti))
            elif isinstance(e, LaneMark):
                self._lane_mark_backward(ti, e)
            elif isinstance(e, CatEntry):
                self._cat_backward(e)
            elif isinstance(e, HeadMixEntry):
                self._head_mix_backward(e)
            elif isinstance(e, SumEntry):
                self._sum_backward(e)
            else:
                self._conv_backward(ti, e)
        if self.batch_wred:
            for l in sorted(self._wred):
                self._flush_wred(l)
            self.bwd.lane = 0
            late = sorted(set(self._deferred_lanes) | self._offload_lanes)
            if late:
                self.bwd.join(late)       # the deferred / offloaded weight gradients (and their slab sums) are done
            self._upload_wred_tables()

    FUSED_CONVS = {'basic': 2, 'bottleneck': 3, 'bottleneck_ds': 4}     # tape entries a fused block covers before its sum

    def _backward_settings(self):
        # Weight gradients by float atomics (default): every workgroup of a weight-gradient / fused backward launch ADDS
        # its tile straight into the OIHW f32 gradient (3x3 tiles go through LDS so that a wave instruction covers 64
        # consecutive floats) instead of writing a slab per split that a reduce launch reads back: no slabs (1.94 GB
        # written and read back per step before), no reduce launches, and nothing left to do when the last
        # weight-gradient launch ends. HRNET_DETERMINISTIC=1 (or HRNET_WGRAD_ATOMIC=0) keeps slabs + ordered sums
        # (HRNET_WGRAD_ATOMIC=1 beside HRNET_DETERMINISTIC=1: ordered batch statistics, atomic weight gradients - tests).
        det = _knob('HRNET_DETERMINISTIC', '0') == '1'
        self.wgrad_atomic = (_knob('HRNET_BATCH_WRED', '1') != '0'
                             and _knob('HRNET_WGRAD_ATOMIC', '0' if det else '1') != '0')
        # batched backward of the fuse sums (HR_OP_EW_TABLE; HRNET_BATCH_SUMBWD=0: one launch per pass and lane)
        self.batch_sums = _knob('HRNET_BATCH_SUMBWD', '1') != '0'
        self._batch = None
        self.n_batched_jobs = 0
        # weight-gradient slab sums are batched: every layer keeps its own slab region and ONE table-driven
        # launch per lane segment (or per ~16 MB of gradient on lane 0) sums them
        self.batch_wred = _knob('HRNET_BATCH_WRED', '1') != '0'
        self._wred = {}            # lane -> pending (slabs tensor, HrWredEnt fields)
        self._wred_tables = []     # (op index, [entries]) patched with the device table at the end
        self._wred_bytes = 0
        self.slab_bytes = 0
        # dgrad epilogue fusion of the BN-backward reduction: the dgrad conv that writes the LAST
        # contribution to an activation gradient gathers (sum dz, sum dz*y) of the BatchNorm behind it.
        self._fuse_stats = self.training and _knob('HRNET_FUSE_BWDSTATS', '1') != '0'
        self.n_fused_bwdstats = 0
        self._bnrefs = []
        self.n_inline_bnbwd = 0
        self.inter_gop = None
        # Deferred weight gradients: the weight-gradient launches of the HighResolutionModules are off the critical
        # path, and the end of the backward pass (transition1, layer1, the stem: one lane, a third of its wall
        # time) leaves the other lanes idle - so they are recorded when their operands are final but ENQUEUED on
        # the side lanes when the walk reaches that single-lane tail. Their gradients are complete only at the
        # end of the program, so this is off under data parallelism (the bucketed exchange relies on gradients
        # completing in reverse layer order); HRNET_DEFER_WGRAD=0 turns it off.
        # Data parallelism (recorded at plan build: hipnet.optim.GradSync checks it): only the convolutions of the flat
        # buffer's LATE region (HipNet._flatten) are deferred - the bucketed exchange relies on every other gradient
        # completing in reverse layer order, and exchanges the late region when the program ends - and nothing is
        # offloaded from lane 0. HRNET_DP_PLAN=1 records that form in a single process (bench.py: what the step of
        # a data-parallel rank costs on one GPU).
        dp = (torch.distributed.is_available() and torch.distributed.is_initialized()
              and torch.distributed.get_world_size() > 1) or _knob('HRNET_DP_PLAN', '0') == '1'
        self.dp_plan = dp
        self.defer_wgrad = (self.nlanes > 1 and self.batch_wred and not self.wlane
                            and _knob('HRNET_DEFER_WGRAD', '1') != '0')
        self.defer_branch_wgrads = _knob('HRNET_DEFER_BRANCH', '1') != '0'   # (measurement: fuse layers only)
        # how much weight-gradient work the single-lane tail can hide: the tail is a stream over the stem / layer1
        # maps, so its length goes with their pixel count; w32 at B=64 needs 3.2 MFLOP per tail pixel to defer everything
        # (773 GFLOP behind a 4 ms tail). w48 has 1.9x the work per tail pixel: part of it stays in the modules
        # (deferring all of it: 43.8 ms/step, none: 37.0 in round 2; round 4, with the 96-channel branch on the fused
        # backward: 2.4 -> 29.1, 3.2 -> 28.8, 4.5 -> 28.4, 6 -> 28.4 ms/step; w32 unchanged)
        tail_pixels = self.N * (self.H // 4) * (self.W // 4)
        self._defer_budget = float(_knob('HRNET_DEFER_MFLOP_PER_PIXEL', '4.5')) * 1e6 * tail_pixels
        self._defer_flops = 0.0
        self.offload_wgrad = self.defer_wgrad and not dp and _knob('HRNET_OFFLOAD_WGRAD', '1') != '0'
        self._offload_rr = 0
        self._offload_lanes = set()
        self._deferred = []
        self._deferred_lanes = []
        self.late_cuts = []        # (backward op index, flat lo, flat hi, lane): late-region groups final on that lane there
        self.n_deferred_wgrads = 0

    def _scan_tape(self):
        """_relu_of: act -> relu flag its consumers apply (uniform per act in this network); _first_use / _use_lanes:
        act -> first tape index / lanes that read it (the LAST contribution to its gradient in the backward pass);
        _producer_sum: act -> the sum entry that wrote it"""
        self._relu_of, self._first_use, self._use_lanes, self._producer_sum = {}, {}, {}, {}
        for ti, e in enumerate(self.tape):
            if isinstance(e, LaneMark):
                continue
            reads = [e.xin] if isinstance(e, ConvEntry) else e.terms if isinstance(e, SumEntry) else e.vals
            if isinstance(e, SumEntry):
                self._producer_sum[id(e.out)] = e
            for v in reads:
                if isinstance(e, (ConvEntry, SumEntry)):
                    self._relu_of[id(v.act)] = v.relu
                self._first_use.setdefault(id(v.act), ti)
                self._use_lanes.setdefault(id(v.act), set()).add(e.lane)

    def _inter_grad_joins_at(self, act):
        """the optional external gradient of inter_feat joins in front of this op (run_backward cuts the program there)"""
        if act is self.inter_act and self.inter_gop is None:
            self.inter_gop = len(self.bwd)

    @staticmethod
    def _bn_term_of_sum(e):
        """the term of sum entry `e` a dgrad epilogue may gather BatchNorm-backward sums for: a raw conv output read
        through its BatchNorm (no ReLU, same resolution) by this sum alone"""
        return next((t for t, sh in zip(e.terms, e.shifts)
                     if t.act.bn is not None and t.act.nuse == 1 and sh == 0 and not t.relu), None)

    def _lane_mark_backward(self, ti, e):
        """a forward join is the backward fork of the same lanes, and vice versa"""
        for l in sorted(self._wred):
            self._flush_wred(l)
        self.bwd.lane = 0
        if self.batch_sums and e.sums:
            # the backward of the module's fuse sums (a dozen reduce / finalize / apply passes over tensors of
            # a few MB, three or four per lane in a row) runs as three batched launches on lane 0 instead:
            # no fork / join around it
            if not e.fork:
                self._batch = {C.OP_POOL_REDUCE: [], C.OP_BN_BWD_REDUCE: [], C.OP_BN_BWD_FINALIZE: [], C.OP_GRAD_TERM: []}
            else:
                self._flush_batch()
        elif not e.fork:
            self.bwd.fork(e.lanes)
        else:
            self.bwd.join(e.lanes)
        if e.fork:
            if self.defer_wgrad and ti == self._first_fork:
                self._emit_deferred_wgrads()
            if self.wlane:
                self.bwd.sync(self.wlane, 0)
            # every gradient of this module (and of everything after it) is complete here
            nxt = next((t for t in self.tape[ti + 1:] if isinstance(t, ConvEntry)), None)
            if nxt is not None and self.batch_wred:
                self.bucket_marks.append((len(self.bwd), nxt.crec.prefix))
        self._in_region = not e.fork

    def _cat_backward(self, e):
        vals, cat = e.vals, e.cat
        self._inter_grad_joins_at(cat)
        assert not any(v.act.ginit for v in vals)
        self.bwd.add(ops.make(C.OP_BILINEAR_CAT_BWD, dtype=self.dtid, nbr=len(vals), n=cat.N, h=cat.H, w=cat.W,
                              hs=[v.act.H for v in vals], ws=[v.act.W for v in vals],
                              cs=[v.act.C for v in vals], align=1.0 if e.align else 0.0, cat=C.ptr(cat.g),
                              x=[C.ptr(v.act.g) for v in vals]))
        for v in vals:
            v.act.ginit = True

    def _sum_backward(self, e):
        out = e.out
        self._inter_grad_joins_at(out)
        if not out.ginit:
            # no consumer produced a gradient (cannot happen for this network)
            raise RuntimeError('no gradient reaches ' + out.name)
        mask = C.ptr(out.t) if e.relu_out else None
        fusable = self._bn_term_of_sum(e)
        plain = [t for t in e.terms if not (t.act.bn is not None and t.act.nuse == 1)]
        # one BN term and one identity/accumulating term share dz: written by the same pass
        paired = (fusable, plain[0]) if fusable is not None and plain else (None, None)
        pooled = self._pool_reduce(e, mask)
        for t, sh in zip(e.terms, e.shifts):
            a = t.act
            if t is paired[1]:
                continue
            if a.bn is not None and a.nuse == 1 and self.training:
                # single consumer: fuse pooling + masks + BatchNorm backward
                self._bn_backward(a, C.ptr(out.g), mask, sh, t.relu,
                                  extra=paired[1].act if t is paired[0] else None, pooled=pooled.get(id(a)))
            else:
                # accumulate d(post-activation value); BN backward runs at the producer
                assert sh == 0
                self._emit(ops.make(C.OP_GRAD_TERM, dtype=self.dtid, n=a.N, h=a.H, w=a.W, c=a.C,
                                    accumulate=1 if a.ginit else 0, dst=C.ptr(a.g), g=C.ptr(out.g), mask=mask))
                a.ginit = True

    def _pool_reduce(self, e, mask):
        """the nearest-up-sampled terms (from the branches below this output): ONE walk over out.g and the mask
        pools every level, stores each level's dz and gathers its sums (HR_OP_POOL_REDUCE).
        -> {id(act): (partial rows, blocks)} of the terms it served"""
        out, pooled = e.out, {}
        ups = sorted([(sh, t) for t, sh in zip(e.terms, e.shifts)
                      if sh > 0 and t.act.bn is not None and t.act.nuse == 1 and self.training and not t.relu
                      and t.act.bwd_rows is None], key=lambda q: q[0])
        if (ups and [q[0] for q in ups] == list(range(1, len(ups) + 1)) and len(ups) <= 3
                and out.H % (1 << len(ups)) == 0 and out.W % (1 << len(ups)) == 0
                and 256 // (out.C // (4 if self.dt == torch.float32 else 8)) >= 4 ** (len(ups) - 1)
                and _knob('HRNET_POOL_REDUCE', '1') != '0' and _knob('HRNET_KEEP_DZ', '1') != '0'):
            pblocks = C.call('hrnet_ew_table_blocks', C.OP_POOL_REDUCE, self.dtid, out.N, out.H >> 1, out.W >> 1, out.C)
            for sh, t in ups:
                pooled[id(t.act)] = (self._f32(pblocks * 2 * out.C), pblocks)
            self._emit(ops.make(C.OP_POOL_REDUCE, dtype=self.dtid, n=out.N, h=out.H, w=out.W, c=out.C, nlev=len(ups),
                                g=C.ptr(out.g), mask=mask, y=[C.ptr(t.act.t) for _, t in ups],
                                dz=[C.ptr(t.act.g) for _, t in ups],
                                partials=[C.ptr(pooled[id(t.act)][0]) for _, t in ups]))
        return pooled

    # ---- backward of a conv entry: BatchNorm backward, bias gradient, weight gradient, input gradient ----
    def _conv_backward(self, ti, e):
        y = e.y
        self.bwd.tags[len(self.bwd)] = e.crec.prefix
        if not y.ginit:
            raise RuntimeError('no gradient reaches ' + y.name)
        if e.bnrec is not None and not y.bn_done:
            # y.g holds d(post-activation) summed over consumers -> d(raw), in place
            self._bn_backward(y, C.ptr(y.g), None, 0, self._relu_of.get(id(y), False))
        self._bias_grad(e.crec, y, e.bnrec)
        self._conv_wgrad(ti, e)
        if not self._head_bwd_stats(e) and e.xin.act.g is not None:
            self._conv_dgrad(ti, e)
        self._bucket_mark_after_conv(e.crec, e.lane)

    def _bias_grad(self, crec, y, bnrec):
        # a bias in front of a batch-statistics BatchNorm has an exactly zero gradient (the BatchNorm-backward
        # gradient sums to zero over every channel; autograd's value is rounding noise): no pass over dY
        if crec.mod.bias is None or (bnrec is not None and self.training):
            return
        blocks = C.call('hrnet_reduce_blocks', 1, 1, y.pixels, y.C)
        self.max_bwd_part = max(self.max_bwd_part, blocks * y.C)
        i = self.bwd.add(ops.make(C.OP_BIAS_GRAD, dtype=self.dtid, pixels=y.pixels, cp=y.C, c=crec.Cout,
                                  accumulate=1, dy=C.ptr(y.g), dbias=C.ptr(self.net.grad_of(crec.mod.bias))))
        self._scratch(self.bwd, i, ops.slot(C.OP_BIAS_GRAD, 'p', 'scratch'), 'bwdpart')

    def _conv_wgrad(self, ti, e):
        net, xin, crec, stride, y, lane = self.net, e.xin, e.crec, e.stride, e.y, e.lane
        x, w = xin.act, crec.mod.weight
        ks = 1 if crec.stem else crec.ks
        # the weight gradient is off the critical path: it runs on its own lane once dY is final
        if self.wlane and (self.wlane_all or lane == 0):
            self.bwd.sync(lane, self.wlane)
            self.bwd.lane = self.wlane
        nsplit = C.call('hrnet_wgrad_splits', self.dtid, x.N, y.H, y.W, y.C, x.C, ks, stride)
        wflops = 2.0 * x.N * y.H * y.W * y.C * x.C * ks * ks
        deferred = (self.batch_wred and self.defer_wgrad and self._in_region and self._first_fork is not None
                    and ti > self._first_fork
                    and (self.defer_branch_wgrads or '.branches.' not in crec.prefix)
                    and (not self.dp_plan or net.is_late(w))
                    and self._defer_flops + wflops <= self._defer_budget)
        if deferred:
            self._defer_flops += wflops
        if deferred and nsplit > 1:
            nsplit = self._deferred_splits(nsplit, x, y, ks, stride)
        # (the stem's weights are a flattened 3x3x3 kernel over im2col columns: its slab layout stays)
        direct = self.batch_wred and self.wgrad_atomic and not crec.stem
        wgrad = dict(dtype=self.dtid, n=x.N, h=x.H, w=x.W, cin=x.C, ho=y.H, wo=y.W, cout=y.C, ks=ks, stride=stride,
                     in_relu=1 if xin.relu else 0, nsplit=nsplit, atomic=1 if direct else 0,
                     cout_real=crec.Cout, cin_real=crec.Cin, x=C.ptr(x.t), dy=C.ptr(y.g),
                     in_scale=C.ptr(xin.bn.scale) if xin.bn else None,
                     in_shift=C.ptr(xin.bn.shift) if xin.bn else None)
        if self.batch_wred:
            slabs, ent = net.grad_of(w), None        # (atomic: the launch adds into the OIHW gradient itself)
            if not direct:
                slabs = self._f32(nsplit * y.C * ks * ks * x.C)
                self.slab_bytes += slabs.numel() * 4
                ent = dict(slabs=C.ptr(slabs), grad=C.ptr(net.grad_of(w)), nsplit=nsplit, Cout_pad=y.C, Cin_pad=x.C,
                           ks=crec.ks if crec.stem else ks, Cout=crec.Cout, Cin=crec.Cin,
                           kflat=1 if crec.stem else 0, accumulate=1)
            self._place_wgrad(ops.make(C.OP_WGRAD, slabs=C.ptr(slabs), **wgrad), ent, wflops, crec, lane, deferred)
        else:
            self.max_slab = max(self.max_slab, nsplit * y.C * ks * ks * x.C)
            i = self.bwd.add(ops.make(C.OP_WGRAD, **wgrad))
            self._scratch(self.bwd, i, ops.slot(C.OP_WGRAD, 'p', 'slabs'), 'slab')
            # (ks: the real taps of the flattened stem kernel)
            i = self.bwd.add(ops.make(C.OP_WGRAD_REDUCE, nsplit=nsplit, cout_pad=y.C, cin_pad=x.C,
                                      ks=crec.ks if crec.stem else ks, cout=crec.Cout, cin=crec.Cin,
                                      kflat=1 if crec.stem else 0, accumulate=1, grad=C.ptr(net.grad_of(w))))
            self._scratch(self.bwd, i, ops.slot(C.OP_WGRAD_REDUCE, 'p', 'slabs'), 'slab')
        self.bwd.lane = lane

    def _deferred_splits(self, nsplit, x, y, ks, stride):
        # A deferred launch runs in the background of the single-lane tail: it does not need the
        # parallelism of many splits, and every split is a slab written and read back - but it must
        # keep ~100 workgroups (the wide w48 layers have few splits to begin with: dividing those
        # cost 6 ms per step). measured (w32 B=64, ms/step): divisor 1: 19.97, 2: 19.56, 4: 19.49, 8: 19.97
        div = int(_knob('HRNET_DEFER_SPLIT_DIV', '4'))
        tiles = C.call('hrnet_wgrad_tiles', self.dtid, x.N, y.H, y.W, y.C, x.C, ks, stride)
        per = C.call('hrnet_wgrad_blocks_per_split', self.dtid, y.H, y.W, y.C, x.C, ks, stride)
        floor_ = min(nsplit, -(-96 // max(per, 1)))
        nsplit = max(1, floor_, nsplit // max(div, 1))
        while nsplit > 1 and tiles % nsplit != 0:
            nsplit -= 1
        return nsplit

    def _offload_lane(self):
        """the next side lane (round robin) for a launch that leaves lane 0, ordered behind what lane 0 holds so far"""
        l = 1 + self._offload_rr % max(1, self.nlanes - 1)
        self._offload_rr += 1
        self.bwd.sync(0, l)
        self._offload_lanes.add(l)
        return l

    def _count_wgrad_bytes(self, crec, lane):
        if lane == 0:
            self._wred_bytes += crec.Cout * crec.Cin * crec.ks * crec.ks * 4      # (towards the next bucket mark)

    def _place_wgrad(self, wop, ent, wflops, crec, lane, deferred):
        """where weight-gradient launch `wop` runs; ent: the HrWredEnt fields of its slab sum (None: the atomic form)"""
        if deferred:
            # x.t, y.g and the BatchNorm coefficients of xin stay untouched until the program ends
            self._deferred.append((wop, ent, wflops, self.net.offsets[id(crec.mod.weight)][0]))
            return
        if self.offload_wgrad and lane == 0 and not self._in_region:
            # a single-lane part of the pass (head, transition1, stem): its weight gradients are off the
            # dependency chain - they go to a side lane, which idles there (the head) or carries the
            # deferred launches (the tail); their gradient is complete at the end of the program
            l = self._offload_lane()
            self.bwd.add(wop, lane=l)
        else:
            l = self.bwd.lane
            self.bwd.add(wop)
            self._count_wgrad_bytes(crec, lane)
        if ent is not None:
            self._wred.setdefault(l, []).append(ent)

    def _head_bwd_stats(self, e):
        """the layer behind the head's BatchNorm (last_layer.3): its input gradient dz = W^T dY is a K = 32
        product per pixel - formed here only to gather the BatchNorm-backward sums, and formed AGAIN by
        the apply launch in _head_mix_backward (hrnet_head_bwd): dz is never stored or re-read.
        -> whether `e` is that layer (it has no input-gradient launch then)"""
        xin, crec, y = e.xin, e.crec, e.y
        x = xin.act
        if not (x is self._head_y and x.g is not None and xin.bn is not None and self.training
                and (1 if crec.stem else crec.ks) == 1
                and crec.mod.weight.shape[0] <= y.C and _knob('HRNET_HEAD_BWD', '1') != '0'
                and C.call('hrnet_head_mix_supported', self.dtid, y.C, x.C) == 1):
            return False
        nrows = C.call('hrnet_head_mix_rows', x.N, x.H, x.W)
        rows = self._f32(nrows * 2 * x.C)
        self.bwd.add(ops.make(C.OP_HEAD_BWD, dtype=self.dtid, n=x.N, h=x.H, w=x.W, k=y.C, cout=x.C, mode=1,
                              inner_relu=1 if xin.relu else 0, dy=C.ptr(y.g), wt=C.ptr(crec.wd), y=C.ptr(x.t),
                              out=C.ptr(rows), bn_scale=C.ptr(xin.bn.scale), bn_shift=C.ptr(xin.bn.shift)))
        x.bwd_rows = (rows, nrows)
        x.ginit = True
        self._head_bwd = (y, crec, 1 if xin.relu else 0)
        self.n_fused_bwdstats += 1
        return True

    def _conv_dgrad(self, ti, e):
        """input gradient = conv of dY with the transposed kernel (zero-stuffed for stride 2); the launch that writes the
        last contribution to x.g gathers the BatchNorm-backward sums behind x in its epilogue"""
        xin, crec, stride, y = e.xin, e.crec, e.stride, e.y
        x = xin.act
        ks = 1 if crec.stem else crec.ks
        bs = {}     # backward statistics: the BS_* slots, the rows and the masked store
        last = (self._first_use.get(id(x)) == ti and self._use_lanes.get(id(x)) == {e.lane}
                and x is not self.inter_act)
        target = None
        if self._fuse_stats and last and xin.bn is not None and x.nuse == 1:
            # x is a raw conv output read through its BatchNorm (+ReLU) by this conv alone
            target = x
            bs['bs_y'] = C.ptr(x.t)
            if xin.relu:
                bs.update(bs_scale=C.ptr(xin.bn.scale), bs_shift=C.ptr(xin.bn.shift))
        elif self._fuse_stats and last and xin.bn is None and id(x) in self._producer_sum:
            # x is the output of a sum: gather for its first plain BatchNorm term
            ps = self._producer_sum[id(x)]
            term = self._bn_term_of_sum(ps)
            if term is not None:
                target = term.act
                bs.update(bs_y=C.ptr(target.t), bs_mask=C.ptr(x.t) if ps.relu_out else None)
        if target is not None:
            nrows = C.call('hrnet_conv_rows_bwdstats', self.dtid, x.N, x.H, x.W, y.C, x.C, ks, stride)
            rows = self._f32(nrows * 2 * x.C)
            bs['stats'] = C.ptr(rows)
            target.bwd_rows = (rows, nrows)
            self.n_fused_bwdstats += 1
            if (target is not x and bs.get('bs_mask') is not None and id(x) in self._fused_out_ids
                    and _knob('HRNET_BS_STORE_MASKED', '1') != '0'):
                # x closes a block whose backward is a fused launch: this (last) contribution stores the
                # gradient already multiplied by x's ReLU mask - no separate mask pass over the tensor
                bs['bs_store_masked'] = 1
            # (a backward-statistics launch is bound to the kernel family its rows buffer was sized for)
            bs['route'] = C.call('hrnet_conv_route', self.dtid, x.N, x.H, x.W, y.C, x.C, ks, stride)
        self.bwd.add(ops.make(C.OP_CONV, dtype=self.dtid, n=y.N, h=y.H, w=y.W, cin=y.C, ho=x.H, wo=x.W, cout=x.C,
                              ks=ks, stride=stride, upz=1 if stride == 2 else 0,
                              accumulate=1 if x.ginit else 0, x=C.ptr(y.g), wgt=C.ptr(crec.wd), y=C.ptr(x.g),
                              **bs))
        x.ginit = True
        if bs.get('bs_store_masked'):
            x.gmasked = True

    # ---- backward of the head without its concat (head_mix) ----
    def _head_mix_backward(self, e):
        """G = d(raw y) (BatchNorm backward in place); g_j = up^T(G) at branch j's resolution (hrnet_upsample_bilinear_t);
        dW[:, slice j] = g_j^T x_j and dx_j = W_j^T g_j as 1x1 launches at branch resolution (g_0 = G, full resolution
        with K = C0): autograd of pose_hrnet.py:560-566, an eighth of the concat form's FLOPs"""
        lane, vals, crec, y, bnrec, ts, offs, align = e.lane, e.vals, e.crec, e.y, e.bnrec, e.ts, e.offs, e.align
        net = self.net
        self.bwd.tags[len(self.bwd)] = crec.prefix
        if not y.ginit:
            raise RuntimeError('no gradient reaches ' + y.name)
        if bnrec is not None and not y.bn_done and self._head_bwd is not None:
            # G = A*dz + B*y + C with dz = W3^T dHM formed again from the next layer's gradient (hrnet_head_bwd mode 2)
            ny, ncrec, relu_flag = self._head_bwd
            b = y.bn
            rows, nrows = y.bwd_rows
            self.bwd.add(self._bn_bwd_finalize_op(y, nrows, C.ptr(rows)))
            self.bwd.add(ops.make(C.OP_HEAD_BWD, dtype=self.dtid, n=y.N, h=y.H, w=y.W, k=ny.C, cout=y.C, mode=2,
                                  inner_relu=relu_flag, dy=C.ptr(ny.g), wt=C.ptr(ncrec.wd), y=C.ptr(y.t), out=C.ptr(y.g),
                                  bn_scale=C.ptr(b.scale), bn_shift=C.ptr(b.shift), coef=C.ptr(b.coef)))
            y.bn_done = True
        elif bnrec is not None and not y.bn_done:
            self._bn_backward(y, C.ptr(y.g), None, 0, self._relu_of.get(id(y), False))
        self._bias_grad(crec, y, bnrec)
        if ts:
            self.bwd.add(ops.make(C.OP_UPSAMPLE_T, dtype=self.dtid, n=y.N, h=y.H, w=y.W, c=y.C, nout=len(ts),
                                  align=1 if align else 0, out_h=[t.H for t in ts], out_w=[t.W for t in ts],
                                  g=C.ptr(y.g), out=[C.ptr(t.g) for t in ts]))
            for t in ts:
                t.ginit = True
        gw = net.grad_of(crec.mod.weight)
        direct = self.batch_wred and self.wgrad_atomic
        for j, v in enumerate(vals):
            x = v.act
            dy = y.g if j == 0 else ts[j - 1].g
            cj = offs[j + 1] - offs[j]
            gptr = gw.data_ptr() + 4 * offs[j]
            # ---- weight gradient of the column slice (rows crec.Cin floats apart)
            nsplit = C.call('hrnet_wgrad_splits', self.dtid, x.N, x.H, x.W, y.C, x.C, 1, 1)
            wgrad = dict(dtype=self.dtid, n=x.N, h=x.H, w=x.W, cin=x.C, ho=x.H, wo=x.W, cout=y.C, ks=1, stride=1,
                         nsplit=nsplit, atomic=1 if direct else 0, cout_real=crec.Cout, cin_real=cj,
                         ld=crec.Cin if direct else 0, x=C.ptr(x.t), dy=C.ptr(dy))
            side = self._offload_lane() if (self.offload_wgrad and lane == 0 and not self._in_region) else None
            if direct:
                self.bwd.add(ops.make(C.OP_WGRAD, slabs=gptr, **wgrad), lane=side)
            elif self.batch_wred:
                slabs = self._f32(nsplit * y.C * x.C)
                self.slab_bytes += slabs.numel() * 4
                ent = dict(slabs=C.ptr(slabs), grad=gptr, nsplit=nsplit, Cout_pad=y.C, Cin_pad=x.C, ks=1,
                           Cout=crec.Cout, Cin=cj, kflat=0, accumulate=1, ld=crec.Cin)
                self.bwd.add(ops.make(C.OP_WGRAD, slabs=C.ptr(slabs), **wgrad), lane=side)
                self._wred.setdefault(side if side is not None else self.bwd.lane, []).append(ent)
            else:
                self.max_slab = max(self.max_slab, nsplit * y.C * x.C)
                i = self.bwd.add(ops.make(C.OP_WGRAD, **wgrad))
                self._scratch(self.bwd, i, ops.slot(C.OP_WGRAD, 'p', 'slabs'), 'slab')
                i = self.bwd.add(ops.make(C.OP_WGRAD_REDUCE, nsplit=nsplit, cout_pad=y.C, cin_pad=x.C, ks=1,
                                          cout=crec.Cout, cin=cj, accumulate=1, ld=crec.Cin, grad=gptr))
                self._scratch(self.bwd, i, ops.slot(C.OP_WGRAD_REDUCE, 'p', 'slabs'), 'slab')
            if side is None and lane == 0:
                self._wred_bytes += crec.Cout * cj * 4
            # ---- input gradient: rows offs[j] .. offs[j+1] of the transposed packed weight ([Cin][Cout_pad])
            if x.g is not None:
                wd = crec.wd.data_ptr() + offs[j] * crec.Cout_pad * self.esize
                self.bwd.add(ops.make(C.OP_CONV, dtype=self.dtid, n=x.N, h=x.H, w=x.W, cin=y.C, ho=x.H, wo=x.W, cout=x.C,
                                      ks=1, stride=1, accumulate=1 if x.ginit else 0, x=C.ptr(dy), wgt=wd, y=C.ptr(x.g)))
                x.ginit = True
        self._bucket_mark_after_conv(crec, lane)

    # ---- fused backward of a BasicBlock (conv3x3+BN+ReLU, conv3x3+BN, +x, ReLU: pose_hrnet.py:41-57) ----
    def _find_fused_blocks(self):
        """tape indices of the 'sum' entries that close a BasicBlock (or a Bottleneck) all of whose convs the fused
        kernels serve -> 'basic' / 'bottleneck' / 'bottleneck_ds'"""
        out = {}
        if not self.training or _knob('HRNET_FUSED_BWD', '1') == '0':
            return out
        # Widths above 64 (the 128-channel instantiation): only where the LDS-ring pipeline does NOT serve the block's
        # input-gradient convs. w32's 128-channel branch (16x16 maps) has the ring: fused loses there, 19.32 vs 18.82 ms -
        # its four input-channel blocks re-stage the same 128-channel g tile. w48's 96-channel branch (48x36 maps) has
        # only the tile-walking body: fused wins, 28.72 vs 29.92 ms/step (round 4).
        maxc = int(_knob('HRNET_FUSED_MAXC', '128'))     # (tests: restrict the fused path to narrow layers)
        pointwise = _knob('HRNET_FUSED_PW', '1') != '0'

        def route(x, cout, cin):
            return C.call('hrnet_conv_route', self.dtid, x.N, x.H, x.W, cout, cin, 3, 1)

        def fused3(cin, cout):
            return C.call('hrnet_bwd_fused_supported', self.dtid, cin, cout)

        def fused1(cin, cout):
            return C.call('hrnet_bwd_pw_supported', self.dtid, cin, cout)
        for ti, e in enumerate(self.tape):
            basic = self._block_chain(ti, (3, 3))
            neck = self._block_chain(ti, (1, 3, 1)) if pointwise else None
            neck_ds = self._block_chain(ti, (1, 3, 1), behind=1) if pointwise else None
            chain = basic or neck or neck_ds
            if not chain:
                continue
            xin, x, idt = chain[0].xin, chain[0].xin.act, e.terms[1]
            y1, y2, y3 = chain[0].y, chain[1].y, chain[-1].y
            ps = self._producer_sum.get(id(x))
            from_relu_sum = xin.bn is None and ps is not None and ps.relu_out
            if basic:
                # the mask the kernel applies to the gradient it stores for x is [a > 0], a = the conv's input as staged:
                # right when x is read through a ReLU, or is the (non-negative) output of a sum that ended in one
                if (idt.act is x and idt.bn is xin.bn and idt.relu == xin.relu and x.nuse == 2
                        and max(x.C, y1.C, y2.C) <= maxc
                        and (max(x.C, y1.C, y2.C) <= 64 or (route(x, y1.C, x.C) != 2 and route(x, y2.C, y1.C) != 2))
                        and fused3(x.C, y1.C) and fused3(y1.C, y2.C) and (xin.relu or from_relu_sum)):
                    out[ti] = 'basic'
            elif neck:
                # Bottleneck with an identity residual (pose_hrnet.py:60-105; layer1 blocks 1..3): conv1 1x1, conv2 3x3,
                # conv3 1x1, + x, ReLU - the pointwise convs through hrnet_conv1x1_bwd_fused
                if (idt.act is x and idt.bn is None and not idt.relu and x.nuse == 2 and from_relu_sum
                        and x is not self.inter_act
                        and fused1(y2.C, y3.C) and fused3(y1.C, y2.C) and fused1(x.C, y1.C)):
                    out[ti] = 'bottleneck'
            else:
                # ... and the first Bottleneck of layer1, whose residual is a 1x1 conv + BatchNorm of the same input
                # (pose_hrnet.py:98-99: downsample): conv1, conv2, conv3, downsample, sum
                ds = self.tape[ti - 1]
                if (idt.act is ds.y and idt.bn is ds.bnrec and ds.bnrec is not None and not idt.relu and ds.y.nuse == 1
                        and ds.xin.act is x and ds.xin.bn is xin.bn and ds.xin.relu == xin.relu and xin.relu
                        and xin.bn is not None and x.nuse == 2 and self._plain_conv(ds, 1) and x is not self.inter_act
                        and fused1(y2.C, y3.C) and fused1(x.C, ds.y.C) and fused3(y1.C, y2.C) and fused1(x.C, y1.C)):
                    out[ti] = 'bottleneck_ds'
        return out

    @staticmethod
    def _plain_conv(c, ks):
        """a stride-1 ks x ks conv entry without bias (what the fused backward kernels serve)"""
        return c.stride == 1 and c.crec.ks == ks and not c.crec.stem and c.crec.mod.bias is None

    def _block_chain(self, ti, kss, behind=0):
        """the conv entries (forward order) of the residual block the sum entry at `ti` closes, or None: a chain of
        plain convs of kernel sizes `kss`, each read through its own BatchNorm + ReLU by the next alone and the last
        through its BatchNorm by the sum's first term alone, then `behind` more convs (the residual's), then the
        two-term ReLU sum - all on one lane, with a gradient wanted for the block input"""
        T, n = self.tape, len(kss) + behind
        e = T[ti]
        if ti < n or not isinstance(e, SumEntry) or not all(isinstance(c, ConvEntry) for c in T[ti - n:ti]):
            return None
        chain, c = T[ti - n:ti - behind], e.terms[0]
        ok = (len(e.terms) == 2 and list(e.shifts) == [0, 0] and e.relu_out and len({t.lane for t in T[ti - n:ti + 1]}) == 1
              and c.act is chain[-1].y and c.bn is chain[-1].bnrec and c.bn is not None and not c.relu
              and chain[-1].y.nuse == 1
              and all(b.xin.act is a.y and b.xin.bn is a.bnrec and a.bnrec is not None and b.xin.relu and a.y.nuse == 1
                      for a, b in zip(chain, chain[1:]))
              and all(self._plain_conv(cv, ks) for cv, ks in zip(chain, kss)) and chain[0].xin.act.g is not None)
        return chain if ok else None

    def _bn_bwd_finalize(self, y, reduce_from=None):
        """coefficients (and dgamma/dbeta) of y's BatchNorm backward from the sums a previous launch left in
        y.bwd_rows, or from a reduction pass over the (already masked) gradient `reduce_from`"""
        if y.bwd_rows is not None:
            rows, blocks = y.bwd_rows
            self.bwd.add(self._bn_bwd_finalize_op(y, blocks, C.ptr(rows)))
        else:
            blocks = C.call('hrnet_reduce_blocks', y.N, y.H, y.W, y.C)
            self.max_bwd_part = max(self.max_bwd_part, blocks * 2 * y.C)
            i = self.bwd.add(ops.make(C.OP_BN_BWD_REDUCE, dtype=self.dtid, n=y.N, h=y.H, w=y.W, c=y.C, g=reduce_from,
                                      y=C.ptr(y.t)))
            self._scratch(self.bwd, i, ops.slot(C.OP_BN_BWD_REDUCE, 'p', 'partials'), 'bwdpart')
            j = self.bwd.add(self._bn_bwd_finalize_op(y, blocks, None))
            self._scratch(self.bwd, j, ops.slot(C.OP_BN_BWD_FINALIZE, 'p', 'partials'), 'bwdpart')
        y.bn_done = True

    def _fused_conv_bwd(self, dz, y, xin, crec, dx, addend, mask_out, rows_for, lane, reduce_from=None):
        """one hrnet_conv3x3_bwd_fused / hrnet_conv1x1_bwd_fused launch: backward of `y = conv(xin)` given the masked
        gradient `dz` of y's BatchNorm output; writes the gradient of xin's activation into `dx` and y's
        weight-gradient slabs. rows_for: the raw activation whose BatchNorm-backward sums the launch gathers.
        The BatchNorm backward of y itself is finished first: by the launch (from the partial rows a previous
        launch left: HrBnBwdRef, no finalize launch in between) when there are few enough rows, else by
        _bn_bwd_finalize (rows, or a reduction pass over `reduce_from`)."""
        net, x = self.net, xin.act
        ks = crec.ks
        ref = None
        lim = 16384 if ks == 3 else 8192
        if (y.bwd_rows is not None and y.bwd_rows[1] * y.C <= lim
                and _knob('HRNET_BNBWD_INLINE', '1') != '0'):
            b, m = y.bn, y.bn.mod
            ref = C.HrBnBwdRef()
            ref.rows, ref.gamma = C.ptr(y.bwd_rows[0]), C.ptr(m.weight)
            ref.save_mean, ref.save_invstd = C.ptr(b.mean), C.ptr(b.invstd)
            ref.dgamma, ref.dbeta = C.ptr(self.net.grad_of(m.weight)), C.ptr(self.net.grad_of(m.bias))
            ref.count, ref.nrows, ref.accumulate = float(y.pixels), int(y.bwd_rows[1]), 1
            self._bnrefs.append(ref)             # host structs the recorded op points at
            self.n_inline_bnbwd += 1
            y.bn_done = True
        else:
            self._bn_bwd_finalize(y, reduce_from=reduce_from)
        if ks == 3:
            ns = C.call('hrnet_bwd_fused_splits', self.dtid, x.N, x.H, x.W, x.C, y.C)
            kind = C.OP_BWD_FUSED
        else:
            ns = C.call('hrnet_bwd_pw_splits', self.dtid, x.pixels, x.C, y.C)
            kind = C.OP_BWD_PW
            if rows_for is not None and not C.call('hrnet_bwd_pw_rows_supported', self.dtid, x.C, y.C):
                rows_for = None               # (the BatchNorm backward behind it runs its own reduction pass)
        w = crec.mod.weight
        atomic = 1 if (self.batch_wred and self.wgrad_atomic
                       and (ks == 3 or (crec.Cout == y.C and crec.Cin == x.C))) else 0
        if atomic:
            slabs = net.grad_of(w)               # the launch adds into the OIHW gradient itself
        else:
            slabs = self._f32(ns * y.C * ks * ks * x.C)
            self.slab_bytes += slabs.numel() * 4
        rows = None
        if rows_for is not None:
            rows = self._f32(ns * 2 * x.C)
            rows_for.bwd_rows = (rows, ns)
            self.n_fused_bwdstats += 1
        self.bwd.add(ops.make(kind, dtype=self.dtid, n=x.N, h=x.H, w=x.W, cin=x.C, cout=y.C, in_relu=1 if xin.relu else 0,
                              mask_out=1 if mask_out else 0, atomic=atomic, cout_real=crec.Cout, cin_real=crec.Cin,
                              dz=dz, y=C.ptr(y.t), coef=None if ref is not None else C.ptr(y.bn.coef), x=C.ptr(x.t),
                              in_scale=C.ptr(xin.bn.scale) if xin.bn else None,
                              in_shift=C.ptr(xin.bn.shift) if xin.bn else None, wt=C.ptr(crec.wd), dx=dx, addend=addend,
                              rows=C.ptr(rows), bs_y=C.ptr(rows_for.t) if rows_for is not None else None,
                              slabs=C.ptr(slabs), bnref=ctypes.addressof(ref) if ref is not None else None))
        if atomic:
            self._count_wgrad_bytes(crec, lane)
        elif self.batch_wred:
            self._wred.setdefault(lane, []).append(dict(
                slabs=C.ptr(slabs), grad=C.ptr(net.grad_of(w)), nsplit=ns, Cout_pad=y.C, Cin_pad=x.C, ks=ks,
                Cout=crec.Cout, Cin=crec.Cin, kflat=0, accumulate=1))
            self._count_wgrad_bytes(crec, lane)
        else:
            self.bwd.add(ops.make(C.OP_WGRAD_REDUCE, nsplit=ns, cout_pad=y.C, cin_pad=x.C, ks=ks, cout=crec.Cout,
                                  cin=crec.Cin, accumulate=1, slabs=C.ptr(slabs), grad=C.ptr(net.grad_of(w))))

    def _mask_gradient(self, out):
        """out.g *= [out > 0], in place: the ReLU mask the fused launches expect on the gradient they read (applied
        once, where the block output's gradient came from unfused consumers)"""
        if not out.ginit:
            raise RuntimeError('no gradient reaches ' + out.name)
        if not out.gmasked:
            self.bwd.add(ops.make(C.OP_GRAD_TERM, dtype=self.dtid, n=out.N, h=out.H, w=out.W, c=out.C, dst=C.ptr(out.g),
                                  g=C.ptr(out.g), mask=C.ptr(out.t)))
            out.gmasked = True

    def _rows_target(self, x, xin):
        """the raw activation behind x whose BatchNorm backward needs (sum dz, sum dz*y) of x's gradient"""
        if x is self.inter_act:
            return None
        if xin.bn is not None:
            return x                             # x is a raw conv output read through its BatchNorm + ReLU
        ps = self._producer_sum.get(id(x))
        term = self._bn_term_of_sum(ps) if ps is not None else None
        return term.act if term is not None else None

    def _fused_bottleneck_backward(self, ti, downsample=False):
        """Bottleneck: fused launches for conv3 1x1, conv2 3x3, conv1 1x1 (+ the residual stream: the identity's
        masked gradient, or the input gradient of the downsample conv written first)"""
        out, lane = self.tape[ti].out, self.tape[ti].lane
        k = 1 if downsample else 0
        c1, c2, c3 = self.tape[ti - 3 - k:ti - k]
        (xin1, crec1, y1), (xin2, crec2, y2), (xin3, crec3, y3) = [(c.xin, c.crec, c.y) for c in (c1, c2, c3)]
        x = xin1.act
        self.bwd.tags[len(self.bwd)] = crec3.prefix
        assert not x.ginit and not y1.ginit and not y2.ginit and not y3.ginit
        self._mask_gradient(out)
        residual = C.ptr(out.g)              # identity: the masked d(out) joins the input gradient of conv1
        if downsample:
            xind, crecd, yd = self.tape[ti - 1].xin, self.tape[ti - 1].crec, self.tape[ti - 1].y
            assert not yd.ginit
            self.bwd.tags[len(self.bwd)] = crecd.prefix
            self._fused_conv_bwd(C.ptr(out.g), yd, xind, crecd, C.ptr(x.g), None, True, None, lane,
                                 reduce_from=C.ptr(out.g))
            yd.ginit = True
            residual = C.ptr(x.g)            # conv1's launch adds its own input gradient in place
            self.bwd.tags[len(self.bwd)] = crec3.prefix
        # conv3: dz = d(out) masked; its input is relu(bn2(y2))
        self._fused_conv_bwd(C.ptr(out.g), y3, xin3, crec3, C.ptr(y2.g), None, True, y2, lane,
                             reduce_from=C.ptr(out.g))
        y2.ginit = y2.gmasked = True
        y3.ginit = True
        self.bwd.tags[len(self.bwd)] = crec2.prefix
        self._fused_conv_bwd(C.ptr(y2.g), y2, xin2, crec2, C.ptr(y1.g), None, True, y1, lane,
                             reduce_from=C.ptr(y2.g))
        y1.ginit = y1.gmasked = True
        # conv1: its input is the block input x; the residual stream joins before the mask
        self.bwd.tags[len(self.bwd)] = crec1.prefix
        self._fused_conv_bwd(C.ptr(y1.g), y1, xin1, crec1, C.ptr(x.g), residual, True,
                             self._rows_target(x, xin1), lane, reduce_from=C.ptr(y1.g))
        x.ginit = x.gmasked = True
        self._bucket_mark_after_conv(crec1, lane)

    def _fused_block_backward(self, ti):
        out, lane = self.tape[ti].out, self.tape[ti].lane
        c1, c2 = self.tape[ti - 2:ti]
        (xin1, crec1, y1), (xin2, crec2, y2) = (c1.xin, c1.crec, c1.y), (c2.xin, c2.crec, c2.y)
        x = xin1.act
        self.bwd.tags[len(self.bwd)] = crec2.prefix
        assert not x.ginit and not y1.ginit and not y2.ginit
        self._mask_gradient(out)
        # conv2: dz = d(out) masked (it is also the identity branch's gradient); its input is relu(bn1(y1))
        self._fused_conv_bwd(C.ptr(out.g), y2, xin2, crec2, C.ptr(y1.g), None, True, y1, lane,
                             reduce_from=C.ptr(out.g))
        y1.ginit = y1.gmasked = True
        y2.ginit = True
        # conv1: its input is the block input x; the residual stream (the masked d(out)) joins before the mask
        self._fused_conv_bwd(C.ptr(y1.g), y1, xin1, crec1, C.ptr(x.g), C.ptr(out.g), True,
                             self._rows_target(x, xin1), lane)
        x.ginit = x.gmasked = True
        self._bucket_mark_after_conv(crec1, lane)

    def _emit_deferred_wgrads(self):
        """enqueue the recorded weight-gradient launches on the side lanes (largest first, least-loaded lane)"""
        # the deferred launches are small grids (32-64 workgroups each): more of them in flight than the three
        # branch lanes fill more of the chip beside the single-lane tail
        side = [l for l in range(1, 1 + self.defer_lanes)]
        if not self._deferred or not side:
            return
        keep = self.bwd.lane
        self.bwd.lane = 0
        self.bwd.fork(side)

        def emit(entries):
            load = {l: 0.0 for l in side}
            for wop, ent, cost, _off in sorted(entries, key=lambda d: -d[2]):
                l = min(side, key=lambda q: load[q])
                load[l] += cost
                self.bwd.add(wop, lane=l)
                if ent is not None:
                    self._wred.setdefault(l, []).append(ent)
        if self.dp_plan and _knob('HRNET_LATE_GROUPS', '1') != '0':
            # Data parallelism: the late region of the flat gradient (net._flatten: module by module) leaves in GROUPS of
            # ~16 MB while the tail runs, instead of in one piece when the program ends. Group by group (highest
            # offsets first: the modules the backward pass finished first): the group's deferred launches spread over
            # the side lanes, (slab mode: their ordered sums,) then the other side lanes are joined into the first one,
            # so that "everything enqueued on side[0] so far" covers the group - and every late gradient that was NOT
            # deferred, which the fork above put in front. hipnet.optim.GradSync issues the group's all-reduce from
            # that stream at the recorded op index (late_cuts): the exchange of group g travels while the launches of
            # group g + 1 run, and nothing of the late region is left when the program ends.
            net = self.net
            lo_all, hi_all = int(net.late_start), int(net.trainable_count)
            starts = sorted({off for (off, n) in (net.offsets[id(p)] for p in net.params if net.is_late(p))})
            target = int(_knob('HRNET_LATE_GROUP_MB', '16')) << 18            # floats per group
            bounds = [hi_all]
            for off in reversed(starts):
                if bounds[-1] - off >= target:
                    bounds.append(off)
            if bounds[-1] != lo_all:
                if len(bounds) > 1 and bounds[-1] - lo_all < target // 2:
                    bounds[-1] = lo_all               # a small remainder joins the last group
                else:
                    bounds.append(lo_all)
            for hi_g, lo_g in zip(bounds, bounds[1:]):
                emit([d for d in self._deferred if lo_g <= d[3] < hi_g])
                for l in side:
                    self._flush_wred(l)
                for l in side[1:]:
                    self.bwd.sync(l, side[0])
                self.late_cuts.append((len(self.bwd), lo_g, hi_g, side[0]))
            self.bwd.lane = 0
        else:
            emit(self._deferred)
        self._deferred_lanes = side
        self.n_deferred_wgrads = len(self._deferred)
        self._deferred = []
        self.bwd.lane = keep

    def _bucket_mark_after_conv(self, crec, lane):
        """a bucket mark behind the backward of a layer on the single-lane parts of the pass (batched slab sums: once
        ~16 MB of weight gradient have gathered)"""
        if lane != 0 or self._in_region:
            return
        if self.batch_wred:
            if self._wred_bytes < (16 << 20):
                return
            for l in sorted(self._wred):
                self._flush_wred(l)
            self.bwd.lane = 0
        if self.wlane:
            self.bwd.sync(self.wlane, 0)    # this bucket's weight gradients are complete
        self.bucket_marks.append((len(self.bwd), crec.prefix))

    def _flush_wred(self, lane):
        ents = self._wred.pop(lane, None)
        if not ents:
            return
        block = 0
        for e in ents:
            e['block0'] = block
            block += (e['Cout'] * e['Cin'] * e['ks'] * e['ks'] + 63) // 64
        keep = self.bwd.lane
        self.bwd.lane = lane
        i = self.bwd.add(ops.make(C.OP_WGRAD_REDUCE_TABLE, n=len(ents), blocks=block))
        self.bwd.lane = keep
        self._wred_tables.append((i, ents))
        if lane == 0 or lane == self.wlane:
            self._wred_bytes = 0

    def _upload_wred_tables(self):
        n = sum(len(e) for _, e in self._wred_tables)
        if not n:
            return
        arr = (C.HrWredEnt * n)()
        k = 0
        starts = []
        for i, ents in self._wred_tables:
            starts.append((i, k))
            for e in ents:
                for name, val in e.items():
                    setattr(arr[k], name, val)
                k += 1
        table = self._device_table(arr)
        slot = ops.slot(C.OP_WGRAD_REDUCE_TABLE, 'p', 'table')
        for i, k0 in starts:
            self.bwd.ops[i].p[slot] = C.ptr(table) + k0 * ctypes.sizeof(C.HrWredEnt)

    def _resolve_scratch(self):
        sizes = {'stats': max(self.max_stats, 1), 'slab': max(self.max_slab, 1), 'bwdpart': max(self.max_bwd_part, 1)}
        table = {}
        for prog, idx, slot, kind in self.pending:
            key = (kind, prog.lane_of(idx))    # concurrent lanes must not share scratch
            if key not in table:
                table[key] = self._f32(sizes[kind])
            prog.ops[idx].p[slot] = C.ptr(table[key])
        self.pending = []
        self.bwd.lane = 0

    def _side_streams(self):
        if self.nlanes <= 1:
            return None
        if self.streams is None:
            # lane 0 = PyTorch's current stream. (Measured on MI355X: high-priority side streams made the
            # backward 2.5x slower, and a separate weight-gradient lane 7 % slower - its big grids take
            # CU slots from the critical path - so both stay off by default.)
            self.streams = [None] + [torch.cuda.Stream(device=self.dev)
                                     for _ in range(max(self.nlanes, self.defer_lanes))]
        return self.streams

    # ---- execution --------------------------------------------------------------------------
    def run_forward(self, x):
        self.gen += 1
        N = self.N
        oa, ia = self.out_act, self.inter_act
        hm = torch.empty((N, self.nj, oa.H, oa.W), dtype=torch.float32, device=self.dev)
        inter = torch.empty((N, ia.C, ia.H, ia.W), dtype=torch.float32, device=self.dev)
        self.fwd.set_ptr(self.in_op, ops.slot(C.OP_IM2COL_STEM, 'p', 'img'), x.data_ptr())
        self.fwd.set_ptr(self.out_op, ops.slot(C.OP_NHWC_TO_NCHW, 'p', 'dst'), hm.data_ptr())
        self.fwd.set_ptr(self.inter_op, ops.slot(C.OP_NHWC_TO_NCHW, 'p', 'dst'), inter.data_ptr())
        self.fwd.run(streams=self._side_streams())
        return hm, inter

    def run_backward(self, g_hm, g_inter=None, segment_hook=None):
        self.bwd.set_ptr(self.gout_op, ops.slot(C.OP_NCHW_TO_NHWC, 'p', 'src'), g_hm.data_ptr())
        if g_inter is not None:
            # d(inter_feat) joins the gradient of stage3's branch-0 output before its consumers'
            # contributions are read: run up to that op, add it, continue
            cut = self.inter_gop
            self._run_segments(0, cut, segment_hook, last=False)     # stage 4's buckets are exchanged on the way
            ia = self.inter_act
            tmp = torch.empty(ia.N * ia.H * ia.W * ia.C * self.esize, dtype=torch.uint8, device=self.dev)
            C.call('hrnet_nchw_to_nhwc', self.dtid, g_inter.data_ptr(), tmp.data_ptr(), ia.N, ia.H, ia.W, ia.C,
                   ia.C, C.stream_ptr())
            C.call('hrnet_grad_term', self.dtid, ia.g.data_ptr(), tmp.data_ptr(), None, None, None, None, None,
                   ia.N, ia.H, ia.W, ia.C, 0, 0, 1, C.stream_ptr())
            self._run_segments(cut, len(self.bwd), segment_hook)
        else:
            self._run_segments(0, len(self.bwd), segment_hook)

    def _run_segments(self, lo, hi, hook, last=True):
        streams = self._side_streams()
        if hook is None:
            self.bwd.run(lo, hi, streams=streams)
            return
        cuts = [c for c in hook.cuts if lo < c <= hi and (c < hi or not last)]
        prev = lo
        for c in cuts:
            self.bwd.run(prev, c, streams=streams)
            hook.after(c)
            prev = c
        self.bwd.run(prev, hi, streams=streams)
        if last:
            hook.after(hi)
