"""The slot names of a recorded op: the enums of include/hrnet_hip.h against hipnet.ops.SLOTS and hipnet._capi.OP_*,
the rules a layout has to keep (no collisions, nothing on the lane slot, nothing under a table job's block range), and
ops.make() against arrays written out by hand - the binary layout the raw-index GPU tests and csrc/api.hip use.
Needs neither a GPU nor the library."""
import os
import re
import struct

import pytest

from hipnet import _capi as C
from hipnet import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, 'include', 'hrnet_hip.h')
SLOT_NAME = re.compile(r'^HR_(\w+?)_([IFP])_(\w+)$')


def _parse_header():
    """-> (every enumerator: value, kind name -> table prefix as the 'slots of HR_OP_...' comments declare it)"""
    text = open(HEADER).read()
    values = {}
    for body in re.findall(r'\benum\s*\{(.*?)\}', re.sub(r'/\*.*?\*/', '', text, flags=re.S), flags=re.S):
        nxt = 0
        for item in filter(None, (t.strip() for t in body.split(','))):
            name, _, expr = (t.strip() for t in item.partition('='))
            if expr:
                nxt = values[expr] if expr in values else int(expr, 0)
            assert name not in values, name
            values[name] = nxt
            nxt += 1
    prefix_of = {}
    for m in re.finditer(r'/\* slots of ((?:HR_OP_\w+(?:, )?)+):.*?\*/\s*enum \{ HR_(\w+?)_[IFP]_', text, flags=re.S):
        for kind in m.group(1).split(', '):
            assert kind not in prefix_of, kind
            prefix_of[kind] = m.group(2)
    return values, prefix_of


VALUES, PREFIX_OF = _parse_header()
KIND_NAMES = {name[3:]: value for name, value in VALUES.items() if name.startswith('HR_OP_')}      # OP_CONV: 1 ...


def _header_tables():
    tables = {}
    for name, value in VALUES.items():
        m = SLOT_NAME.match(name)
        if m and not name.startswith('HR_OP_'):
            tables.setdefault(m.group(1), {'i': {}, 'f': {}, 'p': {}})[m.group(2).lower()][m.group(3)] = value
    return tables


def _expanded(kind, arr, layout=None):
    """[(name or name[k], index)] of one array of a kind, the members of its families written out"""
    out = []
    for name, idx in (layout or ops.SLOTS[kind][arr]).items():
        stride, count = ops.FAMILIES.get((ops.PREFIX[kind], arr, name), (0, 1))
        out += [('{}[{}]'.format(name, k) if stride else name, idx + stride * k) for k in range(count)]
    return out


def test_op_kinds_of_the_header_and_the_binding_agree():
    binding = {n: getattr(C, n) for n in dir(C) if n.startswith('OP_')}
    assert binding == KIND_NAMES
    assert len(set(binding.values())) == len(binding)
    assert re.search(r'#define HR_LANE_SLOT {}\b'.format(C.LANE_SLOT), open(HEADER).read())


def test_slot_tables_of_the_header_and_of_ops_agree():
    tables = _header_tables()
    assert tables.pop('EWJOB') == {'i': ops.EWJOB, 'f': {}, 'p': {}}
    # every kind has a table, in the header and in ops, under the same prefix
    assert {'HR_' + n: p for n, p in ((n, ops.PREFIX[v]) for n, v in KIND_NAMES.items())} == PREFIX_OF
    assert set(ops.SLOTS) == set(ops.PREFIX) == set(KIND_NAMES.values())
    assert set(tables) == set(ops.PREFIX.values())
    for kind, prefix in ops.PREFIX.items():
        assert ops.SLOTS[kind] == tables[prefix], prefix
    for prefix, arr, name in ops.FAMILIES:
        assert name in tables[prefix][arr] and name[-1] in '01', (prefix, arr, name)


@pytest.mark.parametrize('kind', sorted(ops.SLOTS))
def test_layout_rules(kind):
    names = [n for arr in 'ifp' for n in ops.SLOTS[kind][arr]]
    assert len(set(names)) == len(names), 'make() takes a field by its name alone'
    for arr in 'ifp':
        slots = _expanded(kind, arr)
        assert len({idx for _, idx in slots}) == len(slots), (arr, slots)          # (no table declares an alias)
        assert all(0 <= idx < ops.SIZE[arr] for _, idx in slots), (arr, slots)
    assert C.LANE_SLOT not in [idx for _, idx in _expanded(kind, 'i')], 'i[18] is the lane'
    if kind in ops.JOB_KINDS:
        # the job form: the moved slots at their job position, the block range on top
        moves = ops.JOB_MOVES.get(kind, {})
        job = {n: idx for n, idx in _expanded(kind, 'i') if n not in moves}
        under = [n for n, idx in job.items() if idx in (ops.EWJOB['BLOCK0'], ops.EWJOB['BLOCKS'])]
        assert not under, 'the block range of a table job would overwrite {}'.format(under)
        job.update({'job.' + j: ops.EWJOB[j] for j in ['BLOCK0', 'BLOCKS'] + list(moves.values())})
        assert len(set(job.values())) == len(job), job
        assert all(n in ops.SLOTS[kind]['i'] for n in moves)


def test_only_a_sum_job_moves_a_slot():
    assert ops.JOB_MOVES == {C.OP_SUM_TERMS: {'EPS_BITS': 'SUM_EPS_BITS'}}
    assert ops.SLOTS[C.OP_SUM_TERMS]['i']['EPS_BITS'] == ops.EWJOB['BLOCK0'] == 16
    assert (ops.EWJOB['BLOCKS'], ops.EWJOB['SUM_EPS_BITS']) == (17, 18)


def _arrays(op):
    return int(op.kind), [int(v) for v in op.i], [float(v) for v in op.f], [v for v in op.p]


def _bits(x):
    return struct.unpack('i', struct.pack('f', x))[0]


def _f32(x):
    return struct.unpack('f', struct.pack('f', x))[0]


def test_make_conv_matches_the_hand_written_layout():
    # an input-gradient launch with backward statistics, every slot distinct
    op = ops.make(C.OP_CONV, dtype=1, n=2, h=3, w=4, cin=5, ho=6, wo=7, cout=8, ks=9, stride=10, upz=11, in_relu=12,
                  accumulate=13, stats_atomic=14, bs_store_masked=15, in_dy=-16, in_dx=17, route=2,
                  in_inv_count=0.25, in_eps=1e-5,
                  x=100, wgt=101, in_scale=102, in_shift=103, bias=104, y=105, stats=106, bs_y=107, bs_mask=108,
                  bs_scale=109, bs_shift=110, in_sums=111, in_gamma=112, in_beta=113)
    assert _arrays(op) == (1, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, -16, 17, 2, 0],
                           [0.25, _f32(1e-5), 0.0, 0.0], list(range(100, 114)))


def test_make_sum_terms_matches_the_hand_written_layout_in_both_forms():
    # scale / shift arrays, three terms (hrnet_sum_terms)
    op = ops.make(C.OP_SUM_TERMS, dtype=1, n=2, h=64, w=48, c=32, nterms=3, relu_out=1, sh=[0, 1, 2], relu=[0, 1, 0],
                  out=10, src=[11, 12, 13], scale=[None, 22, 23], shift=[None, 32, 33])
    assert _arrays(op) == (5, [1, 2, 64, 48, 32, 3, 1, 0, 1, 2, 0, 0, 1, 0, 0, 0, 0, 0, 0], [0.0] * 4,
                           [10, 11, 12, 13, None, None, 22, 23, None, None, 32, 33, None, None])
    # batch sums (hrnet_sum_terms_bnref): sums in the scale slots, gamma in the shift slots, 1 / count per term, the
    # mode bits and the bits of eps behind the ReLU flags
    op = ops.make(C.OP_SUM_TERMS, dtype=0, n=1, h=8, w=8, c=16, nterms=2, relu_out=1, sh=[0, 0], relu=[0, 0],
                  out=10, src=[11, 12], scale=[21, None], shift=[31, None], inv_count=[1.0 / 64, 0.0], sums_mode=1,
                  eps_bits=ops.f32_bits(1e-5))
    assert _arrays(op) == (5, [0, 1, 8, 8, 16, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, _bits(1e-5), 0, 0],
                           [1.0 / 64, 0.0, 0.0, 0.0],
                           [10, 11, 12, None, None, 21, None, None, None, 31, None, None, None, None])
    assert ops.f32_bits(1e-5) == 0x3727c5ac
    # as a job of a table-driven launch: the block range takes i[16] / i[17], the eps bits move to i[18]
    ops.set_job_blocks(op, 7, 5)
    assert [int(v) for v in op.i][15:] == [1, 7, 5, _bits(1e-5)]


def test_make_grad_term_with_the_second_destination_matches_the_hand_written_layout():
    op = ops.make(C.OP_GRAD_TERM, dtype=1, n=2, h=3, w=4, c=8, accumulate=1, accumulate2=1, dst=10, g=11, mask=12, y=13,
                  scale=14, shift=15, coef=16, dst2=17)
    assert _arrays(op) == (6, [1, 2, 3, 4, 8, 0, 0, 1, 1] + [0] * 10, [0.0] * 4, [10, 11, 12, 13, 14, 15, 16, 17] + [None] * 6)
    ops.set_job_blocks(op, 3, 9)
    assert [int(v) for v in op.i][16:] == [3, 9, 0]


def test_make_head_mix_matches_the_hand_written_layout():
    op = ops.make(C.OP_HEAD_MIX, dtype=1, n=2, h=64, w=48, c0=32, cout=480, nup=3, align=1, up_h=[32, 16, 8],
                  up_w=[24, 12, 6], rows_mode=1, x0=10, w0=11, bias=12, y=13, stats=14, t=[15, 16, 17])
    assert _arrays(op) == (26, [1, 2, 64, 48, 32, 480, 3, 1, 32, 24, 16, 12, 8, 6, 1, 0, 0, 0, 0], [0.0] * 4,
                           [10, 11, 12, 13, 14, 15, 16, 17] + [None] * 6)


def test_make_bwd_fused_matches_the_hand_written_layout():
    fields = dict(dtype=1, n=2, h=3, w=4, cin=32, cout=64, in_relu=1, mask_out=1, atomic=1, cout_real=60, cin_real=30,
                  dz=10, y=11, coef=12, x=13, in_scale=14, in_shift=15, wt=16, dx=17, addend=18, rows=19, bs_y=20, slabs=21,
                  bnref=22)
    want = ([1, 2, 3, 4, 32, 64, 1, 1, 1, 60, 30] + [0] * 8, [0.0] * 4, list(range(10, 23)) + [None])
    assert _arrays(ops.make(C.OP_BWD_FUSED, **fields)) == (21,) + want
    assert _arrays(ops.make(C.OP_BWD_PW, **fields)) == (23,) + want           # (the 1x1 form shares the slots)


def test_make_ew_table_takes_the_jobs_kind_as_a_field():
    op = ops.make(C.OP_EW_TABLE, jobs=3, blocks=40, kind=C.OP_GRAD_TERM, dtype=1, sums=0, table=77)
    assert _arrays(op) == (25, [3, 40, 6, 1] + [0] * 15, [0.0] * 4, [77] + [None] * 13)


def test_make_refuses_what_does_not_fit():
    with pytest.raises(KeyError):
        ops.make(C.OP_CONV, dtype=1, weights=5)                  # unknown field
    with pytest.raises(KeyError):
        ops.make(C.OP_BN_BWD_REDUCE, coef=5)                     # a field of another kind
    with pytest.raises(TypeError):
        ops.make(C.OP_CONV, n=2.0)                               # a float in an integer slot
    with pytest.raises(OverflowError):
        ops.make(C.OP_FILL, bytes_lo=1 << 31)                    # does not fit int32 ...
    assert ops.make(C.OP_FILL, bytes_lo=ops.u32_bits(0xfffffff0)).i[0] == -16     # ... its bits do
    with pytest.raises(ValueError):
        ops.make(C.OP_SUM_TERMS, src=[1, 2, 3, 4, 5])            # more members than the family has
    with pytest.raises(TypeError):
        ops.make(C.OP_CONV, x='0x10')
    assert ops.slot(C.OP_CONV, 'p', 'stats') == 6 and ops.slot(C.OP_CONV_SUM, 'p', 'stats') == 8
    assert ops.slot(C.OP_HEAD_MIX, 'p', 'stats') == 4 and ops.slot(C.OP_WGRAD, 'p', 'slabs') == 4
