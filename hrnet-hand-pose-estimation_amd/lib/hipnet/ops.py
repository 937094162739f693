"""Slot names of a recorded op (HrOp), and constructors that fill an op by field name.

The table below mirrors the HR_<prefix>_<I|F|P>_<NAME> enums of include/hrnet_hip.h one to one
(tests/test_op_slots_cpu.py holds the two together); this file and the header are the only places
that know a slot by its number. Needs neither the library nor a GPU.
"""
import struct

from . import _capi as C


def _names(spec):
    """'A B C=5 D' -> {'A': 0, 'B': 1, 'C': 5, 'D': 6}"""
    out, k = {}, 0
    for tok in spec.split():
        name, _, at = tok.partition('=')
        k = int(at) if at else k
        out[name] = k
        k += 1
    return out


def _slots(i='', f='', p=''):
    return {'i': _names(i), 'f': _names(f), 'p': _names(p)}


_TABLE = _slots(i='N BLOCKS', p='TABLE')                 # WGRAD_REDUCE_TABLE, BN_FINALIZE_TABLE
_EVENT = _slots(p='EVENT')                               # EVENT_RECORD, STREAM_WAIT
_LAYOUT = _slots(i='DTYPE N H W CP C', p='SRC DST')      # NHWC_TO_NCHW, NCHW_TO_NHWC
_CAT = _slots(i='DTYPE NBR N H W HS0 WS0=9 CS0=13 ACCUMULATE=17', f='ALIGN', p='CAT X0')
_BWD_FUSED = _slots(i='DTYPE N H W CIN COUT IN_RELU MASK_OUT ATOMIC COUT_REAL CIN_REAL',
                    p='DZ Y COEF X IN_SCALE IN_SHIFT WT DX ADDEND ROWS BS_Y SLABS BNREF')

# kind -> enum prefix in the header (HR_<prefix>_I_<NAME> ...)
PREFIX = {
    C.OP_CONV: 'CONV', C.OP_WGRAD: 'WGRAD', C.OP_WGRAD_REDUCE: 'WGRAD_REDUCE', C.OP_BN_FINALIZE: 'BN_FINALIZE',
    C.OP_SUM_TERMS: 'SUM', C.OP_GRAD_TERM: 'GRAD_TERM', C.OP_BN_BWD_REDUCE: 'BN_BWD_REDUCE',
    C.OP_BN_BWD_FINALIZE: 'BN_BWD_FINALIZE', C.OP_BILINEAR_CAT: 'CAT', C.OP_BILINEAR_CAT_BWD: 'CAT',
    C.OP_IM2COL_STEM: 'IM2COL', C.OP_NHWC_TO_NCHW: 'LAYOUT', C.OP_NCHW_TO_NHWC: 'LAYOUT',
    C.OP_PACK_WEIGHTS: 'PACK', C.OP_BIAS_GRAD: 'BIAS_GRAD', C.OP_FILL: 'FILL', C.OP_PACK_TABLE: 'PACK_TABLE',
    C.OP_EVENT_RECORD: 'EVENT', C.OP_STREAM_WAIT: 'EVENT', C.OP_WGRAD_REDUCE_TABLE: 'TABLE',
    C.OP_BWD_FUSED: 'BWD_FUSED', C.OP_BN_FINALIZE_TABLE: 'TABLE', C.OP_BWD_PW: 'BWD_FUSED',
    C.OP_CONV_SUM: 'CONV_SUM', C.OP_EW_TABLE: 'EW_TABLE', C.OP_HEAD_MIX: 'HEAD_MIX', C.OP_UPSAMPLE_T: 'UPSAMPLE_T',
    C.OP_HEAD_BWD: 'HEAD_BWD', C.OP_POOL_REDUCE: 'POOL',
}

# kind -> {'i': {NAME: index}, 'f': {...}, 'p': {...}}. Kinds that share a prefix share one layout.
SLOTS = {
    C.OP_CONV: _slots(i='DTYPE N H W CIN HO WO COUT KS STRIDE UPZ IN_RELU ACCUMULATE STATS_ATOMIC BS_STORE_MASKED '
                        'IN_DY IN_DX ROUTE',
                      f='IN_INV_COUNT IN_EPS',
                      p='X WGT IN_SCALE IN_SHIFT BIAS Y STATS BS_Y BS_MASK BS_SCALE BS_SHIFT IN_SUMS IN_GAMMA IN_BETA'),
    C.OP_WGRAD: _slots(i='DTYPE N H W CIN HO WO COUT KS STRIDE IN_RELU NSPLIT ATOMIC COUT_REAL CIN_REAL LD',
                       p='X DY IN_SCALE IN_SHIFT SLABS'),
    C.OP_WGRAD_REDUCE: _slots(i='NSPLIT COUT_PAD CIN_PAD KS COUT CIN KFLAT ACCUMULATE LD', p='SLABS GRAD'),
    C.OP_BN_FINALIZE: _slots(i='TILES C TRAINING', f='COUNT MOMENTUM EPS',
                             p='STATS GAMMA BETA RUNNING_MEAN RUNNING_VAR NUM_BATCHES_TRACKED SCALE SHIFT SAVE_MEAN '
                               'SAVE_INVSTD'),
    C.OP_SUM_TERMS: _slots(i='DTYPE N H W C NTERMS RELU_OUT SH0 RELU0=11 SUMS_MODE=15 EPS_BITS', f='INV_COUNT0',
                           p='OUT SRC0 SCALE0=5 SHIFT0=9'),
    C.OP_GRAD_TERM: _slots(i='DTYPE N H W C SH INNER_RELU ACCUMULATE ACCUMULATE2',
                           p='DST G MASK Y SCALE SHIFT COEF DST2'),
    C.OP_BN_BWD_REDUCE: _slots(i='DTYPE N H W C SH INNER_RELU', p='PARTIALS G MASK Y SCALE SHIFT DZ'),
    C.OP_BN_BWD_FINALIZE: _slots(i='BLOCKS C ACCUMULATE', f='COUNT',
                                 p='PARTIALS GAMMA SAVE_MEAN SAVE_INVSTD DGAMMA DBETA COEF'),
    C.OP_BILINEAR_CAT: _CAT,
    C.OP_BILINEAR_CAT_BWD: _CAT,
    C.OP_IM2COL_STEM: _slots(i='DTYPE N C H W HO WO KPAD', p='IMG COLS'),
    C.OP_NHWC_TO_NCHW: _LAYOUT,
    C.OP_NCHW_TO_NHWC: _LAYOUT,
    C.OP_PACK_WEIGHTS: _slots(i='DTYPE COUT CIN KS COUT_PAD CIN_PAD MODE', p='SRC PACKED'),
    C.OP_BIAS_GRAD: _slots(i='DTYPE PIXELS CP C ACCUMULATE', p='DY DBIAS SCRATCH'),
    C.OP_FILL: _slots(i='BYTES_LO BYTES_HI', p='DST'),
    C.OP_PACK_TABLE: _slots(i='DTYPE N BLOCKS', p='TABLE'),
    C.OP_EVENT_RECORD: _EVENT,
    C.OP_STREAM_WAIT: _EVENT,
    C.OP_WGRAD_REDUCE_TABLE: _TABLE,
    C.OP_BWD_FUSED: _BWD_FUSED,
    C.OP_BN_FINALIZE_TABLE: _TABLE,
    C.OP_BWD_PW: _BWD_FUSED,
    C.OP_CONV_SUM: _slots(i='DTYPE N H W CIN COUT KS STATS_ATOMIC', f='IN_INV_COUNT IN_EPS',
                          p='X WGT IN_SCALE IN_SHIFT IN_SUMS IN_GAMMA IN_BETA Y STATS X2 SIDE'),
    C.OP_EW_TABLE: _slots(i='JOBS BLOCKS KIND DTYPE SUMS', p='TABLE'),
    C.OP_HEAD_MIX: _slots(i='DTYPE N H W C0 COUT NUP ALIGN UP_H1 UP_W1 ROWS_MODE=14', p='X0 W0 BIAS Y STATS T1'),
    C.OP_UPSAMPLE_T: _slots(i='DTYPE N H W C NOUT ALIGN OUT_H1 OUT_W1 STREAMED=13', p='G OUT1'),
    C.OP_HEAD_BWD: _slots(i='DTYPE N H W K COUT MODE INNER_RELU', p='DY WT Y OUT BN_SCALE BN_SHIFT COEF'),
    C.OP_POOL_REDUCE: _slots(i='DTYPE N H W C NLEV', p='G MASK Y0 DZ0 PARTIALS0'),
}

# indexed families: (prefix, array, base name) -> (stride, count); member k sits at base + stride * k
FAMILIES = {
    ('SUM', 'i', 'SH0'): (1, 4), ('SUM', 'i', 'RELU0'): (1, 4), ('SUM', 'f', 'INV_COUNT0'): (1, 4),
    ('SUM', 'p', 'SRC0'): (1, 4), ('SUM', 'p', 'SCALE0'): (1, 4), ('SUM', 'p', 'SHIFT0'): (1, 4),
    ('CAT', 'i', 'HS0'): (1, 4), ('CAT', 'i', 'WS0'): (1, 4), ('CAT', 'i', 'CS0'): (1, 4), ('CAT', 'p', 'X0'): (1, 4),
    ('HEAD_MIX', 'i', 'UP_H1'): (2, 3), ('HEAD_MIX', 'i', 'UP_W1'): (2, 3), ('HEAD_MIX', 'p', 'T1'): (1, 3),
    ('UPSAMPLE_T', 'i', 'OUT_H1'): (2, 3), ('UPSAMPLE_T', 'i', 'OUT_W1'): (2, 3), ('UPSAMPLE_T', 'p', 'OUT1'): (1, 3),
    ('POOL', 'p', 'Y0'): (3, 3), ('POOL', 'p', 'DZ0'): (3, 3), ('POOL', 'p', 'PARTIALS0'): (3, 3),
}

# A job of an OP_EW_TABLE launch is an HrOp of its own kind in a device table with its block range laid over two
# integer slots. A sum's EPS_BITS sits in one of them, so a sum job carries it in SUM_EPS_BITS instead - the slot that
# is the lane of a recorded op (a job has no lane).
EWJOB = {'BLOCK0': 16, 'BLOCKS': 17, 'SUM_EPS_BITS': 18}
JOB_KINDS = (C.OP_SUM_TERMS, C.OP_GRAD_TERM, C.OP_BN_BWD_REDUCE, C.OP_BN_BWD_FINALIZE, C.OP_POOL_REDUCE)
JOB_MOVES = {C.OP_SUM_TERMS: {'EPS_BITS': 'SUM_EPS_BITS'}}      # kind -> {single op's slot: the job's slot}

SIZE = {'i': 19, 'f': 4, 'p': 14}


def _locate(kind, field):
    """field name (any case; a family by its base name without the index) -> (array, index, stride, count)"""
    name = field.upper()
    layout = SLOTS[kind]
    for arr in ('i', 'f', 'p'):
        if name in layout[arr]:
            return arr, layout[arr][name], 0, 1
        for first in ('0', '1'):
            fam = FAMILIES.get((PREFIX[kind], arr, name + first))
            if fam is not None:
                return arr, layout[arr][name + first], fam[0], fam[1]
    raise KeyError('op kind {} ({}) has no field {!r}'.format(kind, PREFIX[kind], field))


def slot(kind, array, name):
    """index of a named slot inside op.i / op.f / op.p (for Program.set_ptr / set_int and scratch patches)"""
    return SLOTS[kind][array][name.upper()]


def f32_bits(x):
    """the bit pattern of float32(x) as the int32 an integer slot carries"""
    return struct.unpack('i', struct.pack('f', float(x)))[0]


def u32_bits(x):
    """an unsigned 32-bit value as the int32 of the same bits"""
    return struct.unpack('i', struct.pack('I', x))[0]


def _store(op, kind, field, arr, index, value):
    if arr == 'i':
        if isinstance(value, float) or not isinstance(value, int):
            raise TypeError('{}.{}: integer slot given {!r}'.format(PREFIX[kind], field, value))
        if not -2 ** 31 <= value < 2 ** 31:
            raise OverflowError('{}.{}: {} does not fit an int32 slot'.format(PREFIX[kind], field, value))
        op.i[index] = value
    elif arr == 'f':
        op.f[index] = float(value)
    else:
        if value is not None and not isinstance(value, int):
            raise TypeError('{}.{}: pointer slot given {!r}'.format(PREFIX[kind], field, value))
        op.p[index] = value


def make(kind, /, **fields):
    """an HrOp of `kind` with the named slots set (everything else zero). A family takes a sequence of up to its
    member count. Unknown names, integers that do not fit and floats in integer slots raise."""
    op = C.HrOp()
    op.kind = kind
    for field, value in fields.items():
        arr, index, stride, count = _locate(kind, field)
        if not stride:
            _store(op, kind, field, arr, index, value)
            continue
        value = list(value)
        if len(value) > count:
            raise ValueError('{}.{}: {} members given, the family has {}'.format(PREFIX[kind], field, len(value), count))
        for k, v in enumerate(value):
            _store(op, kind, field, arr, index + stride * k, v)
    return op


def set_job_blocks(op, block0, blocks):
    """make `op` a job of an OP_EW_TABLE launch: blocks [block0, block0 + blocks) of the launch are its own"""
    for name, job_name in JOB_MOVES.get(op.kind, {}).items():
        op.i[EWJOB[job_name]] = op.i[SLOTS[op.kind]['i'][name]]
    op.i[EWJOB['BLOCK0']], op.i[EWJOB['BLOCKS']] = block0, blocks
