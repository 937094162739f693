"""hipnet._header reads include/hrnet_hip.h and hipnet._capi binds what it found. Held here: prototypes written out by
hand that together use every type spelling of the header, the struct layouts, the rule that tells a status from a value,
and the reader's refusal of C it does not know. Needs no GPU; only the last test loads the library."""
import ctypes
import os

import pytest

from hipnet import _capi as C
from hipnet import _header

H = C.HEADER
I, F, D, I64, VP, CP = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_int64, ctypes.c_void_p, ctypes.c_char_p
PP, IP, FP, I64P = ctypes.POINTER(VP), ctypes.POINTER(I), ctypes.POINTER(F), ctypes.POINTER(I64)

# name -> (restype, returns a status, [(parameter, type)]), typed from the header by hand
EXPECTED = {
    'hrnet_conv2d': (I, True, [
        ('dtype', I), ('x', VP), ('w', VP), ('in_scale', VP), ('in_shift', VP), ('bias', VP), ('y', VP), ('stats', VP),
        ('N', I), ('H', I), ('W', I), ('Cin', I), ('Ho', I), ('Wo', I), ('Cout', I), ('ks', I), ('stride', I),
        ('upz', I), ('in_relu', I), ('accumulate', I), ('stream', VP)]),
    'hrnet_adam_step': (I, True, [
        ('param', VP), ('grad', VP), ('exp_avg', VP), ('exp_avg_sq', VP), ('n', I64), ('lr', F), ('beta1', F),
        ('beta2', F), ('eps', F), ('weight_decay', F), ('step', I), ('grad_scale', F), ('stream', VP)]),
    'hrnet_triangulate_ransac': (I, True, [
        ('pts', VP), ('to_frame', VP), ('proj', VP), ('pairs', VP), ('n_hyp', I), ('pairs_per_point', I),
        ('epsilon', D), ('X', VP), ('inliers', VP), ('pts_frame', VP), ('B', I), ('V', I), ('K', I), ('stream', VP)]),
    'hrnet_sum_terms_bnref': (I, True, [
        ('dtype', I), ('out', VP), ('N', I), ('Ho', I), ('Wo', I), ('C', I), ('nterms', I), ('src', PP), ('scale', PP),
        ('shift', PP), ('shifts', IP), ('relus', IP), ('relu_out', I), ('sums_mode', I), ('inv_counts', FP),
        ('eps', F), ('stream', VP)]),
    'hrnet_program_run_streams_timed': (I, True, [
        ('ops', ctypes.POINTER(C.HrOp)), ('n', I), ('streams', PP), ('nstreams', I), ('end_ms', FP)]),
    'hrnet_conv_kernel_name': (I, False, [
        ('dtype', I), ('N', I), ('Ho', I), ('Wo', I), ('Cin', I), ('Cout', I), ('ks', I), ('stride', I), ('upz', I),
        ('mode', I), ('buf', CP), ('buflen', I)]),
    'hrnet_conv3d_wgrad_scratch': (I, True, [
        ('dtype', I), ('N', I), ('D', I), ('H', I), ('W', I), ('Cin', I), ('Cout', I), ('ks', I), ('deconv', I),
        ('bytes', I64P), ('nsplit', IP), ('split_voxels', I64P)]),
    'hrnet_tf_layernorm_scratch': (I64, False, [('rows', I64), ('C', I)]),
    'hrnet_resize_normalize_u8': (I, True, [
        ('src', VP), ('src_bytes', I64), ('slots', VP), ('n', I), ('out_nchw', VP), ('Ho', I), ('Wo', I),
        ('mean3', FP), ('std3', FP), ('bgr', I), ('stream', VP)]),
    'hrnet_bn_finalize': (I, True, [
        ('stats', VP), ('tiles', I), ('C', I), ('count', F), ('gamma', VP), ('beta', VP), ('running_mean', VP),
        ('running_var', VP), ('num_batches_tracked', VP), ('momentum', F), ('eps', F), ('training', I), ('scale', VP),
        ('shift', VP), ('save_mean', VP), ('save_invstd', VP), ('stream', VP)]),
    'hrnet_event_create': (VP, False, []),
    'hrnet_last_error_string': (CP, False, []),
}


@pytest.mark.parametrize('name', sorted(EXPECTED))
def test_prototype_read_from_the_header_is_the_one_written_by_hand(name):
    restype, status, params = EXPECTED[name]
    p = H.protos[name]
    assert p.restype is restype and p.status is status
    assert [n for n, _ in p.params] == [n for n, _ in params]
    for (pname, got), (_, want) in zip(p.params, params):
        assert got is want, (pname, got, want)
    # ... and it is what the binding hands to ctypes and to call()
    assert C._SIGS[name] == [t for _, t in params] and (name in C._PLAIN) is (not status)


def test_binding_names_come_from_the_header():
    assert C.EXPORTED == sorted(H.protos) == sorted(C._SIGS) and len(C.EXPORTED) >= 130
    assert C._PLAIN == {n for n, p in H.protos.items() if not p.status}
    assert (C.HR_F32, C.HR_BF16, C.LANE_SLOT, C.ABI_VERSION) == (0, 1, 18, 2)
    assert (C.OP_CONV, C.OP_BWD_FUSED, C.OP_POOL_REDUCE) == (1, 21, 29)
    assert H.values['HR_E_BADOP'] == -3 and H.values['HR_VOLUME_MAX_MAP'] == 16384 and 'HR_HOST' not in H.values
    assert H.values['HR_SUM_I_EPS_BITS'] == 16 and H.values['HR_EWJOB_I_SUM_EPS_BITS'] == 18    # implicit / explicit
    for name in ('HrOp', 'HrBnBwdRef', 'HrPackEnt', 'HrWredEnt', 'HrBnEnt'):
        assert getattr(C, name) is H.structs[name]
    from hipnet import transformer
    from utils import volumetric
    assert (transformer.OP_LAYERNORM, transformer.OP_LINEAR, transformer.OP_ATTENTION, transformer.OP_FRAME_MEAN,
            transformer.ACT_NONE, transformer.ACT_GELU) == (0, 1, 2, 3, 0, 1)
    assert volumetric.METHODS == {'sum': 0, 'max': 1, 'softmax': 2} and volumetric.CONF == 3 and volumetric.SPLIT == 32


def test_struct_layouts():
    sizes = {name: ctypes.sizeof(cls) for name, cls in H.structs.items()}
    assert sizes == {'HrOp': 208, 'HrBnBwdRef': 64, 'HrPackEnt': 48, 'HrWredEnt': 56, 'HrBnEnt': 104}
    assert C.HrOp.p.offset == 96 and C.HrBnEnt.count.offset == 80
    assert [n for n, _ in C.HrOp._fields_] == ['kind', 'i', 'f', 'p']
    assert C.HrOp._fields_[1][1] is ctypes.c_int32 * 19 and C.HrOp._fields_[3][1] is VP * 14
    assert dict(C.HrBnBwdRef._fields_)['rows'] is VP and dict(C.HrBnBwdRef._fields_)['accumulate'] is ctypes.c_int32
    assert dict(C.HrBnEnt._fields_)['num_batches_tracked'] is VP        # a device int64_t*: an address, like the rest


def test_a_function_returns_a_status_iff_it_is_declared_plain_int():
    launchers = [p for p in H.protos.values() if p.text.endswith('hr_stream_t stream)')]
    assert len(launchers) >= 85 and all(p.status and p.text.startswith('int ') for p in launchers)
    values = [p for p in H.protos.values() if p.text.startswith('hr_value_t ')]
    assert len(values) >= 34 and not any(p.status for p in values)
    for p in values:        # a value function launches nothing: scalars, host memory and char* only
        assert all(t in (I, F, D, I64, CP) or (t is not VP and hasattr(t, 'contents')) for _, t in p.params), p.text
    assert {p.name for p in H.protos.values() if not p.status} - {p.name for p in values} == {
        'hrnet_last_error_string', 'hrnet_event_create', 'hrnet_tf_layernorm_scratch'}
    # a new function declared `int` is checked by call() without anybody listing it (the parameter has to be named)
    new = _header.parse('typedef int hr_value_t; int hrnet_new_thing(int n); hr_value_t hrnet_new_count(int n);')
    assert new.protos['hrnet_new_thing'].status and not new.protos['hrnet_new_count'].status
    assert new.protos['hrnet_new_count'].restype is I


PRELUDE = '#define HR_HOST /* host */\ntypedef void* hr_stream_t; /* a stream */\n'


@pytest.mark.parametrize('text, quoted', [
    ('int hrnet_x(size_t n, hr_stream_t stream);', r'hrnet_x\(size_t n'),                        # unknown scalar type
    ('int hrnet_x(const float* x, int (*done)(int), hr_stream_t stream);', r'hrnet_x\(const float\* x, int \(\*done'),
    ('int hrnet_x(int, hr_stream_t stream);', r'hrnet_x\(int, hr_stream_t'),                      # unnamed parameter
    ('int hrnet_x(const float*, hr_stream_t stream);', r'hrnet_x\(const float\*,'),
    ('typedef struct HrS { int32_t a : 3; int32_t b; } HrS;', r'struct HrS \{ int32_t a : 3'),    # bit-field
    ('typedef struct HrS { size_t a; } HrS;', r'struct HrS \{ size_t a'),
    ('int hrnet_x(HR_HOST int n);', r'hrnet_x\(HR_HOST int n'),                                   # marker on a scalar
    ('int hrnet_x(HR_HOST void* p);', r'hrnet_x\(HR_HOST void\* p'),                              # host what?
    ('int hrnet_x(float*** p);', r'hrnet_x\(float\*\*\* p'),
    ('int hrnet_x(int n[4]);', r'hrnet_x\(int n\[4\]'),
    ('void hrnet_x(int n);', r'void hrnet_x'),
    ('int hrnet_x(int n); int hrnet_x(int n);', r'hrnet_x'),                                      # declared twice
    ('enum HrKind { HR_A = 0 };', r'enum HrKind'),
    ('enum { HR_A = 1 << 3 };', r'HR_A = 1 << 3'),
    ('#define HR_SIZE (4 * 8)\n', r'HR_SIZE \(4 \* 8\)'),
    ('int hrnet_x(int n); }', r'\}'),
    ('static inline int hrnet_x(int n) { return n; }', r'hrnet_x'),
])
def test_reader_refuses_what_it_does_not_understand(text, quoted):
    with pytest.raises(ValueError, match=quoted):
        _header.parse(PRELUDE + text)


def test_reader_takes_the_c_the_header_uses():
    h = _header.parse(PRELUDE + '''
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define HR_N 0x10 // sixteen
        enum { HR_A = -2, HR_B, HR_C = HR_A };
        typedef struct HrS { const float* a, *b; int64_t n[2]; double d; HR_HOST const int32_t* h; } HrS;
        const char* hrnet_name(void);
        long long hrnet_size(HR_HOST const HrS* s, HR_HOST HrS* const* many, const hr_stream_t* streams,
                             unsigned char* img, int32_t k);
        #ifdef __cplusplus
        }
        #endif''')
    assert h.values == {'HR_N': 16, 'HR_A': -2, 'HR_B': -1, 'HR_C': -2}
    s = h.structs['HrS']
    assert s._fields_ == [('a', VP), ('b', VP), ('n', I64 * 2), ('d', D), ('h', ctypes.POINTER(ctypes.c_int32))]
    assert ctypes.sizeof(s) == 48
    assert h.protos['hrnet_name'].restype is CP and h.protos['hrnet_name'].params == []
    size = h.protos['hrnet_size']
    assert size.restype is I64 and not size.status
    assert size.params == [('s', ctypes.POINTER(s)), ('many', PP), ('streams', PP), ('img', VP), ('k', ctypes.c_int32)]
    assert size.text.startswith('long long hrnet_size(HR_HOST const HrS* s, HR_HOST HrS* const* many,')


def test_call_appends_the_prototype_to_an_argument_error():
    assert os.path.exists(C.LIB_PATH)
    with pytest.raises(TypeError, match=r'hr_value_t hrnet_conv_tiles\(int N, int Ho, int Wo, int Cout, int ks, int'):
        C.call('hrnet_conv_tiles', 2, 8, 8)
    # a device address where the header asks for host memory does not reach the library
    with pytest.raises(ctypes.ArgumentError, match=r'hrnet_conv_tile_walk\(.*HR_HOST int\* out5\)'):
        C.call('hrnet_conv_tile_walk', 2, 8, 8, 256, 3, 1, 0, 0, 0x7f0000000000)
    assert C.call('hrnet_conv_tiles', 2, 8, 8, 256, 3, 1) == 2
