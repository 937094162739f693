"""ctypes binding of libhrnet_hip.so, built from the C ABI's own declaration: include/hrnet_hip.h is read at import
(hipnet._header) and every prototype, struct and constant below comes from it - nothing of it is restated here.

There is deliberately NO fallback: if the library is missing or a call fails, a
RuntimeError is raised. The product path never computes on the CPU.
"""
import ctypes
import os

from hipnet import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(os.path.dirname(_HERE))
LIB_PATH = os.environ.get('HRNET_HIP_LIB', os.path.join(_PKG, 'csrc', 'libhrnet_hip.so'))
HEADER = _header.load(os.path.join(os.path.dirname(_PKG), 'include', 'hrnet_hip.h'))

VALUES = HEADER.values                       # every enumerator and integer HR_* macro of the header
HR_F32, HR_BF16, LANE_SLOT = VALUES['HR_F32'], VALUES['HR_BF16'], VALUES['HR_LANE_SLOT']
ABI_VERSION = VALUES['HR_ABI_VERSION']       # lib() refuses a library built from a header of another version
# op kinds of a recorded program: OP_CONV .. OP_POOL_REDUCE = HR_OP_*; lib/hipnet/ops.py names the slots of each
globals().update({name[3:]: value for name, value in VALUES.items() if name.startswith('HR_OP_')})
# HrOp, HrBnBwdRef, HrPackEnt, HrWredEnt, HrBnEnt: the header's structs (pointer fields are addresses: c_void_p)
globals().update(HEADER.structs)

EXPORTED = sorted(HEADER.protos)
_SIGS = {name: [t for _, t in p.params] for name, p in HEADER.protos.items()}      # name -> argument ctypes
# entry points whose return is a value (a count, flag, mode, size or handle), not a status: call() passes it through
_PLAIN = {name for name, p in HEADER.protos.items() if not p.status}

_lib = None


def lib():
    """Load the shared library once; raise loudly if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'libhrnet_hip.so not found at {} - build it with `python __graft_entry__.py` '
                '(hipcc --offload-arch=gfx950). There is no CPU fallback.'.format(LIB_PATH))
        # PyTorch ships its own libamdhip64; the library must bind to THAT copy (same soname), or the process ends up
        # with two HIP runtimes and this one's launches fail with "no ROCm-capable device is detected" (seen when
        # `python __graft_entry__.py smoke` loaded the library before anything had imported torch)
        import torch  # noqa: F401
        l = ctypes.CDLL(LIB_PATH)
        for name, p in HEADER.protos.items():
            fn = getattr(l, name)
            fn.argtypes = [t for _, t in p.params]
            fn.restype = p.restype
        if l.hrnet_abi_version() != ABI_VERSION:
            raise RuntimeError('{} has ABI version {}, include/hrnet_hip.h has {}: the library was built from another '
                               'header, rebuild it with `python __graft_entry__.py`'.format(
                                   LIB_PATH, l.hrnet_abi_version(), ABI_VERSION))
        _lib = l
    return _lib


def call(name, *args):
    """Call an entry point; a nonzero status -> RuntimeError(hrnet_last_error_string()). Arguments that do not fit
    the prototype raise ctypes' own error with the header's declaration appended."""
    l = lib()
    try:
        rc = getattr(l, name)(*args)
    except (ctypes.ArgumentError, TypeError) as e:
        raise type(e)('{}\n  {};'.format(e, HEADER.protos[name].text)) from None
    if name not in _PLAIN and rc != 0:
        raise RuntimeError('{} failed ({}): {}'.format(name, rc, l.hrnet_last_error_string().decode()))
    return rc


def ptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else t.data_ptr()


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


def dtype_id(torch_dtype):
    import torch
    if torch_dtype == torch.float32:
        return HR_F32
    if torch_dtype == torch.bfloat16:
        return HR_BF16
    raise ValueError('unsupported compute dtype {}'.format(torch_dtype))
