"""ctypes binding of libdvgo_hip.so (include/dvgo_hip.h).

This is the only place the shared library is loaded.  There is no CPU fallback: if the
library is missing the import of any op module raises, and every op rejects non-CUDA tensors
with the reference's own error text (lib/cuda/render_utils.cpp:40-42).
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DVGO_HIP_SO: another build of the same library (kernel A/B runs, tools/)
SO_PATH = os.environ.get('DVGO_HIP_SO') or os.path.join(_HERE, 'csrc', 'libdvgo_hip.so')
ABI_VERSION = 11
# the declarations the boundary is typed from (checkout layout: include/ beside the package)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'dvgo_hip.h')

_lib = None
_nargs = {}          # entry point -> declared parameter count (`call` compares before anything reaches the device)


class _Rec2(ctypes.Structure):
    _fields_ = [('step', ctypes.c_int32), ('exp_d', ctypes.c_float), ('alpha', ctypes.c_float), ('T', ctypes.c_float)]


_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_flt = ctypes.c_float


class _Pointer(ctypes.c_void_p):
    """The parameter type of every pointer of the header.  A tensor is converted to its address inside the foreign call,
    while the argument tuple keeps it alive: call sites pass tensors, never addresses formed earlier."""

    @staticmethod
    def from_param(x):
        if x is None or type(x) is _vp:                  # NULL; a hand-made pointer or a raw stream handle
            return x
        if isinstance(x, torch.Tensor):
            return _vp(x.data_ptr())
        if isinstance(x, (ctypes.Array, _vp)):           # host arrays: `f3`, the pointer tables of dvgo_copy_multi
            return x
        raise TypeError(f'expected a tensor, a ctypes array, a c_void_p or None, got {type(x).__name__}')


_SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float,
            'double': ctypes.c_double}


def declarations(text):
    """{name: (restype, [argtypes])} of every function a header declares.  Strict: after comments, preprocessor lines,
    the record typedefs and the extern "C" braces are gone, every statement must be `int|int64_t dvgo_name(params)` and
    every parameter a pointer or one of `_SCALARS`; anything else is an error, not a guess."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'^\s*#.*$', ' ', text, flags=re.M)
    text = re.sub(r'typedef\s+struct\s*\{[^{}]*\}\s*\w+\s*;', ' ', text)
    text = re.sub(r'extern\s+"C"\s*\{|^\s*\}\s*$', ' ', text, flags=re.M)
    decls = {}
    for stmt in filter(None, (' '.join(s.split()) for s in text.split(';'))):
        m = re.fullmatch(r'(int|int64_t) (dvgo_\w+) ?\((.*)\)', stmt)
        if m is None or m.group(2) in decls:
            raise RuntimeError(f'dvgo_hip.h: cannot read the declaration `{stmt}`')
        argtypes = []
        for param in ([] if m.group(3).strip() == 'void' else m.group(3).split(',')):
            if re.fullmatch(r'\s*(const )?(unsigned )?\w+ ?\*( ?const ?\*)? ?\w+\s*', param):
                argtypes.append(_Pointer)
                continue
            words = param.split()
            if len(words) != 2 or words[0] not in _SCALARS or not words[1].isidentifier():
                raise RuntimeError(f'dvgo_hip.h: {m.group(2)}: cannot read the parameter `{param.strip()}`')
            argtypes.append(_SCALARS[words[0]])
        decls[m.group(2)] = (_SCALARS[m.group(1)], argtypes)
    return decls


def lib():
    """The loaded library, every entry point typed from its declaration in include/dvgo_hip.h; raises (loudly) when it
    has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                f'{SO_PATH} is missing: build it with `python -m directvoxgo_amd.build` '
                '(hipcc --offload-arch=gfx950).  directvoxgo_amd has no CPU fallback.')
        if not os.path.exists(HEADER_PATH):
            raise RuntimeError(f'{HEADER_PATH} is missing: the calls into libdvgo_hip.so are typed from it '
                               '(run from a checkout: include/ beside directvoxgo_amd/)')
        handle = ctypes.CDLL(SO_PATH)
        handle.dvgo_abi_version.restype = ctypes.c_int
        v = handle.dvgo_abi_version()
        if v != ABI_VERSION:
            raise RuntimeError(f'libdvgo_hip.so ABI {v} != expected {ABI_VERSION}: rebuild')
        with open(HEADER_PATH) as f:
            decls = declarations(f.read())
        for name, (restype, argtypes) in decls.items():
            fn = getattr(handle, name, None)
            if fn is None:
                raise RuntimeError(f'{SO_PATH} does not export {name}, which include/dvgo_hip.h declares: rebuild')
            fn.restype, fn.argtypes = restype, argtypes
            _nargs[name] = len(argtypes)
        if os.environ.get('DVGO_SHADE_VARIANT'):          # A/B runs (tools/): colour-head kernel variant bits
            handle.dvgo_shade_variant(int(os.environ['DVGO_SHADE_VARIANT']))
        _lib = handle
    return _lib


def check_input(x, name):
    """CHECK_INPUT of render_utils.cpp:40-42."""
    if not x.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA tensor')
    if not x.is_contiguous():
        raise RuntimeError(f'{name} must be contiguous')


def check_f32(x, name):
    if x.dtype != torch.float32:
        # the reference dispatches float/double but the path runs in fp32
        raise RuntimeError(f'{name} must be float32, got {x.dtype}')


def ptr(t):
    return _vp(t.data_ptr()) if t is not None else _vp(0)


def stream_of(t):
    """torch's current stream on t's device as a raw hipStream_t (the C-level getter: a Stream object per launch costs
    more host time than the launch itself on small batches)."""
    return _vp(torch._C._cuda_getCurrentRawStream(t.device.index))


class _NoCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NOCTX = _NoCtx()


def device_of(t):
    """`torch.cuda.device_of(t)`, free when t already lives on the current device (the usual one-process-per-GPU case)."""
    if t.device.index == torch.cuda.current_device():
        return _NOCTX
    return torch.cuda.device_of(t)


_ERR = {-1: 'invalid argument', -2: 'size exceeds 32-bit launch range'}


# Optional per-entry-point timing with HIP events on the launching (= torch's current) stream.
# bench.py uses it to measure the average launch duration of the hot kernels inside its timed
# region; it is off (None) everywhere else.
_profile = None


def profile_start(names):
    global _profile
    _profile = {n: [] for n in names}


def profile_stop():
    """-> {name: (launches, total_ms)}; synchronises."""
    global _profile
    prof, _profile = _profile, None
    torch.cuda.synchronize()
    return {n: (len(ev), sum(a.elapsed_time(b) for a, b in ev)) for n, ev in (prof or {}).items()}


def call(name, *args):
    handle = lib()
    if len(args) != _nargs.get(name):                    # (ctypes itself lets surplus arguments through)
        raise TypeError(f'{name}: {len(args)} arguments given, include/dvgo_hip.h declares {_nargs.get(name, "no such function")}')
    fn = getattr(handle, name)
    if _profile is not None and name in _profile:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn(*args)
        b.record()
        _profile[name].append((a, b))
    else:
        rc = fn(*args)
    if rc != 0:
        raise RuntimeError(f'{name} failed: {_ERR.get(rc, "hipError %d" % rc)}')


def f3(x):
    """3 floats as a host array (model constants travel as kernel arguments in the fused path)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().tolist()
    return (ctypes.c_float * 3)(*[float(v) for v in x])
