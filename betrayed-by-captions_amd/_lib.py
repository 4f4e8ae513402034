"""ctypes binding of libcgg_hip.so (the C ABI declared in include/cgg_hip.h).

The header is the only statement of that ABI: `PROTOTYPES` (restype and argtypes of every entry point) and `CONSTANTS` (its integer
#defines) are parsed from it at import (`parse_header`), and `dev_ptr` is the one place a tensor becomes a device address.

There is NO fallback: if the shared library is missing, or a wrapped op is handed tensors that do not
live on a ROCm device, the call raises. The CPU restatement under /oracle is test infrastructure and
is never imported from here.
"""
import ctypes
import os
import re

import torch  # noqa: F401  (imported first so libamdhip64.so.7 resolves to torch's HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libcgg_hip.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', 'include', 'cgg_hip.h'))


class CggError(RuntimeError):
    """A libcgg_hip.so entry point returned non-zero."""


# by-value spellings of the header (after `const` and the parameter name are dropped); every pointer is a c_void_p except a plain
# `char*`. Anything else raises: a type this table does not know must never be passed as an int by default.
_SCALARS = {
    'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong,
    'int32_t': ctypes.c_int32, 'uint32_t': ctypes.c_uint32, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64,
    'size_t': ctypes.c_size_t, 'cgg_stream_t': ctypes.c_void_p,
}


def _ctype(decl, where, named):
    """ctypes type of one parameter (`named`) or return type spelled `decl`"""
    words = decl.replace('*', ' * ').replace('[', ' [').split()
    words = [w for w in words if w != 'const']
    if '*' in words or any(w.startswith('[') for w in words):
        return ctypes.c_char_p if words[:2] == ['char', '*'] and words.count('*') == 1 and '[' not in decl else ctypes.c_void_p
    for spelled in (words, words[:-1] if named else None):
        if spelled and ' '.join(spelled) in _SCALARS:
            return _SCALARS[' '.join(spelled)]
    raise CggError(f'{where}: no ctypes type for `{decl.strip()}`')


def parse_header(text):
    """C header text -> ({cgg_* name: (restype, argtypes)}, {CGG_* name: int}): the prototypes and integer #defines of
    include/cgg_hip.h as ctypes sees them, so that no second, hand-written copy of the header exists on the Python side."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    constants = {m.group(1): int(m.group(2).strip('()'))
                 for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(CGG_\w+)[ \t]+(-?\d+|\(-?\d+\))[ \t]*$', text, flags=re.M)}
    text = re.sub(r'^[ \t]*#[^\n]*', ' ', text, flags=re.M)
    prototypes = {}
    for stmt in re.split(r'[;{}]', text):
        m = re.fullmatch(r'\s*(\S.*?)\b(cgg_\w+)\s*\((.*)\)\s*', stmt, flags=re.S)
        if m is None:
            continue
        ret, name, params = m.groups()
        params = [] if params.strip() in ('', 'void') else params.split(',')
        prototypes[name] = (_ctype(ret, name, False), [_ctype(p, name, True) for p in params])
    return prototypes, constants


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise CggError(f'{HEADER_PATH} cannot be read ({e.strerror}): the ctypes prototypes of libcgg_hip.so are '
                       'derived from it') from None


# name -> (restype, argtypes) of every entry point, and the header's integer constants
PROTOTYPES, CONSTANTS = _read_header()
CGG_F32 = CONSTANTS['CGG_F32']
CGG_BF16 = CONSTANTS['CGG_BF16']
CGG_F32_BF16MFMA = CONSTANTS['CGG_F32_BF16MFMA']
CGG_F32_X3 = CONSTANTS['CGG_F32_X3']

_lib = None


def load():
    """Load (once) and return the ctypes handle; raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CggError(
            f'{LIB_PATH} is missing: build it with `python __graft_entry__.py` '
            '(hipcc --offload-arch=gfx950). There is no CPU / eager fallback for the CGG hot path.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().cgg_last_error_string()
        raise CggError(f'{what} failed (rc={rc}): {msg.decode() if msg else "?"}')


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream_ptr(device=None):
    """hipStream_t of torch's current stream on `device` (the raw-handle getter is ~10x cheaper than building a
    torch.cuda.Stream object per launch, which showed up as ~1 ms of host time per forward)."""
    if _raw_stream is not None:
        idx = device.index if isinstance(device, torch.device) else device
        if idx is None:
            idx = torch.cuda.current_device()
        return ctypes.c_void_p(_raw_stream(idx))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def dev_ptr(t, name='tensor', dtype=None, dense=True):
    """data_ptr of a contiguous ROCm tensor (None passes through as NULL). `dtype` is one torch dtype or a tuple of them; it is
    tested BEFORE the device, so a tensor of a type the callee cannot read is refused by that name wherever it lives.
    dense=False skips only the contiguity test: for a view whose strides the caller itself hands to the kernel."""
    if t is None:
        return None
    if dtype is not None and t.dtype is not dtype and not (isinstance(dtype, tuple) and t.dtype in dtype):
        want = ' | '.join(str(d) for d in dtype) if isinstance(dtype, tuple) else str(dtype)
        raise CggError(f'{name} must be {want} (got {t.dtype})')
    if not t.is_cuda:
        raise CggError(f'{name} must live on a ROCm device (got {t.device}); the CGG hot path has '
                       'no CPU implementation outside /oracle')
    if dense and not t.is_contiguous():
        raise CggError(f'{name} must be contiguous')
    return ctypes.c_void_p(t.data_ptr())


def host_ptr(t, name='tensor', dtype=None):
    """data_ptr of a contiguous HOST tensor (None passes through as NULL): the tables the library reads on the CPU during a call and
    the operands of its host functions. Same order of tests as `dev_ptr`, the device test inverted."""
    if t is None:
        return None
    if dtype is not None and t.dtype is not dtype:
        raise CggError(f'{name} must be {dtype} (got {t.dtype})')
    if t.is_cuda:
        raise CggError(f'{name} must live in host memory (got {t.device}): the library reads it on the CPU')
    if not t.is_contiguous():
        raise CggError(f'{name} must be contiguous')
    return ctypes.c_void_p(t.data_ptr())
