"""CPU tests: the C-ABI shared library loads here (no GPU) and exports every symbol that include/cgg_hip.h
declares; the ctypes prototype table covers the header; argument validation returns the documented error
codes without touching a device; the torch wrappers refuse CPU tensors (no silent fallback)."""
import ctypes
import os
import re

import pytest
import torch

import cgg_amd
from cgg_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, 'include', 'cgg_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(cgg_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cgg_hip.h but not exported by libcgg_hip.so'
    assert sorted(_lib.PROTOTYPES) == syms, 'ctypes prototype table and header disagree'
    assert lib.cgg_version() == 100


def test_argument_validation_error_codes_without_a_device():
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.cgg_mask_logits(null, null, null, null, null, 1, 1, 256, 32, null) == -1          # CGG_EINVAL
    assert b'null' in lib.cgg_last_error_string()
    assert lib.cgg_mask_logits(p, p, null, p, null, 1, 100, 128, 32, null) == -2                 # C != 256
    assert lib.cgg_pack_mask_feature(p, p, null, 1, 250, 8, 8, 1, null) == -2                    # C % 16
    assert lib.cgg_pack_mask_feature(p, p, null, 1, 256, 9, 8, 2, null) == -2                    # H % pool
    assert lib.cgg_msda_forward(p, p, p, p, p, p, 1, 10, 8, 30, 3, 5, 4, 0, null) == -2          # D % 4
    assert lib.cgg_msda_forward(p, p, p, p, p, p, 1, 10, 8, 32, 9, 5, 4, 0, null) == -2          # L > 8
    assert lib.cgg_masked_xattn_forward(p, p, null, p, p, 1, 100, 8, 64, 128, 1.0, 0, null) == -2  # D != 32
    assert lib.cgg_masked_xattn_forward(p, p, null, p, p, 1, 200, 8, 32, 128, 1.0, 0, null) == -2  # Q > 128
    assert lib.cgg_linear_rows(p, 30, p, null, null, 0, p, 8, 4, 8, 30, 0, 1, null) == -2        # K % 16
    assert lib.cgg_group_norm(p, p, p, p, p, 1, 30, 4, 4, 32, 1e-5, 0, null) == -1               # C % groups
    assert lib.cgg_masked_xattn_workspace_bytes(2, 100, 8, 32, 16384) > 0


def test_ops_refuse_cpu_tensors():
    x = torch.randn(2, 100, 256)
    feat = torch.randn(2, 256, 8, 8)
    with pytest.raises(_lib.CggError, match='ROCm device'):
        ops.pack_mask_feature(feat)
    with pytest.raises(_lib.CggError):
        ops.linear_rows(x, torch.randn(256, 256))
    with pytest.raises(_lib.CggError):
        ops.masked_xattn(x, torch.randn(2, 64, 512), None, 8)
    with pytest.raises(_lib.CggError):
        ops.msda_forward(torch.randn(1, 80, 8, 32), torch.tensor([[8, 8], [4, 4]]), torch.tensor([0, 64]),
                         torch.rand(1, 5, 8, 2, 4, 2), torch.rand(1, 5, 8, 2, 4))


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libcgg_hip.so')
    with pytest.raises(_lib.CggError, match='no CPU / eager fallback'):
        _lib.load()


_int, _vp, _f, _i64, _dbl = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_int64, ctypes.c_double

# (restype, argtypes) as the hand-written table held them before `_lib.parse_header` replaced it: char* both ways, long long, double,
# int64_t between ints, an int64_t return, void* const*
PINNED = {
    'cgg_last_error_string': (ctypes.c_char_p, []),
    'cgg_blaslt_init': (_int, [ctypes.c_char_p]),
    'cgg_relu_bwd_absmax_f32': (_int, [_vp, _vp, _vp, ctypes.c_longlong, _vp, _vp]),
    'cgg_paint_instances_u8': (_int, [_vp, _vp, _int, _int, _vp, _int, _i64, _int] + [_vp] * 4 + [_dbl, _dbl, _int, _int, _vp]),
    'cgg_panoptic_fuse_batched': (_int, [_vp] * 9 + [_i64] + [_int] * 8 + [_i64, _int, _int, _f, _dbl] + [_int] * 3 + [_vp]),
    'cgg_lsap_device_f32': (_int, [_vp, _i64, _vp, _int, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
    'cgg_msda_backward_hostlevels_ws': (_int, [_vp, _int] + [_vp] * 8 + [_int] * 8 + [_vp, _i64, _vp, _vp]),
    'cgg_rle_encode_bitmasks': (_i64, [_vp, _int, _int, _int, _i64, _int, _int, _vp, _i64, _vp]),
    'cgg_pack_mask_feature_nhwc_f32_x3': (_int, [_vp] * 4 + [_int] * 5 + [_vp]),
}


@pytest.mark.parametrize('name', sorted(PINNED))
def test_derived_prototype_equals_the_pinned_one(name):
    assert _lib.PROTOTYPES[name] == PINNED[name]


def test_header_constants():
    want = dict(CGG_VERSION=100, CGG_OK=0, CGG_EINVAL=-1, CGG_EUNSUPPORTED=-2, CGG_EALIGN=-3, CGG_ELIBRARY=-4, CGG_F32=0, CGG_BF16=1,
                CGG_F32_BF16MFMA=2, CGG_F32_X3=3)
    assert {k: _lib.CONSTANTS[k] for k in want} == want
    assert (_lib.CGG_F32, _lib.CGG_BF16, _lib.CGG_F32_BF16MFMA, _lib.CGG_F32_X3) == (0, 1, 2, 3)
    assert (ops.CGG_F32, ops.CGG_BF16, ops.CGG_F32_BF16MFMA, ops.CGG_F32_X3) == (0, 1, 2, 3)
    assert 'CGG_HIP_H_' not in _lib.CONSTANTS          # a #define without an integer value is no constant


SYNTHETIC = '''
/* int cgg_in_a_comment(int a); */
// int cgg_in_a_line_comment(int a);
#ifndef CGG_GUARD_H_
#define CGG_GUARD_H_
#define CGG_LIMIT 40 /* a trailing comment */
#define CGG_ENEG (-3)
#define CGG_NOT_AN_INT 1.5
typedef void* cgg_stream_t;
int64_t
cgg_broken(const float* x,
           int64_t n, cgg_stream_t stream)
;
int cgg_nothing(void);
const char* cgg_text(const char* path, size_t n, uint32_t a, uint64_t b, int32_t c, double d, long long e);
int cgg_arrays(float taps[4], const int32_t table[], void* const* planes, const char* names[]);
#endif
'''


def test_parse_header_on_synthetic_text():
    protos, consts = _lib.parse_header(SYNTHETIC)
    assert sorted(protos) == ['cgg_arrays', 'cgg_broken', 'cgg_nothing', 'cgg_text']          # nothing out of a comment
    assert protos['cgg_broken'] == (ctypes.c_int64, [_vp, ctypes.c_int64, _vp])              # broken over three lines
    assert protos['cgg_nothing'] == (_int, [])                                              # (void)
    assert protos['cgg_text'] == (ctypes.c_char_p, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64,
                                                    ctypes.c_int32, _dbl, ctypes.c_longlong])
    assert protos['cgg_arrays'] == (_int, [_vp, _vp, _vp, _vp])                              # T name[4], T name[], T* const*
    assert consts == dict(CGG_LIMIT=40, CGG_ENEG=-3)


@pytest.mark.parametrize('decl', ['int cgg_f(short n);', 'int cgg_f(unsigned n);', 'bool cgg_f(int n);', 'int cgg_f(struct s v);'])
def test_parse_header_refuses_a_type_it_does_not_know(decl):
    with pytest.raises(_lib.CggError, match='cgg_f'):
        _lib.parse_header(decl)


def test_missing_header_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, 'HEADER_PATH', '/nonexistent/cgg_hip.h')
    with pytest.raises(_lib.CggError, match='/nonexistent/cgg_hip.h'):
        _lib._read_header()
