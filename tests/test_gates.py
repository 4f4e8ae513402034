"""The decisions taken before a kernel runs, checked without a device: the dtype tags handed across the C ABI.

An `ops.py` wrapper that tells the library "this buffer is f32" or "bf16" by a tag derives the tag from the tensor; a tensor of any
other type must be refused in Python, by argument name and dtype, before a pointer is taken -- the callee would read the buffer as
one of the two. The tensors here live on the CPU, so a wrapper that let the dtype through would report the DEVICE instead (or, with
a device, launch): the message tells the two apart, and a spy on `ops._lib_` shows that the library was never reached."""
import ast
import ctypes
from types import SimpleNamespace

import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import _lib, ops

SHAPES = [(4, 4), (8, 8)]
STARTS = [0, 16]
B, NV, H, D, L, P, NQ = 2, 80, 8, 32, 2, 4, 80


def _msda_args(dt):
    g = torch.Generator().manual_seed(1)
    value = torch.randn(B, NV, H, D, generator=g).to(dt)
    loc = torch.rand(B, NQ, H, L, P, 2, generator=g)
    aw = torch.softmax(torch.randn(B, NQ, H, L * P, generator=g), -1).view(B, NQ, H, L, P)
    return value, loc, aw


def _ln_args(dt_a, dt_b):
    g = torch.Generator().manual_seed(2)
    a = torch.randn(3, 5, 256, generator=g).to(dt_a)
    b = torch.randn(3, 5, 256, generator=g).to(dt_b)
    return a, b, torch.ones(256), torch.zeros(256)


def _call_msda_forward(dt):
    v, loc, aw = _msda_args(dt)
    return ops.msda_forward(v, torch.tensor(SHAPES), torch.tensor(STARTS), loc, aw)


def _call_msda_forward_hostlevels(dt):
    v, loc, aw = _msda_args(dt)
    return ops.msda_forward_hostlevels(v, SHAPES, STARTS, loc, aw)


def _call_msda_forward_fused(dt):
    v, _, _ = _msda_args(dt)
    return ops.msda_forward_fused(v, SHAPES, STARTS, torch.zeros(B, NQ, 3 * H * L * P), torch.zeros(NQ, 2), P)


def _call_add_layernorm_stream_a(dt):
    a, b, g, be = _ln_args(dt, torch.float32)
    return ops.add_layernorm_stream(a, b, g, be)


def _call_add_layernorm_stream_b(dt):
    a, b, g, be = _ln_args(torch.float32, dt)
    return ops.add_layernorm_stream(a, b, g, be)


def _call_add_layernorm_backward_b(dt):
    a, b, g, _ = _ln_args(torch.float32, dt)
    return ops.add_layernorm_backward(torch.ones_like(a), a, b, g, 1e-5)


def _call_add_layernorm_backward_amax_b(dt):
    a, b, g, _ = _ln_args(torch.float32, dt)
    return ops.add_layernorm_backward(torch.ones_like(a), a, b, g, 1e-5, want_amax=True)


def _call_add_layernorm_kv_a(dt):
    a, b, g, be = _ln_args(dt, torch.float32)
    return ops.add_layernorm_kv(a, b, g, be, 1e-5, torch.zeros(5, 256), torch.zeros(5, 256), [0, 2])


def _call_add_layernorm_kv_b(dt):
    a, b, g, be = _ln_args(torch.float32, dt)
    return ops.add_layernorm_kv(a, b, g, be, 1e-5, torch.zeros(5, 256), torch.zeros(5, 256), [0, 2])


# every `CGG_BF16 if ... else CGG_F32` site of ops.py (grep), by the argument whose tag it derives
TAGGED = [
    (_call_msda_forward, 'value'),
    (_call_msda_forward_hostlevels, 'value'),
    (_call_msda_forward_fused, 'value'),
    (_call_add_layernorm_stream_a, 'a'),
    (_call_add_layernorm_stream_b, 'b'),
    (_call_add_layernorm_backward_b, 'b'),
    (_call_add_layernorm_backward_amax_b, 'b'),
    (_call_add_layernorm_kv_a, 'a'),
    (_call_add_layernorm_kv_b, 'b'),
]


def _is_size_query(name):
    """the entry points that answer a size or a yes / no about a geometry and touch no operand"""
    return name.endswith(('_bytes', '_partials')) or name in ('cgg_dynamic_lds_limit', 'cgg_msda_backward_overwrites')


class _NoLibrary:
    """Stands in for the loaded library: any entry point looked up on it is recorded (and fails the call). sizes=True: a size query
    is recorded and answers 1, for the wrappers that size a workspace or check an x3 image before their first pointer."""

    def __init__(self, sizes=False):
        self.reached = []
        self.sizes = sizes

    def __getattr__(self, name):
        self.reached.append(name)
        if self.sizes and _is_size_query(name):
            return lambda *a: 1
        raise AssertionError(f'the library entry {name} was reached')


@pytest.mark.parametrize('dt', [torch.float16, torch.float64], ids=['float16', 'float64'])
@pytest.mark.parametrize('call,arg', TAGGED, ids=[c.__name__[len('_call_'):] for c, _ in TAGGED])
def test_tagged_wrapper_refuses_an_untaggable_dtype_before_any_pointer(monkeypatch, call, arg, dt):
    spy = _NoLibrary()
    monkeypatch.setattr(ops, '_lib_', lambda: spy)
    with pytest.raises(_lib.CggError) as e:
        call(dt)
    msg = str(e.value)
    assert str(dt) in msg, msg                       # the dtype by name ('torch.float16'), not the device
    assert arg in msg.split(' must be ')[0].replace(':', ' ').split(), msg
    assert 'ROCm device' not in msg
    assert spy.reached == []


class _SizesOnly:
    """A library whose every entry answers 1: enough for the workspace / partial-count queries some wrappers make before they take
    their first pointer."""

    def __getattr__(self, name):
        return lambda *a: 1


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
@pytest.mark.parametrize('call,arg', TAGGED, ids=[c.__name__[len('_call_'):] for c, _ in TAGGED])
def test_tagged_wrapper_still_reports_the_device_for_a_taggable_dtype(monkeypatch, call, arg, dt):
    """The other side of the gate: a dtype the tag can name passes it, and the CPU tensor is refused for its device as before."""
    monkeypatch.setattr(ops, '_lib_', lambda: _SizesOnly())
    with pytest.raises(_lib.CggError, match='ROCm device'):
        call(dt)


def test_dev_ptr_tests_dtype_before_device_and_takes_a_tuple():
    t16, t32 = torch.zeros(4, dtype=torch.float16), torch.zeros(4)
    assert _lib.dev_ptr(None, 'x', torch.float32) is None
    with pytest.raises(_lib.CggError, match=r'x must be torch\.float32 \(got torch\.float16\)'):
        _lib.dev_ptr(t16, 'x', torch.float32)
    with pytest.raises(_lib.CggError, match=r'x must be torch\.float32 \| torch\.bfloat16 \(got torch\.float16\)'):
        _lib.dev_ptr(t16, 'x', (torch.float32, torch.bfloat16))
    for ok in (torch.float32, (torch.float32, torch.bfloat16), None):
        with pytest.raises(_lib.CggError, match='ROCm device'):
            _lib.dev_ptr(t32, 'x', ok)
    with pytest.raises(_lib.CggError, match='ROCm device'):
        _lib.dev_ptr(t32.bfloat16(), 'x', (torch.float32, torch.bfloat16))
    # past both tests, a tensor of either dtype of the tuple yields its pointer (a stand-in: no device here)
    from types import SimpleNamespace
    for dt in (torch.float32, torch.bfloat16):
        fake = SimpleNamespace(dtype=dt, is_cuda=True, device='cuda:0', is_contiguous=lambda: True, data_ptr=lambda: 4096)
        assert _lib.dev_ptr(fake, 'x', (torch.float32, torch.bfloat16)).value == 4096
        assert _lib.dev_ptr(fake, 'x', dt).value == 4096


def test_dev_ptr_dense_false_skips_only_the_contiguity_test():
    view = torch.zeros(4, 8)[:, :4]
    assert not view.is_contiguous()
    with pytest.raises(_lib.CggError, match=r'x must live on a ROCm device'):
        _lib.dev_ptr(view, 'x', torch.float32, dense=False)
    with pytest.raises(_lib.CggError, match=r'x must be torch\.float32 \(got torch\.float16\)'):
        _lib.dev_ptr(view.half(), 'x', torch.float32, dense=False)
    fake = SimpleNamespace(dtype=torch.float32, is_cuda=True, device='cuda:0', is_contiguous=lambda: False, data_ptr=lambda: 4096)
    assert _lib.dev_ptr(fake, 'x', torch.float32, dense=False).value == 4096
    with pytest.raises(_lib.CggError, match='x must be contiguous'):
        _lib.dev_ptr(fake, 'x', torch.float32)
    assert _lib.dev_ptr(None, 'x', torch.float32, dense=False) is None


def test_ptr_at_checks_the_tensor_and_adds_elements():
    fake = SimpleNamespace(dtype=torch.float32, is_cuda=True, device='cuda:0', is_contiguous=lambda: False, data_ptr=lambda: 4096,
                           element_size=lambda: 4)
    assert ops._ptr_at(fake, 256, 'rows', torch.float32).value == 4096 + 1024
    assert ops._ptr_at(None, 256, 'rows', torch.float32) is None
    with pytest.raises(_lib.CggError, match='rows must live on a ROCm device'):
        ops._ptr_at(torch.zeros(8), 4, 'rows', torch.float32)
    with pytest.raises(_lib.CggError, match=r'rows must be torch\.bfloat16'):
        ops._ptr_at(torch.zeros(8), 4, 'rows', torch.bfloat16)


def test_host_ptr_is_dev_ptr_with_the_device_test_inverted():
    t = torch.zeros(4, dtype=torch.int32)
    assert _lib.host_ptr(t, 'table', torch.int32).value == t.data_ptr()
    assert _lib.host_ptr(None, 'table') is None
    with pytest.raises(_lib.CggError, match=r'table must be torch\.int32 \(got torch\.int64\)'):
        _lib.host_ptr(t.long(), 'table', torch.int32)
    with pytest.raises(_lib.CggError, match='table must be contiguous'):
        _lib.host_ptr(torch.zeros(4, 2, dtype=torch.int32)[:, 0], 'table', torch.int32)
    fake = SimpleNamespace(dtype=torch.int32, is_cuda=True, device='cuda:0', is_contiguous=lambda: True, data_ptr=lambda: 4096)
    with pytest.raises(_lib.CggError, match='table must live in host memory'):
        _lib.host_ptr(fake, 'table', torch.int32)


def _enclosing_functions(tree):
    """(node, name of the top-level function or class it lies in | None) for every node of the module"""
    for top in tree.body:
        name = top.name if isinstance(top, (ast.FunctionDef, ast.ClassDef)) else None
        for node in ast.walk(top):
            yield node, name


def test_ops_has_one_pointer_path_and_one_call_path():
    """Structure of ops.py: a tensor's address is taken by `dev_ptr` / `host_ptr` (offsets by `_ptr_at`), never by a cast of
    `data_ptr()`; a status is checked in `_call` alone."""
    tree = ast.parse(open(ops.__file__).read())
    raw, checks = [], []
    for node, where in _enclosing_functions(tree):
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        if isinstance(f, ast.Attribute) and f.attr == 'c_void_p' and where != '_ptr_at':
            inner = [n for a in node.args for n in ast.walk(a)]
            if any(isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == 'data_ptr' for n in inner):
                raw.append((where, node.lineno))
        if (isinstance(f, ast.Name) and f.id == 'check' or isinstance(f, ast.Attribute) and f.attr == 'check') and where != '_call':
            checks.append((where, node.lineno))
    assert raw == [], f'raw tensor addresses: {raw}'
    assert checks == [], f'status checks outside _call: {checks}'


M, E = 8, 256


def _rows(*shape, dt=torch.float32):
    return torch.zeros(*shape, dtype=dt)


def _packed():
    return torch.zeros(64, dtype=torch.uint8)


def _x3_image():
    return torch.zeros(1, dtype=torch.uint8).as_subclass(ops.X3Image)       # 1 byte: what the spy's cgg_x3_packed_bytes answers


def _norm():
    return torch.ones(E), torch.zeros(E), 1e-5


# wrappers whose tensor operands all went past `dev_ptr` as raw casts, with legal CPU operands, by their first operand
RAW_CAST_WRAPPERS = {
    'decoder_ffn': ('x', lambda: ops.decoder_ffn(_rows(M, E), _packed(), _rows(E), _packed(), _rows(E), 256)),
    'decoder_mid': ('core', lambda: ops.decoder_mid(_rows(M, E), _packed(), _rows(E), _rows(M, E), _norm())),
    'self_attn_rows_bf16': ('q', lambda: ops.self_attn_rows_bf16(_rows(M, E), _rows(M, 2 * E), 1, 8)),
    'layernorm_chain': ('a', lambda: ops.layernorm_chain(_rows(M, E), _norm())),
    'linear_rows_bf16': ('x', lambda: ops.linear_rows_bf16(_rows(M, E), _packed(), E)),
    'linear_rows_bf16_qkv': ('xqk', lambda: ops.linear_rows_bf16_qkv(_rows(M, E), _rows(M, E), _packed(), _rows(3 * E), E)),
    'gemm_x3': ('a', lambda: ops.gemm_x3(_rows(M, E), _x3_image(), E)),
    'gemm_x3s': ('a', lambda: ops.gemm_x3s(_rows(M, E), _x3_image(), E)),
    'gemm_x3s_batched': ('a', lambda: ops.gemm_x3s(_rows(2, M, E), _x3_image(), E)),
    'gemm_x3_bwd': ('g', lambda: ops.gemm_x3_bwd(_rows(M, E), _x3_image(), E, amax=_rows(1))),
    'wgrad_x3': ('dy', lambda: ops.wgrad_x3(_rows(M, E), _rows(M, E))),
    'topk_select': ('x', lambda: ops.topk_select(_rows(4, 16), 3)),
    'absmax': ('x', lambda: ops.absmax(_rows(M, E))),
    'masked_xattn_bf16': ('q', lambda: ops.masked_xattn_bf16(_rows(1, M, E), _rows(1, 16, E, dt=torch.bfloat16),
                                                             _rows(1, E, 16, dt=torch.bfloat16), None, 8)),
}


@pytest.mark.parametrize('wrapper', sorted(RAW_CAST_WRAPPERS))
def test_raw_cast_wrapper_refuses_cpu_operands_before_the_library(monkeypatch, wrapper):
    """Legal shapes and dtypes on the CPU: the first operand is refused for its device, by name, and no entry point other than a size
    query was looked up -- for the _bf16 / _x3 twins: the symbol is no longer fetched before the pointers are checked."""
    arg, call = RAW_CAST_WRAPPERS[wrapper]
    spy = _NoLibrary(sizes=True)
    monkeypatch.setattr(ops, '_lib_', lambda: spy)
    with pytest.raises(_lib.CggError, match='ROCm device') as e:
        call()
    assert str(e.value).startswith(f'{arg} must live on a ROCm device'), str(e.value)
    assert [n for n in spy.reached if not _is_size_query(n)] == []


def test_a_failed_call_is_reported_under_the_symbol_that_ran(monkeypatch):
    """`gemm_x3s` on a (B, R, K) stack runs cgg_gemm_x3s_batched: its status is reported under that name."""
    ran = []

    class _Fails:
        def cgg_x3_packed_bytes(self, N, K):
            return 1

        def cgg_gemm_x3s_batched(self, *args):
            ran.append(len(args))
            return -2

    monkeypatch.setattr(ops, '_lib_', lambda: _Fails())
    monkeypatch.setattr(ops, 'dev_ptr', lambda t, *a, **k: None if t is None else ctypes.c_void_p(4096))
    monkeypatch.setattr(ops, 'stream_ptr', lambda device=None: None)
    with pytest.raises(_lib.CggError, match=r'cgg_gemm_x3s_batched failed \(rc=-2\)'):
        ops.gemm_x3s(_rows(2, M, E), _x3_image(), E)
    assert ran == [len(_lib.PROTOTYPES['cgg_gemm_x3s_batched'][1])]


# ---- the decoder tail's plane cap: refused by name, never summed short ---------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.is_available(), reason='hands host pointers to the entry: only where no launch can follow a missed check')
def test_cgg_decoder_tail_refuses_more_planes_than_it_sums_without_a_launch():
    """`cgg_decoder_tail_{bf16,x3}` hold DT_MAX_PLANES = 8 planes per row; nsum = 9 is CGG_EUNSUPPORTED with `nsum` in the message
    (it was summed as 8), before any launch: there is no device here, and the pointers are host memory."""
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (lib.cgg_decoder_tail_bf16, lib.cgg_decoder_tail_x3):
        def call(nsum, C=256):
            return fn(p, nsum, 4 * 256, 256, p, p, 1e-5, p, 1, p, p, 1e-5, p, p, p, p, p, p, None, None, p, None, p, None, 4, C, None)
        assert call(ops.DECODER_TAIL_MAX_PLANES + 1) == -2                     # CGG_EUNSUPPORTED
        msg = lib.cgg_last_error_string()
        assert b'nsum=%d' % (ops.DECODER_TAIL_MAX_PLANES + 1) in msg and b'decoder_tail' in msg, msg
        assert b'at most %d are summed' % ops.DECODER_TAIL_MAX_PLANES in msg, msg        # DT_MAX_PLANES itself, by the C side's own word
        assert call(16) == -2
        assert call(0) == -1 and b'bad sizes' in lib.cgg_last_error_string()  # CGG_EINVAL, as before
        assert call(8, C=128) == -2 and b'C=128' in lib.cgg_last_error_string()


@pytest.mark.parametrize('width,planes,inside', [(2048, 8, True), (2304, 9, False), (1000, 1, True), (1100, 8, True)])
def test_lean_decode_gate_looks_at_the_ffn_width(width, planes, inside):
    """`Mask2FormerHeadOpen._lean_decode_ok`: the lean inference decode hands the FFN's planes to `ops.decoder_tail`, so it is taken
    only while every layer produces at most DECODER_TAIL_MAX_PLANES of them: 2048 / 256 = 8 inside, 2304 / 256 = 9 outside; a width
    that is no multiple of 256 goes through the split-K linear (1 or 8 planes)."""
    import util
    cfg = util.small_cfg()
    tl = cfg['panoptic_head']['transformer_decoder']['transformerlayers']
    tl['feedforward_channels'] = width
    tl['ffn_cfgs']['feedforward_channels'] = width
    prod, _ = util.build_heads(cfg)
    layers = prod.transformer_decoder.layers
    assert all(l.ffns[0].layers[0][0].weight.shape[0] == width and l.ffn_planes() == planes for l in layers)
    assert prod._lean_decode_ok(256) == inside
    prod.attn_mask_hook = lambda i, bits: bits
    assert not prod._lean_decode_ok(256)
