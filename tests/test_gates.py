"""The decisions taken before a kernel runs, checked without a device: the dtype tags handed across the C ABI.

An `ops.py` wrapper that tells the library "this buffer is f32" or "bf16" by a tag derives the tag from the tensor; a tensor of any
other type must be refused in Python, by argument name and dtype, before a pointer is taken -- the callee would read the buffer as
one of the two. The tensors here live on the CPU, so a wrapper that let the dtype through would report the DEVICE instead (or, with
a device, launch): the message tells the two apart, and a spy on `ops._lib_` shows that the library was never reached."""
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


class _NoLibrary:
    """Stands in for the loaded library: any entry point looked up on it is recorded (and fails the call)."""

    def __init__(self):
        self.reached = []

    def __getattr__(self, name):
        self.reached.append(name)
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
