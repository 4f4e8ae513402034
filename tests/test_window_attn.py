"""CPU tests of the fused window attention's plumbing (csrc/window_attn.hip): the library exports the three entry points and
refuses unsupported shapes / null pointers without a device, the torch wrappers refuse CPU tensors, and `ShiftWindowMSA` on the
CPU still runs the PyTorch path (equal to the dense oracle) with unchanged state_dict keys."""
import ctypes

import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import _lib, ops, swin
from oracle.swin import _WMSA


def test_library_exports_window_attention_and_validates_without_a_device():
    lib = _lib.load()
    for name in ('cgg_window_attn_forward', 'cgg_window_attn_backward', 'cgg_window_attn_backward_workspace_bytes'):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    null = ctypes.c_void_p(None)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(B=1, Hp=24, Wp=36, C=64, heads=2, ws=12, shift=6, qkv=p):
        return lib.cgg_window_attn_forward(qkv, p, p, p, B, Hp, Wp, C, heads, ws, shift, 0.5, null)

    def bwd(B=1, Hp=24, Wp=36, C=64, heads=2, ws=12, shift=6, gtab=p):
        return lib.cgg_window_attn_backward(p, p, p, p, p, gtab, p, B, Hp, Wp, C, heads, ws, shift, 0.5, null)

    for f in (fwd, bwd):
        assert f(C=128, heads=2) == -2              # head dim 64
        assert f(C=32, heads=2) == -2               # head dim 16
        assert f(Hp=26, Wp=39, ws=13, shift=0) == -2   # 169 tokens per window
        assert f(Hp=25) == -2                       # Hp % ws
        assert f(Wp=35) == -2                       # Wp % ws
        assert f(shift=12) == -2                    # shift >= ws
        assert f(shift=-1) == -2
        assert f(B=0) == -1
    assert fwd(qkv=null) == -1                      # CGG_EINVAL
    assert b'null' in lib.cgg_last_error_string()
    assert bwd(gtab=null) == -1
    assert lib.cgg_window_attn_forward(null, p, p, p, 1, 25, 36, 64, 2, 12, 6, 0.5, null) == -1    # null before the shape limits
    # one N x N plane per (window chunk, head), at most one chunk per window
    n = lib.cgg_window_attn_backward_workspace_bytes(2, 24, 36, 2, 12)
    assert n > 0 and n % (144 * 144 * 4 * 2) == 0 and n <= 12 * 2 * 144 * 144 * 4
    assert lib.cgg_window_attn_backward_workspace_bytes(2, 25, 36, 2, 12) == 0


def test_window_attention_ops_refuse_cpu_tensors():
    qkv = torch.randn(1, 24 * 24, 3 * 64)
    table = torch.randn(23 * 23, 2)
    with pytest.raises(_lib.CggError, match='ROCm device'):
        ops.window_attention(qkv, table, (24, 24), 12, 0, 2)
    with pytest.raises(_lib.CggError, match='ROCm device'):
        ops.window_attention_backward(qkv, table, torch.randn(1, 2, 576), torch.randn(1, 576, 64), (24, 24), 12, 0, 2)
    with pytest.raises(_lib.CggError):
        ops.WindowAttentionFn.apply(qkv, table, (24, 24), 12, 0, 2, None)
    assert not ops.window_attention_ok(qkv, 12, 2, (24, 24), 0)            # a CPU tensor is outside the supported set
    assert ops.window_attention_shape_ok(64, 12, 2, (24, 36), 6) and ops.window_attention_shape_ok(128, 7, 4)
    assert not ops.window_attention_shape_ok(64, 12, 4)                    # head dim 16
    assert not ops.window_attention_shape_ok(64, 13, 2)                    # 169 tokens
    assert not ops.window_attention_shape_ok(64, 12, 2, (25, 36))
    assert not ops.window_attention_shape_ok(64, 12, 2, (24, 36), 12)


@pytest.mark.parametrize('ws,shift,hw', [(12, 6, (30, 41)), (7, 3, (14, 21)), (12, 0, (24, 36))])
def test_shift_window_msa_cpu_fallback_equals_dense_oracle(ws, shift, hw):
    """On the CPU `ShiftWindowMSA` never reaches the fused kernels: it still equals the dense float64 oracle, parameters and buffers
    keep their names (an mmdet checkpoint loads unchanged)."""
    g = torch.Generator().manual_seed(ws * 100 + shift)
    m = swin.ShiftWindowMSA(64, 2, ws, shift)
    assert sorted(m.state_dict()) == ['w_msa.proj.bias', 'w_msa.proj.weight', 'w_msa.qkv.bias', 'w_msa.qkv.weight',
                                      'w_msa.relative_position_bias_table', 'w_msa.relative_position_index']
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.125 if p.dim() > 1 and p.shape[-1] == 64 else 1.0))
    x = torch.randn(2, hw[0] * hw[1], 64, generator=g)
    assert not m._native_ok(x)
    orc = _WMSA(64, 2, ws, shift).double()
    missing, unexpected = orc.load_state_dict(m.state_dict(), strict=False)
    assert not missing and unexpected == ['w_msa.relative_position_index']
    with torch.no_grad():
        got, want = m(x, hw), orc(x.double(), hw)
    assert (got.double() - want).abs().max().item() <= 2e-4 * max(1.0, want.abs().max().item())
