"""The gate and the argument checks of `ops.mask_feature_head_x3` (no GPU): whatever the fused kernel is not built for routes to
the three-call path without raising, and the wrapper refuses bad operands before any native call."""
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import ops
from cgg_amd._lib import CggError


class _Dev(torch.Tensor):
    """a CPU tensor that claims to live on a ROCm device at a 16-byte aligned address: the gate's device / alignment tests pass,
    so that what is under test -- its shape, dtype, pool and contiguity edges -- decides"""

    @property
    def is_cuda(self):
        return True

    def data_ptr(self):
        return 4096


class _DevX3(ops.X3Image):
    @property
    def is_cuda(self):
        return True

    def data_ptr(self):
        return 4096


def _operands(H=16, W=16, C=256, N=256, groups=32, B=1):
    t = lambda *s: torch.zeros(*s).as_subclass(_Dev)
    nbytes = 2 * (N // 32) * (C // 16) * 64 * 16 + (N // 32) * 32 * 4
    wk = torch.zeros(nbytes, dtype=torch.uint8).as_subclass(_DevX3)
    return [t(B, H, W, C), t(B * groups * 2 + 64), (t(C), t(C), 1e-5, groups), wk, t(N), [1, 2, 4, 8]]


def test_gate_passes_on_the_built_shape():
    assert ops.mask_feature_head_x3_ok(*_operands())
    assert ops.mask_feature_head_x3_ok(*_operands(H=200, W=336, B=2))
    a = _operands()
    a[4] = None                                        # no bias
    assert ops.mask_feature_head_x3_ok(*a)


@pytest.mark.parametrize('kw', [dict(H=12), dict(W=20), dict(H=4), dict(C=128, N=128, groups=16), dict(C=512, groups=64), dict(N=128),
                                dict(groups=16)])
def test_gate_shape_edges_route_to_the_old_path(kw):
    assert ops.mask_feature_head_x3_ok(*_operands(**kw)) is False


@pytest.mark.parametrize('pools', [[1, 3], [3], [], [1, 2, 4, 8, 8], [1, 1], [16], None])
def test_gate_pool_edges(pools):
    a = _operands()
    a[5] = pools
    assert ops.mask_feature_head_x3_ok(*a) is False


def test_gate_operand_edges():
    a = _operands()
    a[0] = torch.zeros(1, 16, 256, 16).as_subclass(_Dev).permute(0, 1, 3, 2)       # non-contiguous (1, 16, 16, 256)
    assert tuple(a[0].shape) == (1, 16, 16, 256) and ops.mask_feature_head_x3_ok(*a) is False
    a = _operands()
    a[0] = a[0].double()
    assert ops.mask_feature_head_x3_ok(*a) is False
    a = _operands()
    a[0] = torch.zeros(1, 16, 16, 256)                                              # a CPU tensor
    assert ops.mask_feature_head_x3_ok(*a) is False
    a = _operands()
    a[0] = a[0].view(1, 256, 256)                                                   # rows, not a map
    assert ops.mask_feature_head_x3_ok(*a) is False
    a = _operands()
    a[3] = torch.zeros(a[3].numel(), dtype=torch.uint8).as_subclass(_Dev)           # not an x3 image
    assert ops.mask_feature_head_x3_ok(*a) is False
    a = _operands()
    a[2] = (a[2][0], a[2][1], 1e-5)                                                 # malformed GroupNorm tuple
    assert ops.mask_feature_head_x3_ok(*a) is False
    a = _operands()
    a[1] = torch.zeros(8).as_subclass(_Dev)                                         # workspace too small for the statistics
    assert ops.mask_feature_head_x3_ok(*a) is False
    assert ops.mask_feature_head_x3_ok(None, None, None, None, None, None) is False


@pytest.mark.parametrize('mutate', ['dtype', 'shape', 'cpu', 'pool'])
def test_wrapper_raises_before_any_native_call(monkeypatch, mutate):
    def no_native():
        raise AssertionError('the native library was reached')
    monkeypatch.setattr(ops, '_lib_', no_native)
    a = _operands()
    if mutate == 'dtype':
        a[0] = a[0].to(torch.bfloat16)
    elif mutate == 'shape':
        a = _operands(H=12)
    elif mutate == 'cpu':
        a[0] = torch.zeros(1, 16, 16, 256)
    else:
        a[5] = [1, 3]
    with pytest.raises(CggError):
        ops.mask_feature_head_x3(*a)
