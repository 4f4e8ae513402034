"""GPU tests of cgg_raise_dynamic_lds (csrc/cgg_api.hip): the one place that raises a kernel's dynamic-LDS limit above 64 KiB.
The limit belongs to the function on one device and the helper remembers, per device and kernel, the largest size it has set --
so a limit has to grow with the shape, must never shrink, and has to be raised again on a second device of the same process.
Every check is the existing single-device test of that kernel (same inputs, same float64 reference, same bound), run in the order
or on the device that the bookkeeping has to get right."""
import pytest
import torch

import cgg_amd  # noqa: F401
from test_kernels_gpu import (check_encoder_ffn_ln, check_mask_logits_backward, check_mask_logits_split,
                              check_masked_xattn_backward)
from test_window_attn_gpu import check_window_attention
from test_x3_gpu import check_encoder_layer_tail_x3

pytestmark = pytest.mark.gpu


def test_limit_grows_with_the_shape_and_does_not_shrink(dev):
    """One process, one device. Split-mode cgg_mask_logits keeps ceil(Q / 32) x 32 KiB of query tiles in LDS: Q = 32 needs no
    raise, 72 needs 96 KiB, 128 needs 128 KiB (a remembered yes/no would refuse this launch), then 72 and 32 again (a helper that
    lowered the limit would refuse the way back). Split-mode cgg_mask_logits_backward keeps 16 KiB per 16 queries: 32 KiB, then
    112 KiB."""
    for Q in (32, 72, 128, 72, 32):
        check_mask_logits_split(dev, 1, Q, 16, 24)
    for Q in (32, 100):
        check_mask_logits_backward(dev, 1, Q, 16, 24, True)


def test_second_device_in_the_same_process(dev):
    """Each kernel first on cuda:0, then the same inputs on cuda:1: the limit raised on the first device says nothing about the
    second. encoder_ffn_ln (65 KiB), masked_xattn_backward and the 144-token window_attention_backward used to remember one
    process-wide flag; encoder_layer_tail_x3 kept a per-device array."""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two ROCm devices in one process')
    for d in (0, 1):
        with torch.cuda.device(d):
            dv = torch.device('cuda', d)
            check_encoder_ffn_ln(dv, 64, 64, 256)
            check_masked_xattn_backward(dv, 1, 20, 77, 4, True)
            check_window_attention(dv, 12, (24, 36), 0, 2)
            check_encoder_layer_tail_x3(dv, 64, 64, 256)
