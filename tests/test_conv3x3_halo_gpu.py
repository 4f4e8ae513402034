"""-m gpu tests of the halo-patch 3 x 3 convolution (csrc/x3s_gemm.hip, cgg_conv3x3_halo_kernel; tile configuration id 18 of
`ops.conv_x3s_nhwc(..., cfg=)`): a workgroup stages the (TH + 2) x (TW + 2) input pixels of its output patch in LDS once and reads
every filter tap's A fragments from it. Checked the way tests/test_x3s_gpu.py checks the ring kernel: float64 conv2d of the decoded
x3a input is the truth, the bound is 4 x the plain f32 conv2d's own error + 2e-7 of the output scale, and a launch on 1000.0
comes first so that stale LDS cannot pass for zero padding. Shapes are the smallest at which the patch logic can go wrong: two
images (the image boundary falls inside the grid), maps of one pixel, smaller than a patch, exactly one 8 x 16 patch, one pixel
over in both directions, and several ragged patches; N = 40 leaves a ragged last 32-column tile."""
import pytest
import torch
import torch.nn.functional as F

import cgg_amd  # noqa: F401
from cgg_amd import ops
from cgg_amd._lib import CggError

pytestmark = pytest.mark.gpu

HALO = 18                        # the halo kernel's configuration id
MAPS = [(1, 1), (3, 5), (8, 16), (9, 17), (19, 23), (16, 33)]


def _err(got, want64):
    return (got.detach().cpu().double() - want64).abs().max().item()


def _case(dev, B, H, W, C, N, seed, k=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(N, C, k, k, generator=g) / (C * k * k)**0.5
    b = torch.randn(N, generator=g)
    xe = ops.x3a_encode(x.to(dev))
    xdec = ops.x3a_decode(xe).cpu()                      # what the convolution multiplies (x to 22 bits)
    packed = ops.pack_conv_weight_x3(w.to(dev))
    return x, w, b, xe, xdec, packed


@pytest.mark.parametrize('H,W', MAPS)
@pytest.mark.parametrize('N', [64, 40, 256])
@pytest.mark.parametrize('C', [64, 128, 256])
def test_halo_conv_vs_float64(dev, C, N, H, W):
    """Bias + f32 output, then no bias + ReLU + x3a output. The x3a output's bound adds the storage rounding of the format itself
    (two 11-bit pieces: |v| 2^-21 + 2^-28, the tolerance of test_x3a_roundtrip_and_flag)."""
    B = 2
    x, w, b, xe, xdec, packed = _case(dev, B, H, W, C, N, 900 + C + N + 7 * H + W)
    xn, wn = xdec.permute(0, 3, 1, 2), w
    want = F.conv2d(xn.double(), wn.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    f32_err = (F.conv2d(xn, wn, b, padding=1).permute(0, 2, 3, 1).double() - want).abs().max().item()
    scale = want.abs().max().item()
    ops.x3_overflow_check(dev)
    # poison the LDS-visible neighbourhood: a previous launch with large values must not leak into the padding
    ops.conv_x3s_nhwc(ops.x3a_encode(torch.full_like(x, 1000.0).to(dev)), packed, N, 3, 1, 1, b.to(dev), out_split=False, cfg=HALO)
    y = ops.conv_x3s_nhwc(xe, packed, N, 3, 1, 1, b.to(dev), out_split=False, cfg=HALO)
    assert y.shape == (B, H, W, N)
    assert _err(y, want) <= 4 * f32_err + 2e-7 * scale, (_err(y, want), f32_err)
    # no bias, ReLU, x3a out
    want0 = F.conv2d(xn.double(), wn.double(), None, padding=1).permute(0, 2, 3, 1)
    f32_err0 = (F.conv2d(xn, wn, None, padding=1).permute(0, 2, 3, 1).double() - want0).abs().max().item()
    scale0 = want0.abs().max().item()
    ye = ops.conv_x3s_nhwc(xe, packed, N, 3, 1, 1, None, relu=True, out_split=True, cfg=HALO)
    got = ops.x3a_decode(ye)
    assert (got >= 0).all()
    assert _err(got, want0.relu()) <= 4 * f32_err0 + 2e-7 * scale0 + scale0 * 2.0**-21 + 2.0**-28, (_err(got, want0.relu()), f32_err0)
    # ... and with bias, no ReLU, into x3a (negative values through the split)
    ye = ops.conv_x3s_nhwc(xe, packed, N, 3, 1, 1, b.to(dev), out_split=True, cfg=HALO)
    assert _err(ops.x3a_decode(ye), want) <= 4 * f32_err + 2e-7 * scale + scale * 2.0**-21 + 2.0**-28
    assert not ops.x3_overflow_check(dev)


@pytest.mark.parametrize('H,W', [(9, 17), (19, 23)])
@pytest.mark.parametrize('N', [64, 40, 256])
@pytest.mark.parametrize('C', [64, 128, 256])
def test_halo_conv_is_bit_identical_to_the_ring_kernel_with_the_same_k_groups(dev, C, N, H, W):
    """The halo kernel keeps the ring kernel's accumulation order: tap-major, 32-channel chunks inside a tap, three MFMAs per
    fragment pair into one f32 accumulator, and with two k-groups the even and odd chunks summed apart and added at the end --
    an order no tile shape changes. Its instance for C = 64 uses one k-group, as configuration 13 does, which the shape rule
    picked for the ResNet's layer1 3 x 3 (M = 131072, C = N = 64); those for C = 128 and 256 use two, as configurations 10 and 11
    do, which it picked for layer2 (M = 32768) and layer3 (M = 8192). So every ring configuration with that k-group count gives
    the same bits."""
    x, w, b, xe, xdec, packed = _case(dev, 2, H, W, C, N, 950 + C + N + H)
    rings = (13, 4) if C == 64 else (10, 11, 12)
    for split in (False, True):
        y = ops.conv_x3s_nhwc(xe, packed, N, 3, 1, 1, b.to(dev), relu=split, out_split=split, cfg=HALO)
        for ring in rings:
            assert torch.equal(y, ops.conv_x3s_nhwc(xe, packed, N, 3, 1, 1, b.to(dev), relu=split, out_split=split, cfg=ring)), (ring, split)


def test_halo_id_is_refused_where_it_does_not_apply_and_other_calls_are_untouched(dev):
    """Forcing id 18 for a call the halo kernel does not serve raises (no silent fall-back); unforced, those calls still give one
    of the ring kernel's two possible results (one k-group = id 13, two = id 12: tile shapes do not change the bits)."""
    for B, H, W, C, N, k, s, p in [(2, 18, 20, 64, 64, 3, 2, 1), (2, 9, 17, 64, 64, 1, 1, 0), (2, 9, 17, 96, 64, 3, 1, 1),
                                   (2, 9, 17, 64, 64, 3, 1, 0)]:
        x, w, b, xe, xdec, packed = _case(dev, B, H, W, C, N, 980 + C + k + s, k=k)
        with pytest.raises(CggError):
            ops.conv_x3s_nhwc(xe, packed, N, k, s, p, b.to(dev), cfg=HALO)
        y = ops.conv_x3s_nhwc(xe, packed, N, k, s, p, b.to(dev))
        assert any(torch.equal(y, ops.conv_x3s_nhwc(xe, packed, N, k, s, p, b.to(dev), cfg=ring)) for ring in (13, 12)), (C, k, s, p)
    # a residual launch stays on the ring kernel; forced, it is refused rather than half-supported
    x, w, b, xe, xdec, packed = _case(dev, 2, 9, 17, 64, 64, 990)
    res = ops.x3a_encode(torch.randn(2, 9, 17, 64, generator=torch.Generator().manual_seed(991)).to(dev))
    with pytest.raises(CggError):
        ops.conv_x3s_nhwc(xe, packed, 64, 3, 1, 1, b.to(dev), res=res, cfg=HALO)
    y = ops.conv_x3s_nhwc(xe, packed, 64, 3, 1, 1, b.to(dev), res=res)
    assert any(torch.equal(y, ops.conv_x3s_nhwc(xe, packed, 64, 3, 1, 1, b.to(dev), res=res, cfg=ring)) for ring in (13, 12))
    # the GEMM entry point has no halo form
    with pytest.raises(CggError):
        ops.gemm_x3s(xe.view(-1, 64), ops.pack_linear_weight_x3(torch.randn(64, 64).to(dev)), 64, cfg=HALO)
    assert not ops.x3_overflow_check(dev)


def test_halo_conv_overflow_raises_the_flag(dev):
    """A stored |16 v| > 65504 raises the device-side flag on the halo path too; an f32 output stores no x3a value. A patch pixel
    past the map's edge (the 9 x 17 map leaves most of three patches outside) is not a stored value and raises nothing."""
    x, w, b, xe, xdec, packed = _case(dev, 2, 9, 17, 64, 64, 995)
    big = b.clone()
    big[5] = 6000.0
    ops.x3_overflow_check(dev)
    ops.conv_x3s_nhwc(xe, packed, 64, 3, 1, 1, big.to(dev), out_split=False, cfg=HALO)
    assert not ops.x3_overflow_check(dev)
    ops.conv_x3s_nhwc(xe, packed, 64, 3, 1, 1, big.to(dev), out_split=True, cfg=HALO)
    assert ops.x3_overflow_check(dev)
    assert not ops.x3_overflow_check(dev)
