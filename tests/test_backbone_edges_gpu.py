"""-m gpu tests of the throughput-mode (bf16) ResNet kernels -- what `ResNet._forward_folded` runs under precision_scope('bf16') -- on
exact operands at map edges: stem_conv7x7 (+ its x3 twin and the f32 / x3a max-pool), bottleneck64, bias_relu_maxpool_nhwc,
im2col3x3_nhwc, subsample_nhwc, bias_act_nhwc_, gemm_bias_res_act_bf16, and the layer1 dispatch at the model level.
Operands, float64 references and their conditions: tests/backbone_cases.py; what they cover: tests/test_backbone_cases.py.

The bf16 kernels are held to torch.equal with the float64 reference: the operands are integers small enough that f32 accumulation
in any order is exact and every bf16 rounding is the identity, so a wrong tap, border, packing permutation or channel interleave is an
integer difference. Every kernel call is made twice and must be bit-identical. The LDS-staged kernels (stem, bottleneck) are first
launched on 1000.0, so that stale LDS cannot pass for zero padding.

Outputs that are not exact are held to backbone_cases.yardstick (4 x torch's own f32 error + 2e-7 of the output scale).

Dispatch at the model level: per stage, max |got - ref| / max |ref| against float64 convolutions on the same folded bf16 weights with
bf16 rounding after every convolution's epilogue; the fused layer1 path is held to 2 e_chain + 2^-8, e_chain = the error of the
three-call library path on the same image (the factor 2 is a choice, 2^-8 is one bf16 rounding of the output). Measured on an MI355X
(stages 0 .. 3; every figure is one or two bf16 steps at the stage's largest value, 2^-7 = 0.0078):
  64 x 128   fused 0.0082 0.0078 0.0092 0.0049   three-call 0.0082 0.0078 0.0092 0.0049
             (the two paths differ in 0.023 % of the layer1 outputs; 1.8 %, 11 %, 12 % further down)
  70 x 100   no fused layer1: both runs take the three-call branch and are bit-identical   0.0081 0.0106 0.0091 0.0099
The x3 stem on the small maps spends at most 0.37 of its yardstick (1 x 1 map: 1.39e-07 of 3.81e-07), the pooled map 0.23, its x3a
form 0.15.
"""
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import ops
from cgg_amd._lib import CggError

import backbone_cases as BC

pytestmark = pytest.mark.gpu


def _twice(fn):
    """fn() twice: the outputs must be bit-identical; -> the first"""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    assert torch.equal(a, b), 'two calls differ'
    return a


def _diff(got, want):
    """where an exact comparison fails: the first differing index and both values"""
    got, want = got.detach().cpu().double(), want.double()
    if got.shape != want.shape:
        return 'shape %s != %s' % (tuple(got.shape), tuple(want.shape))
    bad = (got != want).nonzero()
    if not len(bad):
        return 'equal'
    i = tuple(bad[0].tolist())
    return '%d of %d differ, first at %s: got %g, want %g' % (len(bad), got.numel(), i, got[i].item(), want[i].item())


def _assert_exact(got, want64):
    want = want64.to(torch.bfloat16)
    assert got.dtype == torch.bfloat16 and torch.equal(got.cpu(), want), _diff(got, want)


def _err(got, want64):
    return (got.detach().cpu().double() - want64).abs().max().item()


# ------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize('H,W', BC.STEM_MAPS)
def test_stem_conv7x7_coded_filters_on_impulses(dev, H, W):
    """the answer to an impulse is the tap (tap-coded filter) or co + 1 (channel-coded): exact"""
    for which in ['tap'] + BC.STEM_CHANNEL_TAPS:
        c = BC.stem_coded_case(H, W, which)
        packed = ops.pack_stem_weight(c.w.to(dev))
        img = c.img.to(dev)
        ops.stem_conv7x7(torch.full_like(img, 1000.0), packed)
        got = _twice(lambda: ops.stem_conv7x7(img, packed))
        assert got.shape == c.ref.shape
        _assert_exact(got, c.ref)


@pytest.mark.parametrize('H,W', BC.STEM_MAPS)
def test_stem_conv7x7_sparse_integers(dev, H, W):
    c = BC.stem_exact_case(H, W)
    packed = ops.pack_stem_weight(c.w.to(dev))
    img = c.img.to(dev)
    ops.stem_conv7x7(torch.full_like(img, 1000.0), packed)
    got = _twice(lambda: ops.stem_conv7x7(img, packed))
    assert got.shape == (BC.B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)
    _assert_exact(got, c.ref)


@pytest.mark.parametrize('H,W', BC.STEM_MAPS)
def test_stem_conv7x7_x3_and_f32_maxpool_on_small_maps(dev, H, W):
    """parity mode's stem on the same maps, random normal operands: the raw convolution, the f32 (bias, ReLU, max-pool) pass and its
    x3a form (decoded; + the format's storage term), all to the yardstick; the x3 overflow flag stays clear"""
    c = BC.stem_x3_case(H, W)
    pk, sc = ops.pack_stem_weight_x3(c.w.to(dev))
    img, b = c.img.to(dev), c.b.to(dev)
    ops.x3_overflow_check(dev)                                     # clear whatever an earlier test left
    assert not ops.x3_overflow_check(dev)
    ops.stem_conv7x7_x3(torch.full_like(img, 1000.0), pk, sc)
    y = _twice(lambda: ops.stem_conv7x7_x3(img, pk, sc))
    e = _err(y, c.raw)
    print('x3 stem %dx%d: raw %.3g / %.3g' % (H, W, e, BC.yardstick(c.e_ref, c.raw_scale)))
    assert y.shape == c.raw.shape and e <= BC.yardstick(c.e_ref, c.raw_scale), (e, c.e_ref)
    z = _twice(lambda: ops.bias_relu_maxpool_nhwc_f32(y, b))
    e = _err(z, c.pooled)
    print('    pooled %.3g / %.3g' % (e, BC.yardstick(c.e_ref_pooled, c.pooled_scale)))
    assert z.shape == c.pooled.shape and e <= BC.yardstick(c.e_ref_pooled, c.pooled_scale), (e, c.e_ref_pooled)
    za = _twice(lambda: ops.bias_relu_maxpool_nhwc_f32(y, b, x3a=True))
    zd = ops.x3a_decode(za)
    e = _err(zd, c.pooled)
    bound = BC.yardstick(c.e_ref_pooled, c.pooled_scale) + BC.x3a_storage(c.pooled_scale)
    print('    x3a    %.3g / %.3g' % (e, bound))
    assert (zd >= 0).all() and e <= bound, (e, c.e_ref_pooled)
    assert not ops.x3_overflow_check(dev)


# ------------------------------------------------------------------------------------------------ max-pool
@pytest.mark.parametrize('H,W', BC.POOL_MAPS)
def test_bias_relu_maxpool_nhwc_exact(dev, H, W):
    for C in BC.POOL_C:
        for negative in (False, True):
            c = BC.pool_case(H, W, C, 'bf16', negative)
            x, b = c.x.to(dev), c.b.to(dev)
            got = _twice(lambda: ops.bias_relu_maxpool_nhwc(x, b))
            assert torch.equal(got.cpu(), c.want), (C, negative, _diff(got, c.want))
            if negative:
                assert torch.isfinite(got.float()).all() and not got.float().any()          # no -inf escapes, all zero


@pytest.mark.parametrize('H,W', BC.POOL_MAPS)
def test_bias_relu_maxpool_nhwc_f32_exact_and_x3a_decodes_to_it(dev, H, W):
    """the f32 kernel pools, then adds the bias: the same bits as torch's relu(x + b) pooled (f32 addition of b is monotone). The
    x3a form holds those values to the format's 22 bits. The all-negative map gives exact zeros in both forms."""
    ops.x3_overflow_check(dev)
    assert not ops.x3_overflow_check(dev)
    for C in BC.POOL_C:
        for negative in (False, True):
            c = BC.pool_case(H, W, C, 'f32', negative)
            x, b = c.x.to(dev), c.b.to(dev)
            got = _twice(lambda: ops.bias_relu_maxpool_nhwc_f32(x, b))
            assert torch.equal(got.cpu(), c.want), (C, negative, _diff(got, c.want))
            enc = _twice(lambda: ops.bias_relu_maxpool_nhwc_f32(x, b, x3a=True))
            dec = ops.x3a_decode(enc)
            scale = c.want.abs().max().item()
            assert (dec >= 0).all() and _err(dec, c.want.double()) <= BC.x3a_storage(scale), (C, negative)
            if negative:
                assert not dec.any()
    assert not ops.x3_overflow_check(dev)


# ------------------------------------------------------------------------------------------------ patches
@pytest.mark.parametrize('H,W', BC.PATCH_MAPS)
def test_im2col3x3_and_subsample_exact(dev, H, W):
    for C in BC.PATCH_C:
        x = BC.patch_case(H, W, C)
        xd = x.to(dev)
        for st in BC.IM2COL_STRIDES:
            want, Ho, Wo = BC.im2col_ref(x, st)
            got = _twice(lambda: ops.im2col3x3_nhwc(xd, st)[0])
            assert ops.im2col3x3_nhwc(xd, st)[1:] == (Ho, Wo)
            assert torch.equal(got.cpu(), want), (C, st, _diff(got, want))
        for st in BC.SUBSAMPLE_STRIDES:
            got = _twice(lambda: ops.subsample_nhwc(xd, st))
            want = x[:, ::st, ::st, :].contiguous()
            assert got.is_contiguous() and torch.equal(got.cpu(), want), (C, st, _diff(got, want))


# ------------------------------------------------------------------------------------------------ epilogue
@pytest.mark.parametrize('rows,C', BC.BIAS_ACT_SHAPES)
def test_bias_act_nhwc_past_the_grid_cap(dev, rows, C):
    """the control tensor, then totals just over 8192 x 256 vectors: the grid-stride loop's second trip, whose bias index must go on
    from i % c8 (neither 3 nor 24 vectors per row divide the stride)"""
    y, b, r = BC.bias_act_case(rows, C)
    yd, bd, rd = y.to(dev), b.to(dev), r.to(dev)
    for has_b, has_r, relu in BC.BIAS_ACT_COMBOS:
        want = BC.bias_act_ref(y, b if has_b else None, r if has_r else None, relu)
        got = _twice(lambda: ops.bias_act_nhwc_(yd.clone(), bd if has_b else None, rd if has_r else None, relu))
        assert torch.equal(got.cpu(), want), (has_b, has_r, relu, _diff(got, want))


# ------------------------------------------------------------------------------------------------ bottleneck
def _bottleneck(dev, c):
    packed = ops.pack_bottleneck64(*(t.to(dev) for t in (c.w1, c.b1, c.w2, c.b2, c.w3, c.b3)))
    x = c.x.to(dev)
    assert ops.bottleneck64_ok(x)
    ops.bottleneck64(torch.full_like(x, 1000.0), packed)
    got = _twice(lambda: ops.bottleneck64(x, packed))
    _assert_exact(got, c.ref)


@pytest.mark.parametrize('H,W', BC.BOTTLENECK_MAPS)
def test_bottleneck64_sparse_integers(dev, H, W):
    _bottleneck(dev, BC.bottleneck_exact_case(H, W))


@pytest.mark.parametrize('which', ['taps', 'chan'])
@pytest.mark.parametrize('H,W', [(8, 16), (16, 32)])
def test_bottleneck64_coded_weights_on_impulses(dev, H, W, which):
    """b1 = 1 > 0: relu(b1) is non-zero on every pixel of the image and must be ZERO in conv2's padding (bottleneck.hip phase 1);
    'taps': a border pixel's t2 is the sum of the tap codes inside the image; 'chan': channel co answers co + 1 (the row permutation
    of pack_bottleneck64). For 'chan' every tap of w2 takes a turn."""
    taps = [(ky, kx) for ky in range(3) for kx in range(3)] if which == 'chan' else [(0, 2)]
    for tap in taps:
        _bottleneck(dev, BC.bottleneck_coded_case(H, W, which, tap))


def test_bottleneck64_gate_and_forced_call_off_the_tile(dev):
    c = BC.bottleneck_exact_case(8, 16)
    packed = ops.pack_bottleneck64(*(t.to(dev) for t in (c.w1, c.b1, c.w2, c.b2, c.w3, c.b3)))
    for H, W in BC.BOTTLENECK_OFF:
        x = torch.zeros(BC.B, H, W, 256, dtype=torch.bfloat16, device=dev)
        assert not ops.bottleneck64_ok(x), (H, W)
        with pytest.raises(CggError):
            ops.bottleneck64(x, packed)
    for H, W in BC.BOTTLENECK_MAPS:
        assert ops.bottleneck64_ok(torch.zeros(BC.B, H, W, 256, dtype=torch.bfloat16, device=dev))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ library GEMM
@pytest.mark.parametrize('M', BC.GEMM_M)
def test_gemm_bias_res_act_bf16_exact_integers(dev, M):
    """a library call: a mismatch is a finding about how it is called (beta = 1 residual, epilogue order)"""
    for N in BC.GEMM_N:
        for K in BC.GEMM_K:
            for has_res in (False, True):
                for relu in (False, True):
                    c = BC.gemm_exact_case(M, N, K, has_res, relu)
                    x, w, b = c.x.to(dev), c.w.to(dev), c.b.to(dev)
                    r = c.r.to(dev) if has_res else None
                    got = _twice(lambda: ops.gemm_bias_res_act_bf16(x, w, b, r, relu))
                    assert got.shape == (M, N)
                    assert torch.equal(got.cpu(), c.want.to(torch.bfloat16)), (N, K, has_res, relu, _diff(got, c.want))


# ------------------------------------------------------------------------------------------------ model level
_MODEL = {}


def _resnet50(dev):
    if 'bb' not in _MODEL:
        from cgg_amd import registry
        torch.manual_seed(3)
        bb = registry.build_backbone(dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=-1,
                                          norm_cfg=dict(type='BN', requires_grad=False), norm_eval=True, style='pytorch'))
        BC.randomise_bn(bb)
        bb = bb.to(dev).eval()
        _MODEL['bb'] = bb
        _MODEL['folded'] = [tuple(None if t is None else t.cpu() for t in f) for f in bb._folded()]
    return _MODEL['bb'], _MODEL['folded']


@pytest.mark.parametrize('H,W', BC.MODEL_IMAGES)
def test_layer1_dispatch_is_consistent_at_the_model_level(dev, H, W, monkeypatch):
    """64 x 128 reaches bottleneck64 in layer1 (16 x 32 map), 70 x 100 does not (18 x 25: the three-call branch). Each image runs
    as dispatched and again with bottleneck64_ok forced to False."""
    from cgg_amd import runtime
    bb, folded = _resnet50(dev)
    g = torch.Generator().manual_seed(4500 + H)
    img = torch.randn(BC.B, 3, H, W, generator=g)
    ref = BC.folded_resnet_ref(bb, folded, img)
    calls = []
    real = ops.bottleneck64

    def counted(x, packed):
        calls.append(tuple(x.shape))
        return real(x, packed)

    monkeypatch.setattr(ops, 'bottleneck64', counted)
    with torch.no_grad(), runtime.precision_scope('bf16'):
        got = [o.float().cpu() for o in bb(img.to(dev))]
        fused_calls = len(calls)
        monkeypatch.setattr(ops, 'bottleneck64_ok', lambda x: False)
        chain = [o.float().cpu() for o in bb(img.to(dev))]
    h1, w1 = ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1
    fusable = h1 % 8 == 0 and w1 % 16 == 0
    assert fused_calls == (2 if fusable else 0) and len(calls) == fused_calls      # layer1's two identity blocks, or none
    rel = lambda o, r: ((o.double() - r).abs().max() / r.abs().max()).item()
    e_got = [rel(o, r) for o, r in zip(got, ref)]
    e_chain = [rel(o, r) for o, r in zip(chain, ref)]
    print('%dx%d dispatched %s' % (H, W, ' '.join('%.4f' % e for e in e_got)))
    print('%dx%d three-call %s' % (H, W, ' '.join('%.4f' % e for e in e_chain)))
    print('%dx%d elements that differ between the two runs: %s' % (H, W, ' '.join('%.2g' % (a != b).float().mean().item()
                                                                                for a, b in zip(got, chain))))
    for o, r in zip(got, ref):
        assert o.shape == r.shape
    for s, (e, ec) in enumerate(zip(e_got, e_chain)):
        assert e <= 2 * ec + 2.0 ** -8, (s, e, ec)
        assert ec <= 0.06, (s, ec)                    # the three-call path itself: the existing rule of the folded-backbone test
    if not fusable:
        for a, b in zip(got, chain):
            assert torch.equal(a, b)                  # nothing to dispatch: the same launches on the same operands
