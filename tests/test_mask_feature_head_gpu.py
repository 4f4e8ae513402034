"""cgg_mask_feature_head_x3 (csrc/mask_feature_head.hip): GroupNorm apply + ReLU, the 1 x 1 mask_feature convolution and the packed
x3 images in ONE launch, against the three calls it replaces (bit for bit) and against float64."""
import warnings

import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import ops, runtime, synthetic

pytestmark = pytest.mark.gpu

C, G, EPS = 256, 32, 1e-5

# (B, H, W), pools
SHAPES = [
    ((1, 8, 8), [1]),                    # one tile
    ((2, 16, 24), [1, 2, 4, 8]),         # several tiles per row; pool-8 image of 6 pixels: a ragged 32-pixel tile, padding zero
    ((1, 8, 40), [1, 2]),                # pool-1 image of 320 pixels, tiles straddling image rows
    ((2, 24, 16), [1, 4, 8]),            # a pool subset
]

_CACHE = {}


def _case(dev, shape, pools, gamma_scale=1.0):
    """inputs, the three-call path's outputs and the fused outputs of one shape -- computed once, shared by the tests, not modified"""
    key = (shape, tuple(pools), gamma_scale)
    if key in _CACHE:
        return _CACHE[key]
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * H + W + B)
    z = (torch.randn(B, H * W, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + 0.3 * torch.randn(C, generator=g)).to(dev)
    gamma = ((1 + 0.1 * torch.randn(C, generator=g)) * gamma_scale).to(dev)
    beta = (0.1 * torch.randn(C, generator=g)).to(dev)
    wt = (torch.randn(C, C, generator=g) / 16).to(dev)
    bias = (0.1 * torch.randn(C, generator=g)).to(dev)
    wk = ops.pack_linear_weight_x3(wt)
    ops.x3_overflow_check(dev, reset=True)
    # the path it replaces
    ws = ops.group_norm_nhwc_workspace(B, H * W, G, dev)
    a = torch.empty_like(z)
    ops.group_norm_nhwc_x3a(z, gamma, beta, G, EPS, ws, out=(a, 0, H * W * C), relu=True)
    mf = runtime.linear_x3s(a.view(B * H * W, C), wt, bias).view(B, H, W, C)
    old = dict(zip(pools, ops.pack_mask_feature_nhwc_x3(mf, pools)))
    old_flag = ops.x3_overflow_check(dev, reset=True)
    # fused: outputs pre-filled with a pattern, so that a slot the kernel leaves unwritten (padding) shows
    ws2 = ops.group_norm_nhwc_workspace(B, H * W, G, dev)
    ops.group_norm_nhwc_stats(z, G, ws2)
    head = (z.view(B, H, W, C), ws2, (gamma, beta, EPS, G), wk, bias, pools)
    assert ops.mask_feature_head_x3_ok(*head)
    junk = [torch.full((B, ((H // p) * (W // p) + 31) // 32, C // 8, 32, 8), 1.5, dtype=torch.bfloat16, device=dev) for p in pools * 2]
    del junk                                           # freed blocks are what the caching allocator hands to the call below
    new, mf2 = ops.mask_feature_head_x3(*head, want_f32=True)
    new_flag = ops.x3_overflow_check(dev, reset=True)
    new_nomf = ops.mask_feature_head_x3(*head)
    new_cfg0 = ops.mask_feature_head_x3(*head, cfg=0)
    ops.x3_overflow_check(dev, reset=True)
    torch.cuda.synchronize()
    stats = ws[:B * G * 2].view(B, G, 2).clone()
    assert torch.equal(stats, ws2[:B * G * 2].view(B, G, 2))
    out = dict(z=z, gamma=gamma, beta=beta, wt=wt, bias=bias, stats=stats, mf=mf, old=old, new=new, mf2=mf2, new_nomf=new_nomf,
               new_cfg0=new_cfg0, old_flag=old_flag, new_flag=new_flag)
    _CACHE[key] = out
    return out


def _bits(t):
    return t.view(torch.int16)


def _decode(pf, npix):
    """PackedFeature -> (B, npix, C) float64 values (hi + lo) / 16, and the padding slots' raw bits"""
    hi, lo = pf.hi.view(torch.float16).double(), pf.lo.view(torch.float16).double()
    B, T = hi.shape[:2]
    v = ((hi + lo) / 16).permute(0, 1, 3, 2, 4).reshape(B, T * 32, C)          # [b][t][pl][kc][e] -> pixel-major
    raw = torch.stack([_bits(pf.hi), _bits(pf.lo)]).permute(0, 1, 2, 4, 3, 5).reshape(2, B, T * 32, C)
    return v[:, :npix].cpu(), raw[:, :, npix:].cpu()


@pytest.mark.parametrize('shape,pools', SHAPES)
def test_bit_identical_to_three_calls(dev, shape, pools):
    c = _case(dev, shape, pools)
    assert set(c['new']) == set(pools)
    for p in pools:
        for which in ('new', 'new_nomf', 'new_cfg0'):
            assert torch.equal(_bits(c[which][p].hi), _bits(c['old'][p].hi)), (which, p, 'hi')
            assert torch.equal(_bits(c[which][p].lo), _bits(c['old'][p].lo)), (which, p, 'lo')
        assert (c['new'][p].h, c['new'][p].w) == (c['old'][p].h, c['old'][p].w)
    assert torch.equal(c['mf2'], c['mf'])
    assert c['old_flag'] is False and c['new_flag'] is False


@pytest.mark.parametrize('shape,pools', SHAPES)
def test_vs_float64(dev, shape, pools):
    """GroupNorm (with the kernel's f32 statistics), ReLU and the 1 x 1 in float64 on the same f32 inputs: 2e-5 of the unit-scale
    outputs, the bound of tests/test_x3_gpu.py for this arithmetic; pooled images against the float64 2 x 2 centre mean."""
    c = _case(dev, shape, pools)
    B, H, W = shape
    d = lambda t: t.detach().cpu().double()
    st = d(c['stats'])
    mean, var = st[:, :, 0].repeat_interleave(8, 1).view(B, 1, C), st[:, :, 1].repeat_interleave(8, 1).view(B, 1, C)
    a = torch.relu((d(c['z']) - mean) / torch.sqrt(var + EPS) * d(c['gamma']) + d(c['beta']))
    want = (a @ d(c['wt']).t() + d(c['bias'])).view(B, H, W, C)
    assert 0.3 < want.abs().mean().item() < 3.0                                # unit scale
    assert (d(c['mf2']) - want).abs().max().item() <= 2e-5
    for p in pools:
        if p == 1:
            ref = want.reshape(B, H * W, C)
        else:
            o = p // 2 - 1
            ref = ((want[:, o::p, o::p] + want[:, o::p, o + 1::p] + want[:, o + 1::p, o::p] + want[:, o + 1::p, o + 1::p]) / 4)
            ref = ref.reshape(B, (H // p) * (W // p), C)
        got, pad = _decode(c['new'][p], ref.shape[1])
        err = (got - ref).abs().max().item()
        assert err <= 2e-5, (p, err)
        assert not pad.any(), p                                                # padding of a ragged last tile: zeros


def test_overflow_flag_matches(dev):
    """normalised values beyond the x3a range (large gamma): the fused call leaves the overflow flag as the three-call path does"""
    c = _case(dev, (1, 8, 8), [1], gamma_scale=3.0e4)
    assert c['old_flag'] is True and c['new_flag'] is True
    assert ops.x3_overflow_check(dev, reset=True) is False                     # left reset


def test_whole_head_equal_with_gate_off(dev, monkeypatch):
    """`simple_test` of the head at B = 1, 64 x 64 (16 x 16 mask feature), 8 queries: the outputs with the fused kernel equal the
    outputs with the gate forced off, bit for bit."""
    from util import build_heads, small_cfg
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prod, _ = build_heads(small_cfg(num_queries=8, vocab=120))
    prod = prod.to(dev)
    B, H, W = 1, 64, 64
    feats = [f.to(dev) for f in synthetic.backbone_feats(B, H, W, channels=(64, 128, 256, 512), seed=3)]
    metas = synthetic.img_metas(B, H, W)
    calls = []
    real = ops.mask_feature_head_x3
    monkeypatch.setattr(ops, 'mask_feature_head_x3', lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run():
        with torch.no_grad():
            cls, emb, masks, _, _ = prod.simple_test(feats, metas)
            torch.cuda.synchronize()
        return cls.clone(), emb.clone(), masks.upsampled().clone()

    fused = run()
    assert len(calls) == 1, 'the fused kernel did not run'
    monkeypatch.setattr(ops, 'mask_feature_head_x3_ok', lambda *a, **k: False)
    plain = run()
    assert len(calls) == 1
    for a, b in zip(fused, plain):
        assert torch.equal(a, b)
