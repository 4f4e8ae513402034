"""-m gpu parity tests: each HIP kernel, called through the C ABI (ctypes), against the CPU oracle on the
same seeded inputs. Tolerances are written next to each check.
  * integer / index / bit outputs: exact (ties excluded where the oracle's own value is within 1e-5
    of the decision threshold -- stated per test);
  * mask logits, split (f32-class) mode: |err| <= 1e-3 absolute (north_star), bf16 mode: 2^-7 relative
    to sum|a||b| (bf16 input rounding);
  * MSDeformAttn / attention f32: 1e-4 absolute.
"""
import math

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import ops
from oracle import ops as ref

from util import plain  # noqa: E402
import sampling_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu


def _levels(shapes):
    starts, s = [], 0
    for h, w in shapes:
        starts.append(s)
        s += h * w
    return starts, s


def _msda_inputs(B, shapes, H, D, P, Nq, seed, spread=1.0):
    g = torch.Generator().manual_seed(seed)
    starts, Nv = _levels(shapes)
    L = len(shapes)
    value = torch.randn(B, Nv, H, D, generator=g)
    # locations mostly inside [0,1] with some outside (exercise zero padding / skip rule)
    loc = torch.rand(B, Nq, H, L, P, 2, generator=g) * (1 + 0.4 * spread) - 0.2 * spread
    aw = torch.softmax(torch.randn(B, Nq, H, L * P, generator=g), -1).view(B, Nq, H, L, P)
    ss = torch.tensor(shapes, dtype=torch.int64)
    st = torch.tensor(starts, dtype=torch.int64)
    return value, ss, st, loc, aw


@pytest.mark.parametrize('shapes,B,Nq', [
    ([(4, 4), (8, 8), (16, 16)], 2, 336),
    ([(5, 7), (10, 14), (20, 28)], 1, 1190),  # ragged, non power of two
    ([(32, 32), (64, 64), (128, 128)], 1, 3000),
])
def test_msda_forward_vs_oracle(dev, shapes, B, Nq):
    value, ss, st, loc, aw = _msda_inputs(B, shapes, 8, 32, 4, Nq, seed=1)
    want = ref.msda_core(value, ss, loc, aw)
    got = ops.msda_forward(value.to(dev), ss.to(dev), st.to(dev), loc.to(dev), aw.to(dev)).cpu()
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-4
    got2 = ops.msda_forward_hostlevels(value.to(dev), shapes, _levels(shapes)[0], loc.to(dev),
                                       aw.to(dev)).cpu()
    assert torch.equal(got, got2)


def test_msda_forward_loops_oracle_small(dev):
    shapes = [(3, 5), (6, 10)]
    value, ss, st, loc, aw = _msda_inputs(1, shapes, 2, 8, 3, 40, seed=2, spread=2.0)
    want = ref.msda_core_loops(value, ss, loc, aw).float()
    want2 = ref.msda_core(value, ss, loc, aw)
    assert (want - want2).abs().max().item() <= 1e-5  # the two oracle statements agree
    got = ops.msda_forward(value.to(dev), ss.to(dev), st.to(dev), loc.to(dev), aw.to(dev)).cpu()
    assert (got - want).abs().max().item() <= 1e-5


def test_msda_known_answer_one_hot(dev):
    """offsets 0 + one-hot weight on (level l, point 0) == bilinear sample at the reference
    point; at pixel centres that is the value itself."""
    shapes = [(4, 4), (8, 8)]
    starts, Nv = _levels(shapes)
    g = torch.Generator().manual_seed(3)
    value = torch.randn(1, Nv, 8, 32, generator=g)
    h, w = shapes[1]
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    refp = torch.stack([(xs.flatten() + 0.5) / w, (ys.flatten() + 0.5) / h], -1)  # (64,2)
    Nq = h * w
    loc = refp[None, :, None, None, None, :].expand(1, Nq, 8, 2, 4, 2).contiguous()
    aw = torch.zeros(1, Nq, 8, 2, 4)
    aw[..., 1, 0] = 1.0
    got = ops.msda_forward(value.to(dev), torch.tensor(shapes).to(dev), torch.tensor(starts).to(dev),
                           loc.to(dev), aw.to(dev)).cpu()
    want = value[:, starts[1]:starts[1] + Nq].reshape(1, Nq, 256)
    assert (got - want).abs().max().item() <= 1e-6


def test_msda_bf16_value(dev):
    shapes = [(8, 8), (16, 16), (32, 32)]
    value, ss, st, loc, aw = _msda_inputs(2, shapes, 8, 32, 4, 1344, seed=4)
    vb = value.bfloat16()
    want = ref.msda_core(vb.float(), ss, loc, aw)
    got = ops.msda_forward(vb.to(dev), ss.to(dev), st.to(dev), loc.to(dev), aw.to(dev)).cpu()
    assert (got - want).abs().max().item() <= 1e-4  # same bf16-rounded values, f32 arithmetic


@pytest.mark.parametrize('shapes', [
    [(8, 8), (16, 16), (32, 32)],      # every level % 8: a block = the four 4 x 4 tiles of an 8 x 8 pixel block of one head
    [(4, 4), (12, 12), (20, 20)],      # % 4 only: 4 x 4 tiles per wave, a block = 4 heads
    [(5, 7), (10, 14), (20, 28)],      # ragged: 16 x 1 strips
])
def test_msda_fused_prologue(dev, shapes):
    """The f32 stream kernel (offsets / logits rows in, softmax + reference-point arithmetic fused) in its three query -> lane
    mappings (csrc/msda.hip, round 4) against the [3P] op's definition (`ref.msda_core`)."""
    starts, Nv = _levels(shapes)
    B, H, D, L, P = 2, 8, 32, 3, 4
    Nq = Nv
    g = torch.Generator().manual_seed(5)
    value = torch.randn(B, Nv, H, D, generator=g)
    raw = torch.randn(B, Nq, H * L * P * 3, generator=g)
    raw[..., :H * L * P * 2] *= 2.0
    refp = torch.rand(Nq, 2, generator=g)
    off = raw[..., :H * L * P * 2].view(B, Nq, H, L, P, 2)
    logit = raw[..., H * L * P * 2:].view(B, Nq, H, L * P)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32)
    loc = refp[None, :, None, None, None, :] + off / norm[None, None, None, :, None, :]
    aw = logit.softmax(-1).view(B, Nq, H, L, P)
    want = ref.msda_core(value, torch.tensor(shapes), loc, aw)
    got = ops.msda_forward_fused(value.to(dev), shapes, starts, raw.to(dev), refp.to(dev), P).cpu()
    assert (got - want).abs().max().item() <= 1e-4


def test_msda_fused_prologue_reordered_levels(dev):
    """the 2-D query -> lane mappings assume that the levels tile [0, Nq) in ascending order. A level table that is
    legal for the op (every level inside the value rows) but stored in another order must fall back to the strip mapping and give
    the same result as the standard layout."""
    shapes = [(8, 8), (16, 16), (32, 32)]
    starts, Nv = _levels(shapes)
    B, H, D, L, P = 2, 8, 32, 3, 4
    g = torch.Generator().manual_seed(15)
    value = torch.randn(B, Nv, H, D, generator=g)
    raw = torch.randn(B, Nv, H * L * P * 3, generator=g)
    refp = torch.rand(Nv, 2, generator=g)
    std = ops.msda_forward_fused(value.to(dev), shapes, starts, raw.to(dev), refp.to(dev), P).cpu()
    # the same three maps stored finest-first: starts = [5 * 256, 256 * 4, 0]
    parts = [value[:, s:s + h * w] for s, (h, w) in zip(starts, shapes)]
    vperm = torch.cat(parts[::-1], 1).contiguous()
    pstarts = [shapes[2][0] * shapes[2][1] + shapes[1][0] * shapes[1][1], shapes[2][0] * shapes[2][1], 0]
    got = ops.msda_forward_fused(vperm.to(dev), shapes, pstarts, raw.to(dev), refp.to(dev), P).cpu()
    assert torch.equal(got, std)


def test_msda_backward_vs_autograd(dev):
    shapes = [(6, 6), (12, 12)]
    value, ss, st, loc, aw = _msda_inputs(2, shapes, 4, 16, 4, 90, seed=6)
    v64, l64, a64 = (t.double().requires_grad_(True) for t in (value, loc, aw))
    out = ref.msda_core(v64, ss, l64, a64)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(7))
    out.backward(go.double())
    gv, gl, ga = ops.msda_backward(value.to(dev), ss.to(dev), st.to(dev), loc.to(dev), aw.to(dev),
                                   go.to(dev))
    assert (gv.cpu() - v64.grad.float()).abs().max().item() <= 1e-4
    assert (ga.cpu() - a64.grad.float()).abs().max().item() <= 1e-4
    # d/d(loc) is discontinuous at integer pixel coordinates; random inputs stay clear of them
    assert (gl.cpu() - l64.grad.float()).abs().max().item() <= 2e-3
    # ... and off them it is held to 8 max(torch's own f32 error, 2^-24 sum |terms|) (tests/sampling_cases.py)
    SC.assert_grad_loc('msda_backward', value, shapes, loc, aw, go, gl, l64.grad)


@pytest.mark.parametrize('shapes,H,D,P,spread', [
    ([(8, 8), (16, 16), (32, 32)], 8, 32, 4, 0.0),      # local offsets: LDS-window path of the tiled kernel
    ([(8, 8), (16, 16), (32, 32)], 8, 32, 4, 1.0),      # half of the taps far away: global-atomic path
    ([(5, 7), (10, 14), (20, 28)], 2, 32, 4, 0.0),      # ragged pyramid, edge tiles
    ([(6, 6), (12, 12)], 4, 16, 3, 0.3),                # generic P, two levels
    ([(6, 6), (11, 12)], 4, 16, 4, 0.0),                # non-integer scale -> untiled kernel
])
def test_msda_backward_self_attention_tiled(dev, shapes, H, D, P, spread):
    """Encoder case (queries == pixels of the pyramid): sampling locations = the query's own reference point +
    a few pixels (what the trained offsets look like), optionally mixed with far-away samples."""
    g = torch.Generator().manual_seed(60)
    starts, Nv = _levels(shapes)
    L, B = len(shapes), 2
    value = torch.randn(B, Nv, H, D, generator=g)
    refs = []
    for (h, w) in shapes:
        ys, xs = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing='ij')
        refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    refp = torch.cat(refs, 0)                                            # (Nv, 2) in (x, y)
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32)  # (L, 2)
    off = (torch.rand(B, Nv, H, L, P, 2, generator=g) - 0.5) * 9.0       # up to +-4.5 px in the level's units
    loc = refp[None, :, None, None, None, :] + off / wh[None, None, None, :, None, :]
    far = torch.rand(B, Nv, H, L, P, 1, generator=g) < 0.5 * spread
    loc = torch.where(far, torch.rand(B, Nv, H, L, P, 2, generator=g) * 1.4 - 0.2, loc)
    aw = torch.softmax(torch.randn(B, Nv, H, L * P, generator=g), -1).view(B, Nv, H, L, P)
    ss = torch.tensor(shapes, dtype=torch.int64)
    st = torch.tensor(starts, dtype=torch.int64)
    v64, l64, a64 = (t.double().requires_grad_(True) for t in (value, loc, aw))
    out = ref.msda_core(v64, ss, l64, a64)
    go = torch.randn(out.shape, generator=g)
    out.backward(go.double())
    gv, gl, ga = ops.msda_backward(value.to(dev), ss.to(dev), st.to(dev), loc.to(dev), aw.to(dev), go.to(dev))
    assert (gv.cpu() - v64.grad.float()).abs().max().item() <= 2e-4
    assert (ga.cpu() - a64.grad.float()).abs().max().item() <= 2e-4
    d = (gl.cpu() - l64.grad.float()).abs()
    assert d.max().item() <= 5e-3 * max(1.0, l64.grad.abs().max().item())
    SC.assert_grad_loc(f'msda_backward {shapes}', value, shapes, loc, aw, go, gl, l64.grad)     # the tight bound off the lattice
    # round 5: the host-level-table entry point (no read-back; grad_loc / grad_attn WRITTEN by the gather kernel where the split
    # backward applies, un-zeroed outputs) gives the same three gradients
    gv2, gl2, ga2 = ops.msda_backward_hostlevels(value.to(dev), shapes, starts, loc.to(dev), aw.to(dev), go.to(dev))
    assert (gv2.cpu() - v64.grad.float()).abs().max().item() <= 2e-4
    # (written vs accumulated-into-zero: two instantiations of the gather kernel, the compiler contracts their FMAs differently)
    assert (ga2 - ga).abs().max().item() <= 1e-5 * ga.abs().max().item() and (gl2 - gl).abs().max().item() <= 1e-5 * gl.abs().max().item()


@pytest.mark.parametrize('B,shapes,spread,amp', [(2, [(16, 16), (32, 32), (64, 64)], 0.0, 8.0),     # full tiles, patch-mapped gather
                                                 (1, [(12, 20), (24, 40), (48, 80)], 0.6, 8.0),     # ragged tile grid, most taps outside the windows
                                                 (3, [(8, 8), (16, 16), (32, 32)], 0.2, 8.0),
                                                 (2, [(16, 16), (32, 32), (64, 64)], 0.0, 16.0),    # +-8 px: most corners in the SECOND pass' window
                                                 (1, [(12, 20), (24, 40), (48, 80)], 0.1, 40.0),    # +-20 px: all three destinations of a corner
                                                 (2, [(9, 7), (18, 14), (36, 28)], 0.05, 20.0)])    # odd coarse grid (ragged second-pass regions)
def test_msda_backward_sorted_scatter_vs_float64(dev, B, shapes, spread, amp):
    """csrc/msda_bwd.hip at encoder-like sizes: the corner records of a tile sorted by destination pixel, destination-stationary
    sums, out-of-window corners through the second pass (re-sorted on larger tiles, round 6) and the record list's tail -- against
    float64 autograd of the op's definition, local offsets (uniform +- amp / 2 pixels) and far-away samples mixed; two runs differ only
    by f32 summation order; the single-pass form (CGG_MSDA_BWD_2P=0) gives the same gradient."""
    g = torch.Generator().manual_seed(61 + B)
    starts, Nv = _levels(shapes)
    L, H, D, P = len(shapes), 8, 32, 4
    value = torch.randn(B, Nv, H, D, generator=g)
    refs = []
    for (h, w) in shapes:
        ys, xs = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing='ij')
        refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    refp = torch.cat(refs, 0)
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32)
    off = (torch.rand(B, Nv, H, L, P, 2, generator=g) - 0.5) * amp
    loc = refp[None, :, None, None, None, :] + off / wh[None, None, None, :, None, :]
    far = torch.rand(B, Nv, H, L, P, 1, generator=g) < spread
    loc = torch.where(far, torch.rand(B, Nv, H, L, P, 2, generator=g) * 1.4 - 0.2, loc)
    aw = torch.softmax(torch.randn(B, Nv, H, L * P, generator=g), -1).view(B, Nv, H, L, P)
    go = torch.randn(B, Nv, H * D, generator=g) * 1e-3                   # a real gradient magnitude
    v64, l64, a64 = (t.double().requires_grad_(True) for t in (value, loc, aw))
    ref.msda_core(v64, torch.tensor(shapes), l64, a64).backward(go.double())
    gv, gl, ga = ops.msda_backward_hostlevels(value.to(dev), shapes, starts, loc.to(dev), aw.to(dev), go.to(dev))
    sc = v64.grad.abs().max().item()
    assert (gv.cpu().double() - v64.grad).abs().max().item() <= 2e-5 * sc
    assert (ga.cpu().double() - a64.grad).abs().max().item() <= 2e-4 * a64.grad.abs().max().item()
    assert (gl.cpu().double() - l64.grad).abs().max().item() <= 5e-3 * l64.grad.abs().max().item()
    SC.assert_grad_loc(f'msda_backward_hostlevels {shapes}', value, shapes, loc, aw, go, gl, l64.grad)    # the tight bound off the lattice
    gv2, _, _ = ops.msda_backward_hostlevels(value.to(dev), shapes, starts, loc.to(dev), aw.to(dev), go.to(dev))
    assert (gv2 - gv).abs().max().item() <= 1e-5 * sc
    old = ops.MSDA_BWD_2P
    try:
        ops.MSDA_BWD_2P = not old                     # the other form (single pass <-> two passes)
        gv3, _, _ = ops.msda_backward_hostlevels(value.to(dev), shapes, starts, loc.to(dev), aw.to(dev), go.to(dev))
    finally:
        ops.MSDA_BWD_2P = old
    assert (gv3 - gv).abs().max().item() <= 1e-5 * sc


def test_msda_padded_value_rows_equal_packed_rows(dev):
    """`ops.padded_value_rows`: value (and grad_value) rows with a 288-float stride instead of 256 -- the strided-value forms of the
    fused forward (`cgg_msda_forward_fused_vld`) and of the split backward (`cgg_msda_backward_hostlevels_ws`, vld) give the packed
    layout's results (forward bit-identical, grad_value up to the atomics' summation order); the pad columns stay untouched."""
    shapes = [(8, 8), (16, 16), (32, 32)]
    starts, Nv = _levels(shapes)
    B, H, D, L, P = 2, 8, 32, 3, 4
    g = torch.Generator().manual_seed(91)
    value = torch.randn(B, Nv, H, D, generator=g).to(dev)
    rows = torch.randn(B, Nv, 3 * H * L * P, generator=g).to(dev)
    refs = []
    for (h, w) in shapes:
        ys, xs = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing='ij')
        refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    ref_pts = torch.cat(refs, 0).to(dev)
    buf, v4 = ops.padded_value_rows(B, Nv, H, D, dev)
    assert ops.MSDA_VALUE_PAD == 32 and v4.stride(1) == 288
    buf.fill_(7.0)
    v4.copy_(value)
    want = ops.msda_forward_fused(value, shapes, starts, rows, ref_pts, P)
    got = ops.msda_forward_fused(v4, shapes, starts, rows, ref_pts, P)
    assert torch.equal(got, want)
    go = torch.randn(B, Nv, H * D, generator=g).to(dev) * 1e-3
    gv0, gr0 = ops.msda_rows_backward(value, rows, ref_pts, shapes, starts, P, go)
    gv1, gr1 = ops.msda_rows_backward(v4, rows, ref_pts, shapes, starts, P, go)
    assert gv1.stride(1) == 288 and torch.equal(gr0, gr1)
    assert (gv1 - gv0).abs().max().item() <= 1e-5 * gv0.abs().max().item()
    assert bool((buf[..., 256:] == 7.0).all())                                # the pad columns of the value rows were only ever read past


def test_msda_mmcv_function_reads_the_level_table_once_per_tensor(dev):
    """`ops.MultiScaleDeformableAttnFunction` (mmcv's positional signature): the DEVICE level table is read by
    `cgg_msda_read_levels` once per `spatial_shapes` tensor -- the result rides on the tensor with both version counters -- and the
    op itself runs the non-synchronising *_hostlevels entries, forward and backward (== the mmcv-contract entries' results); an
    in-place change of the table invalidates the cached copy; `cgg_init` is idempotent; the two-pass backward reports a workspace
    size only for a tileable pyramid."""
    from cgg_amd import _lib
    lib = _lib.load()
    assert lib.cgg_init(0) == 0 and lib.cgg_init(0) == 0 and lib.cgg_init(99) < 0
    shapes = [(8, 8), (16, 16), (32, 32)]
    value, ss, st, loc, aw = _msda_inputs(2, shapes, 8, 32, 4, 1344, seed=7)
    ssd, std_ = ss.to(dev), st.to(dev)
    calls = []

    class Spy:
        def __getattr__(self, name):
            f = getattr(_lib.load(), name)
            if name == 'cgg_msda_read_levels':
                def g(*a):
                    calls.append(1)
                    return f(*a)
                return g
            return f
    old = ops._lib_
    ops._lib_ = lambda: Spy()
    try:
        v = value.to(dev).requires_grad_(True)
        l, a = loc.to(dev).requires_grad_(True), aw.to(dev).requires_grad_(True)
        out = ops.MultiScaleDeformableAttnFunction.apply(v, ssd, std_, l, a, 64)
        out2 = ops.MultiScaleDeformableAttnFunction.apply(v, ssd, std_, l, a, 64)            # the same tensor: no second read
        assert len(calls) == 1 and torch.equal(out, out2)
        go = torch.randn_like(out)
        out.backward(go)
        assert len(calls) == 1
        ssd.add_(0)                                                                            # in-place write: version bump
        ops.MultiScaleDeformableAttnFunction.apply(v, ssd, std_, l, a, 64)
        assert len(calls) == 2
    finally:
        ops._lib_ = old
    want = ops.msda_forward(value.to(dev), ssd, std_, loc.to(dev), aw.to(dev))
    assert torch.equal(out.detach(), want)
    gv, gl, ga = ops.msda_backward(value.to(dev), ssd, std_, loc.to(dev), aw.to(dev), go)
    sc = gv.abs().max().item()
    assert (v.grad - gv).abs().max().item() <= 1e-5 * sc                                       # (atomics: summation order only)
    assert (l.grad - gl).abs().max().item() <= 1e-5 * gl.abs().max().item() and (a.grad - ga).abs().max().item() <= 1e-5 * ga.abs().max().item()
    hw = ops._int_array([x for pair in shapes for x in pair])
    stt = ops._int_array(_levels(shapes)[0])
    assert lib.cgg_msda_backward_workspace_bytes(hw, stt, 2, 1344, 8, 32, 3, 1344, 4) > 0
    assert lib.cgg_msda_backward_workspace_bytes(hw, stt, 2, 1344, 8, 32, 3, 700, 4) == 0       # queries != pixels: no sorted scatter
    assert lib.cgg_msda_backward_workspace_bytes(hw, stt, 2, 1344, 8, 16, 3, 1344, 4) == 0      # D != 32


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,Q,H,W', [(2, 100, 32, 32), (1, 100, 20, 28), (2, 37, 16, 24), (1, 128, 64, 64)])
def test_mask_logits_split_within_1e3(dev, B, Q, H, W):
    check_mask_logits_split(dev, B, Q, H, W)


def check_mask_logits_split(dev, B, Q, H, W):
    g = torch.Generator().manual_seed(10)
    embed = torch.randn(B, Q, 256, generator=g)
    feat = torch.randn(B, 256, H, W, generator=g)
    want = ref.mask_logits(embed.double(), feat.double())
    packed = ops.pack_mask_feature(feat.to(dev), pool=1, split=True)
    got, _ = ops.mask_logits(embed.to(dev), packed, want_logits=True)
    err = (got.cpu().double() - want).abs().max().item()
    assert err <= 1e-3, err  # north_star: mask logits within 1e-3 (values are O(16) here)


@pytest.mark.parametrize('B,Q,H,W', [(2, 100, 64, 64), (1, 200, 64, 96), (2, 37, 20, 28), (1, 128, 16, 24), (1, 256, 40, 33), (3, 160, 100, 97),
                                     (2, 200, 256, 256), (1, 129, 8, 8)])
def test_mask_logits_bits_astat_equals_streamed_kernel(dev, B, Q, H, W):
    """cgg_mask_logits_bits_astat (query tiles stationary in registers, threshold consumer in the epilogue, logits never stored)
    gives exactly the bits of cgg_mask_logits' bf16 mode (same bf16 operands, same MFMA order) -- one / two query-tile groups,
    ragged last tile, rows that are not a multiple of 32 -- and those are `bf16-operand logit < 0`."""
    g = torch.Generator().manual_seed(12 + Q)
    embed = torch.randn(B, Q, 256, generator=g)
    feat = torch.randn(B, 256, H, W, generator=g)
    packed = ops.pack_mask_feature(feat.to(dev), pool=1, split=False)
    logits, want = ops.mask_logits(embed.to(dev), packed, want_logits=True, want_bits=True)
    got = ops.mask_logits_bits_astat(embed.to(dev), packed)
    assert torch.equal(got, want)
    assert torch.equal(ops.unpack_bits(got, H * W).view(B, Q, H, W), logits < 0)


@pytest.mark.parametrize('rows,N,k', [(184, 37632, 9408), (3, 1000, 1), (5, 777, 777), (2, 4096, 1000), (1, 70, 33)])
def test_topk_select_is_the_topk_set(dev, rows, N, k):
    """cgg_topk_select (radix select, no order) vs torch.topk: the same SET of indices per row when the k-th value is unique, the
    same multiset of VALUES with ties (a quantised row: many equal keys at the threshold), negative / positive / zero values."""
    g = torch.Generator().manual_seed(rows + N)
    x = -torch.randn(rows, N, generator=g).abs()                    # the uncertainty's sign convention: -|logit|
    x[0, : min(N, 50)] = 0.0                                          # exact zeros (the largest values) -- ties above the threshold
    xd = x.to(dev)
    got = ops.topk_select(xd, k)
    assert got.shape == (rows, k) and got.dtype == torch.int64
    want = torch.topk(xd, k, dim=1)[1]
    for r in range(rows):
        assert len(set(got[r].tolist())) == k                       # k distinct indices
    assert torch.equal(torch.sort(xd.gather(1, got), 1)[0], torch.sort(xd.gather(1, want), 1)[0])
    q = (torch.randn(rows, N, generator=g) * 4).round().to(dev)      # heavy ties, both signs
    gq = ops.topk_select(q, k)
    assert torch.equal(torch.sort(q.gather(1, gq), 1)[0], torch.sort(q.gather(1, torch.topk(q, k, dim=1)[1]), 1)[0])
    wide = torch.randn(rows, N + 8, generator=g).to(dev)[:, 3:3 + N] if N + 8 > 11 else None      # strided rows
    if wide is not None and wide.stride(1) == 1:
        gw = ops.topk_select(wide, k)
        assert torch.equal(torch.sort(wide.gather(1, gw), 1)[0], torch.sort(wide.gather(1, torch.topk(wide, k, dim=1)[1]), 1)[0])


def test_mask_logits_bf16_mode(dev):
    g = torch.Generator().manual_seed(11)
    B, Q, H, W = 2, 100, 32, 48
    embed = torch.randn(B, Q, 256, generator=g)
    feat = torch.randn(B, 256, H, W, generator=g)
    packed = ops.pack_mask_feature(feat.to(dev), pool=1, split=False)
    got, _ = ops.mask_logits(embed.to(dev), packed, want_logits=True)
    # exact oracle of the bf16 path: bf16-rounded operands, exact products, f32-class accumulation
    want = ref.mask_logits(embed.bfloat16().double(), feat.bfloat16().double())
    assert (got.cpu().double() - want).abs().max().item() <= 2e-4
    # and against the unrounded reference: 2^-8 relative per operand
    full = ref.mask_logits(embed.double(), feat.double())
    bound = torch.einsum('bqc,bchw->bqhw', embed.abs().double(), feat.abs().double()) * 2 ** -7
    assert ((got.cpu().double() - full).abs() <= bound).all()


def test_mask_logits_transpose_detecting(dev):
    """A = 'identity-like' embed with an ASYMMETRIC feature: catches row/col swaps of the MFMA C layout."""
    B, Q, H, W = 1, 100, 8, 16
    embed = torch.zeros(B, Q, 256)
    for q in range(Q):
        embed[0, q, q] = 1.0
    feat = torch.arange(256 * H * W, dtype=torch.float32).view(1, 256, H, W) % 251
    packed = ops.pack_mask_feature(feat.to(dev), pool=1, split=True)
    got, _ = ops.mask_logits(embed.to(dev), packed)
    assert torch.equal(got.cpu(), feat[:, :Q])


@pytest.mark.parametrize('pool', [2, 4, 8])
def test_attn_mask_bits_vs_reference_rule(dev, pool):
    """bits from the pooled-feature GEMM == (sigmoid(interpolate(mask_pred)) < 0.5) of the reference,
    except where the oracle's own resized logit is within 1e-4 of 0 (numerical ties)."""
    g = torch.Generator().manual_seed(12)
    B, Q, H, W = 2, 100, 64, 96
    embed = torch.randn(B, Q, 256, generator=g)
    feat = torch.randn(B, 256, H, W, generator=g)
    size = (H // pool, W // pool)
    mp = ref.mask_logits(embed, feat)
    want = ref.attn_mask_from_logits(mp, size)
    margin = ref.attn_mask_logits(mp, size).abs() > 1e-4
    packed = ops.pack_mask_feature(feat.to(dev), pool=pool, split=True)
    _, bits = ops.mask_logits(embed.to(dev), packed, want_logits=False, want_bits=True)
    got = ops.unpack_bits(bits, size[0] * size[1]).cpu()
    assert got.shape == want.shape
    assert torch.equal(got[margin], want[margin])
    assert margin.float().mean().item() > 0.999
    # generic path (stored logits -> resize -> bits) gives the same answer
    full, _ = ops.mask_logits(embed.to(dev), ops.pack_mask_feature(feat.to(dev), 1, True))
    bits2 = ops.attn_mask_from_logits(full, size)
    got2 = ops.unpack_bits(bits2, size[0] * size[1]).cpu()
    assert torch.equal(got2[margin], want[margin])


def test_fix_full_rows(dev):
    g = torch.Generator().manual_seed(13)
    npix = 20 * 28  # not a multiple of 32
    mask = torch.rand(3, 50, npix, generator=g) < 0.5
    mask[0, 3] = True
    mask[2, 49] = True
    mask[1, 7] = False
    words = (npix + 31) // 32
    padded = torch.zeros(3, 50, words * 32, dtype=torch.bool)
    padded[..., :npix] = mask
    w = (padded.view(3, 50, words, 32).long() << torch.arange(32)).sum(-1)
    bits = w.to(torch.int64).where(w < 2 ** 31, w - 2 ** 32).to(torch.int32)
    out = ops.attn_mask_fix_full_rows(bits.to(dev), npix)
    got = ops.unpack_bits(out, npix).cpu()
    want = ref.fix_full_rows(mask.clone())
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,Q,S', [(2, 100, 1024), (1, 100, 1050), (2, 37, 200), (1, 128, 4096)])
def test_masked_xattn_vs_oracle(dev, B, Q, S):
    g = torch.Generator().manual_seed(20)
    E, H = 256, 8
    q = torch.randn(B, Q, E, generator=g)
    k = torch.randn(B, S, E, generator=g)
    v = torch.randn(B, S, E, generator=g)
    mask = torch.rand(B, Q, S, generator=g) < 0.6
    mask[0, 1] = False                      # un-masked row
    mask[0, 2] = True
    mask[0, 2, S - 1] = False               # single visible key (the last one)
    want = ref.masked_attention_core(q, k, v, mask, H)
    words = (S + 31) // 32
    padded = torch.zeros(B, Q, words * 32, dtype=torch.bool)
    padded[..., :S] = mask
    w = (padded.view(B, Q, words, 32).long() << torch.arange(32)).sum(-1)
    bits = w.where(w < 2 ** 31, w - 2 ** 32).to(torch.int32)
    kv = torch.cat([k, v], -1).contiguous()
    got = ops.masked_xattn(q.to(dev), kv.to(dev), bits.to(dev), H).cpu()
    assert (got - want).abs().max().item() <= 1e-4
    got_nomask = ops.masked_xattn(q.to(dev), kv.to(dev), None, H).cpu()
    want_nomask = ref.masked_attention_core(q, k, v, None, H)
    assert (got_nomask - want_nomask).abs().max().item() <= 1e-4


def test_masked_xattn_spiked_key(dev):
    """forces the online-softmax rescale branch: one key dominates late in the stream."""
    g = torch.Generator().manual_seed(21)
    B, Q, S, E, H = 1, 64, 2048, 256, 8
    q = torch.randn(B, Q, E, generator=g)
    k = torch.randn(B, S, E, generator=g)
    v = torch.randn(B, S, E, generator=g)
    k[0, 1777] = q[0, 5] * 4.0
    want = ref.masked_attention_core(q.double(), k.double(), v.double(), None, H).float()
    got = ops.masked_xattn(q.to(dev), torch.cat([k, v], -1).to(dev), None, H).cpu()
    assert (got - want).abs().max().item() <= 1e-4


def test_masked_xattn_full_row_is_nan_like_reference(dev):
    B, Q, S, E, H = 1, 4, 64, 256, 8
    g = torch.Generator().manual_seed(22)
    q, k, v = (torch.randn(B, n, E, generator=g) for n in (Q, S, S))
    bits = torch.zeros(B, Q, 2, dtype=torch.int32)
    bits[0, 1] = -1  # all 64 keys blocked
    got = ops.masked_xattn(q.to(dev), torch.cat([k, v], -1).to(dev), bits.to(dev), H).cpu()
    assert torch.isnan(got[0, 1]).all() and not torch.isnan(got[0, 0]).any()


@pytest.mark.parametrize('form', ['x3', 'f32'])
@pytest.mark.parametrize('B,Q,S,H,masked', [(2, 100, 1050, 8, True), (1, 20, 77, 4, True), (2, 100, 100, 8, False),
                                            (3, 128, 4096, 8, True), (1, 33, 16384, 8, True)])
def test_masked_xattn_backward_vs_float64_autograd(dev, B, Q, S, H, masked, form, monkeypatch):
    """cgg_masked_xattn_forward_lse + cgg_masked_xattn_backward against float64 autograd of the reference formulation
    (scores -> masked_fill(-inf) -> softmax -> @ v, the arithmetic of nn.MultiheadAttention at
    mask2former_head.py:829-840): ragged key counts (1050 = the 25 x 42 level of configs[4], 77), fewer queries than one
    tile, the unmasked self-attention case, several key chunks per head, rows with a single visible key. Both forms of the backward:
    `x3` = the f16 x 3 contraction parity mode takes (cgg_masked_xattn_backward_x3; also with a 1e-6-scale grad_out: its pre-scale comes
    from max |grad_out|), `f32` = the exact f32 MFMA (CGG_XATTN_X3_BWD=0) -- the same bound for both."""
    monkeypatch.setattr(ops, 'XATTN_X3_BWD', form == 'x3')
    q, kv, bits, out, lse, go, gq, gkv = check_masked_xattn_backward(dev, B, Q, S, H, masked)
    # run to run bit-identical (no floating-point atomics)
    gq2, gkv2 = ops.masked_xattn_backward(q, kv, bits, out, lse, go, H)
    assert torch.equal(gq, gq2) and torch.equal(gkv, gkv2)
    # a gradient-scale grad_out (what the training step hands over): the backward is linear in it, to the last bit for a power of two
    gq3, gkv3 = ops.masked_xattn_backward(q, kv, bits, out, lse, go * 2.0**-20, H)
    assert torch.equal(gq3 * 2.0**20, gq) and torch.equal(gkv3 * 2.0**20, gkv)


def check_masked_xattn_backward(dev, B, Q, S, H, masked):
    """forward with lse + backward on `dev` within the bounds of test_masked_xattn_backward_vs_float64_autograd; returns the device
    tensors (q, kv, bits, out, lse, grad_out, grad_q, grad_kv)"""
    from cgg_amd.query_decoder import pack_bool_mask
    g = torch.Generator().manual_seed(23 + S)
    D = 32
    E = H * D
    q = torch.randn(B, Q, E, generator=g)
    kv = torch.randn(B, S, 2 * E, generator=g)
    go = torch.randn(B, Q, E, generator=g)
    mask = None
    if masked:
        mask = torch.rand(B, Q, S, generator=g) < 0.6
        mask[0, 1] = False                      # un-masked row
        mask[0, 2] = True
        mask[0, 2, S - 1] = False               # single visible key (the last one)
    qd = q.double().requires_grad_(True)
    kvd = kv.double().requires_grad_(True)
    qh = (qd * D**-0.5).view(B, Q, H, D).transpose(1, 2)
    kh = kvd[..., :E].view(B, S, H, D).transpose(1, 2)
    vh = kvd[..., E:].view(B, S, H, D).transpose(1, 2)
    att = qh @ kh.transpose(-1, -2)
    if mask is not None:
        att = att.masked_fill(mask[:, None], float('-inf'))
    want_lse = torch.logsumexp(att, -1)
    want = (att.softmax(-1) @ vh).transpose(1, 2).reshape(B, Q, E)
    wgq, wgkv = torch.autograd.grad(want, (qd, kvd), go.double())
    bits = None if mask is None else pack_bool_mask(mask).contiguous().to(dev)
    out, lse = ops.masked_xattn(q.to(dev), kv.to(dev), bits, H, return_lse=True)
    assert (out.cpu() - want.detach().float()).abs().max().item() <= 1e-4
    assert (lse.cpu() - want_lse.detach().float()).abs().max().item() <= 1e-4
    gq, gkv = ops.masked_xattn_backward(q.to(dev), kv.to(dev), bits, out, lse, go.to(dev), H)
    for got, ref_, name in ((gq, wgq, 'grad_q'), (gkv, wgkv, 'grad_kv')):
        scale = ref_.abs().max().item()
        err = (got.cpu().double() - ref_).abs().max().item()
        assert err <= 2e-5 * scale + 1e-6, (name, err, scale)
    return q.to(dev), kv.to(dev), bits, out, lse, go.to(dev), gq, gkv


def test_xattn_autograd_function_uses_hip_backward(dev):
    """`_XAttnFn` (what the decoder layers call in training): gradients equal the torch formulation, incl. Q > 128."""
    from cgg_amd.query_decoder import _XAttnFn, pack_bool_mask, xattn_backward_torch
    g = torch.Generator().manual_seed(29)
    B, Q, S, H, E = 2, 200, 333, 8, 256
    q = torch.randn(B, Q, E, generator=g).to(dev).requires_grad_(True)
    kv = torch.randn(B, S, 2 * E, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(B, Q, E, generator=g).to(dev)
    bits = pack_bool_mask(torch.rand(B, Q, S, generator=g) < 0.5).contiguous().to(dev)
    out = _XAttnFn.apply(q, kv, bits, H)
    gq, gkv = torch.autograd.grad(out, (q, kv), go)
    wq, wkv = xattn_backward_torch(q.detach(), kv.detach(), bits, go, H)
    assert (gq - wq).abs().max().item() <= 1e-4 * wq.abs().max().item()
    assert (gkv - wkv).abs().max().item() <= 1e-4 * wkv.abs().max().item()


@pytest.mark.parametrize('B,Q,T,d', [(16, 100, 35, 768), (4, 100, 35, 768), (2, 20, 35, 768), (3, 128, 64, 64), (1, 7, 5, 8),
                                     (4, 200, 35, 768), (2, 256, 64, 64), (2, 129, 33, 16)])
def test_grounding_loss_kernel_vs_oracle(dev, B, Q, T, d):
    """`losses.grounding_loss` on the HIP pair-cost kernel (cgg_grounding_pair_costs + backward) against the oracle's
    literal restatement of grounding_loss.py:9-77 (with the B^2 repeat; pinned by golden G1) in float64: loss value and
    the gradient w.r.t. the predicted embeddings. Includes a caption without nouns (the +100 branch), ragged token counts
    and the global-batch size of configs[2] (B_g = 16)."""
    from cgg_amd import losses
    from oracle import head as OH
    g = torch.Generator().manual_seed(60 + B)
    pred = (torch.randn(B, Q, d, generator=g) * 0.5)
    cap = torch.randn(B, T, d, generator=g)
    ntok = torch.randint(1, min(T, 7) + 1, (B,), generator=g)
    if B > 1:
        ntok[1] = 0                                          # caption without nouns
    mask = (torch.arange(T)[None] < ntok[:, None]).long()
    pd = pred.double().requires_grad_(True)
    want = OH.grounding_loss(pd, cap.double(), mask, 10.0)
    wg, = torch.autograd.grad(want, pd)
    pg = pred.to(dev).requires_grad_(True)
    got = losses.grounding_loss(pg, cap.to(dev), mask.to(dev), 10.0)
    gg, = torch.autograd.grad(got, pg)
    assert abs(float(got) - float(want)) <= 1e-5 * (1 + abs(float(want))), (float(got), float(want))
    scale = wg.abs().max().item()
    assert (gg.cpu().double() - wg).abs().max().item() <= 1e-4 * scale + 1e-9, ((gg.cpu().double() - wg).abs().max().item(), scale)
    # the pair costs themselves against the torch formulation (same arithmetic, (B, B, T, Q) tensors materialised)
    cost = ops.grounding_pair_costs(pred.to(dev), cap.to(dev), mask.to(torch.int32).to(dev), 0.1).cpu()
    sim = torch.einsum('itd,jqd->ijtq', cap.double(), pred.double()) / 10.0
    l2v = ((sim.softmax(3) * mask[:, None, :, None]) * -sim).sum((2, 3)) / ntok.clamp(min=1)[:, None]
    v2l = (sim.softmax(2) * -sim).sum((2, 3)) / Q
    assert (cost[0].double() - l2v).abs().max().item() <= 1e-5 * (1 + l2v.abs().max().item())
    assert (cost[1].double() - v2l).abs().max().item() <= 1e-5 * (1 + v2l.abs().max().item())


# ------------------------------------------------------------------------------------------------
def test_upsample_bilinear(dev):
    g = torch.Generator().manual_seed(30)
    x = torch.randn(3, 5, 20, 28, generator=g)
    for size in [(80, 112), (50, 97), (20, 28), (13, 9)]:
        want = torch.nn.functional.interpolate(x, size, mode='bilinear', align_corners=False)
        got = ops.upsample_bilinear(x.to(dev), size).cpu()
        assert (got - want).abs().max().item() <= 1e-5


def test_rowwise_softmax_argmax(dev):
    g = torch.Generator().manual_seed(31)
    x = torch.randn(100, 66, generator=g) * 5
    x[3, 10] = x[3, 40] = 30.0  # tie: first index wins (torch.max semantics)
    prob, maxv, arg = ops.rowwise_softmax_argmax(x.to(dev))
    want = x.softmax(-1)
    wmax, warg = want.max(-1)
    assert (prob.cpu() - want).abs().max().item() <= 1e-6
    assert torch.equal(arg.cpu(), warg)
    assert (maxv.cpu() - wmax).abs().max().item() <= 1e-6


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,K,N', [(200, 256, 256), (200, 256, 2048), (200, 2048, 256), (37, 256, 50), (300, 768, 768)])
def test_linear_rows(dev, M, K, N):
    g = torch.Generator().manual_seed(40)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K**0.5
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    want = torch.relu(x.double() @ w.double().t() + b.double()) + r.double()
    got = ops.linear_rows(x.to(dev), w.to(dev), b.to(dev), relu=True, res=r.to(dev), split=True).cpu()
    assert (got.double() - want).abs().max().item() <= 1e-4     # f32-class (3x bf16 MFMA on split operands)
    got16 = ops.linear_rows(x.to(dev), w.to(dev), b.to(dev), relu=False, res=None, split=False).cpu()
    want16 = x.bfloat16().double() @ w.bfloat16().double().t() + b.double()
    assert (got16.double() - want16).abs().max().item() <= 1e-3
    # strided output view (writes one half of a wider buffer)
    buf = torch.zeros(M, 2 * N, device=dev)
    ops.linear_rows(x.to(dev), w.to(dev), b.to(dev), split=True, out=buf[:, N:])
    assert (buf[:, N:].cpu().double() - (x.double() @ w.double().t() + b.double())).abs().max().item() <= 1e-4
    assert buf[:, :N].abs().max().item() == 0


def test_add_layernorm(dev):
    g = torch.Generator().manual_seed(41)
    a = torch.randn(2, 100, 256, generator=g)
    b = torch.randn(2, 100, 256, generator=g)
    ln = torch.nn.LayerNorm(256)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(256, generator=g))
        ln.bias.copy_(torch.randn(256, generator=g))
        want = ln(a + b)
        want1 = ln(a)
    got = ops.add_layernorm(a.to(dev), b.to(dev), ln.weight.to(dev), ln.bias.to(dev), ln.eps).cpu()
    got1 = ops.add_layernorm(a.to(dev), None, ln.weight.to(dev), ln.bias.to(dev), ln.eps).cpu()
    assert (got - want).abs().max().item() <= 1e-5
    assert (got1 - want1).abs().max().item() <= 1e-5


@pytest.mark.parametrize('shape,relu', [((2, 256, 64, 64), False), ((1, 64, 20, 28), True), ((2, 256, 8, 8), False), ((1, 64, 5, 7), True)])
def test_group_norm(dev, shape, relu):
    g = torch.Generator().manual_seed(42)
    x = torch.randn(shape, generator=g) * 3 + 1
    gn = torch.nn.GroupNorm(32, shape[1])
    with torch.no_grad():
        gn.weight.copy_(torch.randn(shape[1], generator=g))
        gn.bias.copy_(torch.randn(shape[1], generator=g))
        want = gn(x)
        if relu:
            want = want.relu()
    got = ops.group_norm(x.to(dev), gn.weight.to(dev), gn.bias.to(dev), 32, gn.eps, relu).cpu()
    assert (got - want).abs().max().item() <= 2e-5


@pytest.mark.parametrize('H,W,S,crop', [(32, 48, 4, None), (16, 16, 8, (120, 112)), (40, 24, 2, None), (25, 42, 4, (97, 160))])
def test_instance_masks_integer_fast_path_matches_torch(dev, H, W, S, crop):
    """fused upsample -> (>0) -> mask score -> bbox vs the reference formulation (F.interpolate + torch ops)."""
    from oracle import head as OH
    g = torch.Generator().manual_seed(43)
    Q = 12
    logits = torch.randn(Q, H, W, generator=g) * 3
    up = (H * S, W * S)
    crop = crop or up
    sel = torch.tensor([3, 0, 7, 7, 11, 2], dtype=torch.int32)
    masks, score, bbox = ops.instance_masks(logits.to(dev), sel.to(dev), up, crop, crop)
    ref_up = torch.nn.functional.interpolate(logits[None], up, mode='bilinear', align_corners=False)[0]
    ref_up = ref_up[:, :crop[0], :crop[1]][sel.long()]
    wbin = ref_up > 0
    near = ref_up.abs() < 1e-5
    assert torch.equal(masks.cpu()[~near], wbin[~near])
    wscore = (ref_up.sigmoid() * wbin).flatten(1).sum(1) / (wbin.flatten(1).sum(1) + 1e-6)
    assert (score.cpu() - wscore).abs().max().item() <= 1e-5
    if not near.any():
        assert torch.equal(bbox.cpu(), OH.mask2bbox(wbin))


def test_add_layernorm_stream_and_bf16_msda(dev):
    g = torch.Generator().manual_seed(44)
    a = torch.randn(2, 300, 256, generator=g)
    b = torch.randn(2, 300, 256, generator=g)
    pos = torch.randn(300, 256, generator=g)
    ln = torch.nn.LayerNorm(256)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(256, generator=g))
        ln.bias.copy_(torch.randn(256, generator=g))
        want = ln(a + b.bfloat16().float())
    y32, y16, yp16 = ops.add_layernorm_stream(a.to(dev), b.to(dev).bfloat16(), ln.weight.to(dev), ln.bias.to(dev),
                                              ln.eps, pos=pos.to(dev), want_pos=True)
    assert (y32.cpu() - want).abs().max().item() <= 1e-5
    assert torch.equal(y16.cpu(), y32.cpu().bfloat16())
    assert torch.equal(yp16.cpu(), (y32.cpu() + pos[None]).bfloat16())
    y32b, _, _ = ops.add_layernorm_stream(a.to(dev), b.to(dev), ln.weight.to(dev), ln.bias.to(dev), ln.eps,
                                          want_bf16=False)
    with torch.no_grad():
        assert (y32b.cpu() - ln(a + b)).abs().max().item() <= 1e-5
    # bf16 stream variant of the fused MSDeformAttn kernel == f32-output kernel on the same bf16 inputs, rounded
    shapes = [(8, 8), (16, 16), (32, 32)]
    starts, Nv = _levels(shapes)
    B, H, D, P = 2, 8, 32, 4
    value = torch.randn(B, Nv, H, D, generator=g).bfloat16()
    raw = torch.randn(B, Nv, 288, generator=g)
    raw[..., :192] *= 2
    raw = raw.bfloat16()
    refp = torch.rand(Nv, 2, generator=g)
    ref32 = ops.msda_forward_fused(value.to(dev), shapes, starts, raw.float().to(dev), refp.to(dev), P)
    got = ops.msda_forward_fused_bf16(value.to(dev), shapes, starts, raw.to(dev), refp.to(dev), P)
    assert got.dtype == torch.bfloat16
    # the quad-shared-tap kernel folds w_point * w_corner before the channel loop: the f32 sums agree to rounding, the
    # bf16 outputs to one ulp (round-2 A/B measurement: 0.01 % of the elements differ, never by more than one ulp)
    want = ref32.cpu().bfloat16().float()
    d = (got.cpu().float() - want).abs()
    assert bool((d <= want.abs().clamp(min=1e-3) * 2.0 ** -7).all()), float(d.max())
    assert float((d > 0).float().mean()) <= 1e-3


def test_bias_act_nhwc_and_folded_backbone(dev):
    from cgg_amd import registry, runtime
    g = torch.Generator().manual_seed(45)
    y = torch.randn(2, 9, 7, 64, generator=g).bfloat16()
    b = torch.randn(64, generator=g).bfloat16()
    r = torch.randn(2, 9, 7, 64, generator=g).bfloat16()
    for bias, res, relu in [(b, r, True), (b, None, True), (None, r, True), (b, r, False), (None, None, True)]:
        want = y.clone()
        if bias is not None:
            want = want + bias
        if res is not None:
            want = want + res
        if relu:
            want = want.relu()
        got = ops.bias_act_nhwc_(y.clone().to(dev), None if bias is None else bias.to(dev),
                                 None if res is None else res.to(dev), relu)
        assert torch.equal(got.cpu(), want), (bias is not None, res is not None, relu)
    # throughput-mode ResNet (BN folded, 1x1 convs as GEMMs, fused epilogues) tracks the f32 module
    for depth in (50, 18):
        torch.manual_seed(3)
        bb = registry.build_backbone(dict(type='ResNet', depth=depth, num_stages=4, out_indices=(0, 1, 2, 3),
                                          frozen_stages=-1, norm_cfg=dict(type='BN', requires_grad=False),
                                          norm_eval=True, style='pytorch'))
        for m in bb.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.data.uniform_(0.5, 1.5)
                m.bias.data.normal_(0, 0.1)
        bb = bb.to(dev).eval()
        x = torch.randn(2, 3, 96, 128, generator=g).to(dev)
        with torch.no_grad():
            want = [plain(f) for f in bb(x)]             # parity mode hands over x3a rows (round 4): their values
            with runtime.precision_scope('bf16'):
                got = bb(x)
        for w, o in zip(want, got):
            # throughput mode hands over (B, C, H, W)-shaped views of channel-last bf16 activations
            assert o.shape == w.shape and o.dtype == torch.bfloat16 and o.permute(0, 2, 3, 1).is_contiguous()
            o = o.float()
            scale = w.abs().max().item()
            assert (o - w).abs().max().item() <= 0.06 * scale
            assert (o - w).abs().mean().item() <= 0.01 * scale


def test_group_norm_nhwc_and_pack_nhwc(dev):
    g = torch.Generator().manual_seed(46)
    B, H, W, C = 2, 12, 20, 256
    x = (torch.randn(B, H * W, C, generator=g) * 2 + 0.3).bfloat16()
    gn = torch.nn.GroupNorm(32, C)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(C, generator=g))
        gn.bias.copy_(torch.randn(C, generator=g))
    lo = torch.randn(B, H // 2, W // 2, C, generator=g)
    pos = torch.randn(H * W, C, generator=g)
    with torch.no_grad():
        base = gn(x.float().view(B, H, W, C).permute(0, 3, 1, 2))                       # NCHW
        up = torch.nn.functional.interpolate(lo.permute(0, 3, 1, 2), size=(H, W), mode='bilinear',
                                             align_corners=False)
    ws = ops.group_norm_nhwc_workspace(B, H * W, 32, dev)
    # (a) plain GN -> f32 into a strided (B, N, C) stream at a row offset, bf16 copy, bf16(y + pos)
    N, row0 = H * W + 37, 21
    y32 = torch.zeros(B, N, C, device=dev)
    y16 = torch.zeros(B, N, C, device=dev, dtype=torch.bfloat16)
    yp16 = torch.zeros(B, N, C, device=dev, dtype=torch.bfloat16)
    ops.group_norm_nhwc(x.to(dev), gn.weight.to(dev), gn.bias.to(dev), 32, gn.eps, ws,
                        out32=(y32, row0 * C, N * C), out16=(y16, row0 * C, N * C), pos=(pos.to(dev), 0),
                        outp16=(yp16, row0 * C, N * C))
    want = base.permute(0, 2, 3, 1).reshape(B, H * W, C)
    got = y32[:, row0:row0 + H * W].cpu()
    assert (got - want).abs().max().item() <= 2e-4
    assert y32[:, :row0].abs().sum().item() == 0 and y32[:, row0 + H * W:].abs().sum().item() == 0
    assert torch.equal(y16[:, row0:row0 + H * W].cpu(), got.bfloat16())
    assert torch.equal(yp16[:, row0:row0 + H * W].cpu(), (got + pos[None]).bfloat16())
    # (b) GN + up-sample-add + ReLU -> bf16
    z = torch.empty(B, H * W, C, device=dev, dtype=torch.bfloat16)
    ops.group_norm_nhwc(x.to(dev), gn.weight.to(dev), gn.bias.to(dev), 32, gn.eps, ws, relu=True,
                        up=(lo.to(dev), 0, (H // 2) * (W // 2) * C, H // 2, W // 2), W=W, out16=(z, 0, H * W * C))
    want = (base + up).relu().permute(0, 2, 3, 1).reshape(B, H * W, C)
    assert (z.cpu().float() - want).abs().max().item() <= 0.02 * want.abs().max().item()
    assert (z.cpu().float() - want).abs().mean().item() <= 2e-3 * want.abs().max().item()
    # (c) channel-last pack == NCHW pack of the same values
    f = torch.randn(B, 16, 24, C, generator=g).bfloat16()
    for pool in (1, 2, 4, 8):
        a = ops.pack_mask_feature_nhwc(f.to(dev), pool)
        b = ops.pack_mask_feature(f.float().permute(0, 3, 1, 2).contiguous().to(dev), pool, split=False)
        assert (a.h, a.w, a.npix) == (b.h, b.w, b.npix)
        assert torch.equal(a.hi.cpu().view(torch.int16), b.hi.cpu().view(torch.int16)), pool


@pytest.mark.parametrize('M,N,K', [(200, 256, 256), (37, 49, 256), (200, 2048, 256), (130, 1073, 256), (200, 256, 2048)])
def test_linear_rows_bf16_variants(dev, M, N, K):
    g = torch.Generator().manual_seed(47)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K**0.5
    b = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    packed = ops.pack_linear_weight(w.to(dev))
    xb, wb = x.bfloat16().double(), w.bfloat16().double()       # the kernel's operands, exact products
    base = (xb @ wb.t() + b.double())
    tol = 2e-3 * (1 + base.abs().max().item())
    # plain + ReLU on the first 32 columns + residual
    y = ops.linear_rows_bf16(x.to(dev), packed, N, b.to(dev), res=res.to(dev), relu_cols=32)
    want = base.clone()
    want[:, :32] = want[:, :32].relu()
    want = want + res.double()
    assert (y.cpu().double() - want).abs().max().item() <= tol
    # strided input / output views
    xs = torch.zeros(M, K + 8, device=dev)[:, :K]
    xs.copy_(x)
    out = torch.zeros(M, N + 5, device=dev)[:, :N] if (N + 5) % 1 == 0 else None
    ops.linear_rows_bf16(xs, packed, N, b.to(dev), out=out)
    assert (out.cpu().double() - base).abs().max().item() <= tol
    # split-K
    if K >= 512:
        planes = ops.linear_rows_bf16(x.to(dev), packed, N, b.to(dev), res=res.to(dev), ksplit=8)
        assert planes.shape == (8, M, N)
        assert (planes.sum(0).cpu().double() - (base + res.double())).abs().max().item() <= tol
        again = ops.linear_rows_bf16(x.to(dev), packed, N, b.to(dev), res=res.to(dev), ksplit=8)
        assert torch.equal(planes, again)                       # no atomics: bit-reproducible
        if N % 4 == 0 and N <= 1024:
            ln2 = torch.nn.LayerNorm(N)
            yy, _, _ = ops.layernorm_chain(planes, (ln2.weight.to(dev), ln2.bias.to(dev), ln2.eps))
            with torch.no_grad():
                assert (yy.cpu() - ln2(planes.sum(0).cpu())).abs().max().item() <= 1e-4
    # fused LayerNorm + `y + pos`
    if N <= 256:
        ln = torch.nn.LayerNorm(N)
        with torch.no_grad():
            ln.weight.copy_(torch.randn(N, generator=g))
            ln.bias.copy_(torch.randn(N, generator=g))
        pos = torch.randn(7, N, generator=g)
        y, yp = ops.linear_rows_bf16(x.to(dev), packed, N, b.to(dev), res=res.to(dev),
                                     ln=(ln.weight.to(dev), ln.bias.to(dev), ln.eps), pos=pos.to(dev), want_pos=True)
        with torch.no_grad():
            want = ln((base + res.double()).float())
        assert (y.cpu() - want).abs().max().item() <= 5e-3
        assert torch.equal(yp.cpu(), y.cpu() + pos[torch.arange(M) % 7])


def test_layernorm_chain(dev):
    g = torch.Generator().manual_seed(48)
    a = torch.randn(201, 264, generator=g)[:, :256]
    la, lb = torch.nn.LayerNorm(256), torch.nn.LayerNorm(256)
    with torch.no_grad():
        for m in (la, lb):
            m.weight.copy_(torch.randn(256, generator=g))
            m.bias.copy_(torch.randn(256, generator=g))
    pos = torch.randn(67, 256, generator=g)
    ad = torch.zeros(201, 264, device=dev)[:, :256]
    ad.copy_(a)
    y, yp, z = ops.layernorm_chain(ad, (la.weight.to(dev), la.bias.to(dev), la.eps), pos.to(dev),
                                   (lb.weight.to(dev), lb.bias.to(dev), lb.eps))
    with torch.no_grad():
        wy = la(a)
        wz = lb(wy)
    assert (y.cpu() - wy).abs().max().item() <= 1e-5
    assert torch.equal(yp.cpu(), y.cpu() + pos[torch.arange(201) % 67])
    assert (z.cpu() - wz).abs().max().item() <= 2e-5
    y2, yp2, z2 = ops.layernorm_chain(ad, (la.weight.to(dev), la.bias.to(dev), la.eps))
    assert yp2 is None and z2 is None and torch.equal(y2, y)


@pytest.mark.parametrize('B,Q,S', [(2, 100, 1024), (1, 37, 36), (2, 100, 4100), (1, 128, 16384)])
def test_masked_xattn_bf16_vs_f32_kernel(dev, B, Q, S):
    """bf16 K / transposed-V kernel against the f32 kernel on the same (bf16-representable) K, V and mask."""
    g = torch.Generator().manual_seed(49)
    H, D = 8, 32
    E = H * D
    q = torch.randn(B, Q, E, generator=g)
    k = torch.randn(B, S, E, generator=g).bfloat16()
    v = torch.randn(B, S, E, generator=g).bfloat16()
    mask = torch.rand(B, Q, S, generator=g) < 0.6
    mask[:, 0] = True                      # an all-blocked row ...
    from cgg_amd.query_decoder import pack_bool_mask
    bits = pack_bool_mask(mask).to(dev)
    ops.attn_mask_fix_full_rows(bits, S)   # ... is un-masked, as the head does
    kv = torch.cat([k.float(), v.float()], -1).to(dev)
    want = ops.masked_xattn(q.to(dev), kv, bits, H)
    got = ops.masked_xattn_bf16(q.to(dev), k.to(dev), v.transpose(1, 2).contiguous().to(dev), bits, H)
    assert torch.isfinite(got).all()
    scale = want.abs().max().item()
    assert (got - want).abs().max().item() <= 0.03 * scale
    assert (got - want).abs().mean().item() <= 4e-3 * scale
    got2 = ops.masked_xattn_bf16(q.to(dev), k.to(dev), v.transpose(1, 2).contiguous().to(dev), None, H)
    want2 = ops.masked_xattn(q.to(dev), kv, None, H)
    assert (got2 - want2).abs().max().item() <= 0.03 * want2.abs().max().item()


@pytest.mark.parametrize('up,crop,out', [((64, 96), (64, 96), (64, 96)), ((64, 96), (60, 90), (60, 90)),
                                         ((64, 96), (60, 90), (75, 110))])
def test_instance_masks_multi_equals_per_type_calls(dev, up, crop, out):
    """one mask pass writing every evaluation type's detection slots == one `instance_masks` call per type."""
    g = torch.Generator().manual_seed(63)
    Q, H, W = 23, 16, 24
    logits = (torch.randn(Q, H, W, generator=g) * 3).to(dev)
    lists = [torch.randint(0, Q, (n,), generator=g).to(dev) for n in (17, 5, 0, 30)]
    lists[1][:] = 7                                    # one query picked several times inside a type
    masks_l, qs, qb = ops.instance_masks_multi(logits, lists, up, crop, out)
    for ix, m in zip(lists, masks_l):
        wm, ws_, wb = ops.instance_masks(logits, ix.to(torch.int32), up, crop, out)
        assert m.shape == wm.shape and torch.equal(m, wm)
        if ix.numel():
            assert torch.allclose(qs[ix], ws_, rtol=1e-6, atol=1e-7) and torch.equal(qb[ix], wb)


def test_bias_relu_maxpool_nhwc(dev):
    g = torch.Generator().manual_seed(64)
    for (B, H, W, C) in [(2, 18, 22, 64), (1, 7, 9, 8)]:
        x = torch.randn(B, H, W, C, generator=g).bfloat16()
        b = torch.randn(C, generator=g).bfloat16()
        want = torch.nn.functional.max_pool2d((x + b).relu().permute(0, 3, 1, 2).float(), 3, stride=2, padding=1)
        got = ops.bias_relu_maxpool_nhwc(x.to(dev), b.to(dev))
        assert torch.equal(got.cpu().float(), want.permute(0, 2, 3, 1))


def test_add_layernorm_kv_level_major(dev):
    g = torch.Generator().manual_seed(65)
    B, C = 2, 256
    level_hw = [(2, 4), (4, 4), (8, 6)]
    starts, S = [], 0
    for h, w in level_hw:
        starts.append(S)
        S += h * w
    a = torch.randn(B, S, C, generator=g)
    b = torch.randn(B, S, C, generator=g).bfloat16()
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    shift, pos = torch.randn(S, C, generator=g), torch.randn(S, C, generator=g)
    y = torch.nn.functional.layer_norm(a + b.float(), (C,), gamma, beta, 1e-5)
    y32, m16, mp16 = ops.add_layernorm_kv(a.to(dev), b.to(dev), gamma.to(dev), beta.to(dev), 1e-5, shift.to(dev),
                                          pos.to(dev), starts)
    assert torch.allclose(y32.cpu(), y, atol=2e-5, rtol=1e-5)
    y = y32.cpu()
    for l, (h, w) in enumerate(level_hw):
        s0, n = starts[l], h * w
        got_m = m16[B * s0:B * (s0 + n)].view(B, n, C).cpu()
        got_p = mp16[B * s0:B * (s0 + n)].view(B, n, C).cpu()
        m = y[:, s0:s0 + n] + shift[s0:s0 + n]
        assert torch.equal(got_m, m.bfloat16())
        assert torch.equal(got_p, (m + pos[s0:s0 + n]).bfloat16())


def test_class_topk_matches_softmax_topk(dev):
    g = torch.Generator().manual_seed(66)
    B, Q, k = 2, 100, 100
    ncols = [66, 18, 50]
    col0 = [0, 66, 84]
    dots = (torch.randn(B * Q, sum(ncols), generator=g) * 3).to(dev)
    dots[5, 3] = dots[7, 3] = dots[9, 70] = 9.0          # some exact ties in the input
    labels, scores, qidx = ops.class_topk(dots, B, col0, ncols, k)
    for b in range(B):
        for t, (c0, nc) in enumerate(zip(col0, ncols)):
            prob, _, _ = ops.rowwise_softmax_argmax(dots[b * Q:(b + 1) * Q, c0:c0 + nc].contiguous(), want_prob=True)
            flat = prob[:, :-1].flatten()
            want_s, want_i = flat.sort(descending=True, stable=True)
            want_s, want_i = want_s[:k], want_i[:k]
            assert torch.equal(scores[b, t], want_s)
            # order: descending score, ties by ascending flat index == stable descending sort
            assert torch.equal(labels[b, t] + qidx[b, t] * (nc - 1), want_i)


def test_instance_masks_picks_matches_multi(dev):
    g = torch.Generator().manual_seed(67)
    Q, H, W = 20, 24, 32
    logits = (torch.randn(Q, H, W, generator=g) * 3).to(dev)
    picks = [torch.randint(0, Q, (16,), generator=g), torch.randint(0, Q, (16,), generator=g)]
    cls_scores = torch.rand(32, generator=g).to(dev)
    qidx = torch.cat(picks).to(dev)
    up, crop, out = (96, 128), (90, 120), (90, 120)
    masks, bboxes = ops.instance_masks_picks(logits, qidx, cls_scores, up, crop, out)
    masks_l, qscores, qboxes = ops.instance_masks_multi(logits, [p.to(dev) for p in picks], up, crop, out)
    assert torch.equal(masks, torch.cat(masks_l))
    assert torch.equal(bboxes[:, :4], qboxes[qidx])
    assert torch.allclose(bboxes[:, 4], cls_scores * qscores[qidx], rtol=2e-6, atol=0)


def test_decoder_tail_matches_the_launch_chain(dev):
    """cgg_decoder_tail_bf16 == cgg_layernorm_chain + 3 x cgg_linear_rows_bf16 (mask MLP) + the query projection."""
    g = torch.Generator().manual_seed(68)
    M, C, Q, nsum = 200, 256, 100, 8
    planes = (torch.randn(nsum, M, C, generator=g) * 0.5).to(dev)
    pos = torch.randn(Q, C, generator=g).to(dev)
    na = (torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev), 1e-5)
    nb = (torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev), 1e-5)
    ws = [(torch.randn(C, C, generator=g) / 16).to(dev) for _ in range(4)]
    bs = [torch.randn(C, generator=g).to(dev) for _ in range(4)]
    pk = [ops.pack_linear_weight(w) for w in ws]
    y, yp, me, qn = ops.decoder_tail(planes, na, pos, nb, (pk[0], bs[0], pk[1], bs[1], pk[2], bs[2]), (pk[3], bs[3]),
                                     want_pos=True)
    y0, yp0, z0 = ops.layernorm_chain(planes, na, pos, nb)
    h = ops.linear_rows_bf16(z0, pk[0], C, bs[0], relu_cols=C)
    h = ops.linear_rows_bf16(h, pk[1], C, bs[1], relu_cols=C)
    me0 = ops.linear_rows_bf16(h, pk[2], C, bs[2])
    qn0 = ops.linear_rows_bf16(yp0, pk[3], C, bs[3])
    # same arithmetic per stage, different (but fixed) reduction order inside the LayerNorms
    assert torch.allclose(y, y0, atol=2e-5, rtol=1e-5)
    assert torch.allclose(yp, yp0, atol=2e-5, rtol=1e-5)
    assert torch.allclose(me, me0, atol=3e-2, rtol=2e-2)       # bf16 roundings of near-identical inputs may flip
    assert torch.allclose(qn, qn0, atol=3e-2, rtol=2e-2)
    # and against plain f32 math
    yr = torch.nn.functional.layer_norm(planes.sum(0), (C,), na[0], na[1], 1e-5)
    zr = torch.nn.functional.layer_norm(yr, (C,), nb[0], nb[1], 1e-5)
    mr = torch.relu(torch.relu(zr @ ws[0].t() + bs[0]) @ ws[1].t() + bs[1]) @ ws[2].t() + bs[2]
    assert torch.allclose(y, yr, atol=1e-4, rtol=1e-4)
    assert (me - mr).abs().max() < 0.05 * mr.abs().max()
    assert (qn - ((yr + pos.repeat(M // Q, 1)) @ ws[3].t() + bs[3])).abs().max() < 0.05 * qn.abs().max()
    # deterministic
    y2, _, me2, qn2 = ops.decoder_tail(planes, na, pos, nb, (pk[0], bs[0], pk[1], bs[1], pk[2], bs[2]), (pk[3], bs[3]))
    assert torch.equal(y, y2) and torch.equal(me, me2) and torch.equal(qn, qn2)


def test_self_attn_rows_bf16(dev):
    g = torch.Generator().manual_seed(69)
    for (B, Q, H) in [(2, 100, 8), (1, 37, 8), (3, 128, 4)]:
        E = 32 * H
        q = torch.randn(B * Q, E, generator=g).to(dev)
        kv = torch.randn(B * Q, 2 * E, generator=g).to(dev)
        got = ops.self_attn_rows_bf16(q, kv, B, H)
        qh = q.view(B, Q, H, 32).transpose(1, 2)
        kh = kv[:, :E].reshape(B, Q, H, 32).transpose(1, 2)
        vh = kv[:, E:].reshape(B, Q, H, 32).transpose(1, 2)
        want = torch.nn.functional.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B * Q, E)
        assert (got - want).abs().max() < 2e-2, (got - want).abs().max()      # bf16 operands, f32 accumulation
        assert torch.isfinite(got).all()


def test_decoder_mid_matches_the_launch_chain(dev):
    g = torch.Generator().manual_seed(70)
    M, C, Q = 200, 256, 100
    core = torch.randn(M, C, generator=g).to(dev)
    res = torch.randn(M, C, generator=g).to(dev)
    pos = torch.randn(Q, C, generator=g).to(dev)
    norm = (torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev), 1e-5)
    wo, bo = (torch.randn(C, C, generator=g) / 16).to(dev), torch.randn(C, generator=g).to(dev)
    wqkv, bqkv = (torch.randn(3 * C, C, generator=g) / 16).to(dev), torch.randn(3 * C, generator=g).to(dev)
    pwo, pqkv = ops.pack_linear_weight(wo), ops.pack_linear_weight(wqkv)
    x1, q, kv = ops.decoder_mid(core, pwo, bo, res, norm, pos, (pqkv, bqkv))
    x1_0, x1p_0 = ops.linear_rows_bf16(core, pwo, C, bo, res=res, ln=norm, pos=pos, want_pos=True)
    q0, kv0 = ops.linear_rows_bf16_qkv(x1p_0, x1_0, pqkv, bqkv, C)
    assert torch.allclose(x1, x1_0, atol=3e-5, rtol=1e-5)
    assert torch.allclose(q, q0, atol=3e-2, rtol=2e-2) and torch.allclose(kv, kv0, atol=3e-2, rtol=2e-2)
    ref = torch.nn.functional.layer_norm(core @ wo.t() + bo + res, (C,), norm[0], norm[1], 1e-5)
    assert (x1 - ref).abs().max() < 0.05
    only = ops.decoder_mid(core, pwo, bo, res, norm)
    assert only[1] is None and torch.equal(only[0], x1)


def test_decoder_ffn_matches_the_two_launches(dev):
    g = torch.Generator().manual_seed(71)
    M, C, F = 200, 256, 2048
    x = torch.randn(M, C, generator=g).to(dev)
    w1, b1 = (torch.randn(F, C, generator=g) / 16).to(dev), torch.randn(F, generator=g).to(dev)
    w2, b2 = (torch.randn(C, F, generator=g) / 45).to(dev), torch.randn(C, generator=g).to(dev)
    p1, p2 = ops.pack_linear_weight(w1), ops.pack_linear_weight(w2)
    planes = ops.decoder_ffn(x, p1, b1, p2, b2, F)
    assert planes.shape == (F // 256, M, C)
    h = ops.linear_rows_bf16(x, p1, F, b1, relu_cols=F)
    want = ops.linear_rows_bf16(h, p2, C, b2, res=x, ksplit=8)
    # same bf16 operands, same per-plane K ranges -> the planes themselves agree exactly
    assert torch.equal(planes, want)
    ref = x + torch.relu(x @ w1.t() + b1) @ w2.t() + b2
    assert (planes.sum(0) - ref).abs().max() < 0.05 * ref.abs().max()


def test_gemm_bias_res_act_bf16(dev):
    g = torch.Generator().manual_seed(72)
    for (M, N, K, relu, has_res) in [(1024, 256, 64, True, True), (520, 512, 128, False, True), (256, 64, 256, True, False)]:
        x = torch.randn(M, K, generator=g).bfloat16().to(dev)
        w = (torch.randn(N, K, generator=g) / 8).bfloat16().to(dev)
        b = torch.randn(N, generator=g).bfloat16().to(dev)
        r = torch.randn(M, N, generator=g).bfloat16().to(dev) if has_res else None
        got = ops.gemm_bias_res_act_bf16(x, w, b, r, relu)
        want = x.float() @ w.float().t() + b.float() + (r.float() if has_res else 0)
        if relu:
            want = want.relu()
        assert (got.float() - want).abs().max() <= 0.02 * want.abs().max() + 0.02


def test_im2col3x3_gemm_equals_conv(dev):
    g = torch.Generator().manual_seed(73)
    for (B, H, W, C, Co, st) in [(2, 16, 20, 32, 64, 1), (1, 17, 13, 16, 32, 2)]:
        x = torch.randn(B, H, W, C, generator=g).bfloat16().to(dev)
        w = (torch.randn(Co, C, 3, 3, generator=g) / 8).bfloat16().to(dev)
        b = torch.randn(Co, generator=g).bfloat16().to(dev)
        cols, Ho, Wo = ops.im2col3x3_nhwc(x, st)
        ref_cols = torch.nn.functional.unfold(x.permute(0, 3, 1, 2).float(), 3, padding=1, stride=st)   # (B, C*9, L)
        ref_cols = ref_cols.view(B, C, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, 9 * C)
        assert torch.equal(cols.float(), ref_cols)
        y = ops.gemm_bias_res_act_bf16(cols, w.permute(0, 2, 3, 1).reshape(Co, -1).contiguous(), b, None, True)
        want = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).float(), w.float(), b.float(), stride=st, padding=1).relu()
        want = want.permute(0, 2, 3, 1).reshape(B * Ho * Wo, Co)
        assert (y.float() - want).abs().max() <= 0.02 * want.abs().max() + 0.02


def test_stem_conv7x7_matches_conv2d(dev):
    g = torch.Generator().manual_seed(74)
    w = (torch.randn(64, 3, 7, 7, generator=g) / 8).to(dev)
    packed = ops.pack_stem_weight(w)
    for (B, H, W) in [(2, 64, 96), (1, 50, 70), (1, 17, 33)]:            # incl. ragged tiles and odd sizes
        img = torch.randn(B, 3, H, W, generator=g).to(dev)
        got = ops.stem_conv7x7(img, packed)
        want = torch.nn.functional.conv2d(img.bfloat16().float(), w.bfloat16().float(), None, stride=2, padding=3)
        assert got.shape == (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)
        err = (got.float().permute(0, 3, 1, 2) - want).abs().max().item()
        assert err <= 0.02 * want.abs().max().item() + 0.02, err


def test_xattn_bf16_auto_unmask_equals_fix_full_rows(dev):
    """fix_full_rows=True (decided inside the partial / combine kernels) == clearing fully-masked rows beforehand."""
    from cgg_amd.query_decoder import pack_bool_mask
    g = torch.Generator().manual_seed(75)
    B, Q, H, E = 2, 100, 8, 256
    for S in (1024, 4096, 1000):
        q = torch.randn(B, Q, E, generator=g).to(dev)
        k = torch.randn(B, S, E, generator=g).bfloat16().to(dev)
        vt = torch.randn(B, E, S, generator=g).bfloat16().to(dev)
        mask = torch.rand(B, Q, S, generator=g) < 0.6
        mask[0, 3] = True                      # blocked everywhere -> attends to everything
        mask[1, 77] = True
        mask[0, 5, :S // 2] = True             # blocked in whole chunks only -> those chunks must be dropped
        mask[1, 9, S // 4:] = True
        bits = pack_bool_mask(mask.to(dev))
        got = ops.masked_xattn_bf16(q, k, vt, bits.clone(), H, fix_full_rows=True)
        fixed = bits.clone()
        ops.attn_mask_fix_full_rows(fixed, S)
        want = ops.masked_xattn_bf16(q, k, vt, fixed, H)
        assert torch.isfinite(got).all()
        assert torch.equal(got, want)


def test_pack_mask_feature_nhwc_multi_equals_single(dev):
    g = torch.Generator().manual_seed(76)
    mf = torch.randn(2, 32, 48, 256, generator=g).bfloat16().to(dev)
    pools = [1, 2, 4, 8]
    multi = ops.pack_mask_feature_nhwc_multi(mf, pools)
    for p, m in zip(pools, multi):
        one = ops.pack_mask_feature_nhwc(mf, p)
        assert (m.h, m.w) == (one.h, one.w) and torch.equal(m.hi, one.hi)


def test_point_sample_nhwc_matches_grid_sample(dev):
    g = torch.Generator().manual_seed(77)
    B, C, H, W, P = 2, 64, 24, 40, 500
    feat = torch.randn(B, C, H, W, generator=g).to(dev)
    pts = torch.rand(B, P, 2, generator=g).to(dev)
    pts[0, :4] = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.999, 0.001], [0.5, 0.5]])      # borders: zero padding taps
    got = ops.point_sample_nhwc(feat.permute(0, 2, 3, 1).contiguous(), pts)
    want = torch.nn.functional.grid_sample(feat, (pts * 2.0 - 1.0).unsqueeze(2), align_corners=False).squeeze(3)   # (B, C, P)
    assert torch.allclose(got, want.transpose(1, 2), atol=1e-6, rtol=1e-6)
    assert (got == want.transpose(1, 2)).float().mean() > 0.99          # same arithmetic: bitwise on (nearly) all samples


def test_point_sample_nhwc_x3_images_equal_pack_of_samples_and_point_logits_are_f32_class(dev):
    """`cgg_point_sample_nhwc_x3` (sampler + x3 pack in one launch, layer-major images) against the two-step form it replaces --
    `point_sample_nhwc` rows packed by `pack_mask_feature_nhwc_x3`: the same 16-bit pieces bit for bit; and the per-layer point logits
    `mask_logits(embed_g, packed[g])` against float64 mask_embed . grid_sample(feature) within 4 x the f32 bmm's own error."""
    from cgg_amd import runtime
    g = torch.Generator().manual_seed(79)
    B, C, H, W, n, P, Q = 2, 256, 24, 40, 3, 96, 37
    feat = (torch.randn(B, C, H, W, generator=g) * 2).to(dev)
    nhwc = feat.permute(0, 2, 3, 1).contiguous()
    pts = torch.rand(B, n * P, 2, generator=g).to(dev)
    pts[0, :4] = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.999, 0.001], [0.5, 0.5]])      # borders: zero padding taps
    embeds = [(torch.randn(B, Q, C, generator=g) * 2).to(dev) for _ in range(n)]
    assert ops.point_sample_nhwc_x3_ok(nhwc, pts, n) and not ops.point_sample_nhwc_x3_ok(nhwc, pts[:, :n * P - 8], n)
    packs = ops.point_sample_nhwc_x3(nhwc, pts, n)
    rows = ops.point_sample_nhwc(nhwc, pts)                                               # (B, n P, C)
    want64 = torch.nn.functional.grid_sample(feat.double(), (pts.double() * 2.0 - 1.0).unsqueeze(2), align_corners=False).squeeze(3)
    with runtime.precision_scope('fp32'):
        for li in range(n):
            two = ops.pack_mask_feature_nhwc_x3(rows[:, li * P:(li + 1) * P].contiguous().view(B, 1, P, C), [1])[0]
            assert torch.equal(packs[li].hi.view(torch.int16), two.hi.view(torch.int16))
            assert torch.equal(packs[li].lo.view(torch.int16), two.lo.view(torch.int16))
            out = torch.empty((B, Q, P), dtype=torch.float32, device=dev)
            got, _ = ops.mask_logits(embeds[li], packs[li], out=out)
            assert got.data_ptr() == out.data_ptr()
            fs = want64[:, :, li * P:(li + 1) * P]                                        # (B, C, P)
            want = torch.bmm(embeds[li].double(), fs)
            f32_err = (torch.bmm(embeds[li], fs.float()).double() - want).abs().max().item()
            err = (out.double() - want).abs().max().item()
            assert err <= 4 * f32_err + 1e-6 * want.abs().max().item(), (li, err, f32_err)


def test_relu_backward_absmax_equals_threshold_backward_and_absmax(dev):
    g = torch.Generator().manual_seed(80)
    for shape in ((3, 17, 20, 64), (5, 1000), (4,)):
        gy = (torch.randn(shape, generator=g) * 1e-5).to(dev)
        y = torch.relu(torch.randn(shape, generator=g)).to(dev)
        got, amax = ops.relu_backward_absmax(gy, y)
        want = torch.ops.aten.threshold_backward(gy, y, 0.0)
        assert torch.equal(got, want) and float(amax) == float(want.abs().max())
    with pytest.raises(ops.CggError):
        ops.relu_backward_absmax(gy[:3], y[:3])                          # numel % 4


def test_instance_masks_picks_bitpacked(dev):
    g = torch.Generator().manual_seed(78)
    Q, H, W = 20, 24, 32
    logits = (torch.randn(Q, H, W, generator=g) * 3).to(dev)
    qidx = torch.randint(0, Q, (40,), generator=g).to(dev)
    sc = torch.rand(40, generator=g).to(dev)
    for up, crop in (((96, 128), (96, 128)), ((96, 128), (90, 112)), ((48, 64), (48, 64))):
        assert ops.instance_masks_bitpack_ok((H, W), up, crop, crop)
        m, bb = ops.instance_masks_picks(logits, qidx, sc, up, crop, crop)
        p, bb2 = ops.instance_masks_picks(logits, qidx, sc, up, crop, crop, bitpack=True)
        assert p.dtype == torch.uint8 and tuple(p.shape) == (40, crop[0], crop[1] // 8)
        unpacked = np.unpackbits(p.cpu().numpy(), axis=-1, bitorder='little').astype(bool)
        assert np.array_equal(unpacked, m.cpu().numpy())
        assert torch.equal(bb[:, :4], bb2[:, :4]) and torch.allclose(bb[:, 4], bb2[:, 4], rtol=1e-5)
    assert not ops.instance_masks_bitpack_ok((H, W), (96, 128), (90, 112), (45, 56))       # second resize
    assert not ops.instance_masks_bitpack_ok((H, W), (72, 96), (72, 96), (72, 96))         # scale 3


def test_subsample_nhwc(dev):
    g = torch.Generator().manual_seed(79)
    for (B, H, W, C, st) in [(2, 16, 20, 32, 2), (1, 7, 9, 8, 2), (1, 6, 6, 16, 3)]:
        x = torch.randn(B, H, W, C, generator=g).bfloat16().to(dev)
        assert torch.equal(ops.subsample_nhwc(x, st), x[:, ::st, ::st, :].contiguous())


@pytest.mark.parametrize('shape,square', [((3, 2, 7, 12544), False), ((5, 8), True), ((1, 100, 1000), False)])
def test_match_cost_rows_vs_float64(dev, shape, square):
    """`cgg_match_cost_rows`: sigmoid(x), sum_p softplus(x) and sum_p sigmoid(x) [^2] of point-sampled mask logits in one pass
    (the prediction-only halves of mmdet's CrossEntropyLossCost / DiceCost, mask2former_head.py:320-390) against float64, with
    saturating logits on both sides; and the identity the caller relies on: pos . t + neg . (1 - t) = sum softplus(x) - x . t."""
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g) * 6
    x.view(-1)[:6] = torch.tensor([120.0, -120.0, 20.0, -20.0, 0.0, 88.0])
    sig, sp, ss = ops.match_cost_rows(x.to(dev), square=square)
    xd = x.double()
    wsig = xd.sigmoid()
    assert (sig.cpu().double() - wsig).abs().max().item() <= 2e-7
    wsp = torch.nn.functional.softplus(xd).sum(-1)
    assert (sp.cpu().double() - wsp).abs().max().item() <= 2e-6 * wsp.abs().max().item()
    wss = (wsig ** 2 if square else wsig).sum(-1)
    assert (ss.cpu().double() - wss).abs().max().item() <= 2e-6 * wss.abs().max().item()
    t = (torch.rand(shape, generator=g) < 0.3).double()
    F = torch.nn.functional
    ref = (F.binary_cross_entropy_with_logits(xd, torch.ones_like(xd), reduction='none') * t
           + F.binary_cross_entropy_with_logits(xd, torch.zeros_like(xd), reduction='none') * (1 - t)).sum(-1)
    got = sp.cpu().double() - (xd * t).sum(-1)
    assert (got - ref).abs().max().item() <= 2e-6 * (1 + ref.abs().max().item())


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_generator_ce_rows_vs_materialised_logits(dev, precision):
    """`CaptionTransformer.generator_ce_rows` (cgg_ce_rows_forward / _backward over GEMM row chunks; the logits are never
    stored) against `F.cross_entropy(generator(hidden), target, reduction='none', ignore_index=0)` on materialised logits:
    row losses and the gradients w.r.t. hidden / generator weight / bias. Vocabulary 30522 (not a multiple of 8: padded
    columns), several row chunks, ignored rows, a target in the last column."""
    from cgg_amd import registry, runtime
    from cgg_amd.caption_transformer import _GeneratorCEFn
    torch.manual_seed(5)
    V, K, M = 30522, 768, 600
    cg = registry.build_head(dict(type='CaptionTransformer', nb_layers=1, input_dim=K, hidden_dim=K, ff_dim=64, nb_heads=8,
                                  drop_val=0.0, pre_norm=False, seq_length=35, nb_tokens=V)).to(dev)
    with torch.no_grad():
        cg.generator.weight.normal_(0, 0.05)
        cg.generator.bias.normal_(0, 0.5)
    hidden = torch.randn(M, K, device=dev, requires_grad=True)
    target = torch.randint(1, V, (M,), device=dev)
    target[::5] = 0                      # ignored positions (caption padding)
    target[1] = V - 1
    grow = torch.rand(M, device=dev)
    old = _GeneratorCEFn.CHUNK
    _GeneratorCEFn.CHUNK = 256           # 3 chunks, the last one ragged
    try:
        with runtime.precision_scope(precision):
            rows = cg.generator_ce_rows(hidden, target, 0)
            g = torch.autograd.grad(rows, (hidden, cg.generator.weight, cg.generator.bias), grow)
    finally:
        _GeneratorCEFn.CHUNK = old
    # reference: the formulation the reference runs (in bf16 mode: what bf16 autocast of it computes)
    h2 = hidden.detach().clone().requires_grad_(True)
    if precision == 'bf16':
        logits = torch.nn.functional.linear(h2.bfloat16(), cg.generator.weight.bfloat16(), cg.generator.bias.bfloat16()).float()
    else:
        logits = torch.nn.functional.linear(h2.double(), cg.generator.weight.double(), cg.generator.bias.double())
    want = torch.nn.functional.cross_entropy(logits, target, reduction='none', ignore_index=0)
    wg = torch.autograd.grad(want, (h2, cg.generator.weight, cg.generator.bias), grow.to(want.dtype))
    tol = 2e-5 if precision == 'fp32' else 2e-2
    assert float(rows[::5].abs().max()) == 0.0
    assert (rows.double() - want.double()).abs().max().item() <= tol * (1 + want.abs().max().item())
    for a, b, name in zip(g, wg, ('hidden', 'weight', 'bias')):
        scale = b.abs().max().item()
        assert (a.double() - b.double()).abs().max().item() <= tol * scale + 1e-9, (name, (a.double() - b.double()).abs().max().item(), scale)


@pytest.mark.parametrize('B,Q,h,w,split', [(2, 100, 64, 64, True), (1, 37, 40, 56, True), (2, 200, 64, 64, False),
                                           (2, 160, 32, 72, True), (1, 300, 16, 24, False), (2, 100, 256, 256, False)])
def test_mask_logits_backward_vs_float64(dev, B, Q, h, w, split):
    """cgg_mask_logits_backward (the transposed contractions of the einsum at mask2former_head.py:748) against float64:
    split (hi, lo) mode to 2e-5 of the gradient scale, plain bf16 mode to the bf16 bound; ragged pixel tiles
    (40 x 56 = 70 tiles of 32), row counts that are not multiples of 16 / 32, row groups beyond one launch (160 split,
    300 plain), full resolution; and the autograd function end to end."""
    from cgg_amd.mask2former_head import _MaskLogitsFn
    E, F_, go, ge, gf = check_mask_logits_backward(dev, B, Q, h, w, split)
    tol = 2e-5 if split else 1e-2
    ge2, gf2 = ops.mask_logits_backward(E.to(dev), F_.to(dev), go.to(dev), split)
    assert torch.equal(ge, ge2) and torch.equal(gf, gf2)                    # deterministic
    # autograd function (forward on the packed image + this backward)
    Ed, Fd = E.to(dev).requires_grad_(True), F_.to(dev).requires_grad_(True)
    packed = ops.pack_mask_feature(Fd.detach(), 1, split)
    out = _MaskLogitsFn.apply(Ed, Fd, packed)
    want_o = torch.einsum('bqc,bchw->bqhw', E.double(), F_.double())
    assert (out.detach().cpu().double() - want_o).abs().max().item() <= tol * want_o.abs().max().item()
    a, b = torch.autograd.grad(out, (Ed, Fd), go.to(dev))
    assert torch.equal(a, ge) and torch.equal(b, gf)


def check_mask_logits_backward(dev, B, Q, h, w, split):
    """one cgg_mask_logits_backward on `dev` within the bound of test_mask_logits_backward_vs_float64; returns the host inputs and
    the device gradients (E, F_, grad_out, grad_embed, grad_feat)"""
    g = torch.Generator().manual_seed(70 + Q)
    C = 256
    E = torch.randn(B, Q, C, generator=g)
    F_ = torch.randn(B, C, h, w, generator=g)
    go = torch.randn(B, Q, h, w, generator=g)
    want_e = torch.einsum('bqhw,bchw->bqc', go.double(), F_.double())
    want_f = torch.einsum('bqc,bqhw->bchw', E.double(), go.double())
    ge, gf = ops.mask_logits_backward(E.to(dev), F_.to(dev), go.to(dev), split)
    tol = 2e-5 if split else 1e-2
    for got, want, name in ((ge, want_e, 'grad_embed'), (gf, want_f, 'grad_feat')):
        scale = want.abs().max().item()
        err = (got.cpu().double() - want).abs().max().item()
        assert err <= tol * scale, (name, err, scale)
    return E, F_, go, ge, gf


def test_point_sample_planes_vs_grid_sample(dev):
    """cgg_point_sample_planes == [3P] point_sample (F.grid_sample(2 p - 1, bilinear, zeros, align_corners=False)) of the
    indexed plane, incl. points on / outside the border."""
    g = torch.Generator().manual_seed(81)
    N, H, W, rows, P = 7, 37, 52, 11, 300
    planes = torch.randn(N, H, W, generator=g)
    index = torch.randint(0, N, (rows,), generator=g).to(torch.int32)
    pts = torch.rand(rows, P, 2, generator=g) * 1.2 - 0.1            # some outside [0, 1]
    pts[0, 0] = torch.tensor([0.0, 0.0])
    pts[0, 1] = torch.tensor([1.0, 1.0])
    want = torch.nn.functional.grid_sample(planes[index.long()][:, None], (2.0 * pts - 1.0)[:, :, None, :],
                                           align_corners=False)[:, 0, :, 0]
    got = ops.point_sample_planes(planes.to(dev), index.to(dev), pts.to(dev)).cpu()
    assert (got - want).abs().max().item() <= 1e-6


@pytest.mark.parametrize('B,Q,h,w,pool', [(2, 100, 64, 64, 1), (1, 37, 40, 56, 1), (2, 100, 64, 64, 2), (1, 200, 32, 40, 4)])
def test_mask_logits_exact_f32_kernel(dev, B, Q, h, w, pool, monkeypatch):
    """cgg_mask_logits_f32 (round 2's parity-mode kernel: f32 MFMA; since round 3 only behind CGG_X3=0, parity mode runs the
    f16 x 3 split kernel -- tests/test_x3_gpu.py) vs float64: logits to f32 rounding (1e-6 of the operand scale),
    attention-mask bits equal to (interpolated logit < 0) away from rounding, for the full-resolution and the pooled feature,
    ragged pixel tiles and more than 128 queries."""
    from cgg_amd import runtime
    monkeypatch.setattr(runtime, '_X3', False)       # read once at import: the test flips the module switch, not the environment
    g = torch.Generator().manual_seed(90 + Q)
    C = 256
    E = torch.randn(B, Q, C, generator=g)
    F_ = torch.randn(B, C, h, w, generator=g)
    packed = ops.pack_mask_feature(F_.to(dev), pool, split=True)
    assert packed.f32 is not None
    out, bits = ops.mask_logits(E.to(dev), packed, want_logits=True, want_bits=True)
    full = torch.einsum('bqc,bchw->bqhw', E.double(), F_.double())
    want = full if pool == 1 else torch.nn.functional.interpolate(full, (h // pool, w // pool), mode='bilinear',
                                                                  align_corners=False)
    scale = (E.abs().double() @ F_.abs().double().flatten(2)).max().item()
    err = (out.cpu().double() - want).abs().max().item()
    assert err <= 2e-6 * scale, (err, scale)
    got_bits = ops.unpack_bits(bits, packed.npix).cpu().view(B, Q, -1)
    clear = want.flatten(2).abs() > 1e-5 * scale
    assert torch.equal(got_bits[clear], (want.flatten(2) < 0)[clear])


@pytest.mark.parametrize('M,N,FF', [(43008, 21504, 1024), (4071, 1357, 1024), (100, 50, 512), (64, 64, 256)])
def test_encoder_ffn_ln_fused_vs_float64(dev, M, N, FF):
    """Fused encoder FFN + residual LayerNorm (one launch, hidden activation on chip) against float64 on the SAME
    bf16-rounded operands (x, W1, W2; hidden rounded to bf16 as the kernel does): outputs are bf16, so the bound is one
    bf16 ulp of |y| <= ~4 (2^-6 = 0.0157) for both y and y + pos; ragged M (not a multiple of the 64-row block) and
    pos rows wrapping per image (row % N); three runs bit-identical."""
    check_encoder_ffn_ln(dev, M, N, FF, n_runs=3)


def check_encoder_ffn_ln(dev, M, N, FF, n_runs=1):
    """`n_runs` bit-identical launches on `dev`, the first within the bounds of test_encoder_ffn_ln_fused_vs_float64"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(M + FF)
    C = 256
    x16 = torch.randn(M, C, generator=g).to(dev).bfloat16()
    w1 = (torch.randn(FF, C, generator=g) * 0.05).to(dev)
    b1 = (torch.randn(FF, generator=g) * 0.1).to(dev)
    w2 = (torch.randn(C, FF, generator=g) * 0.03).to(dev)
    b2 = (torch.randn(C, generator=g) * 0.1).to(dev)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev)
    beta = (torch.randn(C, generator=g) * 0.1).to(dev)
    pos = torch.randn(N, C, generator=g).to(dev)
    w1p, w2p = ops.pack_linear_weight(w1), ops.pack_linear_weight(w2)
    runs = []
    for _ in range(n_runs):
        y32, y16, yp16 = ops.encoder_ffn_ln(x16, w1p, b1, w2p, b2, gamma, beta, 1e-5, pos=pos, want_f32=True,
                                            want_bf16=True, want_pos=True)
        torch.cuda.synchronize()
        runs.append((y32.clone(), y16.clone(), yp16.clone()))
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))
    xd = x16.double()
    h = torch.relu(xd @ w1.bfloat16().double().t() + b1.double()).bfloat16().double()
    ref64 = F.layer_norm(xd + h @ w2.bfloat16().double().t() + b2.double(), (C,), gamma.double(), beta.double(), 1e-5)
    refp = ref64 + pos.double().repeat((M + N - 1) // N, 1)[:M]
    y32, y16, yp16 = runs[0]
    assert (y32.double() - ref64).abs().max().item() <= 2e-3          # f32 output: accumulation-order error only
    assert (y16.double() - ref64).abs().max().item() <= 2 ** -6 + 2e-3
    assert (yp16.double() - refp).abs().max().item() <= 2 ** -5 + 2e-3  # |y + pos| < 8: one ulp = 2^-5 at most


def test_encoder_ffn_ln_kv_variant_matches_two_pass_path(dev):
    """Last-layer variant: fused FFN + LayerNorm + level-major K / V operands == `encoder_ffn_ln` (f32 output) followed by the
    existing `add_layernorm_kv` row remap, bit for bit on m16 / mp16 / y32 (same arithmetic order in both epilogues)."""
    g = torch.Generator().manual_seed(5)
    B, C, FF = 2, 256, 1024
    shapes = [(8, 12), (16, 24), (32, 48)]
    starts, S = _levels(shapes)
    x16 = torch.randn(B, S, C, generator=g).to(dev).bfloat16()
    w1 = (torch.randn(FF, C, generator=g) * 0.05).to(dev)
    b1 = (torch.randn(FF, generator=g) * 0.1).to(dev)
    w2 = (torch.randn(C, FF, generator=g) * 0.03).to(dev)
    b2 = (torch.randn(C, generator=g) * 0.1).to(dev)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev)
    beta = (torch.randn(C, generator=g) * 0.1).to(dev)
    shift = torch.randn(S, C, generator=g).to(dev)
    pos = torch.randn(S, C, generator=g).to(dev)
    w1p, w2p = ops.pack_linear_weight(w1), ops.pack_linear_weight(w2)
    y32, m16, mp16 = ops.encoder_ffn_ln_kv(x16, w1p, b1, w2p, b2, gamma, beta, 1e-5, shift, pos, starts)
    y_ref, _, _ = ops.encoder_ffn_ln(x16, w1p, b1, w2p, b2, gamma, beta, 1e-5, want_f32=True, want_bf16=False)
    assert torch.equal(y32, y_ref)
    # level-major remap of bf16(y + shift) and bf16(y + shift + pos), row by row
    m = y_ref + shift[None]
    z = m + pos[None]
    want_m = torch.cat([m[:, s:s + h * w].reshape(-1, C) for s, (h, w) in zip(starts, shapes)], 0).bfloat16()
    want_z = torch.cat([z[:, s:s + h * w].reshape(-1, C) for s, (h, w) in zip(starts, shapes)], 0).bfloat16()
    assert torch.equal(m16, want_m) and torch.equal(mp16, want_z)


@pytest.mark.parametrize('M,NC', [(43008, 288), (4071, 384), (37, 288), (300, 320), (129, 256)])
def test_encoder_proj_fused_vs_float64(dev, M, NC):
    """value_proj + [sampling_offsets; attention_weights] projections as one launch against float64 on the same bf16-rounded
    operands: bf16 outputs, so the bound is half a bf16 ulp of the value (|v| < 4 -> 2^-7; offsets reach |o| < 8 -> 2^-6)
    plus f32 accumulation noise; the column-interleaved weight packing is transparent (outputs in natural column order);
    ragged M; two runs bit-identical."""
    g = torch.Generator().manual_seed(M)
    C = 256
    x16 = torch.randn(M, C, generator=g).to(dev).bfloat16()
    xp16 = torch.randn(M, C, generator=g).to(dev).bfloat16()
    wv = (torch.randn(256, C, generator=g) * 0.05).to(dev)
    bv = (torch.randn(256, generator=g) * 0.1).to(dev)
    wc = (torch.randn(NC, C, generator=g) * 0.05).to(dev)
    bc = torch.randn(NC, generator=g).to(dev)
    wvp, wcp = ops.pack_encoder_proj_weight(wv), ops.pack_encoder_proj_weight(wc)
    v, o = ops.encoder_proj(x16, xp16, wvp, bv, wcp, bc)
    v2, o2 = ops.encoder_proj(x16, xp16, wvp, bv, wcp, bc)
    torch.cuda.synchronize()
    assert torch.equal(v, v2) and torch.equal(o, o2)
    assert v.shape == (M, 256) and o.shape == (M, NC)
    rv = x16.double() @ wv.bfloat16().double().t() + bv.double()
    ro = xp16.double() @ wc.bfloat16().double().t() + bc.double()
    assert ((v.double() - rv).abs() / rv.abs().clamp_min(1.0)).max().item() <= 2 ** -8 + 1e-4    # relative half ulp
    assert ((o.double() - ro).abs() / ro.abs().clamp_min(1.0)).max().item() <= 2 ** -8 + 1e-4


@pytest.mark.parametrize('M,N', [(43008, 21504), (4071, 1357), (64, 64)])
def test_encoder_layer_tail_fused_vs_float64(dev, M, N):
    """Post-attention half of an encoder layer in one launch (output_proj + residual LayerNorm + FFN + residual LayerNorm)
    against float64 on the same bf16-rounded operands (x1 and the hidden activation rounded to bf16 where the kernel
    rounds them). bf16 outputs: one ulp of |y| < 4 (2^-6) plus the propagated bf16 rounding of x1 (<= 2^-8 relative, through
    the FFN and a LayerNorm with gamma <= 1.5: measured < 0.02 total); f32 output checked at 0.02 as well. Ragged M."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(M + 1)
    C, FF = 256, 1024
    a16 = torch.randn(M, C, generator=g).to(dev).bfloat16()
    x16 = torch.randn(M, C, generator=g).to(dev).bfloat16()
    wo = (torch.randn(C, C, generator=g) * 0.05).to(dev)
    bo = (torch.randn(C, generator=g) * 0.1).to(dev)
    g0 = (torch.rand(C, generator=g) + 0.5).to(dev)
    be0 = (torch.randn(C, generator=g) * 0.1).to(dev)
    w1 = (torch.randn(FF, C, generator=g) * 0.05).to(dev)
    b1 = (torch.randn(FF, generator=g) * 0.1).to(dev)
    w2 = (torch.randn(C, FF, generator=g) * 0.03).to(dev)
    b2 = (torch.randn(C, generator=g) * 0.1).to(dev)
    g1 = (torch.rand(C, generator=g) + 0.5).to(dev)
    be1 = (torch.randn(C, generator=g) * 0.1).to(dev)
    pos = torch.randn(N, C, generator=g).to(dev)
    wop, w1p, w2p = ops.pack_linear_weight(wo), ops.pack_linear_weight(w1), ops.pack_linear_weight(w2)
    outs = [ops.encoder_layer_tail(a16, x16, wop, bo, (g0, be0, 1e-5), w1p, b1, w2p, b2, (g1, be1, 1e-5), pos=pos,
                                   want_f32=True, want_bf16=True, want_pos=True) for _ in range(2)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    y32, y16, yp16 = outs[0]
    bfd = lambda t: t.bfloat16().double()
    x1 = bfd(F.layer_norm(x16.double() + a16.double() @ bfd(wo).t() + bo.double(), (C,), g0.double(), be0.double(), 1e-5))
    h = bfd(torch.relu(x1 @ bfd(w1).t() + b1.double()))
    ref64 = F.layer_norm(x1 + h @ bfd(w2).t() + b2.double(), (C,), g1.double(), be1.double(), 1e-5)
    refp = ref64 + pos.double().repeat((M + N - 1) // N, 1)[:M]
    e32 = (y32.double() - ref64).abs().max().item()
    e16 = (y16.double() - ref64).abs().max().item()
    ep = (yp16.double() - refp).abs().max().item()
    assert e32 <= 0.02 and e16 <= 0.02 + 2 ** -6 and ep <= 0.02 + 2 ** -5, (e32, e16, ep)
    # and the composition of the two-launch path gives the same rows up to the bf16 rounding of the projection output
    o16 = torch.nn.functional.linear(a16, wo.bfloat16(), bo.bfloat16())
    _, x1_16, _ = ops.add_layernorm_stream(x16, o16, g0, be0, 1e-5, want_f32=False)
    y_two, _, _ = ops.encoder_ffn_ln(x1_16, w1p, b1, w2p, b2, g1, be1, 1e-5, want_f32=True, want_bf16=False)
    assert (y32 - y_two).abs().max().item() <= 0.06


def test_encoder_layer_tail_kv_mode_matches_plain_mode(dev):
    """K / V mode of the one-launch layer tail: y32 identical to the plain mode, m16 / mp16 the level-major remap."""
    g = torch.Generator().manual_seed(9)
    B, C, FF = 2, 256, 1024
    shapes = [(8, 12), (16, 24), (32, 48)]
    starts, S = _levels(shapes)
    mk = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(dev)
    a16, x16 = mk(B, S, C).bfloat16(), mk(B, S, C).bfloat16()
    wo, bo, w1, b1, w2, b2 = mk(C, C, sc=0.05), mk(C, sc=0.1), mk(FF, C, sc=0.05), mk(FF, sc=0.1), mk(C, FF, sc=0.03), mk(C, sc=0.1)
    n0 = (mk(C, sc=0.2) + 1, mk(C, sc=0.1), 1e-5)
    n1 = (mk(C, sc=0.2) + 1, mk(C, sc=0.1), 1e-5)
    shift, pos = mk(S, C), mk(S, C)
    wop, w1p, w2p = ops.pack_linear_weight(wo), ops.pack_linear_weight(w1), ops.pack_linear_weight(w2)
    y32, m16, mp16 = ops.encoder_layer_tail(a16, x16, wop, bo, n0, w1p, b1, w2p, b2, n1, kv=(shift, pos, starts), want_f32=True)
    y_ref, _, _ = ops.encoder_layer_tail(a16, x16, wop, bo, n0, w1p, b1, w2p, b2, n1, want_f32=True, want_bf16=False)
    assert torch.equal(y32, y_ref)
    m = y_ref + shift[None]
    z = m + pos[None]
    want_m = torch.cat([m[:, s:s + h * w].reshape(-1, C) for s, (h, w) in zip(starts, shapes)], 0).bfloat16()
    want_z = torch.cat([z[:, s:s + h * w].reshape(-1, C) for s, (h, w) in zip(starts, shapes)], 0).bfloat16()
    assert torch.equal(m16, want_m) and torch.equal(mp16, want_z)


def test_encoder_proj_forms_x_plus_pos_in_kernel(dev):
    """xp16=None: the projection kernel forms bf16(x16 + pos16[row % N]) itself -- identical (bit for bit) to handing it the
    rows computed the same way by torch (bf16 + bf16 -> f32 add -> one bf16 rounding)."""
    g = torch.Generator().manual_seed(11)
    M, N, C, NC = 4071, 1357, 256, 288
    x16 = torch.randn(M, C, generator=g).to(dev).bfloat16()
    pos16 = torch.randn(N, C, generator=g).to(dev).bfloat16()
    wv = (torch.randn(256, C, generator=g) * 0.05).to(dev)
    wc = (torch.randn(NC, C, generator=g) * 0.05).to(dev)
    bv, bc = torch.randn(256, generator=g).to(dev), torch.randn(NC, generator=g).to(dev)
    wvp, wcp = ops.pack_encoder_proj_weight(wv), ops.pack_encoder_proj_weight(wc)
    xp16 = (x16.float() + pos16.repeat((M + N - 1) // N, 1)[:M].float()).bfloat16()
    v_a, o_a = ops.encoder_proj(x16, xp16, wvp, bv, wcp, bc)
    v_b, o_b = ops.encoder_proj(x16, None, wvp, bv, wcp, bc, pos16=pos16)
    assert torch.equal(v_a, v_b) and torch.equal(o_a, o_b)


@pytest.mark.parametrize('B,hw,n', [(2, 16384, 3), (2, 1024, 3), (1, 64, 1), (3, 4096, 2),
                                    (2, 1050, 3), (1, 4200, 3), (1, 16800, 3), (3, 1085, 2), (2, 37, 1)])   # ragged: configs[4] levels, odd hw
def test_decoder_kv_proj_fused_vs_float64(dev, B, hw, n):
    """Decoder K / V projections of one memory level in one launch: k = mp16 Wk^T + bk (row-major) and vt = Wv m16^T
    (transposed, straight from the swapped-operand MFMA tiles) against float64 on the same bf16-rounded operands: half a bf16
    ulp relative (2^-8 of max(|v|, 1)) + f32 accumulation noise; layouts exactly those of F.linear / torch.matmul."""
    g = torch.Generator().manual_seed(B * hw + n)
    C, NK = 256, 256 * n
    m16 = torch.randn(B, hw, C, generator=g).to(dev).bfloat16()
    mp16 = torch.randn(B, hw, C, generator=g).to(dev).bfloat16()
    wk = (torch.randn(NK, C, generator=g) * 0.05).to(dev)
    wv = (torch.randn(NK, C, generator=g) * 0.05).to(dev)
    bk = torch.randn(NK, generator=g).to(dev)
    k, vt = ops.decoder_kv_proj(m16, mp16, ops.pack_decoder_k_weight(wk), bk, ops.pack_linear_weight(wv))
    k2, vt2 = ops.decoder_kv_proj(m16, mp16, ops.pack_decoder_k_weight(wk), bk, ops.pack_linear_weight(wv))
    torch.cuda.synchronize()
    assert torch.equal(k, k2) and torch.equal(vt, vt2)
    assert k.shape == (B, hw, NK) and vt.shape == (B, NK, hw)
    rk = mp16.double() @ wk.bfloat16().double().t() + bk.double()
    rv = wv.bfloat16().double() @ m16.double().transpose(1, 2)
    assert ((k.double() - rk).abs() / rk.abs().clamp_min(1.0)).max().item() <= 2 ** -8 + 1e-4
    assert ((vt.double() - rv).abs() / rv.abs().clamp_min(1.0)).max().item() <= 2 ** -8 + 1e-4


def test_msda_head_major_value_path_is_bit_identical(dev):
    """Head-major value layout, (B, 8, N, 32), written by `encoder_proj(value_head_major=True)` and gathered by
    `msda_forward_fused_bf16(head_major=True)`: same arithmetic, different addresses -- both the projection output (after
    the permute) and the attention output are bit-identical to the row-layout path."""
    g = torch.Generator().manual_seed(3)
    B, C = 2, 256
    shapes = [(16, 24), (32, 48), (64, 96)]
    starts, N = _levels(shapes)
    x16 = torch.randn(B, N, C, generator=g).to(dev).bfloat16()
    pos16 = torch.randn(N, C, generator=g).to(dev).bfloat16()
    wv = (torch.randn(256, C, generator=g) * 0.05).to(dev)
    wc = torch.randn(288, C, generator=g).to(dev) * 0.05
    bv, bc = torch.randn(256, generator=g).to(dev) * 0.1, torch.randn(288, generator=g).to(dev) * 0.5
    wvp, wcp = ops.pack_encoder_proj_weight(wv), ops.pack_encoder_proj_weight(wc)
    ref_pts = torch.cat([torch.stack([(xs.flatten() + .5) / w, (ys.flatten() + .5) / h], -1)
                         for h, w in shapes
                         for ys, xs in [torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing='ij')]]).to(dev)
    v_rows, offs = ops.encoder_proj(x16, None, wvp, bv, wcp, bc, pos16=pos16)
    v_hm, offs2 = ops.encoder_proj(x16, None, wvp, bv, wcp, bc, pos16=pos16, value_head_major=True)
    assert torch.equal(offs, offs2)
    assert v_hm.shape == (B, 8, N, 32)
    assert torch.equal(v_hm.permute(0, 2, 1, 3).reshape(B, N, 256), v_rows)
    a = ops.msda_forward_fused_bf16(v_rows.view(B, N, 8, 32), shapes, starts, offs, ref_pts, 4)
    b = ops.msda_forward_fused_bf16(v_hm, shapes, starts, offs, ref_pts, 4, head_major=True)
    assert torch.equal(a, b)


@pytest.mark.parametrize('rows,bdt', [(344064, torch.bfloat16), (4071, torch.float32), (37, torch.bfloat16)])
def test_add_layernorm_train_forward_backward_vs_autograd(dev, rows, bdt):
    """One-pass LayerNorm(a + b) forward + backward (training encoder stream) against torch autograd of the same expression in
    float64: y and d/da within 2e-5 (f32 arithmetic), d/db the bf16 rounding of d/da for a bf16 b, dgamma / dbeta (sums over
    all rows) within 1e-4 relative to their scale; ragged row counts."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(rows)
    a = torch.randn(rows, 256, generator=g).to(dev).requires_grad_(True)
    b = (torch.randn(rows, 256, generator=g) * 0.5).to(dev).to(bdt).requires_grad_(True)
    norm = torch.nn.LayerNorm(256).to(dev)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(256, generator=g).to(dev) + 0.5)
        norm.bias.copy_(torch.randn(256, generator=g).to(dev) * 0.1)
    gy = torch.randn(rows, 256, generator=g).to(dev)
    assert ops.add_layernorm_train_ok(a, b, norm)
    y = ops.add_layernorm_train(a, b, norm)
    y.backward(gy)
    got = (y.detach(), a.grad.clone(), b.grad.clone(), norm.weight.grad.clone(), norm.bias.grad.clone())
    a64 = a.detach().double().requires_grad_(True)
    b64 = b.detach().double().requires_grad_(True)
    w64 = norm.weight.detach().double().requires_grad_(True)
    c64 = norm.bias.detach().double().requires_grad_(True)
    y64 = F.layer_norm(a64 + b64, (256,), w64, c64, norm.eps)
    y64.backward(gy.double())
    assert (got[0].double() - y64.detach()).abs().max().item() <= 2e-5
    assert (got[1].double() - a64.grad).abs().max().item() <= 2e-5 * max(1.0, a64.grad.abs().max().item())
    tol_b = 2 ** -8 if bdt == torch.bfloat16 else 2e-5
    assert ((got[2].double() - b64.grad).abs() / b64.grad.abs().clamp_min(1.0)).max().item() <= tol_b
    assert (got[3].double() - w64.grad).abs().max().item() <= 1e-4 * max(1.0, w64.grad.abs().max().item())
    assert (got[4].double() - c64.grad).abs().max().item() <= 1e-4 * max(1.0, c64.grad.abs().max().item())


def test_add_layernorm_train_bf16_outputs_and_their_gradients(dev):
    """The three-output form: (y, bf16(y), bf16(y + pos)) with gradients arriving on all three (f32, bf16, bf16) and flowing to
    a, b, gamma, beta AND the pos table (sum over the batch repeats) == torch autograd of the same graph in float64 up to the
    bf16 rounding of the two bf16 gradients' sum path (they are added in f32 inside the kernel: 2e-5) ."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5)
    B, N = 3, 1357
    a = torch.randn(B, N, 256, generator=g).to(dev).requires_grad_(True)
    b = (torch.randn(B, N, 256, generator=g) * 0.5).to(dev).bfloat16().requires_grad_(True)
    pos = torch.randn(N, 256, generator=g).to(dev).requires_grad_(True)
    norm = torch.nn.LayerNorm(256).to(dev)
    gy = torch.randn(B, N, 256, generator=g).to(dev)
    g16 = torch.randn(B, N, 256, generator=g).to(dev).bfloat16()
    gp16 = torch.randn(B, N, 256, generator=g).to(dev).bfloat16()
    y, y16, yp16 = ops.add_layernorm_train(a, b, norm, pos=pos, want_bf16=True, want_pos=True)
    torch.autograd.backward([y, y16, yp16], [gy, g16, gp16])
    a64, b64, p64 = (t.detach().double().requires_grad_(True) for t in (a, b, pos))
    w64, c64 = norm.weight.detach().double().requires_grad_(True), norm.bias.detach().double().requires_grad_(True)
    y64 = F.layer_norm(a64 + b64, (256,), w64, c64, norm.eps)
    torch.autograd.backward([y64, y64, y64 + p64[None]], [gy.double(), g16.double(), gp16.double()])
    assert (y.double() - y64).abs().max().item() <= 2e-5
    assert (y16.double() - y64).abs().max().item() <= 2 ** -6 and (yp16.double() - (y64 + p64[None])).abs().max().item() <= 2 ** -5
    assert (a.grad.double() - a64.grad).abs().max().item() <= 1e-4
    assert ((b.grad.double() - b64.grad).abs() / b64.grad.abs().clamp_min(1.0)).max().item() <= 2 ** -8
    assert (pos.grad.double() - p64.grad).abs().max().item() <= 1e-4
    assert (norm.weight.grad.double() - w64.grad).abs().max().item() <= 1e-3 and (norm.bias.grad.double() - c64.grad).abs().max().item() <= 1e-3


def test_msda_rows_function_matches_unfused_autograd(dev):
    """Training form of the MSDeformAttn core on the raw projection rows (prologue inside the kernels, forward and backward) ==
    the un-fused formulation (torch prologue recorded by autograd + MultiScaleDeformableAttnFunction): output and the gradients
    wrt value and the rows within 2e-5 relative to their scale (same kernels for the gather, f32 prologue arithmetic)."""
    g = torch.Generator().manual_seed(21)
    B, H, D, P = 2, 8, 32, 4
    shapes = [(6, 9), (12, 18), (24, 36)]
    starts, N = _levels(shapes)
    L = len(shapes)
    value = torch.randn(B, N, H, D, generator=g).to(dev).requires_grad_(True)
    rows = torch.randn(B, N, 3 * H * L * P, generator=g).to(dev)
    rows[..., :2 * H * L * P] *= 2.0
    rows.requires_grad_(True)
    ref_pts = torch.cat([torch.stack([(xs.flatten() + .5) / w, (ys.flatten() + .5) / h], -1)
                         for h, w in shapes
                         for ys, xs in [torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing='ij')]]).to(dev)
    gout = torch.randn(B, N, H * D, generator=g).to(dev)
    out = ops.MSDeformAttnRowsFunction.apply(value, rows, ref_pts, shapes, starts, P)
    out.backward(gout)
    got = (out.detach(), value.grad.clone(), rows.grad.clone())
    value.grad = None
    rows.grad = None
    n_off = H * L * P * 2
    offs = rows[..., :n_off].view(B, N, H, L, P, 2)
    aw = rows[..., n_off:].view(B, N, H, L * P).softmax(-1).view(B, N, H, L, P)
    norm = rows.new_tensor([[w, h] for h, w in shapes])
    loc = ref_pts[None, :, None, None, None, :] + offs / norm[None, None, None, :, None, :]
    ss = torch.tensor(shapes, dtype=torch.int64, device=dev)
    st = torch.tensor(starts, dtype=torch.int64, device=dev)
    ref_out = ops.MultiScaleDeformableAttnFunction.apply(value, ss, st, loc.contiguous(), aw.contiguous(), 64)
    ref_out.backward(gout)
    for a, b in zip(got, (ref_out.detach(), value.grad, rows.grad)):
        assert (a - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize('rows,H,W,P', [(37, 64, 96, 500), (5, 256, 256, 3000), (3, 50, 1000, 700)])
def test_point_sample_rows_forward_backward_vs_grid_sample(dev, rows, H, W, P):
    """Single-channel point sampling with the scatter backward == F.grid_sample (bilinear, zeros, align_corners=False) and
    its autograd on the same points, incl. points outside [0, 1] (zero padding): forward 1e-6, gradient 1e-5 (atomic order)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(17)
    # (backward: a workgroup per band of 16 384 / W plane rows in LDS -- one band, four bands, 16-row bands of a wide map)
    planes = torch.randn(rows, H, W, generator=g).to(dev).requires_grad_(True)
    pts = (torch.rand(rows, P, 2, generator=g) * 1.2 - 0.1).to(dev)
    gout = torch.randn(rows, P, generator=g).to(dev)
    assert ops.point_sample_rows_ok(planes, pts)
    out = ops.point_sample_rows(planes, pts)
    out.backward(gout)
    got_g = planes.grad.clone()
    planes.grad = None
    ref_out = F.grid_sample(planes.unsqueeze(1), (pts * 2.0 - 1.0).unsqueeze(2), align_corners=False).squeeze(3).squeeze(1)
    ref_out.backward(gout)
    assert (out - ref_out).abs().max().item() <= 1e-6 * max(1.0, ref_out.abs().max().item())
    assert (got_g - planes.grad).abs().max().item() <= 1e-5 * max(1.0, planes.grad.abs().max().item())
    # the dispatch inside assigner.point_sample takes the same path and keeps the (N, 1, P) contract
    from cgg_amd.assigner import point_sample
    o2 = point_sample(planes.detach().unsqueeze(1), pts)
    assert o2.shape == (rows, 1, P) and torch.equal(o2[:, 0], out.detach())


@pytest.mark.parametrize('B,H,W', [(2, 256, 256), (1, 8, 16), (1, 24, 48)])
def test_bottleneck64_fused_vs_float64(dev, B, H, W):
    """ResNet layer1 identity Bottleneck in one launch against float64 convolutions on the same bf16 operands with the same bf16
    rounding points (t1, t2 rounded to bf16 like the three-call path): the output is bf16, so half an ulp of max(|y|, 1) (2^-8
    relative) plus the effect of a t1 / t2 element landing on the other side of a bf16 rounding boundary (bounded by 0.03 absolute
    for these operand scales); borders (zero padding of t1, not of x) included; two runs bit-identical."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(B * H + W)
    x = (torch.randn(B, H, W, 256, generator=g) * 0.7).to(dev).bfloat16()
    w1 = (torch.randn(64, 256, generator=g) * 0.06).to(dev).bfloat16()
    w2 = (torch.randn(64, 64, 3, 3, generator=g) * 0.05).to(dev).bfloat16()
    w3 = (torch.randn(256, 64, generator=g) * 0.1).to(dev).bfloat16()
    b1, b2, b3 = (torch.randn(n, generator=g).to(dev).bfloat16() * 0.2 for n in (64, 64, 256))
    packed = ops.pack_bottleneck64(w1, b1, w2, b2, w3, b3)
    assert ops.bottleneck64_ok(x)
    y = ops.bottleneck64(x, packed)
    y2 = ops.bottleneck64(x, packed)
    torch.cuda.synchronize()
    assert torch.equal(y, y2)
    xd = x.double().permute(0, 3, 1, 2)
    t1 = F.relu(F.conv2d(xd, w1.double().view(64, 256, 1, 1), b1.double())).bfloat16().double()
    t2 = F.relu(F.conv2d(t1, w2.double(), b2.double(), padding=1)).bfloat16().double()
    ref64 = F.relu(F.conv2d(t2, w3.double().view(256, 64, 1, 1), b3.double()) + xd).permute(0, 2, 3, 1)
    err = (y.double() - ref64).abs()
    assert (err / ref64.abs().clamp_min(1.0)).max().item() <= 0.03
    assert (err / ref64.abs().clamp_min(1.0)).mean().item() <= 2e-3


@pytest.mark.parametrize('B,Q,S,H', [(2, 100, 1050, 8), (1, 33, 16384, 8), (2, 100, 100, 8)])
def test_masked_xattn_training_kernels_on_bf16_mfma_operands(dev, B, Q, S, H):
    """Throughput-mode training: `cgg_masked_xattn_forward_lse` / `cgg_masked_xattn_backward` with kv_dtype CGG_F32_BF16MFMA (f32 rows
    in memory, products on bf16 MFMA operands, f32 accumulation) against float64 autograd of the same formulation: bf16 operand
    rounding (2^-9 per factor) bounds the error -- output and gradients within 2e-2 of their scale, cosine > 0.9999."""
    from cgg_amd import runtime
    from cgg_amd.query_decoder import pack_bool_mask
    g = torch.Generator().manual_seed(31 + S)
    D = 32
    E = H * D
    q = torch.randn(B, Q, E, generator=g)
    kv = torch.randn(B, S, 2 * E, generator=g)
    go = torch.randn(B, Q, E, generator=g)
    mask = torch.rand(B, Q, S, generator=g) < 0.6
    mask[0, 1] = False
    qd, kvd = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    qh = (qd * D**-0.5).view(B, Q, H, D).transpose(1, 2)
    kh = kvd[..., :E].view(B, S, H, D).transpose(1, 2)
    vh = kvd[..., E:].view(B, S, H, D).transpose(1, 2)
    att = (qh @ kh.transpose(-1, -2)).masked_fill(mask[:, None], float('-inf'))
    want = (att.softmax(-1) @ vh).transpose(1, 2).reshape(B, Q, E)
    wgq, wgkv = torch.autograd.grad(want, (qd, kvd), go.double())
    bits = pack_bool_mask(mask).contiguous().to(dev)
    with runtime.precision_scope('bf16'):
        assert ops._xattn_train_dtype() == ops.CGG_F32_BF16MFMA
        out, lse = ops.masked_xattn(q.to(dev), kv.to(dev), bits, H, return_lse=True)
        gq, gkv = ops.masked_xattn_backward(q.to(dev), kv.to(dev), bits, out, lse, go.to(dev), H)
    with runtime.precision_scope('fp32'):
        assert ops._xattn_train_dtype() == 0
    for got, ref_, name in ((out, want.detach(), 'out'), (gq, wgq, 'grad_q'), (gkv, wgkv, 'grad_kv')):
        gd = got.cpu().double()
        scale = ref_.abs().max().item()
        assert (gd - ref_).abs().max().item() <= 2e-2 * scale, (name, (gd - ref_).abs().max().item(), scale)
        cos = float((gd * ref_).sum() / (gd.norm() * ref_.norm()))
        assert cos > 0.9999, (name, cos)


@pytest.mark.parametrize('B,Q,S,H', [(2, 100, 1050, 8), (1, 33, 16384, 8), (2, 100, 100, 8)])
def test_masked_xattn_parity_training_forward_on_x3_saves_the_same_rows(dev, B, Q, S, H):
    """Parity-mode training: `cgg_masked_xattn_forward_lse` with kv_dtype CGG_F32_X3 (the inference kernel of csrc/xattn_x3.hip, one
    chunk or combined) writes the output AND the natural-log log-sum-exp rows; with the exact-f32-MFMA backward on top, output, rows
    and both gradients stay f32-class against float64 autograd (1e-5 / 1e-4 of scale)."""
    from cgg_amd import runtime
    from cgg_amd.query_decoder import pack_bool_mask
    g = torch.Generator().manual_seed(77 + S)
    D = 32
    E = H * D
    q = torch.randn(B, Q, E, generator=g)
    kv = torch.randn(B, S, 2 * E, generator=g)
    go = torch.randn(B, Q, E, generator=g)
    mask = torch.rand(B, Q, S, generator=g) < 0.6
    mask[0, 1] = False
    qd, kvd = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    qh = (qd * D**-0.5).view(B, Q, H, D).transpose(1, 2)
    kh = kvd[..., :E].view(B, S, H, D).transpose(1, 2)
    vh = kvd[..., E:].view(B, S, H, D).transpose(1, 2)
    att = (qh @ kh.transpose(-1, -2)).masked_fill(mask[:, None], float('-inf'))
    want = (att.softmax(-1) @ vh).transpose(1, 2).reshape(B, Q, E)
    want_lse = att.logsumexp(-1).detach()                     # (B, H, Q)
    wgq, wgkv = torch.autograd.grad(want, (qd, kvd), go.double())
    bits = pack_bool_mask(mask).contiguous().to(dev)
    with runtime.precision_scope('fp32'):
        assert ops._xattn_train_dtype(forward=True) == ops.CGG_F32_X3 and ops._xattn_train_dtype() == 0
        out, lse = ops.masked_xattn(q.to(dev), kv.to(dev), bits, H, return_lse=True)
        gq, gkv = ops.masked_xattn_backward(q.to(dev), kv.to(dev), bits, out, lse, go.to(dev), H)
    assert (lse.cpu().double() - want_lse).abs().max().item() <= 1e-5 * max(1.0, want_lse.abs().max().item())
    for got, ref_, name, tol in ((out, want.detach(), 'out', 1e-5), (gq, wgq, 'grad_q', 1e-4), (gkv, wgkv, 'grad_kv', 1e-4)):
        gd = got.cpu().double()
        scale = ref_.abs().max().item()
        assert (gd - ref_).abs().max().item() <= tol * scale, (name, (gd - ref_).abs().max().item(), scale)
