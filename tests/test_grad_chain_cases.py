"""tests/grad_chain_cases.py before it meets a kernel. CPU only.

EXACT -- for every case: the pre-scaled operands are exact f16 values with empty low pieces (normal or, for p = -118, subnormal), the
contraction sums stay below 2^24 units, the float64 reference equals f32 matmuls in two different summation orders and survives the
power-of-two un-scale, and the LayerNorm splits add up without rounding.

RULES -- `x3_scale`, the tile template per GEMM case, the split plan per weight-gradient case, and the epilogue forms reached.

TEETH -- host restatements of four faults (mask test `>=`, maximum taken over clamped rows, column sums taken over clamped rows,
a pre-scale without its un-scale) each change the result of a named case."""
import math

import pytest
import torch

import grad_chain_cases as GC

GEMM_NAMES = list(GC.GEMM_SPECS)
WGRAD_CASES = [(M, N, K) for N, K in GC.WGRAD_NK for M in GC.WGRAD_M]


def _fits_f16_with_empty_low_piece(a, s):
    hi, lo = GC.split_pieces(a, s)
    return torch.equal(hi, a.double() * s) and not lo.any() and torch.isfinite(hi).all()


def _two_orders_f32(a, b):
    """a b^T in f32: the library's order, and chunks of 8 contraction indices taken from the far end, accumulated one by one"""
    first = a @ b.t()
    acc = torch.zeros_like(first)
    for k1 in range(a.shape[1], 0, -8):
        k0 = max(0, k1 - 8)
        acc = acc + a[:, k0:k1].flip(1) @ b[:, k0:k1].flip(1).t()
    return first, acc


# ------------------------------------------------------------------------------------------------
# RULES
# ------------------------------------------------------------------------------------------------
def test_x3_scale_follows_the_definition():
    for e in (-126, -100, -92, -91, -30, -1, 0, 1, 9, 10, 50, 108, 109, 110, 127):
        want = 2.0 ** max(-100, min(100, 9 - e))
        assert GC.x3_scale(2.0 ** e) == want, e
        assert GC.x3_scale(-(2.0 ** e)) == want, e                                  # the sign bit is not part of the exponent field
        assert GC.x3_scale(2.0 ** e * (2 - 2.0 ** -23)) == want, e                  # largest value with this exponent
        if e > -126:
            below = 2.0 ** e * (1 - 2.0 ** -24)                                     # one ulp below the power of two
            assert GC.x3_scale(below) == 2.0 ** max(-100, min(100, 10 - e)), e
    assert GC.x3_scale(0.0) == 16.0 and GC.x3_scale(-0.0) == 16.0
    assert GC.x3_scale(2.0 ** -127) == 16.0 and GC.x3_scale(2.0 ** -149) == 16.0    # denormal: exponent field 0
    assert GC.x3_scale(math.inf) == 16.0 and GC.x3_scale(math.nan) == 16.0          # exponent field 255
    assert GC.x3_scale(15.0) == 2.0 ** 6 and GC.x3_scale(15 * 2.0 ** -110) == 2.0 ** 100 and GC.x3_scale(15 * 2.0 ** 40) == 2.0 ** -34


@pytest.mark.parametrize('name', GEMM_NAMES)
def test_gemm_case_selects_its_tile_template(name):
    M, N, K, want = GC.GEMM_SPECS[name]
    assert GC.xg_tiles(M, N) == want
    assert K % 32 == 0 and K * 225 < 2 ** 24


def test_every_template_and_every_epilogue_form_is_reached():
    assert {GC.GEMM_SPECS[n][3] for n in GEMM_NAMES} == {(2, 2), (1, 2), (2, 1), (1, 1)}
    assert (12200 + 127) // 128 == 96 and 12200 - 95 * 128 == 40
    assert {GC.GEMM_SPECS[n][2] // 32 for n in GEMM_NAMES} >= {1, 3, 9}             # one chunk, odd chunk counts
    forms = {n: GC.xg_tile_forms(*GC.GEMM_SPECS[n][:2]) for n in GEMM_NAMES}
    assert forms['t22'] == {'interior', 'ragged_m'} and forms['t12'] == {'interior', 'ragged_m'}
    assert forms['t21'] == {'ragged_n', 'ragged_m'}                                 # N = 36 inside a 64-wide tile: no interior tile
    assert forms['t11'] == {'interior', 'ragged_m', 'ragged_n'}
    assert forms['t11_one_row'] == {'ragged_m', 'ragged_n'} and forms['t11_interior'] == {'interior'}
    # smallest shapes: one row or one column less no longer selects the template
    assert GC.xg_tiles(12160, 256) != (2, 2) and GC.xg_tiles(6080, 256) != (1, 2) and GC.xg_tiles(24448, 36) != (2, 1)


def test_wgrad_plans():
    kinds = {(M, N, K): GC.wgrad_split_kind(M, N, K) for M, N, K in WGRAD_CASES}
    for N, K in GC.WGRAD_NK:
        assert GC.wgrad_tile(N, K) == (256 if (N, K) == (256, 256) else 128)
        got = {M: kinds[M, N, K] for M in GC.WGRAD_M}
        assert got == {1: 'one', 31: 'one', 32: 'one', 33: 'one', 256: 'one', 257: 'ragged', 300: 'ragged', 512: 'full', 1000: 'ragged'}
    assert GC.wgrad_plan(257, 256, 256) == (2, 160) and GC.wgrad_plan(300, 36, 68) == (2, 160)
    assert GC.wgrad_plan(512, 128, 128) == (2, 256) and GC.wgrad_plan(1000, 288, 256) == (4, 256)      # last split: 232 = 7 x 32 + 8 rows
    assert max(GC.WGRAD_M) <= GC.M_CAP_WGRAD and GC.M_CAP_WGRAD * 225 * 8 < 2 ** 24 <= (GC.M_CAP_WGRAD + 1) * 225 * 8
    # row counts under one 32-row chunk, at it, over it
    assert {1, 31, 32, 33} <= set(GC.WGRAD_M)


# ------------------------------------------------------------------------------------------------
# EXACT: operands
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,K', [(256, 32), (36, 32), (100, 32), (32, 32), (100, 96), (256, 288), (32, 256), (160, 256)])
def test_weights_pack_with_row_scale_2_7_both_ways(N, K):
    w = GC.weight(N, K, 12)
    assert w.abs().max() <= 15 and torch.equal(w, w.round())
    for m in (w, w.t()):
        top = m.abs().max(1).values
        assert (top >= 8).all() and (top < 16).all()                                # frexp exponent 4 -> row scale 2^(11 - 4)
        assert torch.equal((m * 128).half().float(), m * 128)


@pytest.mark.parametrize('p', GC.P_ALL + (None,))
@pytest.mark.parametrize('name', ['t11', 't22', 't11_one_row'])
def test_gemm_operands_fit_f16(name, p):
    c = GC.gemm_case(name, p)
    s = GC.x3_scale(c.amax)
    if p is None:
        assert c.amax == 0.0 and s == 16.0
    else:
        assert c.amax == 15 * 2.0 ** p and s == 2.0 ** max(-100, min(100, 6 - p))
        tiny = torch.finfo(torch.float32).tiny
        assert c.g[c.g != 0].abs().min() >= tiny and c.ref64[c.ref64 != 0].abs().min() >= tiny      # no f32 denormal anywhere
    assert _fits_f16_with_empty_low_piece(c.g, s)
    t = c.g.double() * s
    if p == GC.P_SUBNORMAL:
        assert t.abs().max() < 2.0 ** -14 and torch.equal(t * 2.0 ** 24, (t * 2.0 ** 24).round())     # the f16 subnormal grid
    elif p is not None:
        assert t[t != 0].abs().min() >= 2.0 ** -14                                                    # normal f16, p = -110 included
    assert _fits_f16_with_empty_low_piece(c.mask, 16.0) and _fits_f16_with_empty_low_piece(c.res, 16.0)


@pytest.mark.parametrize('p', GC.P_ALL + (None,))
@pytest.mark.parametrize('M,N,K', [(1000, 36, 68), (257, 256, 256), (1, 128, 128)])
def test_wgrad_operands_fit_f16(M, N, K, p):
    c = GC.wgrad_case(M, N, K, p)
    assert _fits_f16_with_empty_low_piece(c.dy, GC.x3_scale(c.amax)) and _fits_f16_with_empty_low_piece(c.x, 16.0)
    assert c.amax == (0.0 if p is None else 15 * 2.0 ** p)


# ------------------------------------------------------------------------------------------------
# EXACT: sums
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,variant', [(n, 'plain') for n in GEMM_NAMES] + [(n, v) for n in GC.GEMM_RAGGED_M for v in GC.VARIANTS[1:]])
def test_gemm_reference_is_exact(name, variant):
    c = GC.gemm_case(name, 0, variant)
    first, second = _two_orders_f32(c.g, c.w)
    assert torch.equal(first.double(), c.ref64) and torch.equal(second.double(), c.ref64)
    unit = 2.0 ** -3
    bound = (c.g.double().abs() @ c.w.double().abs().t()).max().item() / unit
    assert bound <= c.K * 225 * 8 < 2 ** 24
    assert torch.equal(c.ref64.float().double(), c.ref64)
    assert torch.equal((c.ref64 + c.res.double()).float().double(), c.ref64 + c.res.double())           # gemm_x3(res=)
    # the mask really has every kind of entry, and each kind meets a non-zero product
    h, live = c.mask, c.ref64 != 0
    neg0 = (h == 0) & torch.signbit(h)
    if c.M > 1:
        for kind in (h > 0, h < 0, (h == 0) & ~torch.signbit(h), neg0):
            assert (kind & live).any()
    if c.M > 61:
        assert not h[3].any() and not h[:, 5].any()
    if variant == 'plain' and c.M > 1:
        assert (h[c.M - 1] > 0).any() and (h[0] > 0).any()
    top = c.ref_masked64.abs().max().item()
    last = c.ref_masked64[c.M - 1].abs().max().item()
    if variant == 'last_row_max':
        assert last == top and c.ref_masked64[:c.M - 1].abs().max().item() < top                          # the maximum is in row M - 1 alone
        assert c.ref64[c.M - 1].abs().max().item() == c.ref64.abs().max().item() > c.ref64[:c.M - 1].abs().max().item()
    if variant == 'masked_last_row':
        assert last == 0 and c.ref64[c.M - 1].abs().max().item() > top                                 # would dominate if counted
        assert (c.mask_tall[c.M:] > 0).all() and torch.equal(c.mask_tall[:c.M], c.mask)


@pytest.mark.parametrize('p', GC.P_ALL)
def test_gemm_reference_scales_exactly(p):
    c0, c = GC.gemm_case('t11', 0), GC.gemm_case('t11', p)
    assert torch.equal(c.g.double(), c0.g.double() * 2.0 ** p) and torch.equal(c.ref64, c0.ref64 * 2.0 ** p)
    assert torch.equal(c.ref64.float().double(), c.ref64)


@pytest.mark.parametrize('M,N,K', WGRAD_CASES)
def test_wgrad_reference_is_exact(M, N, K):
    c = GC.wgrad_case(M, N, K)
    first, second = _two_orders_f32(c.dy.t().contiguous(), c.x.t().contiguous())
    assert torch.equal(first.double(), c.dw64) and torch.equal(second.double(), c.dw64)
    assert (c.dy.double().abs().t() @ c.x.double().abs()).max().item() / 2.0 ** -3 <= M * 225 * 8 < 2 ** 24
    assert torch.equal(c.dy.sum(0).double(), c.db64) and torch.equal(c.dy.flip(0).sum(0).double(), c.db64)
    for p in (GC.P_CLAMP, 40):
        cp = GC.wgrad_case(M, N, K, p)
        assert torch.equal(cp.dw64, c.dw64 * 2.0 ** p) and torch.equal(cp.dw64.float().double(), cp.dw64)
        assert torch.equal(cp.db64, c.db64 * 2.0 ** p) and torch.equal(cp.db64.float().double(), cp.db64)


@pytest.mark.parametrize('p', GC.CHAIN_P)
def test_chain_is_exact(p):
    k = GC.chain_case(p)
    dh = k.dh64.float()
    assert torch.equal(dh.double(), k.dh64) and k.amax_h == dh.abs().max().item() > 0
    s = GC.x3_scale(k.amax_h)
    hi, lo = GC.split_pieces(dh, s)
    assert torch.equal(hi + lo, k.dh64 * s)                                       # the two pieces hold it exactly
    assert not lo.any() or lo[lo != 0].abs().min() >= 2.0 ** -14                  # ... the low one, where in use, as a normal f16
    unit = 2.0 ** p
    assert (k.dh64.abs().t() @ k.x.double().abs()).max().item() / unit < 2 ** 24
    first, second = _two_orders_f32(dh.t().contiguous(), k.x.t().contiguous())
    assert torch.equal(first.double(), k.dw1) and torch.equal(second.double(), k.dw1)
    assert torch.equal(k.db1.float().double(), k.db1)


@pytest.mark.parametrize('mag', [1.0, 1e-3, 1e-5, 3e-7, 100.0])
def test_selector_selects(mag):
    c = GC.selector_case(300, 36, 68, mag)
    assert torch.equal(c.x.sum(0), torch.ones(68)) and set(c.x.unique().tolist()) == {0.0, 1.0}
    assert torch.equal(c.dy.double().t() @ c.x.double(), c.dy[c.rows].double().t())
    for s in (16.0, GC.x3_scale(float(c.dy.abs().max()))):
        assert torch.isfinite(GC.selector_ref(c, s)).all()


# ------------------------------------------------------------------------------------------------
# EXACT: LayerNorm operands
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', GC.LN_ROWS)
def test_layernorm_operands_add_without_rounding(rows):
    c = GC.ln_case(rows)
    assert torch.equal(c.b.bfloat16().float(), c.b)
    assert torch.equal(c.a.double() + c.b.double(), c.s.double()) and torch.equal(c.a + c.b, c.s)         # a + b == s exactly
    for d in (c.d32, c.d16a, c.d16b, c.dy):
        assert torch.equal(d * 64, (d * 64).round()) and d.abs().max() < 12
    for d in (c.d32, c.d16a, c.d16b):
        assert torch.equal(d.bfloat16().float(), d) and d.abs().max() < 4
        if rows > 1:
            assert d[rows - 1].abs().min() >= 2 * d[:rows - 1].abs().max()
    sum64 = c.d32.double() + c.d16a.double() + c.d16b.double()
    assert torch.equal(c.dy.double(), sum64) and torch.equal(((c.d16b + c.d16a) + c.d32).double(), sum64)
    assert {1, 255, 256, 257} <= set(GC.LN_ROWS) and 513 % 256 == 1                  # a last workgroup with one live row


# ------------------------------------------------------------------------------------------------
# TEETH
# ------------------------------------------------------------------------------------------------
def test_faults_change_named_cases():
    c = GC.gemm_case('t11', 0)
    ge = torch.where(c.mask >= 0, c.ref64, torch.zeros((), dtype=torch.float64))
    assert not torch.equal(ge, c.ref_masked64)                                          # `>= 0`: the +-0.0 entries let products through
    ragged = c.mask[64:] == 0
    assert (ge[64:][ragged] != 0).any()                                                 # ... in the ragged row tile too
    for name in GC.GEMM_RAGGED_M:                                                       # maximum over the clamped rows of the last tile
        k = GC.gemm_case(name, 0, 'masked_last_row')
        dup = torch.where(k.mask_tall[k.M] > 0, k.ref64[k.M - 1], torch.zeros((), dtype=torch.float64))
        assert dup.abs().max().item() > k.ref_masked64.abs().max().item()
    for rows in (17, 257, 513):                                                         # column sums over the clamped rows
        n = GC.ln_case(rows)
        pad = -rows % 4
        assert pad > 0
        shifted = n.dy.double().sum(0) + pad * n.dy[rows - 1].double()
        assert ((shifted - n.dy.double().sum(0)).abs() > 1.0).all()
    w = GC.wgrad_case(33, 36, 68)
    assert not torch.equal(w.dw64 * 2, w.dw64)                                          # a pre-scale without its un-scale: a factor of 2
