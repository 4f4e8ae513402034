"""The training backward chain of parity mode on the exact operands of tests/grad_chain_cases.py (whose docstring derives every
exactness condition; the cases are proven on the CPU by tests/test_grad_chain_cases.py). Parts 1, 2 and the chain of part 4 assert
every bit (`torch.equal`); part 3 asserts bit identities between the kernel's forms plus the float64 bound of
tests/test_norm_conditioning_gpu.py (`_grad_check`, imported); the nodes of part 4 keep the bound of
tests/test_x3s_gpu.py::test_x3_training_ffn_node_vs_float64. Kernels reached, per test:

  test_gemm_x3_bwd_templates        cgg_absmax_f32, cgg_x3_pack -> cgg_gemm_x3_bwd: cgg_gemm_x3_kernel<false, TM, TN> for all four
                                    (TM, TN); mask absent / present x out_amax off / on; an all-zero mask; K = 32, 96, 288
  test_gemm_x3_bwd_amax_at_row_edge cgg_gemm_x3_bwd: the maximum in the last live row; a dominating row M - 1 under a zero mask row,
                                    with live mask and output rows behind row M - 1
  test_gemm_x3_bwd_strided          cgg_absmax_f32 (strided), cgg_gemm_x3_bwd with g, mask and out as column slices; guard columns
  test_gemm_x3_bwd_scale_range      cgg_gemm_x3_bwd at p = -40 .. +40, the clamped exponents of p = -110 and -118, and all-zero g
  test_gemm_x3_residual_in_place    cgg_gemm_x3_scaled with res, out of place and with out = res (interior tiles; ragged tiles)
  test_wgrad_x3_scaled_edges        cgg_wgrad_x3_scaled: cgg_wgrad_x3_kernel<256> / <128>, with and without ws_bias, dense and strided
  test_wgrad_x3_scaled_scale_range  cgg_wgrad_x3_scaled at every p, and all-zero dy
  test_wgrad_x3_split_of_dy         cgg_wgrad_x3_scaled / cgg_wgrad_x3: the in-kernel split of dy through a one-hot x
  test_add_layernorm_backward_forms cgg_add_layernorm_backward / _amax: <float> and <uint16_t> b, b absent, dy / dy16a / dy16b, dx16
  test_add_layernorm_backward_vs_float64   the same, against float64 autograd of F.layer_norm
  test_ffn_nodes_at_ragged_rows     runtime._X3FfnFn, runtime._X3FfnBlockFn at M = 303: the whole chain
  test_chain_hands_amax_on          cgg_gemm_x3_bwd (out_amax) -> cgg_wgrad_x3_scaled (dy_amax), and the dW2 / db2 call beside it"""
import functools

import pytest
import torch
import torch.nn.functional as F

import grad_chain_cases as GC
from cgg_amd import ops, runtime
from test_norm_conditioning_gpu import _grad_check

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5


def _bits(t):
    return t.detach().reshape(-1).contiguous().view(torch.int32)


def _assert_is_max_of(amax, t, what):
    """the device scalar holds max |t| of the RETURNED tensor, bit for bit"""
    assert amax.shape == (1,) and amax.dtype == torch.float32
    assert torch.equal(_bits(amax), _bits(t.abs().max())), f'{what}: out_amax {amax.item()!r} != max |out| {t.abs().max().item()!r}'


def _assert_equal(got, want64, what):
    want = want64.float()
    assert torch.equal(want.double(), want64), f'{what}: the reference is not an f32'
    got = got.detach().cpu()
    if not torch.equal(got, want):
        bad = (got != want) | (got != got)
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {i}: {got[i].item()!r} != {want[i].item()!r}')


@functools.lru_cache(maxsize=None)
def _image(name, dev):
    return ops.pack_linear_weight_x3(GC.gemm_case(name).w.to(dev))


# ------------------------------------------------------------------------------------------------
# 1. gemm_x3_bwd
# ------------------------------------------------------------------------------------------------
def _run_bwd(c, img, g, amax, mask, want_amax, what, out=None):
    got, oa = ops.gemm_x3_bwd(g, img, c.N, amax=amax, mask=mask, out=out, want_amax=want_amax)
    assert (oa is not None) == want_amax
    _assert_equal(got, c.ref_masked64 if mask is not None else c.ref64, what)
    if mask is not None:
        assert not got[mask <= 0].any(), f'{what}: not zero where mask <= 0'
    if want_amax:
        _assert_is_max_of(oa, got, what)
        assert oa.item() == (c.ref_masked64 if mask is not None else c.ref64).abs().max().item()
    return got, oa


@pytest.mark.parametrize('name', list(GC.GEMM_SPECS))
def test_gemm_x3_bwd_templates(dev, name):
    c = GC.gemm_case(name)
    img, g, h = _image(name, dev), c.g.to(dev), c.mask.to(dev)
    amax = ops.absmax(g)
    assert amax.item() == c.amax
    for use_mask in (False, True):
        for want_amax in (False, True):
            _run_bwd(c, img, g, amax, h if use_mask else None, want_amax, f'{name} mask={use_mask} want_amax={want_amax}')
    # an all-zero mask (both signs of zero): zeros out, maximum 0
    zero = torch.where(h > 0, 0.0, -0.0)
    assert not zero.any() and torch.signbit(zero).any()
    got, oa = ops.gemm_x3_bwd(g, img, c.N, amax=amax, mask=zero, want_amax=True)
    assert not got.any() and _bits(oa).item() == 0


@pytest.mark.parametrize('variant', GC.VARIANTS[1:])
@pytest.mark.parametrize('name', GC.GEMM_RAGGED_M)
def test_gemm_x3_bwd_amax_at_row_edge(dev, name, variant):
    """rows past M read row M - 1 and must count for nothing: the mask and the output are the first M rows of taller buffers whose
    other rows are a live mask (all positive) and a sentinel that must survive"""
    c = GC.gemm_case(name, 0, variant)
    img, g = _image(name, dev), c.g.to(dev)
    tall_mask = c.mask_tall.to(dev)
    tall_out = torch.full((c.M + 160, c.N), SENTINEL, device=dev)
    amax = ops.absmax(g)
    what = f'{name} {variant}'
    got, oa = _run_bwd(c, img, g, amax, tall_mask[:c.M], True, what, out=tall_out[:c.M])
    assert (tall_out[c.M:] == SENTINEL).all(), f'{what}: stored past row M'
    top = c.ref_masked64.abs().max().item()
    if variant == 'last_row_max':
        assert oa.item() == top == c.ref_masked64[c.M - 1].abs().max().item()
    else:
        assert oa.item() == top < c.ref64[c.M - 1].abs().max().item() and not got[c.M - 1].any()
    _run_bwd(c, img, g, amax, None, True, what + ' no mask')          # without the mask the last row does hold the maximum
    _run_bwd(c, img, g, amax, tall_mask[:c.M], False, what + ' want_amax off')


@pytest.mark.parametrize('name', ['t11', 't22', 't21'])
def test_gemm_x3_bwd_strided(dev, name):
    c = GC.gemm_case(name)
    M, N, K = c.M, c.N, c.K
    gw = torch.full((M, K + 8), 7.0, device=dev)
    mw = torch.full((M, N + 12), 1.0, device=dev)
    ow = torch.full((M, N + 8), SENTINEL, device=dev)
    g, h, out = gw[:, 4:4 + K], mw[:, 8:8 + N], ow[:, 4:4 + N]
    g.copy_(c.g)
    h.copy_(c.mask)
    for t in (g, h, out):
        assert t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 and not t.is_contiguous()
    amax = ops.absmax(g)
    assert amax.item() == c.amax
    for use_mask in (False, True):
        ow.fill_(SENTINEL)
        got, _ = _run_bwd(c, _image(name, dev), g, amax, h if use_mask else None, True, f'{name} strided mask={use_mask}', out=out)
        assert got.data_ptr() == out.data_ptr()
        assert (ow[:, :4] == SENTINEL).all() and (ow[:, 4 + N:] == SENTINEL).all(), f'{name}: stored outside the column slice'


@pytest.mark.parametrize('p', GC.P_ALL + (None,), ids=lambda p: f'p{p}')
@pytest.mark.parametrize('name', ['t11', 't12'])
def test_gemm_x3_bwd_scale_range(dev, name, p):
    c = GC.gemm_case(name, p)
    img, g, h = _image(name, dev), c.g.to(dev), c.mask.to(dev)
    amax = ops.absmax(g)
    assert amax.item() == c.amax == (0.0 if p is None else 15 * 2.0 ** p)
    for use_mask in (False, True):
        got, oa = _run_bwd(c, img, g, amax, h if use_mask else None, True, f'{name} p={p} mask={use_mask}')
        assert torch.isfinite(got).all()
        if p is None:
            assert not got.any() and _bits(oa).item() == 0


@pytest.mark.parametrize('name', ['t11_interior', 't11', 't22'])
def test_gemm_x3_residual_in_place(dev, name):
    """gemm_x3(g, W^T, res=r, amax=): the fan-in of two gradient paths in the epilogue, out of place and with out = r (the form
    `runtime._X3MsdaBlockFn` uses): both the float64 result, hence each other"""
    c = GC.gemm_case(name)
    img, g, r = _image(name, dev), c.g.to(dev), c.res.to(dev)
    amax = ops.absmax(g)
    want = c.ref64 + c.res.double()
    apart = ops.gemm_x3(g, img, c.N, res=r, amax=amax)
    _assert_equal(apart, want, f'{name} res out of place')
    assert torch.equal(r.cpu(), c.res)
    inplace = r.clone()
    back = ops.gemm_x3(g, img, c.N, res=inplace, out=inplace, amax=amax)
    assert back.data_ptr() == inplace.data_ptr()
    _assert_equal(inplace, want, f'{name} res in place')
    assert torch.equal(inplace, apart)


# ------------------------------------------------------------------------------------------------
# 2. wgrad_x3, scaled
# ------------------------------------------------------------------------------------------------
def _run_wgrad(c, dy, x, what):
    amax = ops.absmax(dy)
    assert amax.item() == c.amax
    dw, db = ops.wgrad_x3(dy, x, want_bias=True, amax=amax)
    alone = ops.wgrad_x3(dy, x, want_bias=False, amax=amax)
    assert tuple(dw.shape) == (c.N, c.K) and tuple(db.shape) == (c.N,)
    _assert_equal(dw, c.dw64, f'{what} dW')
    _assert_equal(db, c.db64, f'{what} db')
    _assert_equal(alone, c.dw64, f'{what} dW without the bias sum')
    return dw, db


@pytest.mark.parametrize('M', GC.WGRAD_M)
@pytest.mark.parametrize('N,K', GC.WGRAD_NK)
def test_wgrad_x3_scaled_edges(dev, N, K, M):
    c = GC.wgrad_case(M, N, K)
    what = f'wgrad M={M} N={N} K={K} ({GC.wgrad_split_kind(M, N, K)})'
    _run_wgrad(c, c.dy.to(dev), c.x.to(dev), what)
    dy_w = torch.full((M, N + 8), 3.0, device=dev)              # strided rows, x 16 B into its row (as test_wgrad_x3_vs_float64)
    x_w = torch.full((M, K + 4), 5.0, device=dev)
    dy_w[:, :N] = c.dy.to(dev)
    x_w[:, 4:] = c.x.to(dev)
    _run_wgrad(c, dy_w[:, :N], x_w[:, 4:], what + ' strided')


@pytest.mark.parametrize('p', GC.P_ALL + (None,), ids=lambda p: f'p{p}')
@pytest.mark.parametrize('M,N,K', [(1000, 36, 68), (257, 256, 256), (33, 288, 256)])
def test_wgrad_x3_scaled_scale_range(dev, M, N, K, p):
    c = GC.wgrad_case(M, N, K, p)
    dw, db = _run_wgrad(c, c.dy.to(dev), c.x.to(dev), f'wgrad M={M} N={N} K={K} p={p}')
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    if p is None:
        assert not dw.any() and not db.any()


@pytest.mark.parametrize('mag', [1.0, 1e-3, 1e-5, 3e-7, 100.0])
@pytest.mark.parametrize('M,N,K', [(300, 36, 68), (257, 256, 256)])
def test_wgrad_x3_split_of_dy(dev, M, N, K, mag):
    """x one-hot per column: dW[n][k] is ((hi + lo) / s) of dy[m_k][n] alone -- the dy-side in-kernel split against its definition
    (hi = f16(s a), lo = f16(s a - hi)), s from the tensor's maximum, and the fixed 2^4 when no maximum is given; as
    tests/test_x3s_gpu.py::test_in_kernel_split_is_the_stored_split_bit_for_bit does for gemm_x3"""
    c = GC.selector_case(M, N, K, mag)
    dy, x = c.dy.to(dev), c.x.to(dev)
    amax = ops.absmax(dy)
    assert amax.item() == c.dy.abs().max().item()
    s = GC.x3_scale(amax.item())
    scaled, db = ops.wgrad_x3(dy, x, want_bias=True, amax=amax)
    assert torch.equal(scaled.cpu(), GC.selector_ref(c, s)), f'split of dy, s = {s}'
    assert torch.equal(ops.wgrad_x3(dy, x, amax=amax), scaled)
    assert torch.equal(ops.wgrad_x3(dy, x).cpu(), GC.selector_ref(c, 16.0)), 'split of dy, fixed 2^4'
    assert torch.equal(ops.wgrad_x3(dy, x, want_bias=True)[0].cpu(), GC.selector_ref(c, 16.0))


# ------------------------------------------------------------------------------------------------
# 3. add_layernorm_backward
# ------------------------------------------------------------------------------------------------
def _ln(dev, c, dy=None, a=None, b=None, **kw):
    to = lambda t: None if t is None else t.to(dev)      # noqa: E731
    return ops.add_layernorm_backward(to(dy), to(c.s if a is None else a), to(b), c.gamma.to(dev), GC.LN_EPS,
                                      **{k: (to(v) if torch.is_tensor(v) else v) for k, v in kw.items()})


def _assert_same(got, base, what):
    for name, a, b in zip(('dx', 'dgamma', 'dbeta'), (got[0], got[2], got[3]), (base[0], base[2], base[3])):
        assert torch.equal(a, b), f'{what}: {name} differs ({int((a != b).sum())} elements)'


@pytest.mark.parametrize('rows', GC.LN_ROWS)
def test_add_layernorm_backward_forms(dev, rows):
    """identities that hold bit for bit whatever the rounding inside the kernel: the operands of the forms compared are equal"""
    c = GC.ln_case(rows)
    base = _ln(dev, c, c.dy)
    assert base[1] is None and len(base) == 4 and tuple(base[0].shape) == (rows, 256)
    # want_amax / want_bf16 change nothing; amax is max |dx|; dx16 is bf16(dx), ties to even
    for want_amax in (False, True):
        for want_bf16 in (False, True):
            got = _ln(dev, c, c.dy, want_amax=want_amax, want_bf16=want_bf16)
            what = f'rows {rows} want_amax={want_amax} want_bf16={want_bf16}'
            _assert_same(got, base, what)
            if want_amax:
                _assert_is_max_of(got[4], got[0], what)
            if want_bf16:
                assert got[1].dtype == torch.bfloat16 and torch.equal(got[1], got[0].bfloat16()), f'{what}: dx16'
            else:
                assert got[1] is None
    # a bf16-representable dy as dy, as dy16a, as dy16b
    one = _ln(dev, c, c.d16a)
    _assert_same(_ln(dev, c, None, dy16a=c.d16a.bfloat16()), one, f'rows {rows} dy16a alone')
    _assert_same(_ln(dev, c, None, dy16b=c.d16a.bfloat16(), want_amax=True), one, f'rows {rows} dy16b alone')
    # exact splits of dy
    _assert_same(_ln(dev, c, c.d32, dy16a=c.d16a.bfloat16(), dy16b=c.d16b.bfloat16(), want_amax=True, want_bf16=True), base,
                 f'rows {rows} d32 + d16a + d16b')
    _assert_same(_ln(dev, c, c.d32 + c.d16b, dy16a=c.d16a.bfloat16()), base, f'rows {rows} (d32 + d16b) + d16a')
    _assert_same(_ln(dev, c, None, dy16a=c.d16a.bfloat16(), dy16b=c.d16b.bfloat16()), _ln(dev, c, c.d16a + c.d16b),
                 f'rows {rows} d16a + d16b')
    # b absent with a = s, an f32 b, a bf16 b
    _assert_same(_ln(dev, c, c.dy, a=c.a, b=c.b), base, f'rows {rows} f32 b')
    _assert_same(_ln(dev, c, c.dy, a=c.a, b=c.b.bfloat16(), want_amax=True), base, f'rows {rows} bf16 b')


@functools.lru_cache(maxsize=None)
def _ln_autograd(rows, dt):
    c = GC.ln_case(rows)
    ts = [t.clone().to(dt).requires_grad_() for t in (c.s, c.gamma, c.beta)]
    F.layer_norm(ts[0], (256,), ts[1], ts[2], GC.LN_EPS).backward(c.dy.to(dt))
    return [t.grad for t in ts]


@pytest.mark.parametrize('b_form', ['none', 'f32', 'bf16'])
@pytest.mark.parametrize('rows', GC.LN_ROWS)
def test_add_layernorm_backward_vs_float64(dev, rows, b_form):
    """float64 autograd of F.layer_norm under `_grad_check`; the last live row's dy is the largest of the tensor, so one clamped
    duplicate of it in dgamma / dbeta is a hundred times the bound"""
    c = GC.ln_case(rows)
    g64, g32 = _ln_autograd(rows, torch.float64), _ln_autograd(rows, torch.float32)
    a, b = (c.s, None) if b_form == 'none' else (c.a, c.b if b_form == 'f32' else c.b.bfloat16())
    dx, dx16, dgamma, dbeta, amax = _ln(dev, c, c.dy, a=a, b=b, want_amax=True, want_bf16=True)
    tag = f'add_layernorm_backward rows={rows} b={b_form}'
    _grad_check(f'{tag} dx', dx, g64[0], g32[0])
    _grad_check(f'{tag} dgamma', dgamma, g64[1], g32[1])
    _grad_check(f'{tag} dbeta', dbeta, g64[2], g32[2])
    _assert_equal(dbeta, c.dy.double().sum(0), f'{tag} dbeta (sums of multiples of 2^-6: exact)')
    _assert_is_max_of(amax, dx, tag)
    assert torch.equal(dx16, dx.bfloat16())


# ------------------------------------------------------------------------------------------------
# 4. nodes at a ragged row count; the amax hand-off
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mag', [1.0, 1e-6])
@pytest.mark.parametrize('hidden', [32, 160])
@pytest.mark.parametrize('block', [False, True], ids=['ffn', 'ffn_block'])
def test_ffn_nodes_at_ragged_rows(dev, block, hidden, mag, monkeypatch):
    """`runtime._X3FfnFn` and `_X3FfnBlockFn` at (3, 101, 256) -- M = 303: ragged row tiles in every GEMM, a ragged last split in
    every weight gradient, a last LayerNorm workgroup of 47 rows -- with the smallest hidden width the gate accepts (32) and one that
    is no multiple of 128 (160), at unit and at real gradient magnitude; float64 autograd, the f32 autograd of the same formulation
    as the yardstick: 4 x its error + 2e-6 relative (the bound of test_x3_training_ffn_node_vs_float64)"""
    B, S, K = 3, 101, 256
    g = torch.Generator().manual_seed(100 + hidden)
    x = torch.randn(B, S, K, generator=g)
    w1, b1 = torch.randn(hidden, K, generator=g) / K ** 0.5, torch.randn(hidden, generator=g) * 0.1
    w2, b2 = torch.randn(K, hidden, generator=g) / hidden ** 0.5, torch.randn(K, generator=g) * 0.1
    gamma, beta = 1 + 0.25 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    gy = torch.randn(B, S, K, generator=g) * mag
    leaves = (x, w1, b1, w2, b2) + ((gamma, beta) if block else ())

    def run(dt, device):
        ts = [t.detach().clone().to(device=device, dtype=dt).requires_grad_(True) for t in leaves]
        y = F.linear(torch.relu(F.linear(ts[0], ts[1], ts[2])), ts[3], ts[4])
        if block:
            y = F.layer_norm(ts[0] + y, (K,), ts[5], ts[6], GC.LN_EPS)
        y.backward(gy.to(device=device, dtype=dt))
        return y, [t.grad for t in ts]
    y64, g64 = run(torch.float64, 'cpu')
    y32, g32 = run(torch.float32, 'cpu')
    ts = [t.detach().clone().to(dev).requires_grad_(True) for t in leaves]
    monkeypatch.setattr(runtime, 'X3_TRAIN_ROWS', 1)             # the row threshold is a speed rule; the widths are what the gate is asked
    with runtime.precision_scope('fp32'):
        assert runtime.x3_train_ffn_ok(*ts[:5])
        if hidden == 32:
            assert not runtime.x3_train_ffn_ok(ts[0], ts[1][:16], ts[2][:16], ts[3][:, :16], ts[4])
        y = runtime._X3FfnBlockFn.apply(*ts, GC.LN_EPS) if block else runtime.ffn_x3_train(*ts)
        y.backward(gy.to(dev))
    rel = lambda a, r: ((a.double().cpu() - r).abs().max() / r.abs().max()).item()      # noqa: E731
    assert tuple(y.shape) == (B, S, K)
    assert rel(y.detach(), y64) <= 4 * rel(y32.detach(), y64) + 1e-6
    names = ('x', 'w1', 'b1', 'w2', 'b2', 'gamma', 'beta')
    for name, got, want, f32 in zip(names, [t.grad for t in ts], g64, g32):
        print(f'{name}: {rel(got, want):.3g} (f32 autograd {rel(f32, want):.3g})')
        assert rel(got, want) <= 4 * rel(f32, want) + 2e-6, (name, mag, rel(got, want), rel(f32, want))


@pytest.mark.parametrize('p', GC.CHAIN_P, ids=lambda p: f'p{p}')
def test_chain_hands_amax_on(dev, p):
    """The calls of `_X3FfnBlockFn.backward` behind the LayerNorm backward, in its order, on exact operands (dz takes the place of
    the LayerNorm backward's output, which rounds): dh and max |dh| from the masked grad-input GEMM, then dW1 / db1 pre-scaled by THAT
    device scalar -- every bit against the float64 chain. A maximum that is stale, zero or taken of another tensor puts dh's pieces
    outside f16's exact range and the weight gradient off its lattice."""
    k = GC.chain_case(p)
    c = k.c
    dz, h, x = c.g.to(dev), c.mask.to(dev), k.x.to(dev)
    amax = ops.absmax(dz)
    dw2, db2 = ops.wgrad_x3(dz, h, want_bias=True, amax=amax)
    _assert_equal(dw2, c.g.double().t() @ c.mask.double(), f'chain p={p} dW2')
    _assert_equal(db2, c.g.double().sum(0), f'chain p={p} db2')
    dh, amax_h = ops.gemm_x3_bwd(dz, _image('t11', dev), c.N, amax=amax, mask=h, want_amax=True)
    _assert_equal(dh, k.dh64, f'chain p={p} dh')
    _assert_is_max_of(amax_h, dh, f'chain p={p}')
    assert amax_h.item() == k.amax_h
    dw1, db1 = ops.wgrad_x3(dh, x, want_bias=True, amax=amax_h)
    _assert_equal(dw1, k.dw1, f'chain p={p} dW1')
    _assert_equal(db1, k.db1, f'chain p={p} db1')
