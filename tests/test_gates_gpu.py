"""-m gpu tests of the decisions taken BEFORE a kernel runs: the Python predicates that choose between a HIP fast path and a library
fallback, and the dtype tags handed across the C ABI. A gate that is too wide does not fail a parity test at the shapes the kernels
were built for; it fails for the first model that is not one of the shipped configs. Every gate here is placed at its own boundary --
one step inside, one step outside -- and both sides are compared with a float64 reference:
  inside:  the fast path ran (spy / autograd node) and is within that kernel's existing test bound;
  outside: the PUBLIC caller returns a result within the same bound through its fallback (or None / CggError where that is the
           caller's contract, stated per row) -- never a silent wrong answer, never another exception.
Parts (docstrings give the bounds): A dtype tags (mmcv drop-in with half / double values), B point-logit and mask-logit gates,
C the x3 cross-attention backward across its documented operand range, D stale channel-last rows, E the remaining gates."""
import functools

import pytest
import torch
import torch.nn.functional as F

import cgg_amd  # noqa: F401
from cgg_amd import ops, runtime
from oracle import ops as ref

from test_kernels_gpu import _msda_inputs

pytestmark = pytest.mark.gpu


def _err(got, want64):
    return (got.detach().cpu().double() - want64.detach()).abs().max().item()


class _Spy:
    """Counts the calls of module attribute `name` (and keeps their arguments) while forwarding them."""

    def __init__(self, monkeypatch, module, name):
        self.calls = []
        real = getattr(module, name)

        def fn(*a, **k):
            self.calls.append((a, k))
            return real(*a, **k)
        monkeypatch.setattr(module, name, fn)


# ------------------------------------------------------------------------------------------------
# A. dtype tags cannot lie
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', [torch.float16, torch.float64], ids=['half', 'double'])
def test_msda_mmcv_function_takes_half_and_double_values(dev, dt):
    """`ops.MultiScaleDeformableAttnFunction` with a half / double `value` (mmcv's op accepts both; the kernels read f32 | bf16): computed
    on an f32 copy, output and grad_value in value's dtype. Reference: `oracle.ops.msda_core` in float64 on the dtype-rounded values.
    Bounds: the f32 kernel's existing absolute ones (forward 1e-4, `test_msda_backward_vs_autograd`: grad_value / grad_attn 1e-4,
    grad_loc 2e-3) plus ONE rounding of the result to value's dtype, u |want| with u = eps(dtype) / 2 (2^-11 for half, 2^-53 for
    double), for the two results that are returned in that dtype -- the output and grad_value."""
    shapes = [(4, 4), (8, 8)]
    value, ss, st, loc, aw = _msda_inputs(2, shapes, 8, 32, 4, 80, seed=8)
    u = torch.finfo(dt).eps / 2
    vq = value.to(dt)
    v64, l64, a64 = (t.to(torch.float64, copy=True).requires_grad_(True) for t in (vq, loc, aw))
    want = ref.msda_core(v64, ss, l64, a64)
    go = torch.randn(want.shape, generator=torch.Generator().manual_seed(9)).to(dt)
    want.backward(go.double())
    v = vq.to(dev).requires_grad_(True)
    l, a = loc.to(dev).requires_grad_(True), aw.to(dev).requires_grad_(True)
    out = ops.MultiScaleDeformableAttnFunction.apply(v, ss.to(dev), st.to(dev), l, a, 64)
    assert out.dtype == dt and out.shape == want.shape
    d = (out.detach().cpu().double() - want.detach()).abs()
    print(f'msda {dt}: forward err {d.max().item():.2e}')
    assert bool((d <= 1e-4 + u * want.detach().abs()).all())
    out.backward(go.to(dev))
    assert v.grad.dtype == dt and l.grad.dtype == torch.float32 and a.grad.dtype == torch.float32
    dv = (v.grad.cpu().double() - v64.grad).abs()
    print(f'msda {dt}: grad_value err {dv.max().item():.2e}, grad_attn {_err(a.grad, a64.grad):.2e}, grad_loc {_err(l.grad, l64.grad):.2e}')
    assert bool((dv <= 1e-4 + u * v64.grad.abs()).all())
    assert _err(a.grad, a64.grad) <= 1e-4
    assert _err(l.grad, l64.grad) <= 2e-3           # (random locations stay clear of the integer pixel coordinates where it jumps)
    # the low-level entries refuse the same tensor by name and dtype instead of reading it as f32
    for call in (lambda: ops.msda_forward_hostlevels(v.detach(), shapes, [0, 16], l.detach(), a.detach()),
                 lambda: ops.msda_forward_fused(v.detach(), shapes, [0, 16], torch.zeros(2, 80, 192, device=dev),
                                                torch.zeros(80, 2, device=dev), 4)):
        with pytest.raises(ops.CggError, match=str(dt).replace('.', r'\.')):
            call()


# ------------------------------------------------------------------------------------------------
# B. the point-logit and mask-logit gates imply their kernels
# ------------------------------------------------------------------------------------------------
def test_point_sample_nhwc_x3_gate_is_the_width_mask_logits_is_built_for(dev):
    """B = 2, 16 x 16, 3 groups of 32 points: the sampler's images have one consumer, `mask_logits`, built for 256 channels."""
    pts = torch.rand(2, 3 * 32, 2, device=dev)
    assert not ops.point_sample_nhwc_x3_ok(torch.randn(2, 16, 16, 128, device=dev), pts, 3)
    assert ops.point_sample_nhwc_x3_ok(torch.randn(2, 16, 16, 256, device=dev), pts, 3)
    assert not ops.point_sample_nhwc_x3_ok(torch.randn(2, 16, 16, 264, device=dev), pts, 3)


@pytest.mark.parametrize('C', [128, 256])
def test_targets_batched_point_logits_at_a_width_the_x3_branch_is_not_built_for(dev, C, monkeypatch):
    """The matching-cost branch of `Mask2FormerHeadOpen._targets_batched` with `LazyMasks` of C = 128 (the gate must send it to
    `point_sample_nhwc` + bmm; it raised CGG_EUNSUPPORTED from `mask_logits` before) and of C = 256 (the x3 branch must be the one
    taken): Q = 12, n = 2 layers, pinned points. The point logits -- what `match_cost_rows` is handed -- equal
    mask_embed @ grid_sample(feature) in float64 within the bound of
    `test_point_sample_nhwc_x3_images_equal_pack_of_samples_and_point_logits_are_f32_class`: 4 x the f32 bmm's own error + 1e-6 max."""
    import warnings
    from cgg_amd import synthetic
    from cgg_amd.mask2former_head import LazyMasks
    from util import Bank, build_heads, small_cfg
    cfg = small_cfg(num_queries=12, num_points=256)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prod, _ = build_heads(cfg)
    prod = prod.to(dev).train()
    B, n, Q, P = 2, 2, 12, 256
    K1 = prod.class_embs.shape[0]
    g = torch.Generator().manual_seed(31)
    batch = synthetic.train_batch(B, 64, 64, num_classes=cfg['panoptic_head']['num_things_classes'], max_inst=4, vocab=500, seed=3)
    gt_labels = [t.to(dev) for t in batch['gt_labels']]
    gt_f = [m.float().to(dev) for m in batch['gt_masks']]
    cls = [torch.randn(B, Q, K1, generator=g).to(dev) for _ in range(n)]
    emb = [(torch.randn(B, Q, K1, generator=g) * 2).to(dev) for _ in range(n)]
    feat = (torch.randn(B, C, 16, 16, generator=g) * 2).to(dev)
    embeds = [(torch.randn(B, Q, C, generator=g) * 2).to(dev) for _ in range(n)]
    masks = [LazyMasks(e, feat) for e in embeds]
    x3 = _Spy(monkeypatch, ops, 'point_sample_nhwc_x3')
    f32 = _Spy(monkeypatch, ops, 'point_sample_nhwc')
    rows = _Spy(monkeypatch, ops, 'match_cost_rows')
    prod.point_hook = Bank(11)
    with runtime.precision_scope('fp32'):
        out = prod._targets_batched(cls, emb, masks, gt_labels, gt_f)
    assert len(out) == n
    assert (len(x3.calls), len(f32.calls)) == ((1, 0) if C == 256 else (0, 1))
    assert len(rows.calls) == 1
    all_pts = (x3.calls or f32.calls)[0][0][1]                                      # (B, n P, 2), layer li at [li P, (li + 1) P)
    got = rows.calls[0][0][0]                                                       # (n, B, Q, P)
    assert tuple(got.shape) == (n, B, Q, P) and tuple(all_pts.shape) == (B, n * P, 2)
    fs64 = F.grid_sample(feat.double(), (all_pts.double() * 2.0 - 1.0).unsqueeze(2), align_corners=False).squeeze(3).cpu()   # (B, C, n P)
    for li in range(n):
        fs = fs64[:, :, li * P:(li + 1) * P]
        want = torch.bmm(embeds[li].cpu().double(), fs)
        f32_err = (torch.bmm(embeds[li].cpu(), fs.float()).double() - want).abs().max().item()
        err = _err(got[li], want)
        print(f'C={C} layer {li}: point logits err {err:.2e}, f32 bmm {f32_err:.2e}')
        assert err <= 4 * f32_err + 1e-6 * want.abs().max().item(), (li, err, f32_err)


@pytest.mark.parametrize('C', [128, 256])
def test_mask_logits_fn_outside_its_kernels_falls_back_in_both_directions(dev, C):
    """`_MaskLogitsFn` forward + backward at (h, w) = (5, 7) -- 35 pixels, outside the backward kernels' npix % 8 -- with C = 256 (the
    forward kernel runs, the backward keeps torch.einsum) and C = 128 (neither kernel is built: the forward raised CGG_EUNSUPPORTED
    before, now both directions are torch.einsum) against float64 einsum autograd, bounds of `test_mask_logits_backward_vs_float64`
    in split mode: 2e-5 of each result's scale."""
    from cgg_amd.mask2former_head import _MaskLogitsFn
    g = torch.Generator().manual_seed(70 + C)
    B, Q, h, w = 2, 12, 5, 7
    E = torch.randn(B, Q, C, generator=g)
    F_ = torch.randn(B, C, h, w, generator=g)
    go = torch.randn(B, Q, h, w, generator=g)
    E64, F64 = E.double().requires_grad_(True), F_.double().requires_grad_(True)
    want = torch.einsum('bqc,bchw->bqhw', E64, F64)
    we, wf = torch.autograd.grad(want, (E64, F64), go.double())
    Ed, Fd = E.to(dev).requires_grad_(True), F_.to(dev).requires_grad_(True)
    with runtime.precision_scope('fp32'):
        packed = ops.pack_mask_feature(Fd.detach(), 1, True)
        assert ops.mask_logits_ok(Ed, packed) == (C == 256) and not ops.mask_logits_backward_ok(Ed, Fd)
        out = _MaskLogitsFn.apply(Ed, Fd, packed)
        ge, gf = torch.autograd.grad(out, (Ed, Fd), go.to(dev))
    for got, ref_, name in ((out, want, 'logits'), (ge, we, 'grad_embed'), (gf, wf, 'grad_feat')):
        scale, err = ref_.abs().max().item(), _err(got, ref_)
        print(f'C={C} {name}: err {err:.2e} of scale {scale:.2e}')
        assert got.shape == ref_.shape and err <= 2e-5 * scale, (name, err, scale)


# ------------------------------------------------------------------------------------------------
# C. x3 cross-attention backward across its documented operand range
# ------------------------------------------------------------------------------------------------
def _xattn_reference(q, kv, go, mask, H):
    """float64 autograd of scores -> masked_fill(-inf) -> softmax -> @ v (nn.MultiheadAttention's arithmetic): (grad_q, grad_kv)"""
    B, Q, E = q.shape
    S, D = kv.shape[1], E // H
    qd, kvd = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    qh = (qd * D**-0.5).view(B, Q, H, D).transpose(1, 2)
    kh = kvd[..., :E].view(B, S, H, D).transpose(1, 2)
    vh = kvd[..., E:].view(B, S, H, D).transpose(1, 2)
    att = qh @ kh.transpose(-1, -2)
    if mask is not None:
        att = att.masked_fill(mask[:, None], float('-inf'))
    out = (att.softmax(-1) @ vh).transpose(1, 2).reshape(B, Q, E)
    return torch.autograd.grad(out, (qd, kvd), go.double())


def _xattn_backward_check(dev, q, kv, go, mask, H, tag):
    """forward (saved output / log-sum-exp rows) + `ops.masked_xattn_backward` against `_xattn_reference`: finite, and within the bound
    of `test_masked_xattn_backward_vs_float64_autograd`, err <= 2e-5 max |ref| + 1e-6, for grad_q and grad_kv."""
    from cgg_amd.query_decoder import pack_bool_mask
    wq, wkv = _xattn_reference(q, kv, go, mask, H)
    bits = None if mask is None else pack_bool_mask(mask).contiguous().to(dev)
    out, lse = ops.masked_xattn(q.to(dev), kv.to(dev), bits, H, return_lse=True)
    gq, gkv = ops.masked_xattn_backward(q.to(dev), kv.to(dev), bits, out, lse, go.to(dev), H)
    for got, ref_, name in ((gq, wq, 'grad_q'), (gkv, wkv, 'grad_kv')):
        scale, err = ref_.abs().max().item(), _err(got, ref_)
        print(f'{tag} {name}: err {err:.3e}, bound {2e-5 * scale + 1e-6:.3e}, finite {bool(torch.isfinite(got).all())}')
        assert bool(torch.isfinite(got).all()), (tag, name)
        assert err <= 2e-5 * scale + 1e-6, (tag, name, err, scale)
    return gq, gkv


@pytest.mark.parametrize('form', ['x3', 'f32'])
@pytest.mark.parametrize('c', [256.0, 1024.0, 4000.0])
def test_masked_xattn_backward_two_opposite_value_rows(dev, c, form, monkeypatch):
    """Derivable by hand: B = H = Q = 1, E = 32, S = 2, no mask, q = 0 (P = (1/2, 1/2)), K uniform in [-1, 1], V[0] = +c, V[1] = -c in
    all 32 channels, grad_out = 1. Then O = 0, delta = 0, dP = (32 c, -32 c), dS = (16 c, -16 c): grad_q = scale (dS_0 K_0 + dS_1 K_1)
    = scale 16 c (K_0 - K_1), grad_K = 0 (q = 0), grad_V = 1/2. A dS pre-scale tied to max |grad_out| alone (8 here) put
    8 x 16 c = 131 072 > 65 504 into an f16 piece at c = 1024 -- inf / NaN gradients, far inside the operand range |a| < 4094 of
    csrc/x3.h; the kernel now takes the scale from its own bound on |dS|. `f32` (the exact f32 MFMA form) is the yardstick."""
    monkeypatch.setattr(ops, 'XATTN_X3_BWD', form == 'x3')
    g = torch.Generator().manual_seed(41)
    q = torch.zeros(1, 1, 32)
    k = torch.rand(1, 2, 32, generator=g) * 2 - 1
    v = torch.stack([torch.full((32,), c), torch.full((32,), -c)])[None]
    kv = torch.cat([k, v], -1).contiguous()
    go = torch.ones(1, 1, 32)
    with runtime.precision_scope('fp32'):
        gq, gkv = _xattn_backward_check(dev, q, kv, go, None, 1, f'c={c:g} {form}')
    hand_q = 32 ** -0.5 * 16 * c * (k[0, 0].double() - k[0, 1].double())
    assert _err(gq[0, 0], hand_q) <= 2e-5 * hand_q.abs().max().item() + 1e-6
    assert float(gkv[..., :32].abs().max()) <= 1e-6 and _err(gkv[..., 32:], torch.full((1, 2, 32), 0.5).double()) <= 1e-5


@functools.lru_cache(maxsize=None)
def _xattn_random_case():
    """B = 2, Q = 20, S = 77, H = 4, masked as `test_masked_xattn_backward_vs_float64_autograd`. (The seed is the first from 100 whose
    value rows times 1024 stay inside the x3 operand range |a| < 4094 -- the precondition of the behaviour under test; 19 712 normal
    draws exceed 4094 / 1024 = 3.998 sigma with probability 0.7.)"""
    g = torch.Generator().manual_seed(101)
    B, Q, S, H = 2, 20, 77, 4
    E = H * 32
    q = torch.randn(B, Q, E, generator=g)
    kv = torch.randn(B, S, 2 * E, generator=g)
    go = torch.randn(B, Q, E, generator=g)
    mask = torch.rand(B, Q, S, generator=g) < 0.6
    mask[0, 1] = False                      # un-masked row
    mask[0, 2] = True
    mask[0, 2, S - 1] = False               # single visible key (the last one)
    return q, kv, go, mask, H, E


@pytest.mark.parametrize('form', ['x3', 'f32'])
@pytest.mark.parametrize('gscale', [1.0, 2.0 ** -20])
@pytest.mark.parametrize('vscale', [1.0, 64.0, 1024.0])
def test_masked_xattn_backward_value_and_gradient_scales(dev, vscale, gscale, form, monkeypatch):
    """Random operands with the value half of kv scaled by 1 / 64 / 1024 (max |V| ~ 3.8, 240, 3816: up to the edge of the operand
    range) and grad_out by 1 / 2^-20 (a training step's gradient magnitude): finite gradients within the existing test's bound in both
    forms."""
    monkeypatch.setattr(ops, 'XATTN_X3_BWD', form == 'x3')
    q, kv, go, mask, H, E = _xattn_random_case()
    kv = kv.clone()
    kv[..., E:] *= vscale
    assert float(kv.abs().max()) < 4094 and float(q.abs().max()) * 32 ** -0.5 < 4094
    with runtime.precision_scope('fp32'):
        _xattn_backward_check(dev, q, kv, go * gscale, mask, H, f'V x {vscale:g}, dO x {gscale:g} {form}')


# ------------------------------------------------------------------------------------------------
# D. stale channel-last rows after an in-place edit
# ------------------------------------------------------------------------------------------------
def test_input_level_rows_are_dropped_after_an_in_place_edit_of_the_map(dev, monkeypatch):
    """`runtime.nhwc_to_nchw_train` hands the channel-last original of its NCHW result along (`_cgg_rows`); `input_level_x3_train` read
    it after a shape / dtype check only. The level of `test_encoder_input_level_rows_path_vs_float64` at B = 2, 64 x 64, 64 -> 256
    channels (8192 rows, the smallest count `x3_train_linear_ok` accepts): un-edited, the rows path runs on the very rows handed
    over; after the NCHW map is doubled in place through a detached alias the call returns None (module path) or rows that equal the
    float64 GN(conv1x1(2 x)) within that test's bound, 2e-5 max |ref| -- never the rows of the un-scaled map, whose distance to the
    right answer is asserted to be > 100 x the bound so that the test cannot pass by accident."""
    from cgg_amd.pixel_decoder import ConvModule
    torch.manual_seed(21)
    Cin, C, B, H, W = 64, 256, 2, 64, 64
    cm = ConvModule(Cin, C, kernel_size=1, norm_cfg=dict(type='GN', num_groups=32), act_cfg=None, bias=True).to(dev).train()
    with torch.no_grad():
        cm.conv.bias.normal_(0, 0.1)
        cm.gn.weight.uniform_(0.5, 1.5)
        cm.gn.bias.normal_(0, 0.1)
    nhwc = torch.randn(B, H, W, Cin, generator=torch.Generator().manual_seed(22)).to(dev)

    def want(scale):
        p = {k: v.detach().cpu().double() for k, v in dict(w=cm.conv.weight, b=cm.conv.bias, g=cm.gn.weight, be=cm.gn.bias).items()}
        y = F.group_norm(F.conv2d(nhwc.cpu().double().permute(0, 3, 1, 2) * scale, p['w'], p['b']), 32, p['g'], p['be'], cm.gn.eps)
        return y.flatten(2).transpose(1, 2)

    seen = []
    real = runtime._X3LinearFn.apply
    monkeypatch.setattr(runtime._X3LinearFn, 'apply', staticmethod(lambda *a: (seen.append(a[0]), real(*a))[1]))
    with runtime.precision_scope('fp32'):
        out = runtime.nhwc_to_nchw_train(nhwc.clone().requires_grad_())
        fresh = runtime.input_level_x3_train(cm, out)
        assert fresh is not None and len(seen) == 1 and seen[0] is out._cgg_rows           # the rows path, on the handed rows
        out.detach().mul_(2.0)                                                             # e.g. a hook that rescales the map
        assert torch.equal(out.detach(), nhwc.permute(0, 3, 1, 2) * 2.0)
        got = runtime.input_level_x3_train(cm, out)
    w1, w2 = want(1.0), want(2.0)
    bound = 2e-5 * w2.abs().max().item()
    stale = _err(fresh, w2)
    print(f'fresh rows err {_err(fresh, w1):.2e}; rows of the un-scaled map vs GN(conv(2 x)): {stale:.3e} (bound {bound:.2e}); '
          f'after the edit: {"None" if got is None else format(_err(got, w2), ".2e")}')
    assert _err(fresh, w1) <= 2e-5 * w1.abs().max().item()
    assert stale > 100 * bound
    assert got is None or _err(got, w2) <= bound
    assert got is not None or len(seen) == 1                                               # None: the x3 node did not run again


# ------------------------------------------------------------------------------------------------
# E. each remaining gate, one step inside and one step outside
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,K,N,inside,noted', [(512, 96, 64, True, False), (511, 96, 64, False, False),
                                                   (512, 80, 64, False, True), (512, 96, 50, True, False)])
def test_x3_linear_gate_inference(dev, rows, K, N, inside, noted, monkeypatch):
    """`runtime.x3_linear_ok` through `runtime.linear` under no_grad in parity mode: rows 512 / 511, K 96 / 80 (K % 32; the only row that
    counts as a `library_fallbacks()` event: enough rows for the x3 GEMM, a K it cannot tile), N = 50 stays inside. Inside:
    `ops.gemm_x3` ran; outside: the f32 library GEMM. Both within the bound of `test_gemm_x3_vs_float64`: 4 x the f32 product's own
    error + 2e-7 max |want|."""
    g = torch.Generator().manual_seed(rows + K + N)
    x = torch.randn(rows, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    want = x.double() @ w.double().t() + b.double()
    f32_err = ((x @ w.t() + b).double() - want).abs().max().item()
    spy = _Spy(monkeypatch, ops, 'gemm_x3')
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    with runtime.precision_scope('fp32'), torch.no_grad():
        assert runtime.x3_linear_ok(xd, wd) == inside
        before = runtime.library_fallbacks()
        y = runtime.linear(xd, wd, bd)
        assert runtime.library_fallbacks() - before == int(noted)
    assert len(spy.calls) == int(inside)
    err = _err(y, want)
    print(f'rows {rows} K {K} N {N}: err {err:.2e}, f32 {f32_err:.2e}, x3 {inside}')
    assert tuple(y.shape) == (rows, N) and err <= 4 * f32_err + 2e-7 * want.abs().max().item()


@pytest.mark.parametrize('rows,K,N,inside', [(8192, 96, 96, True), (8191, 96, 96, False), (8192, 96, 100, False), (8192, 80, 96, False)])
def test_x3_train_linear_gate(dev, rows, K, N, inside):
    """`runtime.x3_train_linear_ok` through `runtime.linear` under autograd: rows 8192 / 8191, N 96 / 100, K 96 / 80. Inside: the
    `_X3LinearFn` node; outside: `F.linear`. Forward, grad-input, grad-weight and grad-bias against float64 autograd within the bound of
    `test_x3_training_linear_forward_and_gradients_vs_float64`: 2e-5 of each result's scale."""
    g = torch.Generator().manual_seed(rows + K + N)
    x = torch.randn(rows, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    gy = torch.randn(rows, N, generator=g)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    yd = F.linear(xd, wd, bd)
    yd.backward(gy.double())
    xg, wg, bg = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    with runtime.precision_scope('fp32'):
        assert runtime.x3_train_linear_ok(xg, wg) == inside
        y = runtime.linear(xg, wg, bg)
        assert ('X3Linear' in type(y.grad_fn).__name__) == inside
        y.backward(gy.to(dev))
    for got, want, name in ((y, yd, 'y'), (xg.grad, xd.grad, 'dx'), (wg.grad, wd.grad, 'dW'), (bg.grad, bd.grad, 'db')):
        scale, err = want.abs().max().item(), _err(got, want)
        print(f'rows {rows} K {K} N {N} {name}: err {err / scale:.2e} of scale, x3 {inside}')
        assert err <= 2e-5 * scale, (name, err, scale)


@pytest.mark.parametrize('C,N,H,W,inside', [(32, 32, 16384, 4, True), (32, 32, 21846, 3, False), (48, 32, 16384, 4, False),
                                            (32, 32, 16383, 4, False)])
def test_x3_train_conv3x3_gate(dev, C, N, H, W, inside):
    """`runtime.x3_train_conv3x3_ok` through its caller `pixel_decoder.ConvModule.forward`: map width 4 / 3 (at >= X3_CONV_ROWS output
    pixels), input channels 32 / 48, X3_CONV_ROWS = 65 536 output pixels exactly (16384 x 4) and one map row fewer. Inside: the
    `_X3Conv3x3Fn` node; outside: the library convolution. Forward, grad-input and grad-weight against float64 autograd of F.conv2d
    within the bound of `test_x3_training_conv3x3_forward_and_gradients_vs_float64`: 4 x the f32 convolution's own error + 3e-7 of
    the result's scale."""
    from cgg_amd.pixel_decoder import ConvModule
    g = torch.Generator().manual_seed(C + H + W)
    x = torch.randn(1, C, H, W, generator=g)
    w = torch.randn(N, C, 3, 3, generator=g) / (3 * C ** 0.5)
    go = torch.randn(1, N, H, W, generator=g)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, 1, 1)
    y64.backward(go.double())
    x32, w32 = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y32 = F.conv2d(x32, w32, None, 1, 1)
    y32.backward(go)
    cm = ConvModule(C, N, 3, padding=1, bias=False, norm_cfg=None, act_cfg=None).to(dev)
    with torch.no_grad():
        cm.conv.weight.copy_(w)
    xd = x.to(dev).requires_grad_(True)
    with runtime.precision_scope('fp32'):
        assert (H * W >= runtime.X3_CONV_ROWS) == (H != 16383)
        assert runtime.x3_train_conv3x3_ok(cm.conv, xd) == inside
        y = cm(xd)
        assert ('X3Conv3x3' in type(y.grad_fn).__name__) == inside
        y.backward(go.to(dev))
    for got, want, f32, name in ((y, y64, y32, 'y'), (xd.grad, x64.grad, x32.grad, 'dx'), (cm.conv.weight.grad, w64.grad, w32.grad, 'dW')):
        scale, err, r = want.abs().max().item(), _err(got, want), _err(f32, want)
        print(f'C {C} {H} x {W} {name}: err {err:.2e}, f32 conv {r:.2e}, scale {scale:.2e}, x3 {inside}')
        assert err <= 4 * r + 3e-7 * scale, (name, err, r, scale)


@pytest.mark.parametrize('Q,ncols,k,inside', [(96, [164], 64, True), (96, [165], 64, False), (10, [11, 30], 100, True),
                                              (10, [11, 30], 101, False)])
def test_class_topk_gate(dev, Q, ncols, k, inside, monkeypatch):
    """`ops.class_topk_supported` through `MaskFormerFusionHeadOpen._batch_picks`: the kernel's LDS budget 8 k + 4 Q (n - 1) + 4 Q equal
    to 62 KiB exactly (Q = 96, 164 columns, k = 64 -> 63 488 bytes) and one class more; k == Q (n - 1) exactly (10 x 10 = 100) and
    k = 101. Inside: `cgg_class_topk` ran and its picks equal softmax + stable descending sort of the dot products it was handed, as
    in `test_class_topk_matches_softmax_topk` (scores bitwise, order with ties by flat index). Outside: the caller's contract is None
    (the per-type torch path then runs) with no kernel call."""
    from types import SimpleNamespace
    from cgg_amd.maskformer_fusion_head import MaskFormerFusionHeadOpen
    if inside and len(ncols) == 1:
        assert 8 * k + 4 * Q * (ncols[0] - 1) + 4 * Q == 62 * 1024
    g = torch.Generator().manual_seed(Q + k)
    B, D = 2, 16
    emb = torch.randn(B, Q, D, generator=g).to(dev)
    tables = [torch.randn(n, D, generator=g).to(dev) for n in ncols]
    spy = _Spy(monkeypatch, ops, 'class_topk')
    stub = SimpleNamespace(test_cfg=dict(max_per_image=k))
    assert ops.class_topk_supported(Q, ncols, k) == inside
    res = MaskFormerFusionHeadOpen._batch_picks(stub, emb, tables)
    assert len(spy.calls) == int(inside)
    if not inside:
        assert res is None
        return
    labels, scores, qidx = res
    dots = spy.calls[0][0][0]
    want_dots = emb.reshape(B * Q, D).double() @ torch.cat(tables, 0).double().t()
    assert _err(dots, want_dots.cpu()) <= 2e-5 * want_dots.abs().max().item()
    c0 = 0
    for t, nc in enumerate(ncols):
        for b in range(B):
            prob, _, _ = ops.rowwise_softmax_argmax(dots[b * Q:(b + 1) * Q, c0:c0 + nc].contiguous(), want_prob=True)
            want_s, want_i = prob[:, :-1].flatten().sort(descending=True, stable=True)
            assert torch.equal(scores[b, t], want_s[:k])
            assert torch.equal(labels[b, t] + qidx[b, t] * (nc - 1), want_i[:k])
        c0 += nc


@pytest.mark.parametrize('Q,T,d,inside', [(256, 64, 8, True), (257, 64, 8, False), (256, 65, 8, False), (256, 64, 12, False)])
def test_grounding_gate(dev, Q, T, d, inside, monkeypatch):
    """`ops.grounding_supported` through `losses.grounding_loss`: Q 256 / 257, T 64 / 65, d 8 / 12 (d % 8). Inside: the HIP pair-cost
    kernel; outside: the torch formulation. Loss and gradient against the oracle in float64 within the bounds of
    `test_grounding_loss_kernel_vs_oracle`: 1e-5 (1 + |loss|), 1e-4 of the gradient's scale."""
    from cgg_amd import losses
    from oracle import head as OH
    g = torch.Generator().manual_seed(Q + T + d)
    B = 2
    pred = torch.randn(B, Q, d, generator=g) * 0.5
    cap = torch.randn(B, T, d, generator=g)
    ntok = torch.tensor([5, 0])                                  # one caption without nouns
    mask = (torch.arange(T)[None] < ntok[:, None]).long()
    pd = pred.double().requires_grad_(True)
    want = OH.grounding_loss(pd, cap.double(), mask, 10.0)
    wg, = torch.autograd.grad(want, pd)
    spy = _Spy(monkeypatch, ops, 'grounding_pair_costs')
    pg = pred.to(dev).requires_grad_(True)
    assert ops.grounding_supported(pg, cap.to(dev)) == inside
    got = losses.grounding_loss(pg, cap.to(dev), mask.to(dev), 10.0)
    gg, = torch.autograd.grad(got, pg)
    assert len(spy.calls) == int(inside)
    scale, err = wg.abs().max().item(), _err(gg, wg)
    lg, lw = got.item(), want.item()
    print(f'Q {Q} T {T} d {d}: loss err {abs(lg - lw):.2e}, grad err {err:.2e} of scale {scale:.2e}, kernel {inside}')
    assert abs(lg - lw) <= 1e-5 * (1 + abs(lw)), (lg, lw)
    assert err <= 1e-4 * scale + 1e-9, (err, scale)


def _decoder_ffn_head(dev, width):
    import warnings
    import util
    cfg = util.small_cfg()
    tl = cfg['panoptic_head']['transformer_decoder']['transformerlayers']
    tl['feedforward_channels'] = width
    tl['ffn_cfgs']['feedforward_channels'] = width
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prod, _ = util.build_heads(cfg)
    return prod.to(dev)


@pytest.mark.parametrize('mode', ['bf16', 'fp32'])
@pytest.mark.parametrize('width,inside', [(2048, True), (2304, False)])
def test_lean_decode_gate_at_the_decoder_tail_plane_cap(dev, width, inside, mode, monkeypatch):
    """`Mask2FormerHeadOpen._lean_decode_ok` at the plane cap of `ops.decoder_tail` (DECODER_TAIL_MAX_PLANES = 8 planes of 256 FFN
    columns), in both precision modes. Inside (2048): the lean inference decode hands the FFN planes to `ops.decoder_tail`. Outside
    (2304 = 9 planes, which the kernel used to sum as 8): `ops.decoder_tail` is not called, `ops.layernorm_chain` adds all 9, and
    the inference outputs equal, bit for bit, those with `_lean_decode_ok` forced to False."""
    from cgg_amd import synthetic
    from cgg_amd.mask2former_head import Mask2FormerHeadOpen
    prod = _decoder_ffn_head(dev, width)
    B, H, W = 2, 64, 96
    feats = [f.to(dev) for f in synthetic.backbone_feats(B, H, W, channels=(64, 128, 256, 512), seed=21)]
    if mode == 'bf16':
        feats = [f.bfloat16().contiguous(memory_format=torch.channels_last) for f in feats]
    metas = synthetic.img_metas(B, H, W)
    tail, chain = _Spy(monkeypatch, ops, 'decoder_tail'), _Spy(monkeypatch, ops, 'layernorm_chain')
    assert prod._lean_decode_ok(256) == inside
    with torch.no_grad(), runtime.precision_scope(mode):
        got = prod._forward(feats, metas, all_masks=False)
        planes = [a[0].shape[0] for a, _ in chain.calls if a[0].dim() == 3]
        assert len(tail.calls) == (prod.num_transformer_decoder_layers - 1 if inside else 0)
        assert planes == ([8] if inside else [9] * prod.num_transformer_decoder_layers), planes
        monkeypatch.setattr(Mask2FormerHeadOpen, '_lean_decode_ok', lambda self, C: False)
        want = prod._forward(feats, metas, all_masks=False)
    for g, w in zip(got, want):
        assert torch.isfinite(g[-1]).all()
        if not inside:
            assert torch.equal(g[-1], w[-1])


@pytest.mark.parametrize('x3', [False, True], ids=['bf16', 'x3'])
def test_decoder_tail_refuses_nine_planes(dev, x3):
    pack = ops.pack_linear_weight_x3 if x3 else ops.pack_linear_weight
    w = pack(torch.eye(256, device=dev))
    v = torch.ones(256, device=dev)
    norm = (v, v, 1e-5)
    mlp = (w, v, w, v, w, v)
    for nsum in (9, 16):
        with pytest.raises(ops.CggError, match=f'nsum={nsum} planes .at most {ops.DECODER_TAIL_MAX_PLANES} '):
            ops.decoder_tail(torch.zeros(nsum, 4, 256, device=dev), norm, torch.zeros(2, 256, device=dev), norm, mlp, (w, v))
    assert ops.decoder_tail(torch.zeros(8, 4, 256, device=dev), norm, torch.zeros(2, 256, device=dev), norm, mlp, (w, v))[0].shape == (4, 256)


# ------------------------------------------------------------------------------------------------
# F. one operand on the CPU among device operands (the case the CPU suite cannot build)
# ------------------------------------------------------------------------------------------------
class _SizesOnlyReal:
    """Stands in for the loaded library: a `*_bytes` query goes to the real one, any other entry point raises when it is looked up --
    whatever the wrapper under test does, it cannot launch a kernel."""

    def __init__(self, real):
        self.real = real
        self.refused = []

    def __getattr__(self, name):
        if name.endswith('_bytes'):
            return getattr(self.real, name)
        self.refused.append(name)
        raise AssertionError(f'the library entry {name} was reached')


def _mixed_device_calls(dev, real):
    M, K, N = 8, 256, 256
    a, on_dev, on_cpu = torch.zeros(M, K, device=dev), torch.zeros(M, N, device=dev), torch.zeros(M, N)
    x3 = torch.zeros(real.cgg_x3_packed_bytes(N, K), dtype=torch.uint8, device=dev).as_subclass(ops.X3Image)
    bf16 = torch.zeros(real.cgg_linear_rows_packed_bytes(N, K), dtype=torch.uint8, device=dev)
    bias = torch.zeros(N, device=dev)
    norm = (torch.ones(N, device=dev), torch.zeros(N, device=dev), 1e-5)
    return [
        ('gemm_x3', 'res', lambda: ops.gemm_x3(a, x3, N, bias=bias, res=on_cpu)),
        ('gemm_x3', 'out', lambda: ops.gemm_x3(a, x3, N, bias=bias, res=on_dev, out=on_cpu)),
        ('linear_rows_bf16', 'res', lambda: ops.linear_rows_bf16(a, bf16, N, bias=bias, res=on_cpu)),
        ('linear_rows_bf16', 'out', lambda: ops.linear_rows_bf16(a, bf16, N, bias=bias, res=on_dev, out=on_cpu)),
        ('decoder_mid', 'res', lambda: ops.decoder_mid(a, bf16, bias, on_cpu, norm)),
    ]


def test_one_cpu_operand_among_device_operands_is_refused_by_name(dev, monkeypatch):
    """M = 8, K = N = 256, every operand on the device except `res` (or a caller's `out`): these went to the kernel as raw addresses
    -- a host pointer in a device launch. Now a CggError names the operand and no entry point but a size query was looked up."""
    real = ops._lib_()
    calls = _mixed_device_calls(dev, real)
    guard = _SizesOnlyReal(real)
    monkeypatch.setattr(ops, '_lib_', lambda: guard)
    for wrapper, arg, call in calls:
        with pytest.raises(ops.CggError, match='ROCm device') as e:
            call()
        assert str(e.value).startswith(f'{arg} must live on a ROCm device (got cpu)'), (wrapper, arg, str(e.value))
    assert guard.refused == []
