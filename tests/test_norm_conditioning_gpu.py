"""The normalisation kernels on rows where the variance formula matters (tests/norm_cases.py): mean far from zero, spread below eps,
constant rows, large and small scales, one outlier on the first element of the row in memory order and one elsewhere.

Every output is compared with float64, per family, and no element is left out:

    |got - want| <= FACTOR * max(e_ref, U * S)          (norm_cases.family_ratios)

e_ref = the largest error of torch's own f32 operator on the CPU over the family, U = 2^-24, S = the family's largest
|x| |gamma| rstd + |beta| (+ |up-sampled map|, + |pos| where they are added): one rounding of the largest term an f32 implementation
forms. FACTOR = 8 allows three bits for another summation order and rsqrtf. An x3a output adds 2^-22 |want|. A bf16 output adds one
bf16 rounding of want, half a bf16 ulp at |want| = 2^(floor(log2 |want|) - 8): between 2^-9 |want| at the top of a binade and
2^-8 |want| at its bottom (round-to-nearest of 1.0039 is off by 2^-8, so 2^-9 |want| everywhere would refuse a correctly rounded
output); where the kernel also returns the f32 output, the bf16 one must in addition be its rounding, bit for bit.
Each test prints its worst error / bound per family. Measured on an MI355X: the one-pass E[x^2] - mean^2 statistics these tests were
written against stood at 130 to 355 (offset) and 14 to 41 (tight) for `group_norm`, 8.5 and 24 for the bf16 channel-last input, and
the first-element pivot of the f32 channel-last statistics at 337 to 853 on pivot_outlier; two-pass statistics stay at or below
0.25 in every family, the control included, i.e. within twice torch's own f32 error, so FACTOR = 8 stands."""
import pytest
import torch
import torch.nn.functional as F

import cgg_amd  # noqa: F401
from cgg_amd import ops

import norm_cases as NC
from layer_cases import bf16_rounding as _bf16_rounding          # the rule lives with the layer cases now; unchanged

pytestmark = pytest.mark.gpu

EPS = 1e-5
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C, generator=g), torch.randn(C, generator=g)


def _interp(lo, size, dt):
    return F.interpolate(lo.to(dt), size=size, mode='bilinear', align_corners=False)


def _gn_refs(x, groups, gamma, beta, up=None):
    """x (B, C, H, W) contiguous f32 on the CPU [, up (B, C, h, w)] -> GroupNorm(x) [+ bilinear up-sample of up] in float64, the
    same from torch in f32, and S per element; before any ReLU"""
    def run(dt):
        y = F.group_norm(x.to(dt), groups, gamma.to(dt), beta.to(dt), EPS)
        return y + _interp(up, x.shape[2:], dt) if up is not None else y
    S = NC.gn_scale(x.double(), groups, gamma.double(), beta.double(), EPS)
    if up is not None:
        S = S + _interp(up, x.shape[2:], torch.float64).abs()
    return run(torch.float64), run(torch.float32), S


def _check(label, got, want, ref32, S, fam, relu=False, extra=None):
    if relu:
        want, ref32 = want.relu(), ref32.relu()
    r = NC.family_ratios(got.detach().cpu(), want, ref32, S, fam, extra=extra)
    NC.assert_within(label, r)
    return r


# ------------------------------------------------------------------------------------------------
# ops.group_norm (channel-first f32)
# ------------------------------------------------------------------------------------------------
def _nchw_case(shape):
    def make():
        B, C, H, W = shape
        c = NC.gn_nchw(B, C, H, W, 32, seed=100 + H)
        gamma, beta = _affine(C, 200 + H)
        return c, gamma, beta, _gn_refs(c.x, 32, gamma, beta)
    return _cached(('nchw', shape), make)


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape', [(2, 64, 20, 28), (1, 64, 5, 7), (1, 64, 96, 96)])
def test_group_norm_nchw(dev, shape, relu):
    """`ops.group_norm`: the float4 path in one chunk, the scalar path, and rows of 18 432 elements = two chunks of statistics"""
    c, gamma, beta, (want, ref32, S) = _nchw_case(shape)
    got = ops.group_norm(c.x.to(dev), gamma.to(dev), beta.to(dev), 32, EPS, relu)
    _check(f'group_norm{shape} relu={relu}', got, want, ref32, S, c.fam, relu)


# ------------------------------------------------------------------------------------------------
# channel-last f32 statistics and their consumers
# ------------------------------------------------------------------------------------------------
B_, H_, W_, C_, G_ = 2, 24, 20, 256, 32
HW_ = H_ * W_


def _nhwc_refs(c, H, W, groups, gamma, beta, lo=None, lo_hw=None):
    """the references of a channel-last case (x (B, HW, C), lo (B, h w, C)) in its own layout"""
    up = NC.nhwc_to_nchw(lo, *lo_hw) if lo is not None else None
    return tuple(NC.nchw_to_nhwc(t) for t in _gn_refs(NC.nhwc_to_nchw(c.x, H, W), groups, gamma, beta, up))


def _nhwc_case():
    def make():
        c = NC.gn_nhwc(B_, HW_, C_, G_, seed=7)
        gamma, beta = _affine(C_, 8)
        g = torch.Generator().manual_seed(9)
        lo = torch.randn(B_, (H_ // 2) * (W_ // 2), C_, generator=g)
        pos = torch.randn(HW_, C_, generator=g)
        return dict(c=c, gamma=gamma, beta=beta, lo=lo, pos=pos, plain=_nhwc_refs(c, H_, W_, G_, gamma, beta),
                    up=_nhwc_refs(c, H_, W_, G_, gamma, beta, lo, (H_ // 2, W_ // 2)))
    return _cached('nhwc', make)


@pytest.mark.parametrize('variant', ['plain', 'relu', 'up', 'in_place'])
def test_group_norm_nhwc_f32(dev, variant):
    """`ops.group_norm_nhwc` on an f32 map -> out32: plain, with the fused ReLU, with the bilinear up-sample of a 12 x 10 map added,
    and in place as the pixel decoder calls it (out32 aliasing x: whatever the statistics need of x is read before the apply pass
    overwrites it)"""
    k = _nhwc_case()
    x = k['c'].x.to(dev)
    gamma, beta = k['gamma'].to(dev), k['beta'].to(dev)
    ws = ops.group_norm_nhwc_workspace(B_, HW_, G_, dev)
    y = x if variant == 'in_place' else torch.empty_like(x)
    lo = k['lo'].to(dev)
    ops.group_norm_nhwc(x, gamma, beta, G_, EPS, ws, relu=variant == 'relu', W=W_, out32=(y, 0, HW_ * C_),
                        up=(lo, 0, lo.shape[1] * C_, H_ // 2, W_ // 2) if variant == 'up' else None)
    want, ref32, S = k['up' if variant == 'up' else 'plain']
    _check(f'group_norm_nhwc f32 {variant}', y, want, ref32, S, k['c'].fam, relu=variant == 'relu')


def test_group_norm_nhwc_x3a(dev):
    """`ops.group_norm_nhwc_x3a`: y and y + pos as x3a rows, decoded (22 significant bits: + 2^-22 |want|)"""
    k = _nhwc_case()
    x = k['c'].x.to(dev)
    ws = ops.group_norm_nhwc_workspace(B_, HW_, G_, dev)
    y, yp = torch.empty_like(x), torch.empty_like(x)
    ops.x3_overflow_check(dev, reset=True)
    ops.group_norm_nhwc_x3a(x, k['gamma'].to(dev), k['beta'].to(dev), G_, EPS, ws, out=(y, 0, HW_ * C_), pos=(k['pos'].to(dev), 0),
                            outp=(yp, 0))
    assert ops.x3_overflow_check(dev, reset=True) is False
    want, ref32, S = k['plain']
    _check('group_norm_nhwc_x3a y', ops.x3a_to_f32(y), want, ref32, S, k['c'].fam, extra=2.0 ** -22 * want.abs())
    pos = k['pos'][None]
    wantp = want + pos.double()
    _check('group_norm_nhwc_x3a y+pos', ops.x3a_to_f32(yp), wantp, ref32 + pos, S + pos.abs().double(), k['c'].fam,
           extra=2.0 ** -22 * wantp.abs())


@pytest.mark.parametrize('with_lo', [False, True])
def test_group_norm_nhwc_padout(dev, with_lo):
    """`ops.group_norm_nhwc_padout`: the interior of the padded map, and a border that stays zero"""
    k = _nhwc_case()
    ws = ops.group_norm_nhwc_workspace(B_, HW_, G_, dev)
    yp = ops.zero_border_map(B_, H_, W_, C_, dev)
    ops.group_norm_nhwc_padout(k['c'].x.to(dev), k['gamma'].to(dev), k['beta'].to(dev), G_, EPS, ws, (H_, W_), yp,
                               lo=k['lo'].to(dev) if with_lo else None, lo_hw=(H_ // 2, W_ // 2) if with_lo else None)
    want, ref32, S = k['up' if with_lo else 'plain']
    _check(f'group_norm_nhwc_padout lo={with_lo}', yp[:, 1:H_ + 1, 1:W_ + 1].reshape(B_, HW_, C_), want, ref32, S, k['c'].fam)
    border = yp.clone()
    border[:, 1:H_ + 1, 1:W_ + 1] = 0
    assert border.abs().sum().item() == 0


def _row_moments(c, groups):
    """(mean, var, rstd) of the rows of a case in float64 and from the two passes in f32 on the CPU, each (B, groups)"""
    B = c.rows.values.shape[0] // groups
    out = []
    for dt in (torch.float64, torch.float32):
        _, mean, var = NC.two_pass(c.rows.values.to(dt), EPS)
        out.append(tuple(t.double().view(B, groups) for t in (mean, var, 1.0 / torch.sqrt(var + EPS))))
    return out


def test_group_norm_nhwc_stats(dev):
    """`ops.group_norm_nhwc_stats`: (mean, variance) per (b, group) against float64. Mean and variance relative to the row's
    mean^2 + var = E[x^2] (the mean to its square root), and, because that scale forgives the cancellation of E[x^2] - mean^2,
    rstd = 1 / sqrt(var + eps) -- what every consumer forms -- relative to itself. Bounds: FACTOR * max(e_ref, U) with e_ref the
    same relative error of the two passes in f32 on the CPU, per family."""
    k = _nhwc_case()
    c = k['c']
    ws = ops.group_norm_nhwc_workspace(B_, HW_, G_, dev)
    ops.group_norm_nhwc_stats(c.x.to(dev), G_, ws)
    st = ws[:B_ * G_ * 2].view(B_, G_, 2).cpu().double()
    (m64, v64, r64), (m32, v32, r32) = _row_moments(c, G_)
    ex2 = m64 * m64 + v64
    got = dict(mean=st[..., 0], var=st[..., 1], rstd=1.0 / torch.sqrt(st[..., 1] + EPS))
    scale = dict(mean=ex2.sqrt(), var=ex2, rstd=r64)
    fam = c.rows.fam.view(B_, G_)
    for name, w64, w32 in (('mean', m64, m32), ('var', v64, v32), ('rstd', r64, r32)):
        sc = scale[name].clamp_min(1e-300)                       # the all-zero rows: 0 / tiny = 0, anything else = inf
        ratios = {}
        for i, f in enumerate(NC.FAMILIES):
            m = fam == i
            bound = NC.FACTOR * max(((w32[m] - w64[m]).abs() / sc[m]).max().item(), NC.U)
            err = ((got[name][m] - w64[m]).abs() / sc[m]).max().item()
            ratios[f] = (err, bound, err / bound if err == err else float('inf'))
        NC.assert_within(f'group_norm_nhwc_stats {name}', ratios)


def _decode_pool1(pf, npix, C):
    """PackedFeature -> (B, npix, C) float64 values (hi + lo) / 16 (the layout of tests/test_mask_feature_head_gpu.py)"""
    hi, lo = pf.hi.view(torch.float16).double(), pf.lo.view(torch.float16).double()
    B, T = hi.shape[:2]
    return ((hi + lo) / 16).permute(0, 1, 3, 2, 4).reshape(B, T * 32, C)[:, :npix].cpu()


def test_mask_feature_head_x3_off_centre(dev):
    """`ops.mask_feature_head_x3` fed from `group_norm_nhwc_stats` on an off-centre z, against relu(GroupNorm(z)) -> 1 x 1
    convolution wholly in float64 (statistics included). The 1 x 1 mixes the groups, so there are no families on the output:
    every element is held to 2e-5 -- the bound of tests/test_mask_feature_head_gpu.py for this x3 arithmetic on unit-scale
    outputs -- plus FACTOR * max(e_ref, U * S), e_ref = the error of the same composite from torch in f32 on the CPU,
    S = max sum_k |a_k| |w_k| + |bias|."""
    B, H, W, C = 2, 16, 24, 256
    c = NC.gn_nhwc(B, H * W, C, 32, seed=11)
    gamma, beta = _affine(C, 12)
    g = torch.Generator().manual_seed(13)
    wt, bias = torch.randn(C, C, generator=g) / 16, 0.1 * torch.randn(C, generator=g)
    x = NC.nhwc_to_nchw(c.x, H, W)

    def run(dt):
        a = NC.nchw_to_nhwc(F.group_norm(x.to(dt), 32, gamma.to(dt), beta.to(dt), EPS).relu())
        return a, a @ wt.to(dt).t() + bias.to(dt)
    a64, want = run(torch.float64)
    _, ref32 = run(torch.float32)
    S = (a64.abs() @ wt.double().abs().t() + bias.double().abs()).max().item()
    e_ref = (ref32.double() - want).abs().max().item()
    bound = 2e-5 + NC.FACTOR * max(e_ref, NC.U * S)
    assert 0.3 < want.abs().mean().item() < 3.0                               # unit scale, what the 2e-5 is stated for

    z = c.x.to(dev)
    ws = ops.group_norm_nhwc_workspace(B, H * W, 32, dev)
    ops.group_norm_nhwc_stats(z, 32, ws)
    wk = ops.pack_linear_weight_x3(wt.to(dev))
    ops.x3_overflow_check(dev, reset=True)
    head = (z.view(B, H, W, C), ws, (gamma.to(dev), beta.to(dev), EPS, 32), wk, bias.to(dev), [1])
    assert ops.mask_feature_head_x3_ok(*head)
    imgs, mf = ops.mask_feature_head_x3(*head, want_f32=True)
    assert ops.x3_overflow_check(dev, reset=True) is False
    err_mf = (mf.view(B, H * W, C).cpu().double() - want).abs().max().item()
    err_img = (_decode_pool1(imgs[1], H * W, C) - want).abs().max().item()
    print(f'mask_feature_head_x3 off-centre: mf {err_mf / bound:.3g}  image {err_img / bound:.3g}  (bound {bound:.3g}, e_ref {e_ref:.3g})')
    assert err_mf <= bound and err_img <= bound


# ------------------------------------------------------------------------------------------------
# ops.GroupNormRowsFn: forward and backward
# ------------------------------------------------------------------------------------------------
def _grad_check(label, got, want, ref32, fam=None):
    """|got - want| <= FACTOR * max(e_ref_grad, 2e-5 max |want|): e_ref_grad from torch's f32 autograd on the CPU, 2e-5 the
    tolerance of the existing gradient tests; per family where the gradient has rows (fam), else over the whole tensor"""
    got, want, ref32 = got.detach().cpu().double(), want.double(), ref32.double()
    groups = {'all': torch.ones_like(want, dtype=torch.bool)} if fam is None else {f: fam == i for i, f in enumerate(NC.FAMILIES)}
    ratios = {}
    for f, m in groups.items():
        bound = NC.FACTOR * max((ref32[m] - want[m]).abs().max().item(), 2e-5 * want[m].abs().max().item())
        err = (got[m] - want[m]).abs().max().item()
        ratios[f] = (err, bound, err / bound if err == err else float('inf'))
    NC.assert_within(label, ratios)


@pytest.mark.parametrize('relu,up', [(True, False), (False, True), (False, False)])
def test_group_norm_rows_fn_forward_backward(dev, relu, up):
    """`ops.GroupNormRowsFn` on off-centre x at the shape of tests/test_x3s_gpu.py's test: y per family as above, the gradients
    against float64 autograd. relu' is discontinuous at 0, so the upstream gradient is zero on the elements whose float64 |y| is
    below the forward bound of their family (a rounding-sized y may take either sign); every element of every gradient is
    still compared."""
    B, C, H, W, G = 3, 64, 24, 20, 8
    c = NC.gn_nhwc(B, H * W, C, G, seed=17)
    g = torch.Generator().manual_seed(18 + relu + 2 * up)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    lo = torch.randn(B, (H // 2) * (W // 2), C, generator=g) if up else None
    gy = torch.randn(B, H * W, C, generator=g)
    want, ref32, S = _nhwc_refs(c, H, W, G, gamma, beta, lo, (H // 2, W // 2))
    if relu:
        for i in range(len(NC.FAMILIES)):
            m = c.fam == i
            margin = NC.FACTOR * max((ref32.double()[m] - want[m]).abs().max().item(), NC.U * S[m].max().item())
            gy[m & (want.abs() <= margin)] = 0.0

    def autograd(dt):
        xs = NC.nhwc_to_nchw(c.x, H, W).to(dt).requires_grad_()
        ps = [t.clone().to(dt).requires_grad_() for t in (gamma, beta)]      # clone: .to(its own dtype) is the tensor itself
        y = F.group_norm(xs, G, ps[0], ps[1], EPS)
        lod = None
        if up:
            lod = NC.nhwc_to_nchw(lo, H // 2, W // 2).to(dt).requires_grad_()
            y = y + _interp(lod, (H, W), dt)
        if relu:
            y = y.relu()
        y.backward(NC.nhwc_to_nchw(gy, H, W).to(dt))
        return [NC.nchw_to_nhwc(xs.grad), ps[0].grad, ps[1].grad] + ([NC.nchw_to_nhwc(lod.grad)] if up else [])
    g64, g32 = autograd(torch.float64), autograd(torch.float32)

    x = c.x.to(dev).requires_grad_()
    gm, bt = gamma.to(dev).requires_grad_(), beta.to(dev).requires_grad_()
    lod = lo.to(dev).requires_grad_() if up else None
    y = ops.GroupNormRowsFn.apply(x, gm, bt, G, EPS, relu, lod, (H, W), (H // 2, W // 2))
    y.backward(gy.to(dev))
    tag = f'GroupNormRowsFn relu={relu} up={up}'
    _check(f'{tag} y', y, want, ref32, S, c.fam, relu)
    _grad_check(f'{tag} dx', x.grad, g64[0], g32[0], c.fam)
    _grad_check(f'{tag} dgamma', gm.grad, g64[1], g32[1])
    _grad_check(f'{tag} dbeta', bt.grad, g64[2], g32[2])
    if up:
        _grad_check(f'{tag} dlo', lod.grad, g64[3], g32[3])


# ------------------------------------------------------------------------------------------------
# ops.group_norm_nhwc on a bf16 map
# ------------------------------------------------------------------------------------------------
def test_group_norm_nhwc_bf16(dev):
    """bf16 input (offsets 8 and 32, references from the rounded values) -> out32, out16 = bf16(y), outp16 = bf16(y + pos)"""
    c = NC.gn_nhwc(B_, HW_, C_, G_, seed=21, bf16=True)
    gamma, beta = _affine(C_, 22)
    pos = torch.randn(HW_, C_, generator=torch.Generator().manual_seed(23))
    want, ref32, S = _nhwc_refs(c, H_, W_, G_, gamma, beta)
    x = c.x.to(dev).bfloat16()
    assert torch.equal(x.float().cpu(), c.x)
    ws = ops.group_norm_nhwc_workspace(B_, HW_, G_, dev)
    y32 = torch.empty(B_, HW_, C_, device=dev)
    y16 = torch.empty(B_, HW_, C_, device=dev, dtype=torch.bfloat16)
    yp16 = torch.empty_like(y16)
    ops.group_norm_nhwc(x, gamma.to(dev), beta.to(dev), G_, EPS, ws, out32=(y32, 0, HW_ * C_), out16=(y16, 0, HW_ * C_),
                        pos=(pos.to(dev), 0), outp16=(yp16, 0, HW_ * C_))
    _check('group_norm_nhwc bf16 out32', y32, want, ref32, S, c.fam)
    _check('group_norm_nhwc bf16 out16', y16.float(), want, ref32, S, c.fam, extra=_bf16_rounding(want))
    wantp = want + pos[None].double()
    _check('group_norm_nhwc bf16 outp16', yp16.float(), wantp, ref32 + pos[None], S + pos[None].abs().double(), c.fam,
           extra=_bf16_rounding(wantp))
    assert torch.equal(y16, y32.bfloat16()) and torch.equal(yp16, (y32 + pos.to(dev)[None]).bfloat16())


# ------------------------------------------------------------------------------------------------
# LayerNorm guards: every kernel is two-pass today
# ------------------------------------------------------------------------------------------------
ROWS = [37, 300]          # ragged against the 4, 8 and 256 rows per workgroup


def _ln_case(rows, N, a_dt=torch.float32, b_dt=torch.float32, seed=31):
    def make():
        c = NC.ln_rows(rows, N, seed + rows + N, bf16=a_dt == torch.bfloat16)
        a, b, x = NC.split_ab(c.x, a_dt, b_dt)
        gamma, beta = _affine(N, seed + 1)
        want = F.layer_norm(x, (N,), gamma.double(), beta.double(), EPS)
        ref32 = F.layer_norm(a.float() + b.float(), (N,), gamma, beta, EPS)
        return dict(c=c, a=a, b=b, x=x, gamma=gamma, beta=beta, want=want, ref32=ref32,
                    S=NC.ln_scale(x, gamma.double(), beta.double(), EPS))
    return _cached(('ln', rows, N, a_dt, b_dt, seed), make)


@pytest.mark.parametrize('N', [256, 200])
@pytest.mark.parametrize('rows', ROWS)
def test_add_layernorm(dev, rows, N):
    k = _ln_case(rows, N)
    got = ops.add_layernorm(k['a'].to(dev), k['b'].to(dev), k['gamma'].to(dev), k['beta'].to(dev), EPS)
    _check(f'add_layernorm rows={rows} N={N}', got, k['want'], k['ref32'], k['S'], k['c'].fam)


@pytest.mark.parametrize('a_dt,b_dt', [(torch.float32, torch.float32), (torch.float32, torch.bfloat16),
                                       (torch.bfloat16, torch.bfloat16)], ids=['f32+f32', 'f32+bf16', 'bf16+bf16'])
@pytest.mark.parametrize('rows', ROWS)
def test_add_layernorm_stream(dev, rows, a_dt, b_dt):
    """`ops.add_layernorm_stream` (bf16 + bf16 is the 8-wide kernel): y, bf16(y) and bf16(y + pos[row % len(pos)])"""
    k = _ln_case(rows, 256, a_dt, b_dt)
    pos = torch.randn(19, 256, generator=torch.Generator().manual_seed(32))
    y32, y16, yp16 = ops.add_layernorm_stream(k['a'].to(dev), k['b'].to(dev), k['gamma'].to(dev), k['beta'].to(dev), EPS,
                                              pos=pos.to(dev), want_pos=True)
    tag = f'add_layernorm_stream rows={rows} {a_dt}+{b_dt}'
    want, ref32, S, fam = k['want'], k['ref32'], k['S'], k['c'].fam
    _check(f'{tag} y', y32, want, ref32, S, fam)
    _check(f'{tag} y16', y16.float(), want, ref32, S, fam, extra=_bf16_rounding(want))
    p = pos[torch.arange(rows) % 19]
    _check(f'{tag} yp16', yp16.float(), want + p.double(), ref32 + p, S + p.abs().double(), fam, extra=_bf16_rounding(want + p.double()))
    assert torch.equal(y16, y32.bfloat16()) and torch.equal(yp16, (y32 + p.to(dev)).bfloat16())


@pytest.mark.parametrize('B,level_hw', [(1, [(1, 5), (4, 4), (4, 4)]), (2, [(5, 6), (6, 8), (8, 9)])], ids=['rows37', 'rows300'])
def test_add_layernorm_kv(dev, B, level_hw):
    """`ops.add_layernorm_kv`: y, and the level-major bf16(y + shift) and bf16(y + shift + pos)"""
    starts, S_ = [], 0
    for h, w in level_hw:
        starts.append(S_)
        S_ += h * w
    k = _ln_case(B * S_, 256, torch.float32, torch.bfloat16)
    g = torch.Generator().manual_seed(33)
    shift, pos = torch.randn(S_, 256, generator=g), torch.randn(S_, 256, generator=g)
    y32, m16, mp16 = ops.add_layernorm_kv(k['a'].view(B, S_, 256).to(dev), k['b'].view(B, S_, 256).to(dev), k['gamma'].to(dev),
                                          k['beta'].to(dev), EPS, shift.to(dev), pos.to(dev), starts)
    want, ref32, S, fam = k['want'], k['ref32'], k['S'], k['c'].fam
    tag = f'add_layernorm_kv rows={B * S_}'
    _check(f'{tag} y', y32.view(B * S_, 256), want, ref32, S, fam)
    # level-major (B * S, 256): level l = rows [B start_l, B start_{l+1}) laid out (B, hw_l, 256) -> back to (B, S, 256)
    unlevel = lambda t: torch.cat([t[B * s0:B * (s0 + h * w)].view(B, h * w, 256) for s0, (h, w) in zip(starts, level_hw)], 1)  # noqa: E731
    sh, ps = shift.repeat(B, 1), pos.repeat(B, 1)
    wm = want + sh.double()
    _check(f'{tag} m16', unlevel(m16).reshape(B * S_, 256).float(), wm, ref32 + sh, S + sh.abs().double(), fam, extra=_bf16_rounding(wm))
    wp = wm + ps.double()
    _check(f'{tag} mp16', unlevel(mp16).reshape(B * S_, 256).float(), wp, ref32 + sh + ps, S + sh.abs().double() + ps.abs().double(), fam,
           extra=_bf16_rounding(wp))


@pytest.mark.parametrize('two', [False, True], ids=['one_norm', 'two_norms'])
@pytest.mark.parametrize('rows', ROWS)
def test_layernorm_chain(dev, rows, two):
    """`ops.layernorm_chain`: y = LN_a(x), y + pos, and z = LN_b(y) (z's S from the float64 y)"""
    c = NC.ln_rows(rows, 256, seed=41 + rows)
    ga, ba = _affine(256, 42)
    gb, bb = _affine(256, 43)
    pos = torch.randn(19, 256, generator=torch.Generator().manual_seed(44))
    x = c.x.double()
    want = F.layer_norm(x, (256,), ga.double(), ba.double(), EPS)
    ref32 = F.layer_norm(c.x, (256,), ga, ba, EPS)
    S = NC.ln_scale(x, ga.double(), ba.double(), EPS)
    y, yp, z = ops.layernorm_chain(c.x.to(dev), (ga.to(dev), ba.to(dev), EPS), pos.to(dev),
                                   (gb.to(dev), bb.to(dev), EPS) if two else None)
    tag = f'layernorm_chain rows={rows} two={two}'
    _check(f'{tag} y', y, want, ref32, S, c.fam)
    p = pos[torch.arange(rows) % 19]
    _check(f'{tag} yp', yp, want + p.double(), ref32 + p, S + p.abs().double(), c.fam)
    if two:
        _check(f'{tag} z', z, F.layer_norm(want, (256,), gb.double(), bb.double(), EPS), F.layer_norm(ref32, (256,), gb, bb, EPS),
               NC.ln_scale(want, gb.double(), bb.double(), EPS), c.fam)
    else:
        assert z is None


@pytest.mark.parametrize('rows', ROWS)
def test_add_layernorm_train_forward_backward(dev, rows):
    """`ops.add_layernorm_train`: forward, and the backward through csrc/ln_bwd.hip against float64 autograd (the gradient bound of
    `_grad_check`)"""
    k = _ln_case(rows, 256)
    gy = torch.randn(rows, 256, generator=torch.Generator().manual_seed(51))

    def autograd(dt):
        ts = [t.clone().to(dt).requires_grad_() for t in (k['a'], k['b'], k['gamma'], k['beta'])]    # clone: the cached case stays as it is
        F.layer_norm(ts[0] + ts[1], (256,), ts[2], ts[3], EPS).backward(gy.to(dt))
        return [t.grad for t in ts]
    g64, g32 = autograd(torch.float64), autograd(torch.float32)
    a, b = k['a'].to(dev).requires_grad_(), k['b'].to(dev).requires_grad_()
    norm = torch.nn.LayerNorm(256, eps=EPS).to(dev)
    with torch.no_grad():
        norm.weight.copy_(k['gamma'])
        norm.bias.copy_(k['beta'])
    assert ops.add_layernorm_train_ok(a, b, norm)
    y = ops.add_layernorm_train(a, b, norm)
    y.backward(gy.to(dev))
    tag = f'add_layernorm_train rows={rows}'
    _check(f'{tag} y', y, k['want'], k['ref32'], k['S'], k['c'].fam)
    _grad_check(f'{tag} da', a.grad, g64[0], g32[0], k['c'].fam)
    _grad_check(f'{tag} db', b.grad, g64[1], g32[1], k['c'].fam)
    _grad_check(f'{tag} dgamma', norm.weight.grad, g64[2], g32[2])
    _grad_check(f'{tag} dbeta', norm.bias.grad, g64[3], g32[3])
