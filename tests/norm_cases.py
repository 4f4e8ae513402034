"""Inputs on which a normalisation kernel's variance formula matters, and the bound its outputs are held to. Plain torch on the CPU.

One tensor holds rows of several named families, so that one launch covers them all. A row is what one (mean, variance) pair is taken
over: a (batch, group) pair for GroupNorm, a token for LayerNorm. Row r of a tensor is of kind r % len(kinds):

  centred            N(0, 1), the control
  offset             N(m, 1), m = 10, -100, 1000 (8, 32 for a bf16 input, where bf16 still resolves the unit spread)
  tight              N(1, 1e-3): variance 1e-6, below eps
  flat               every value 3.0; a second kind, every value 0.0 (f32 sums are exact, the expected output is beta)
  scaled             N(0, 1) * 1e3 and N(0, 1) * 1e-3
  pivot_outlier      N(0, 1) with the FIRST element of the row in memory order set to 100
  outlier_elsewhere  N(0, 1) with an interior element (`interior_index`) set to 100

`family_ratios` states the bound: |got - want| <= FACTOR * max(e_ref, U * S) per family, with `want` in float64, e_ref the largest
error of torch's own f32 operator on the CPU over the family, U = 2^-24 and S the largest |x| |gamma| rstd + |beta| of the family."""
import torch
import torch.nn.functional as F

FAMILIES = ('centred', 'offset', 'tight', 'flat', 'scaled', 'pivot_outlier', 'outlier_elsewhere')
U = 2.0 ** -24                  # one f32 rounding
FACTOR = 8.0                    # three bits for another summation order and rsqrtf (the one place to change it)
OUTLIER = 100.0
F32_OFFSETS = (10.0, -100.0, 1000.0)
BF16_OFFSETS = (8.0, 32.0)


def kinds(bf16=False):
    """[(family, parameter)] in row order"""
    offs = BF16_OFFSETS if bf16 else F32_OFFSETS
    return ([('centred', None)] + [('offset', m) for m in offs] + [('tight', None), ('flat', 3.0), ('flat', 0.0), ('scaled', 1e3),
            ('scaled', 1e-3), ('pivot_outlier', None), ('outlier_elsewhere', None)])


def interior_index(n):
    return n // 2 + 3


class Rows:
    """values (nrows, n) f32 in the row's memory order; kind[r] = (family, parameter); fam (nrows,) = index into FAMILIES"""

    def __init__(self, values, kind):
        self.values, self.kind = values, kind
        self.fam = torch.tensor([FAMILIES.index(k[0]) for k in kind])


def rows(nrows, n, seed, bf16=False):
    ks = kinds(bf16)
    assert nrows >= len(ks), f'{nrows} rows cannot hold the {len(ks)} kinds'
    assert n >= 16
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(nrows, n, generator=g)
    kind = [ks[r % len(ks)] for r in range(nrows)]
    for r, (fam, par) in enumerate(kind):
        if fam == 'offset':
            z[r] += par
        elif fam == 'tight':
            z[r] = 1.0 + 1e-3 * z[r]
        elif fam == 'flat':
            z[r] = par
        elif fam == 'scaled':
            z[r] *= par
        elif fam == 'pivot_outlier':
            z[r, 0] = OUTLIER
        elif fam == 'outlier_elsewhere':
            z[r, interior_index(n)] = OUTLIER
    if bf16:
        z = z.bfloat16().float()          # the kernel's input; every reference starts from the rounded values
    return Rows(z, kind)


class Case:
    """x: the kernel's input (f32 values; bf16-exact when bf16) in the kernel's layout; fam: family index of every element of x;
    rows: the Rows it was laid out from"""

    def __init__(self, x, fam, rows_):
        self.x, self.fam, self.rows = x, fam, rows_


def gn_nchw(B, C, H, W, groups, seed):
    """(B, C, H, W): row (b, g) = channels [g cpg, (g + 1) cpg), contiguous in memory; its element 0 is x[b, g cpg, 0, 0]"""
    n = (C // groups) * H * W
    r = rows(B * groups, n, seed)
    return Case(r.values.view(B, C, H, W), r.fam[:, None].expand(-1, n).reshape(B, C, H, W), r)


def gn_nhwc(B, HW, C, groups, seed, bf16=False):
    """(B, HW, C) channel-last: row (b, g) in memory order = pixel-major, then the cpg channels of the group; its element 0 is
    pixel 0, first channel of the group: x[b, 0, g cpg]"""
    cpg = C // groups
    n = HW * cpg
    r = rows(B * groups, n, seed, bf16)
    lay = lambda t: t.reshape(B, groups, HW, cpg).permute(0, 2, 1, 3).reshape(B, HW, C).contiguous()      # noqa: E731
    return Case(lay(r.values), lay(r.fam[:, None].expand(-1, n)), r)


def ln_rows(nrows, N, seed, bf16=False):
    """(nrows, N): one row per token"""
    r = rows(nrows, N, seed, bf16)
    return Case(r.values, r.fam[:, None].expand(-1, N).contiguous(), r)


def split_ab(x, a_dtype=torch.float32, b_dtype=torch.float32):
    """x -> (a, b, a + b in float64) for the residual-add LayerNorms: b = x / 4 and a = x - b in their dtypes. a + b is the
    kernel's input and what the references start from; it is x itself for f32 operands up to one rounding, and exactly x on
    the flat rows in either dtype."""
    b = (0.25 * x).to(b_dtype)
    a = (x - b.float()).to(a_dtype)
    return a, b, a.double() + b.double()


def nhwc_to_nchw(x, H, W):
    """contiguous (B, C, H, W) copy. Not the permuted view: on a channels-last view torch's CPU group_norm takes a kernel that
    forms E[x^2] - mean^2 (1e-9 relative at |mean| / std = 1000 even in float64, tests/test_norm_cases.py), which is no
    reference for these inputs; on contiguous NCHW it is Welford's."""
    B, HW, C = x.shape
    return x.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def nchw_to_nhwc(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B, H * W, C)


def two_pass(r, eps):
    """(x - mean) / sqrt(var + eps) of every row of r (R, n), the textbook two passes, in r's dtype; also (mean, var)"""
    n = r.shape[1]
    mean = r.sum(1, keepdim=True) / n
    d = r - mean
    var = (d * d).sum(1, keepdim=True) / n
    return d / torch.sqrt(var + eps), mean, var


def gn_scale(x, groups, gamma, beta, eps):
    """S's term per element for x (B, C, H, W) float64: |x| |gamma| rstd + |beta|"""
    B, C = x.shape[:2]
    _, _, var = two_pass(x.reshape(B * groups, -1), eps)
    rstd = (1.0 / torch.sqrt(var + eps)).view(B, groups, 1).expand(-1, -1, C // groups).reshape(B, C, 1, 1)
    return x.abs() * gamma.abs().view(1, C, 1, 1) * rstd + beta.abs().view(1, C, 1, 1)


def ln_scale(x, gamma, beta, eps):
    """the same for x (rows, N) float64"""
    _, _, var = two_pass(x, eps)
    return x.abs() * gamma.abs() / torch.sqrt(var + eps) + beta.abs()


def family_ratios(got, want, ref32, S, fam, extra=None, factor=FACTOR):
    """{family: (largest |got - want|, its bound, worst |got - want| / bound)} over every element; all tensors of one shape
    (fam: family index per element). bound = factor * max(e_ref, U * S_family) + extra (elementwise, e.g. the rounding of a bf16
    output)."""
    got, want, ref32, S = got.double(), want.double(), ref32.double(), S.double()
    assert got.shape == want.shape == ref32.shape == S.shape == fam.shape
    out = {}
    for k, name in enumerate(FAMILIES):
        m = fam == k
        assert bool(m.any()), f'no element of family {name}'
        e_ref = (ref32[m] - want[m]).abs().max().item()
        base = factor * max(e_ref, U * S[m].max().item())
        bound = base + (extra.double()[m] if extra is not None else 0.0)
        err = (got[m] - want[m]).abs()
        ratio = err / bound
        ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf')))     # NaN in got -> inf
        out[name] = (err.max().item(), base, ratio.max().item())
    return out


def assert_within(label, ratios):
    """prints the worst ratio of every family, then asserts all of them"""
    print(f'{label}: ' + '  '.join(f'{k}={v[2]:.3g}' for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v[2] <= 1.0}
    assert not bad, f'{label}: (error, bound, error / bound) {bad}'
