"""tests/norm_cases.py produces what it claims (no GPU): the families' conditioning, the exact flat rows, the outlier's memory position
in both layouts, and a float64 reference that can be trusted on these inputs."""
import pytest
import torch
import torch.nn.functional as F

import norm_cases as NC

EPS = 1e-5


def _row_stats(r):
    v = r.values.double()
    mean = v.mean(1)
    std = v.var(1, unbiased=False).sqrt()
    return mean, std


@pytest.mark.parametrize('bf16', [False, True])
def test_families_are_conditioned_as_named(bf16):
    r = NC.rows(2 * len(NC.kinds(bf16)) + 3, 1120, seed=1, bf16=bf16)
    mean, std = _row_stats(r)
    seen = set()
    for i, (fam, par) in enumerate(r.kind):
        seen.add((fam, par))
        m, s, v = mean[i].item(), std[i].item(), r.values[i]
        if fam == 'centred':
            assert abs(m) / s < 0.2 and 0.9 < s < 1.1
        elif fam == 'offset':
            assert 0.85 * abs(par) < abs(m) / s < 1.15 * abs(par) and m * par > 0
        elif fam == 'tight':
            assert s * s < EPS                                     # the variance is below eps ...
            assert abs(m) / s > 200                                # ... and the mean far above the spread
            if not bf16:
                assert 800 < abs(m) / s < 1250
        elif fam == 'flat':
            assert bool((v == par).all()) and s == 0.0
        elif fam == 'scaled':
            assert abs(m) / s < 0.2 and 0.9 * par < s < 1.1 * par
        else:                                                      # the two outlier families: N(0, 1) but for one element
            at = 0 if fam == 'pivot_outlier' else NC.interior_index(v.numel())
            assert v[at].item() == NC.OUTLIER
            rest = torch.cat([v[:at], v[at + 1:]])
            assert rest.abs().max().item() < 6 and abs(rest.mean().item()) < 0.2 and 0.9 < rest.std().item() < 1.1
    assert seen == set(NC.kinds(bf16))
    assert {NC.FAMILIES[k] for k in r.fam.tolist()} == set(NC.FAMILIES)
    if bf16:
        assert torch.equal(r.values.bfloat16().float(), r.values)
        assert {p for f, p in r.kind if f == 'offset'} == {8.0, 32.0}
    else:
        assert {p for f, p in r.kind if f == 'offset'} == {10.0, -100.0, 1000.0}


def test_flat_rows_sum_exactly_in_f32():
    """at the largest row of the GPU tests (18 432 elements): every prefix of the f32 sum of a flat row is exact, in any order"""
    n = 18432
    r = NC.rows(len(NC.kinds()), n, seed=2)
    for i, (fam, par) in enumerate(r.kind):
        if fam == 'flat':
            want = par * torch.arange(1, n + 1, dtype=torch.float64)
            assert torch.equal(torch.cumsum(r.values[i], 0).double(), want)
            assert (r.values[i] * r.values[i]).sum().double().item() == par * par * n
            assert par * par * n < 2 ** 24


def test_outlier_position_in_both_layouts():
    B, C, H, W, G = 2, 64, 5, 7, 16
    cpg, n = C // G, (C // G) * H * W
    at = NC.interior_index(n)
    nchw = NC.gn_nchw(B, C, H, W, G, seed=3)
    nhwc = NC.gn_nhwc(B, H * W, C, G, seed=3)
    assert torch.equal(nchw.rows.values, nhwc.rows.values)         # the same rows, two layouts
    hits = 0
    for row, (fam, _) in enumerate(nchw.rows.kind):
        b, g = divmod(row, G)
        mem_nchw = nchw.x[b, g * cpg:(g + 1) * cpg].reshape(-1)                 # the row as it lies in memory
        mem_nhwc = nhwc.x[b, :, g * cpg:(g + 1) * cpg].reshape(-1)
        assert torch.equal(mem_nchw, nchw.rows.values[row]) and torch.equal(mem_nhwc, nhwc.rows.values[row])
        assert bool((nchw.fam[b, g * cpg:(g + 1) * cpg] == nchw.rows.fam[row]).all())
        assert bool((nhwc.fam[b, :, g * cpg:(g + 1) * cpg] == nhwc.rows.fam[row]).all())
        if fam == 'pivot_outlier':
            assert nchw.x[b, g * cpg, 0, 0].item() == NC.OUTLIER                # element 0 of the row
            assert nhwc.x[b, 0, g * cpg].item() == NC.OUTLIER                   # pixel 0, first channel of the group
            assert int((mem_nchw == NC.OUTLIER).sum()) == 1 and int((mem_nhwc == NC.OUTLIER).sum()) == 1
            hits += 1
        elif fam == 'outlier_elsewhere':
            assert nchw.x.view(B, G, n)[b, g, at].item() == NC.OUTLIER
            assert nhwc.x[b, at // cpg, g * cpg + at % cpg].item() == NC.OUTLIER
            assert nchw.x[b, g * cpg, 0, 0].item() != NC.OUTLIER and nhwc.x[b, 0, g * cpg].item() != NC.OUTLIER
            assert 0 < at // cpg < H * W - 1
            hits += 1
    assert hits >= 4
    ln = NC.ln_rows(37, 200, seed=3)
    for row, (fam, _) in enumerate(ln.rows.kind):
        if fam == 'pivot_outlier':
            assert ln.x[row, 0].item() == NC.OUTLIER
        assert bool((ln.fam[row] == ln.rows.fam[row]).all())


def _rel(a, b, fam):
    """per family: max |a - b| / max |a|"""
    out = {}
    for k, name in enumerate(NC.FAMILIES):
        m = fam == k
        out[name] = (a[m] - b[m]).abs().max().item() / max(a[m].abs().max().item(), 1e-300)
    return out


@pytest.mark.parametrize('bf16', [False, True])
def test_float64_reference_agrees_with_two_pass(bf16):
    """torch's float64 group_norm / layer_norm against the hand-written two passes, 1e-12 relative per family"""
    g = torch.Generator().manual_seed(4)
    B, H, W, C, G = 2, 12, 10, 256, 32
    c = NC.gn_nhwc(B, H * W, C, G, seed=4, bf16=bf16)
    gamma, beta = torch.randn(C, generator=g).double(), torch.randn(C, generator=g).double()
    x = NC.nhwc_to_nchw(c.x.double(), H, W)
    ref = F.group_norm(x, G, gamma, beta, EPS)
    xhat, _, _ = NC.two_pass(x.reshape(B * G, -1), EPS)
    hand = xhat.view(B, C, H, W) * gamma.view(1, C, 1, 1) + beta.view(1, C, 1, 1)
    fam = NC.nhwc_to_nchw(c.fam, H, W)
    for name, v in _rel(ref, hand, fam).items():
        assert v <= 1e-12, ('group_norm', name, v)
    flat = fam == NC.FAMILIES.index('flat')
    assert torch.equal(hand[flat], beta.view(1, C, 1, 1).expand_as(hand)[flat])        # the expected output of a flat row is beta
    if not bf16:
        n = NC.gn_nchw(1, 64, 5, 7, 32, seed=4)
        g2, b2 = gamma[:64], beta[:64]
        xh, _, _ = NC.two_pass(n.x.double().reshape(32, -1), EPS)
        hand = xh.view(1, 64, 5, 7) * g2.view(1, 64, 1, 1) + b2.view(1, 64, 1, 1)
        for name, v in _rel(F.group_norm(n.x.double(), 32, g2, b2, EPS), hand, n.fam).items():
            assert v <= 1e-12, ('group_norm nchw', name, v)
    for N in (256, 200):
        ln = NC.ln_rows(37, N, seed=5, bf16=bf16)
        a, b, x = NC.split_ab(ln.x, torch.bfloat16 if bf16 else torch.float32, torch.bfloat16 if bf16 else torch.float32)
        ref = F.layer_norm(x, (N,), gamma[:N], beta[:N], EPS)
        xhat, _, _ = NC.two_pass(x, EPS)
        for name, v in _rel(ref, xhat * gamma[:N] + beta[:N], ln.fam).items():
            assert v <= 1e-12, ('layer_norm', N, name, v)


def test_split_ab_keeps_the_family():
    ln = NC.ln_rows(37, 256, seed=6)
    a, b, x = NC.split_ab(ln.x)
    assert a.dtype == b.dtype == torch.float32
    assert bool(((x - ln.x.double()).abs() <= 2.0 ** -23 * ln.x.double().abs()).all())
    for bf16 in (False, True):
        l2 = NC.ln_rows(37, 256, seed=6, bf16=bf16)
        dt = torch.bfloat16 if bf16 else torch.float32
        a, b, x = NC.split_ab(l2.x, dt, dt)
        assert a.dtype == b.dtype == dt
        flat = l2.fam == NC.FAMILIES.index('flat')
        assert torch.equal(x[flat], l2.x.double()[flat])
        assert bool(((x - l2.x.double()).abs() <= 2.0 ** -8 * l2.x.double().abs()).all())


def test_family_ratios_bound():
    """the bound is FACTOR * max(e_ref, U * S) per family, plus the elementwise extra; NaN counts as a miss"""
    fam = torch.arange(len(NC.FAMILIES)).repeat_interleave(2)
    want = torch.zeros(fam.numel(), dtype=torch.float64)
    ref32 = want.clone()
    ref32[0] = 1e-3                                              # e_ref of family 0
    S = torch.full_like(want, 2.0)
    got = want.clone()
    got[1] = 8e-3                                                # at the bound of family 0
    got[2] = NC.FACTOR * NC.U * 2.0 * 1.01                       # just past U * S of family 1
    r = NC.family_ratios(got, want, ref32, S, fam)
    assert abs(r['centred'][2] - 1.0) < 1e-9 and 1.0 < r['offset'][2] < 1.02 and r['tight'][2] == 0.0
    r = NC.family_ratios(got, want, ref32, S, fam, extra=torch.full_like(want, NC.FACTOR * NC.U * 2.0))
    assert r['offset'][2] < 0.51
    got[4] = float('nan')
    assert NC.family_ratios(got, want, ref32, S, fam)['tight'][2] == float('inf')
    with pytest.raises(AssertionError):
        NC.assert_within('x', NC.family_ratios(got, want, ref32, S, fam))
