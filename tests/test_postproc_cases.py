"""tests/postproc_cases.py produces what it claims (no GPU): the rule agrees with torch's own f32 bilinear resize, no thresholded output
of torch's operator flips outside the exclusion band, the bands exclude at most 1e-3 of the pixels of every case, the planted queries
and ties are what they are named, and torch's own f32 softmax stays inside the softmax bound."""
import numpy as np
import pytest
import torch

import postproc_cases as PC


def test_taps_restate_torch():
    """up and down, borders included: the rule and torch's f32 operator differ by no more than the band"""
    g = torch.Generator().manual_seed(1)
    for (H, W), size in [((13, 19), (50, 70)), ((24, 20), (72, 60)), ((20, 28), (13, 9)), ((1, 8), (4, 32)), ((8, 1), (32, 4)),
                         ((5, 7), (5, 7)), ((32, 32), (16, 16))]:
        x = torch.randn(2, H, W, generator=g) * 3
        want = torch.nn.functional.interpolate(x[None], size, mode='bilinear', align_corners=False)[0]
        got = PC.resize_rule(x, size)
        assert got.dtype == torch.float64 and tuple(got.shape) == (2,) + size
        err = (got - want.double()).abs().max().item()
        print(f'{H}x{W} -> {size}: |rule - torch f32| = {err:.2e}')
        assert err <= PC.band(x, size, size, size).max().item()         # blend roundings; an ulp of the coordinate where inexact
    i0, i1, l1 = PC.taps(4, 16)
    assert i0[:2].tolist() == [0, 0] and l1[:2].tolist() == [0.0, 0.0]              # the source clamps to 0 at the near border
    assert i0[-1].item() == 3 and i1[-1].item() == 3                                 # and the second tap to the last element
    assert l1[2].item() == 0.125 and (i0[2].item(), i1[2].item()) == (0, 1)


def test_exact_coordinates_are_exact():
    for n_in, n_out in [(4, 8), (4, 16), (4, 32), (25, 100), (40, 160), (32, 16), (8, 64)]:
        assert PC._pow2_ratio(n_in, n_out)
        o = np.arange(n_out, dtype=np.float64)
        src = np.maximum(n_in / n_out * (o + 0.5) - 0.5, 0.0)
        i0, _, l1 = PC.taps(n_in, n_out)
        assert np.array_equal(i0.numpy() + l1.numpy(), src)                          # the f32 coordinate is the real one
    assert not PC._pow2_ratio(13, 50) and not PC._pow2_ratio(24, 72) and not PC._pow2_ratio(20, 13)
    assert PC.exact_coordinates((25, 42), (100, 168), (97, 96), (97, 96))
    assert not PC.exact_coordinates((16, 24), (64, 96), (60, 90), (75, 110))         # the second stage is not


@pytest.mark.parametrize('name', sorted(PC.INSTANCE_GEOMS))
def test_instance_case_band(name):
    ref = PC.instance_case(name)
    hw, up, crop, out = PC.INSTANCE_GEOMS[name]
    t32 = PC.torch_f32_resized(ref.logits, up, crop, out)
    flips = ((t32 > 0) != ref.mask) & ~ref.inside
    worst = ((t32.double() - ref.v).abs() / ref.band).max().item()
    print(f'{name}: band {ref.band.min().item():.2e} .. {ref.band.max().item():.2e}, excluded share {ref.share:.2e} '
          f'({int(ref.n_inside.sum())} of {ref.inside.numel()}), torch f32 within {worst:.3f} of the band')
    assert not bool(flips.any()), f'{int(flips.sum())} sign flips of torch f32 outside the band'
    assert worst <= 1.0
    assert ref.share <= PC.SHARE_CAP
    # the planted queries
    npix = out[0] * out[1]
    assert ref.count[PC.EMPTY].item() == 0 and ref.score[PC.EMPTY].item() == 0.0 and ref.box[PC.EMPTY].tolist() == [0, 0, 0, 0]
    assert ref.count[PC.FULL].item() == npix and ref.box[PC.FULL].tolist() == [0, 0, out[1], out[0]]
    assert ref.n_inside[PC.EMPTY].item() == 0 and ref.n_inside[PC.FULL].item() == 0
    assert torch.equal(ref.v[PC.COPY], ref.v[PC.COPY_OF])
    assert set(PC.SEL) >= {PC.EMPTY, PC.FULL, PC.CORNER, PC.COPY} and len(set(PC.SEL)) < len(PC.SEL)
    if out == crop == up and up[0] > hw[0]:
        c = ref.mask[PC.CORNER]
        assert bool(c[-1, -1]) and 0 < int(c.sum()) < npix / 4          # the bottom-right corner alone
        assert ref.box[PC.CORNER][2:].tolist() == [out[1], out[0]]


def test_fast_and_generic_pair_share_logits():
    a, b = PC.instance_case('fast_w96'), PC.instance_case('generic_w100')
    assert torch.equal(a.logits, b.logits)
    assert torch.equal(a.v, b.v[:, :, :96])
    for name, (hw, up, crop, out) in PC.INSTANCE_GEOMS.items():
        s = up[0] // hw[0]
        fast = (s in (2, 4, 8) and s * hw[0] == up[0] and s * hw[1] == up[1] and crop == out and out[1] % 16 == 0)
        assert fast == PC.bitpack_expected(name), name


@pytest.mark.parametrize('name', sorted(PC.PICKS_GEOMS))
def test_picks_case(name):
    ref, qidx, cls = PC.picks_case(name)
    print(f'{name}: excluded share {ref.share:.2e}')
    assert ref.share <= PC.SHARE_CAP
    assert qidx.numel() == 300 and cls.numel() == 300 and ref.logits.shape[0] == 5
    assert set(qidx.tolist()) == {0, 1, 2, 4}


@pytest.mark.parametrize('name', sorted(PC.PANOPTIC_CASES))
def test_panoptic_case(name):
    ref = PC.panoptic_case(name)
    n, npix = ref.n, ref.out[0] * ref.out[1]
    print(f'{name}: band {ref.band.max().item():.2e}, gap threshold up to {ref.gap_thr.max().item():.2e}, excluded share {ref.share:.2e} '
          f'(ids {int(ref.ids_excluded.sum())}, win_half {int(ref.half_excluded.sum())} of {npix})')
    assert ref.share <= PC.SHARE_CAP
    assert ref.counts[:, 0].sum().item() == npix and bool((ref.counts[:, 2] <= ref.counts[:, 0]).all())
    assert bool((ref.counts[:, 2] <= ref.counts[:, 1]).all())
    assert int(ref.keep.max()) < PC.PAN_Q and ref.keep.dtype == torch.int32
    if 1 < n <= PC.PAN_Q and name != 'n7_twins':
        assert ref.keep.unique().numel() == n and not torch.equal(ref.keep.sort().values, ref.keep)       # a permuted subset
    # torch's own f32 chain decides the same winner and the same half outside the exclusions
    v32 = PC.torch_f32_resized(ref.logits[ref.keep.long()], ref.up, ref.crop, ref.out)
    pv32 = ref.score[:, None, None] * torch.sigmoid(v32)
    ids32 = pv32.argmax(0)
    assert torch.equal(ids32[~ref.ids_excluded], ref.ids[~ref.ids_excluded])
    half32 = v32.gather(0, ids32[None])[0] >= 0
    assert torch.equal(half32[~ref.half_excluded], ref.win_half[~ref.half_excluded])
    if name == 'n7_twins':
        assert ref.keep[3] == ref.keep[5] and ref.score[3] == ref.score[5]
        assert ref.shadowed.tolist() == [False] * 5 + [True, False]
        assert int((ref.ids == 3).sum()) > 0 and int((ref.ids == 5).sum()) == 0
        assert ref.counts[5].tolist() == [0, ref.counts[3, 1].item(), 0]
    else:
        assert not bool(ref.shadowed.any())


def test_paint_case():
    ids, win_half, lut_val, lut_half, void, want = PC.paint_case()
    assert ids.numel() == 1000 and ids.numel() % 256 != 0
    assert bool((lut_val < 0).any()) and bool((lut_half != 0).any())
    k = ids.long()
    assert bool((want[lut_val[k] < 0] == void).all())
    sel = (lut_half[k] != 0) & (lut_val[k] >= 0)
    assert bool((want[sel & (win_half == 0)] == void).all()) and bool((want[sel & (win_half != 0)] != void).all())
    assert int((want == void).sum()) not in (0, 1000)


@pytest.mark.parametrize('rows', PC.SOFTMAX_ROWS)
def test_softmax_rows_and_bound(rows):
    """torch's f32 softmax stays inside the bound; rows over- or underflow without the max subtraction; the ties are exact"""
    for n in PC.SOFTMAX_N:
        x, ties = PC.softmax_rows(rows, n)
        p64, bound = PC.softmax_ref(x)
        assert bool(torch.isfinite(p64).all()) and bool(((p64.sum(1) - 1).abs() < 1e-12).all())
        ratio = ((torch.softmax(x, -1).double() - p64).abs() / bound).max().item()
        print(f'rows {rows} n {n}: torch f32 softmax at {ratio:.3f} of the bound')
        assert ratio < 1.0
        for r, first in ties.items():
            top = x[r].max()
            where = (x[r] == top).nonzero().flatten().tolist()
            assert len(where) == 2 and where[0] == first
            if r != 0:
                assert where[1] - where[0] == 64                         # the same lane
            else:
                assert (where[1] - where[0]) % 64 != 0                   # two lanes
        if rows >= 5:
            if n >= 63:
                assert bool(torch.isinf(x[1].exp()).any()) and bool((x[2].exp() < 2.0 ** -126).any())     # f32 exp, no max
                assert bool((p64[3] < 2.0 ** -126).any())                # the scaled row: probabilities underflow f32
                assert bool(torch.isinf(x[4]).any()) and bool(torch.isfinite(x[4, 0]))
    assert (rows - 1 in ties or rows == 1) and 0 in ties


@pytest.mark.parametrize('name', sorted(PC.TOPK_CASES))
def test_topk_cases_fit_and_check_topk_checks(name):
    B, Q, ld, col0, ncols, k, _ = PC.TOPK_CASES[name]
    dots = PC.topk_dots(name)
    assert dots.shape == (B * Q, ld)
    assert 8 * k + 4 * Q * (max(ncols) - 1) + 4 * Q <= 62 * 1024 and k <= 1024
    for c0, nc in zip(col0, ncols):
        assert c0 + nc <= ld and k <= Q * (nc - 1)
    # torch's own f32 softmax + a stable sort passes the checks; damaged results do not
    c0, nc = col0[-1], ncols[-1]
    p64, bound = PC.topk_ref(dots, B - 1, Q, c0, nc)
    flat32 = torch.softmax(dots[(B - 1) * Q:, c0:c0 + nc], -1)[:, :-1].reshape(-1)
    s, i = flat32.sort(descending=True, stable=True)
    s, i = s[:k], i[:k]
    PC.check_topk(i % (nc - 1), s, i // (nc - 1), p64, bound, Q, nc, k)
    if k < Q * (nc - 1):
        worst = flat32.argmin()
        i2, s2 = i.clone(), s.clone()
        i2[-1], s2[-1] = worst, flat32[worst]                            # incomplete: a better pair was left out
        with pytest.raises(AssertionError):
            PC.check_topk(i2 % (nc - 1), s2, i2 // (nc - 1), p64, bound, Q, nc, k)
    if k > 1:
        with pytest.raises(AssertionError):
            PC.check_topk(i.flip(0) % (nc - 1), s.flip(0), i.flip(0) // (nc - 1), p64, bound, Q, nc, k)
        i3 = i.clone()
        i3[1] = i3[0]
        with pytest.raises(AssertionError):
            PC.check_topk(i3 % (nc - 1), s, i3 // (nc - 1), p64, bound, Q, nc, k)


def test_tie_case_cuts_a_group():
    dots = PC.tie_dots()
    p64, _ = PC.topk_ref(dots, 0, PC.TIE_Q, 0, PC.TIE_NC)
    s, i = p64.sort(descending=True, stable=True)
    k = PC.TIE_K
    assert s[k - 1] == s[k] and s[k - 1] == s[k - 3] and s[k - 3] < s[k - 4]         # the k-th and (k+1)-th entries are equal
    assert (i[k - 3:k] // (PC.TIE_NC - 1)).tolist() == [0, 1, 2]                     # the cut group yields its lowest flat indices
    vals = p64.unique()
    assert vals.numel() == PC.TIE_NC - 1 and float((vals[1:] / vals[:-1]).min()) > 1 + 1e-3      # groups far apart: f32 keeps the order


@pytest.mark.parametrize('hw,size', PC.UPSAMPLE_CASES)
def test_upsample_case(hw, size):
    x, want, bound = PC.upsample_case(hw, size)
    t32 = torch.nn.functional.interpolate(x[None], size, mode='bilinear', align_corners=False)[0]
    ratio = ((t32.double() - want).abs() / bound).max().item()
    print(f'{hw} -> {size}: bound {bound.max().item():.2e}, torch f32 at {ratio:.3f} of it')
    assert ratio <= 1.0 and (size[0] * size[1]) % 256 != 0
