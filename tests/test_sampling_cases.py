"""CPU only: the cases, references and bounds of tests/sampling_cases.py are sound -- the closed form is the op (and where
F.grid_sample is not), every lattice combination occurs, the exclusion share of the off-lattice family is small, the sorted
scatter's corner counts sit exactly on its thresholds, and a correct kernel emulated in f32 (the closed form in f32) stands
below 1.0 of every bound."""
import pytest
import torch

import sampling_cases as SC
from oracle import ops as ref

PYR_RAGGED, PYR_POW2, PYR_TILED, DEGENERATE = SC.PYR_RAGGED, SC.PYR_POW2, SC.PYR_TILED, SC.DEGENERATE


@pytest.fixture(scope='module')
def lattice_case():
    return SC.case('B/pow2')


def test_closed_form_is_the_loop_oracle():
    c = SC.off_lattice([(3, 5), (6, 10)], 1, seed=1)
    out = SC.msda_closed_form(c.value, c.shapes, c.loc, c.aw, c.go)[0]
    want = ref.msda_core_loops(c.value, torch.tensor(c.shapes), c.loc, c.aw)
    assert (out - want).abs().max().item() <= 1e-12


def test_closed_form_equals_float64_autograd_off_the_minus_one_line(lattice_case):
    """... to 1e-10 wherever no pixel coordinate is exactly -1; AT -1 F.grid_sample keeps a one-sided grad_loc where mmcv's rule
    (and the kernels) skip the sample: the reason the closed form is the lattice reference"""
    c = lattice_case
    cf = SC._closed(c.value, c.shapes, c.loc, c.aw, c.go)
    ag = SC.msda_autograd(c.value, c.shapes, c.loc, c.aw, c.go)
    pc = c.loc.double() * SC._wh(c.shapes, torch.float64)[None, None, None, :, None, :] - 0.5
    on_line = (pc == -1.0).any(-1)
    assert bool(on_line.any())
    for k in ('out', 'grad_value', 'grad_attn'):
        assert (cf[k] - ag[k]).abs().max().item() <= 1e-10, k
    d = (cf['grad_loc'] - ag['grad_loc']).abs().amax(-1)
    assert d[~on_line].max().item() <= 1e-10
    assert d[on_line].max().item() > 1.0                     # grid_sample's one-sided derivative; the closed form's is 0 there
    assert cf['grad_loc'][on_line].abs().max().item() == 0.0
    # off the lattice the two agree everywhere
    a = SC.off_lattice(PYR_RAGGED, 1, seed=2)
    cf, ag = SC._closed(a.value, a.shapes, a.loc, a.aw, a.go), SC.msda_autograd(a.value, a.shapes, a.loc, a.aw, a.go)
    for k in cf:
        assert (cf[k] - ag[k]).abs().max().item() <= 1e-10 * max(1.0, ag[k].abs().max().item()), k


@pytest.mark.parametrize('shapes', [PYR_POW2, PYR_RAGGED, *DEGENERATE], ids=str)
def test_every_lattice_combination_occurs(shapes):
    c = SC.lattice(shapes, 2, seed=11)
    wh = SC._wh(c.shapes, torch.float64)[None, None, None, :, None, :]
    pc = torch.round((c.loc.double() * wh - 0.5) * 2) / 2              # nominal on a pyramid that is not of powers of two
    assert c.exact == all(SC._pow2(h) and SC._pow2(w) for h, w in shapes)
    if c.exact:
        assert torch.equal(pc, c.loc.double() * wh - 0.5)
    for l, (h, w) in enumerate(shapes):
        cx, cy = SC.lattice_classes(pc[:, :, :, l, :, 0], w), SC.lattice_classes(pc[:, :, :, l, :, 1], h)
        have = set(zip(cx.flatten().tolist(), cy.flatten().tolist()))
        # the classes a map of that size has along each axis (a 1-pixel axis has no interior, 0 == W - 1 there)
        ax = lambda n: set(SC.lattice_classes(torch.arange(-3, 2 * n + 2).double() / 2, n).tolist()) - {-1}    # noqa: E731
        for a in ax(w):
            for b in ax(h):
                assert (a, b) in have, (l, SC.LATTICE_CLASSES[a], SC.LATTICE_CLASSES[b])
        if h >= 3 and w >= 3:
            assert ax(w) == set(range(8)) and ax(h) == set(range(8))
    assert bool((c.aw == 0).any()) and bool((c.aw < 0).any())


@pytest.mark.parametrize('shapes', [PYR_RAGGED, PYR_TILED], ids=str)
def test_off_lattice_exclusion_share_is_below_one_percent(shapes):
    c = SC.off_lattice(shapes, 2, seed=3)
    share = SC.near_integer(c).double().mean().item()
    share_fused = SC.near_integer(c, c.fused_operands()[0]).double().mean().item()
    print(f'{shapes}: excluded {share:.4%} (fused operands {share_fused:.4%})')
    assert share <= 0.01 and share_fused <= 0.01
    for f in range(len(c.fams)):
        assert bool((c.fam == f).any())


@pytest.mark.parametrize('count', [255, 256, 767, 768])
def test_scatter_thresholds_are_hit_exactly(count):
    c = SC.threshold(count)
    a = SC.scatter_counts(c)                                           # (B, 4, 4, H, L)
    h, l = SC.THRESHOLD_HEAD, SC.THRESHOLD_LEVEL
    want = {255: [255], 256: [256], 767: [511, 256], 768: [512, 256]}[count]
    got = [int(a[0, 0, x, h, l]) for x in range(len(want))]
    assert got == want
    rest = a.clone()
    rest[0, 0, :len(want), h, l] = 0
    assert int(rest.max()) == 0                                        # everything else inside its first-pass window
    tot = SC.deferred_totals(a)
    assert int(tot[0, 0, 0, h, l]) == (0 if count == 255 else count)
    assert int(tot.sum()) == int(tot[0, 0, 0, h, l])
    assert SC.DEFER_MIN == 256 and SC.LIGHT_MAX == 768
    # some of the moved corners lie beyond the second pass' window as well, some inside it
    b = SC.scatter_counts(c, *SC.PASS_B)
    assert 0 < int(b[0, 0, 0, h, l]) < count


def test_one_pixel_level_known_answer():
    """a 1 x 1 level: every valid sample is the pixel times (1 - |wim|) (1 - |him|)"""
    shapes = [(1, 1), (2, 2), (4, 4)]
    c = SC.lattice(shapes, 2, seed=12)
    aw = torch.zeros_like(c.aw)
    aw[:, :, :, 0, 0] = 1.0
    out = SC.msda_closed_form(c.value, shapes, c.loc, aw, c.go)[0]
    pc = c.loc.double()[:, :, :, 0, 0] - 0.5                           # W = H = 1
    wgt = ((1 - pc.abs()).clamp_min(0)).prod(-1)                       # (B, Nq, H); 0 at |pc| >= 1: skipped
    want = wgt[..., None] * c.value.double()[:, 0][:, None]            # pixel 0 is the 1 x 1 level
    assert (out.view(c.B, c.Nq, SC.H, SC.D) - want).abs().max().item() <= 1e-15
    assert bool((wgt == 0.25).any()) and bool((wgt == 1.0).any()) and bool((wgt == 0).any())


def _emulation_ratios(c, fused):
    r = SC.Refs(c, fused)
    loc32, aw32 = c.fused_operands(torch.float32) if fused else (c.loc, c.aw)
    emu = SC._closed(c.value, c.shapes, loc32, aw32, c.go, torch.float32)
    names = ['out', 'grad_value', 'grad_attn'] + (['grad_loc'] if r.loc_compared else [])
    if fused:
        emu['grad_rows'] = SC.rows_gradient(c, emu['grad_loc'], emu['grad_attn'], aw32, torch.float32)
        names.append('grad_rows')
    return {n: r.ratios(n, emu[n]) for n in names}, r


EMULATED = [n for n in SC.CASES if n not in ('D/outside', 'F', 'E/255', 'E/256', 'E/768')]


@pytest.mark.parametrize('name', EMULATED)
@pytest.mark.parametrize('fused', [False, True], ids=['given', 'fused'])
def test_f32_emulation_of_a_correct_kernel_is_inside_every_bound(name, fused):
    c = SC.case(name)
    res, r = _emulation_ratios(c, fused)
    for out, rat in res.items():
        SC.assert_within(f'{name} {"fused" if fused else "given"} {out}', rat)
    assert r.excluded <= 0.01 or (c.lattice and not c.exact)


def test_bound_rejects_border_errors_that_five_per_mille_of_the_maximum_lets_through(lattice_case):
    """two wrong kernels, emulated: a flipped sign of grad_loc x on samples whose right corner is dropped (pixel coordinate W - 1 or
    W - 0.5), and a missing W_l factor on the same samples -- wherever the value is below 0.25 % of max |grad_loc|, so that the
    earlier tolerance (5e-3 max |grad_loc|) passes both. Each stands far above the bound."""
    c, r = lattice_case, SC.refs('B/pow2')
    want = r.want['grad_loc']
    emu = SC._closed(c.value, c.shapes, c.loc, c.aw, c.go, torch.float32)['grad_loc'].double()
    wh = SC._wh(c.shapes, torch.float64)[None, None, None, :, None, :]
    pcx = (c.loc.double() * wh - 0.5)[..., 0]
    w = wh[..., 0].expand_as(pcx)
    small = (want[..., 0].abs() < 2.5e-3 * want.abs().max()) & (want[..., 0] != 0)
    border = ((pcx == w - 1) | (pcx == w - 0.5)) & small
    assert int(border.sum()) > 100
    for wrong_x in (-emu[..., 0], emu[..., 0] / w):
        wrong = emu.clone()
        wrong[..., 0] = torch.where(border, wrong_x, emu[..., 0])
        assert (wrong - want).abs().max().item() <= 5e-3 * want.abs().max().item()
        worst = max(v[2] for v in r.ratios('grad_loc', wrong).values())
        assert worst > 100.0, worst


def test_outside_case_is_all_zeros_and_inf_row_reference_stays_finite_elsewhere():
    c = SC.outside(seed=20)
    for t in SC.msda_closed_form(c.value, c.shapes, c.loc, c.aw, c.go):
        assert float(t.abs().max()) == 0.0
    a = SC.off_lattice(PYR_TILED, 1, seed=4)
    f = SC.with_inf_row(a, 0, 700)
    gv = SC.msda_closed_form(f.value, f.shapes, f.loc, f.aw, f.go)[1]
    gv0 = SC.msda_closed_form(a.value, a.shapes, a.loc, a.aw, a.go)[1]
    fin = torch.isfinite(gv)
    assert 0.5 < fin.double().mean().item() < 1.0                      # the row reaches some pixels of head h, not all
    touched = (~fin).any(-1)                                           # (B, Nv, H): whole heads of a pixel
    assert torch.equal(touched[..., None].expand_as(fin), ~fin)
    # a pixel the row does not reach keeps the gradient of the other rows (the row's own share of it is 0)
    g2 = a.go.clone()
    g2[0, 700] = 0.0
    gv2 = SC.msda_closed_form(a.value, a.shapes, a.loc, a.aw, g2)[1]
    assert torch.equal(gv[fin], gv2[fin]) and not torch.equal(gv0, gv2)


def test_point_sets_hold_the_special_points():
    pts, fam = SC.points(7, 12, 200, seed=1)
    assert len(pts) == (2 * 12 + 1) * (2 * 7 + 1) + 200 and int((fam == 1).sum()) == 200
    xs = set(pts[fam == 0][:, 0].tolist())
    assert 0.0 in xs and 1.0 in xs and all(float(torch.tensor(i / 12)) in xs for i in range(13))
    assert all(float(torch.tensor((i + 0.5) / 12)) in xs for i in range(12))
    pts, fam = SC.points(16, 16, 250, seed=1, full=False)
    assert len(pts) == 320 and len(set(pts[fam == 0][:, 0].tolist())) == 33 and len(set(pts[fam == 0][:, 1].tolist())) == 33
    # the band-stationary backward: rows 3 | 4 and 7 | 8 are the band edges of (H, W) = (9, 4096), every row one of (3, 16384)
    for (hh, ww, band) in ((9, 4096, 4), (3, 16384, 1)):
        assert band == min(hh, max(1, 16384 // ww))
        pts, fam = SC.band_points(hh, ww, band, 300, seed=2)
        assert pts.shape == (300, 2) and int((fam == 1).sum()) >= 150
        iy = pts[fam == 0][:, 1].double() * hh - 0.5
        for e in range(band, hh, band):
            assert int(((iy > e - 1) & (iy < e)).sum()) >= 20         # tap rows e - 1 and e: two workgroups
            assert bool(((iy - (e - 1)).abs() < 1e-5).any()) and bool(((iy - e).abs() < 1e-5).any())   # nominally ON a row's centre
    r = SC.grid_sample_refs(torch.randn(2, 1, 9, 64), torch.rand(2, 50, 2), torch.randn(2, 1, 50))
    assert r['out'][0].dtype == torch.float64 and r['grad'][2].min().item() >= 0.0
