"""-m gpu: the bilinear samplers on the pixel lattice, at map borders and at the thresholds of the sorted scatter -- the cases,
float64 references and bounds of tests/sampling_cases.py (tests/test_sampling_cases.py shows on the CPU that they are sound)
through every entry point of the two families:

  MSDeformAttn   ops.msda_forward, msda_forward_hostlevels, msda_forward_fused (all three lane mappings: 8 x 8 blocks on
                 (8,8),(16,16),(32,32), 4 x 4 tiles on (4,4),(8,8),(16,16), strips on every other pyramid; the generic fused kernel
                 on the two-level pyramid), msda_forward_fused_bf16 row- and head-major, msda_backward, msda_backward_hostlevels
                 in both forms of ops.MSDA_BWD_2P, msda_rows_backward, MultiScaleDeformableAttnFunction; the generic kernels
                 (CGG_MSDA_GENERIC=1, read when the library loads) in a child process
  point samplers point_sample_nhwc, point_sample_planes, point_sample_rows forward and band-stationary backward,
                 point_sample_nhwc_x3

Every test prints the worst |error| / bound of each family of samples; the bound is FACTOR = 8 times max(e_ref, 2^-24 S), see
sampling_cases. Nothing is left out of any comparison except, in the off-lattice family A, the grad_loc elements whose sample
has a pixel coordinate within 1e-3 px of an integer in float64 (their share is asserted <= 1 %).

Out of scope: a non-finite `value`. The forward multiplies a zero weight into the clamped load of an outside corner, so an inf at
a border pixel reaches samples the reference would not let it reach; whether to pay for selects there is a performance decision,
and no test here pins either behaviour. (A non-finite grad_out ROW is in scope: family F.)

The thresholds of family E (MSDA_DEFER_MIN = 256, MSDA_LIGHT_MAX = 768) are the kernel's constants at the time of writing; if
they are retuned the four cases stop sitting on them but remain valid correctness tests of the two-pass scatter.

Measured on the MI355X (worst error / bound over the families; 1.0 is the limit). No finding: every entry point of both families
is inside every bound, so no kernel changed.

  case         forward f32  fused f32  fused bf16*  grad_value  grad_loc  grad_attn  row gradient  grad_loc left out
  A/ragged     0.13         0.13       0.99         0.13        0.18      0.14       0.18          0.38 %
  A/tiled      0.035        0.13       1.00         0.13        0.084     0.068      0.13          0.40 %
  B/pow2       0.10         0.11       1.00         0.062       0.12      0.089      0.064         none
  B/ragged     0.12         0.12       0.99         0.13        --        0.14       0.12          (nominal lattice: not compared)
  C/1x1        0.088        0.091      1.00         0.063       0.13      0.13       0.078         none
  C/1x3        0.15         0.13       0.99         0.18        --        0.13       0.13          (nominal)
  C/3x1        0.16         0.11       1.00         0.13        --        0.13       0.077         (nominal)
  C/1x1/off    0.11         0.15       1.00         0.074       0.084     0.20       0.099         0.30 %
  C/1x3/off    0.13         0.13       1.00         0.11        0.13      0.13       0.14          0.41 %
  C/3x1/off    0.13         0.14       1.00         0.11        0.10      0.13       0.087         0.21 %
  D/collide    0.11         0.17       1.00         0.17        0.12      0.093      0.066         none
  D/outside    every output of every entry exactly zero
  E/255 .. 768 grad_value 0.025 .. 0.036 in both forms of MSDA_BWD_2P
  F            grad_value 0.068 (two passes), 0.070 (one pass), 0.058 (msda_backward), 0.12 (generic kernel); finite wherever
               the reference is
  generic kernels (child process): A/ragged, B/pow2, C/1x1, C/3x1/off, D/collide at most 0.22 (bf16 output 1.00*), D/outside zeros
  point_sample_nhwc / _planes / _rows forward and grad_planes, both maps: 0.125 (the kernels reproduce ATen's f32 arithmetic to
  the bit, so their error IS e_ref); point_sample_nhwc_x3: 0.18 (lattice), 0.12 (random)
  * a bf16 output: the bound adds half a bf16 ulp of the reference (`_bf16_rounding`), which the output's own rounding all but uses
    up whenever the f32 result lies next to a rounding boundary; the f32 part of the error is that of the f32 fused column.

On lattice cases e_ref is the closed form in f32, i.e. of the size of one summation over the 32 channels; the kernels' 0.06 .. 0.13
there say their error is of that size too. The earlier tolerance of the backward tests, 5e-3 max |grad_loc|, is about a thousand
bounds wide on the ragged pyramid (tests/test_sampling_cases.py shows two border errors it passes and this bound rejects by a factor > 100)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cgg_amd  # noqa: E402, F401
from cgg_amd import ops  # noqa: E402

import sampling_cases as SC  # noqa: E402
from test_norm_conditioning_gpu import _bf16_rounding  # noqa: E402

pytestmark = pytest.mark.gpu

P = SC.P
MSDA_CASES = ['A/ragged', 'A/tiled', 'B/pow2', 'B/ragged', 'C/1x1', 'C/1x3', 'C/3x1', 'C/1x1/off', 'C/1x3/off', 'C/3x1/off', 'D/collide']
GENERIC_CASES = ['A/ragged', 'B/pow2', 'C/1x1', 'C/3x1/off', 'D/collide', 'D/outside', 'F']


def _report(label, ratios):
    SC.assert_within(label, ratios)


def _dev_levels(c, dev):
    return torch.tensor(c.shapes, dtype=torch.int64, device=dev), torch.tensor(c.starts, dtype=torch.int64, device=dev)


class _TwoPass:
    """ops.MSDA_BWD_2P set to `on` inside the block"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old, ops.MSDA_BWD_2P = ops.MSDA_BWD_2P, self.on

    def __exit__(self, *a):
        ops.MSDA_BWD_2P = self.old


def forward_entries(dev, name, R, RF, RB, generic=False):
    """{entry: out (B, Nq, H D) on the host} of every forward entry point, and the Refs each is held to"""
    c, cb = R.case, RB.case
    ss, st = _dev_levels(c, dev)
    v, loc, aw, rows, refp = (t.to(dev) for t in (c.value, c.loc, c.aw, c.rows, c.refp))
    res = [('msda_forward', ops.msda_forward(v, ss, st, loc, aw), R, None),
           ('msda_forward_hostlevels', ops.msda_forward_hostlevels(v, c.shapes, c.starts, loc, aw), R, None),
           ('msda_forward_fused', ops.msda_forward_fused(v, c.shapes, c.starts, rows, refp, P), RF, None)]
    vb, rb = cb.value.bfloat16().to(dev), cb.rows.bfloat16().to(dev)
    assert torch.equal(vb.float().cpu(), cb.value) and torch.equal(rb.float().cpu(), cb.rows)          # bf16-representable
    ex = _bf16_rounding(RB.want['out'])
    res.append(('msda_forward_fused_bf16', ops.msda_forward_fused_bf16(vb, c.shapes, c.starts, rb, refp, P).float(), RB, ex))
    if c.L == 3 and not generic:            # (the head-major kernel is the 3-level, 4-point stream's; it has no generic form)
        vhm = vb.permute(0, 2, 1, 3).contiguous()
        res.append(('msda_forward_fused_bf16 head-major',
                    ops.msda_forward_fused_bf16(vhm, c.shapes, c.starts, rb, refp, P, head_major=True).float(), RB, ex))
    return res


def backward_entries(dev, name, R, RF):
    """[(entry, {output: tensor}, Refs)] of every backward entry point"""
    c = R.case
    ss, st = _dev_levels(c, dev)
    v, loc, aw, rows, refp, go = (t.to(dev) for t in (c.value, c.loc, c.aw, c.rows, c.refp, c.go))
    res = []
    gv, gl, ga = ops.msda_backward(v, ss, st, loc, aw, go)
    res.append(('msda_backward', dict(grad_value=gv, grad_loc=gl, grad_attn=ga), R))
    for on in (True, False):
        with _TwoPass(on):
            gv, gl, ga = ops.msda_backward_hostlevels(v, c.shapes, c.starts, loc, aw, go)
            res.append((f'msda_backward_hostlevels 2P={int(on)}', dict(grad_value=gv, grad_loc=gl, grad_attn=ga), R))
    gv, grows = ops.msda_rows_backward(v, rows, refp, c.shapes, c.starts, P, go)
    res.append(('msda_rows_backward', dict(grad_value=gv, grad_rows=grows), RF))
    v2, l2, a2 = (t.clone().requires_grad_(True) for t in (v, loc, aw))
    out = ops.MultiScaleDeformableAttnFunction.apply(v2, ss, st, l2, a2, 64)
    out.backward(go)
    res.append(('MultiScaleDeformableAttnFunction', dict(out=out.detach(), grad_value=v2.grad, grad_loc=l2.grad, grad_attn=a2.grad), R))
    return res


def check_case(dev, name, R, RF, RB, generic=False):
    """every entry point on one case: prints the worst ratio of each family per (entry, output), asserts them all"""
    assert R.excluded <= 0.01 and RF.excluded <= 0.01 or not R.loc_compared, (R.excluded, RF.excluded)
    worst = 0.0
    for entry, out, refs, extra in forward_entries(dev, name, R, RF, RB, generic):
        rat = refs.ratios('out', out, extra)
        _report(f'{name} {entry} out', rat)
        worst = max(worst, max(v[2] for v in rat.values()))
    for entry, outs, refs in backward_entries(dev, name, R, RF):
        for k, t in outs.items():
            if k == 'grad_loc' and not refs.loc_compared:
                continue
            rat = refs.ratios(k, t)
            _report(f'{name} {entry} {k}', rat)
            worst = max(worst, max(v[2] for v in rat.values()))
    print(f'{name}: worst error / bound {worst:.3g}; grad_loc elements left out {R.excluded:.3%}')


def _refs3(name):
    return SC.refs(name), SC.refs(name, True), SC.refs(name + '/bf16', True)


@pytest.mark.parametrize('name', MSDA_CASES)
def test_msda_entry_points(dev, name):
    """families A (off-lattice, tight grad_loc), B (on the lattice), C (one-row / one-column levels), D (collisions)"""
    check_case(dev, name, *_refs3(name))


def _dirty(dev, *shapes):
    """the caching allocator's next blocks of these sizes hold NaN"""
    junk = [torch.full(s, float('nan'), device=dev) for s in shapes]
    del junk


def check_outside(dev, generic=False):
    """every sample outside every map: the four outputs are zeros -- also grad_loc / grad_attn of the hostlevels entries, which
    WRITE them into uninitialised memory where the split backward applies"""
    c = SC.case('D/outside')
    R, RF, RB = _refs3('D/outside')
    for r in (R, RF):
        assert all(float(t.abs().max()) == 0.0 for t in r.want.values())
    for entry, out, _, _ in forward_entries(dev, 'D/outside', R, RF, RB, generic):
        assert float(out.abs().max()) == 0.0, entry
    _dirty(dev, tuple(c.loc.shape), tuple(c.aw.shape), tuple(c.loc.shape), tuple(c.aw.shape))
    for entry, outs, _ in backward_entries(dev, 'D/outside', R, RF):
        for k, t in outs.items():
            assert float(t.abs().max()) == 0.0, (entry, k)             # (NaN fails this too)
    print('D/outside: every output of every entry is zero')


def test_msda_all_samples_outside_give_zeros(dev):
    check_outside(dev)


def test_msda_one_pixel_level_known_answer(dev):
    """a 1 x 1 level with a one-hot weight: the pixel times (1 - |wim|) (1 - |him|), exact in f32 on the half-integer lattice"""
    c = SC.case('C/1x1')
    ss, st = _dev_levels(c, dev)
    aw = torch.zeros_like(c.aw)
    aw[:, :, :, 0, 0] = 1.0
    got = ops.msda_forward(c.value.to(dev), ss, st, c.loc.to(dev), aw.to(dev)).cpu().view(c.B, c.Nq, SC.H, SC.D)
    pc = c.loc[:, :, :, 0, 0] - 0.5
    wgt = ((1 - pc.abs()).clamp_min(0)).prod(-1)
    want = wgt[..., None] * c.value[:, 0][:, None]
    assert torch.equal(got, want)
    assert bool((wgt == 0.25).any()) and bool((wgt == 1.0).any()) and bool((wgt == 0).any())


@pytest.mark.parametrize('count', [255, 256, 767, 768])
def test_msda_sorted_scatter_thresholds(dev, count):
    """family E: a first-pass unit with exactly 255 / 256 out-of-window corners (below MSDA_DEFER_MIN it scatters them itself, from
    it on it defers them), a second-pass region with exactly 767 / 768 deferred corners (below MSDA_LIGHT_MAX the no-sort form, from
    it on the sort) -- grad_value against float64 in both forms of ops.MSDA_BWD_2P. The counts are asserted in
    tests/test_sampling_cases.py from the documented geometry; should the constants be retuned, this remains a valid test of
    the scatter away from its thresholds."""
    name = f'E/{count}'
    c, R = SC.case(name), SC.refs(name)
    v, loc, aw, go = (t.to(dev) for t in (c.value, c.loc, c.aw, c.go))
    for on in (True, False):
        with _TwoPass(on):
            gv, _, _ = ops.msda_backward_hostlevels(v, c.shapes, c.starts, loc, aw, go)
        _report(f'{name} msda_backward_hostlevels 2P={int(on)} grad_value', R.ratios('grad_value', gv))


def check_inf_row(dev, generic=False):
    """family F: wherever the float64 grad_value is finite the kernel's is finite and within the bound (one direction only: at an
    exactly zero weight the reference itself forms 0 x inf)"""
    c, R = SC.case('F'), SC.refs('F')
    fin = torch.isfinite(R.want['grad_value'])
    assert 0.5 < fin.double().mean().item() < 1.0
    v, loc, aw, go = (t.to(dev) for t in (c.value, c.loc, c.aw, c.go))
    for on in ((None,) if generic else (True, False)):
        with _TwoPass(bool(on)):
            gv, _, _ = ops.msda_backward_hostlevels(v, c.shapes, c.starts, loc, aw, go)
        assert bool(torch.isfinite(gv.cpu()[fin]).all()), 'the +inf row leaked into pixels it does not touch'
        _report(f'F msda_backward_hostlevels {"generic" if generic else f"2P={int(on)}"} grad_value', R.ratios('grad_value', gv))
    if not generic:
        ss, st = _dev_levels(c, dev)
        gv, _, _ = ops.msda_backward(v, ss, st, loc, aw, go)
        _report('F msda_backward grad_value', R.ratios('grad_value', gv))


def test_msda_non_finite_grad_out_row_stays_in_its_pixels(dev):
    check_inf_row(dev)


def test_msda_generic_kernels_in_a_child_process(dev, tmp_path):
    """CGG_MSDA_GENERIC=1 is read when the library loads: a fresh process runs GENERIC_CASES through the same checks (the
    references travel in a file, they are not computed twice)"""
    path = str(tmp_path / 'refs.pt')
    refs = {n: (_refs3(n) if n != 'F' else (SC.refs('F'),)) for n in GENERIC_CASES}
    torch.save(refs, path)
    env = dict(os.environ, CGG_MSDA_GENERIC='1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and 'sampling generic worker OK' in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------------
# point samplers
# ------------------------------------------------------------------------------------------------
def _point_report(label, got, refs, fam=None, extra=None):
    _report(label, SC.sample_ratios(got, *refs, fam, SC.POINT_FAMILIES if fam is not None else ('all',), None, extra))


def test_point_sample_nhwc_and_planes_on_the_pixel_lattice(dev):
    """(H, W) = (7, 12): exactly 0, exactly 1, every pixel centre and boundary in every (x, y) combination, 200 random points"""
    Hh, Ww, C, B = 7, 12, 8, 2
    g = torch.Generator().manual_seed(31)
    pts, fam = SC.points(Hh, Ww, 200, seed=31)
    pts = torch.stack([pts, pts.flip(0)], 0)                            # (B, N, 2)
    fam = torch.stack([fam, fam.flip(0)], 0)
    feat = torch.randn(B, C, Hh, Ww, generator=g)
    refs = SC.grid_sample_refs(feat, pts)['out']                        # (B, C, N)
    got = ops.point_sample_nhwc(feat.permute(0, 2, 3, 1).contiguous().to(dev), pts.to(dev)).transpose(1, 2)
    _point_report('point_sample_nhwc', got, refs, fam[:, None, :].expand(B, C, -1))
    planes = torch.randn(3, Hh, Ww, generator=g)
    index = torch.tensor([2, 0, 1, 2], dtype=torch.int32)
    pts4 = torch.stack([pts[0], pts[1], pts[0].roll(7, 0), pts[1].roll(11, 0)], 0)
    fam4 = torch.stack([fam[0], fam[1], fam[0].roll(7, 0), fam[1].roll(11, 0)], 0)
    refs = SC.grid_sample_refs(planes[index.long()][:, None], pts4)['out']                      # (4, 1, N)
    got = ops.point_sample_planes(planes.to(dev), index.to(dev), pts4.to(dev))[:, None]
    _point_report('point_sample_planes', got, refs, fam4[:, None, :])


@pytest.mark.parametrize('Hh,Ww,band', [(9, 4096, 4), (3, 16384, 1)])
def test_point_sample_rows_band_edges(dev, Hh, Ww, band):
    """the band-stationary backward: a workgroup owns `band` = 16384 / W rows of a plane. (9, 4096): bands of 4, 4 and 1 rows,
    with points whose two tap rows straddle each band edge; (3, 16384), the stated width limit: bands of one row, so every
    sample's taps fall in two workgroups. 2 planes, 300 points each; forward and gradient against float64 grid_sample."""
    rows, n = 2, 300
    g = torch.Generator().manual_seed(33)
    pf = [SC.band_points(Hh, Ww, band, n, seed=40 + j) for j in range(rows)]
    pts, fam = torch.stack([p for p, _ in pf], 0), torch.stack([f for _, f in pf], 0)
    planes = torch.randn(rows, Hh, Ww, generator=g)
    gout = torch.randn(rows, n, generator=g)
    refs = SC.grid_sample_refs(planes[:, None], pts, gout[:, None])
    pd = planes.to(dev).requires_grad_(True)
    assert ops.point_sample_rows_ok(pd, pts.to(dev))
    out = ops.point_sample_rows(pd, pts.to(dev))
    out.backward(gout.to(dev))
    _point_report(f'point_sample_rows ({Hh}, {Ww}) out', out.detach()[:, None], refs['out'], fam[:, None, :])
    _point_report(f'point_sample_rows ({Hh}, {Ww}) grad_planes', pd.grad[:, None], refs['grad'])
    assert int((refs['grad'][0] != 0).sum()) > 2 * n                    # the gradient is not trivially empty


def test_point_sample_nhwc_x3_on_the_pixel_lattice(dev):
    """(16, 16), C = 256, 5 groups of 64 points: the special x of a row, the special y of a column, the corners, 250 random
    points. The x3 images are unpacked (16 x = hi + lo in f16 pieces); their 22 significand bits add 2^-22 |want| to the bound."""
    Hh, Ww, C, B, groups = 16, 16, 256, 2, 5
    g = torch.Generator().manual_seed(35)
    pts, fam = SC.points(Hh, Ww, 250, seed=35, full=False)
    assert len(pts) == groups * 64
    perm = torch.randperm(len(pts), generator=g)
    pts, fam = torch.stack([pts, pts[perm]], 0), torch.stack([fam, fam[perm]], 0)
    feat = torch.randn(B, C, Hh, Ww, generator=g) * 2
    refs = SC.grid_sample_refs(feat, pts)['out']                        # (B, C, N)
    nhwc = feat.permute(0, 2, 3, 1).contiguous().to(dev)
    assert ops.point_sample_nhwc_x3_ok(nhwc, pts.to(dev), groups)
    packs = ops.point_sample_nhwc_x3(nhwc, pts.to(dev), groups)
    got = []
    for pk in packs:                                                    # hi / lo (B, P / 32, C / 8, 32, 8) f16 bits
        x = (pk.hi.view(torch.float16).double() + pk.lo.view(torch.float16).double()) / 16.0
        got.append(x.permute(0, 1, 3, 2, 4).reshape(B, 64, C))
    got = torch.cat(got, 1).transpose(1, 2)                             # (B, C, N)
    _point_report('point_sample_nhwc_x3', got, refs, fam[:, None, :].expand(B, C, -1), SC.x3_rounding(refs[0]))


# ------------------------------------------------------------------------------------------------
# the child process of test_msda_generic_kernels_in_a_child_process
# ------------------------------------------------------------------------------------------------
def main(path):
    assert os.environ.get('CGG_MSDA_GENERIC') and torch.cuda.is_available()
    dev = torch.device('cuda:0')
    refs = torch.load(path, weights_only=False)
    for name, r in refs.items():
        SC._CASES[name] = r[0].case
        SC._REFS[(name, False)] = r[0]
        if len(r) == 3:
            SC._REFS[(name, True)], SC._REFS[(name + '/bf16', True)] = r[1], r[2]
            SC._CASES[name + '/bf16'] = r[2].case
    for name in GENERIC_CASES:
        if name == 'F':
            check_inf_row(dev, generic=True)
        elif name == 'D/outside':
            check_outside(dev, generic=True)
        else:
            check_case(dev, name, *_refs3(name), generic=True)
    print('sampling generic worker OK', flush=True)


if __name__ == '__main__':
    main(sys.argv[1])
