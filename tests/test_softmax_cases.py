"""tests/softmax_cases.py on the CPU: every family has what it claims (read from the float64 scores), the families tell a wrong
softmax from a right one, and the bound is achievable -- an emulation of a correct kernel of this project's design (f16 x 3
operands, log2 domain, f32 lse, lse-recompute backward; bf16 operands likewise) stays inside it in every family at the shapes the
GPU tests use."""
import pytest
import torch

import softmax_cases as SC

# (B, Q, S, masked): the shapes of tests/test_softmax_conditioning_gpu.py, section A
SHAPES = [(1, 37, 333, True), (2, 130, 200, True), (1, 100, 100, False)]
H = 4
_CACHE = {}


def _case(shape, bf16=False):
    key = (shape, bf16)
    if key not in _CACHE:
        B, Q, S, masked = shape
        c = SC.attention(B, Q, S, H, seed=S, masked=masked, bf16=bf16)
        go = torch.randn(B, Q, H * SC.D_HEAD, generator=torch.Generator().manual_seed(S + 1))
        if bf16:
            go = go.bfloat16().float()
        _CACHE[key] = (c, go, SC.attention_refs(c, go),
                       SC.attention_refs(c, go, torch.float32, p_dtype=torch.bfloat16 if bf16 else None))
    return _CACHE[key]


def _rows(c, s, name):
    """the float64 score rows (n, S) of one family and their blocked bits (n, S)"""
    sel = c.fam_of('lse') == c.fams.index(name)
    blocked = c.mask[:, None].expand_as(s)[sel] if c.mask is not None else torch.zeros_like(s[sel], dtype=torch.bool)
    return s[sel], blocked


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES)
def test_families_have_what_they_claim(shape, bf16):
    c = _case(shape, bf16)[0]
    S = c.S
    s = SC.scores(c)
    assert torch.isfinite(s).all()
    for t in (c.q * c.scale, c.k, c.v):
        assert t.abs().max().item() < SC.X3_RANGE
    if c.mask is not None:
        assert bool((~c.mask).any(-1).all())                                    # no row is fully masked
    vis = lambda name: [t.masked_fill(b, float('-inf')) for t, b in [_rows(c, s, name)]][0]      # noqa: E731
    top2 = lambda t: t.topk(2, -1).values                                                          # noqa: E731
    # the control and its scaled form
    u = _rows(c, s, 'unit')[0]
    assert 0.8 < u.std().item() < 1.2 and u.abs().max().item() < 7
    assert 4.8 < _rows(c, s, 'large')[0].std().item() < 7.2
    for name, m in (('shift_pos', SC.SHIFT), ('shift_neg', -SC.SHIFT)):
        r = _rows(c, s, name)[0]
        assert (r - m).abs().max().item() < 7 and 0.7 < (r - m).std().item() < 1.3
    # spikes: the arg-max position, its tile, the gap to the runner-up
    mid, last_tile = SC.mid_key(S), (S - 1) // SC.TILE
    assert 0 < mid // SC.TILE < last_tile and (S < 3 * SC.CHUNK or 0 < mid // SC.CHUNK < (S - 1) // SC.CHUNK)
    assert S % SC.TILE != 0                                                     # the last key sits in a ragged tail
    for name, key in (('spike_first', 0), ('spike_mid', mid), ('spike_last', S - 1)):
        r = vis(name)
        assert bool((r.argmax(-1) == key).all())
        t = top2(r)
        assert (t[:, 0] - t[:, 1]).min().item() > SC.SPIKE - 10
    # ramps: strictly rising along the keys up to the unit noise, so the maximum of every tile exceeds that of the tile before
    for name, amp in (('ramp', SC.RAMP), ('underflow', SC.UNDERFLOW)):
        r = _rows(c, s, name)[0]
        assert r.amax(-1).min().item() > amp - 10 and r[:, 0].abs().max().item() < 7
        if name == 'underflow':
            rv = vis(name)
            p = (rv - rv.amax(-1, keepdim=True)).float().exp()
            assert ((p == 0) & torch.isfinite(rv)).sum().item() > 0.5 * torch.isfinite(rv).sum().item()
    # tie: two maxima, equal to the bit, in different tiles and chunks, both visible
    t1, t2 = SC.tie_keys(S)
    assert t1 // SC.TILE != t2 // SC.TILE and t1 // SC.CHUNK != t2 // SC.CHUNK
    r = vis('tie')
    assert bool((r[:, t1] == r[:, t2]).all()) and bool((r[:, t1] == r.amax(-1)).all())
    assert bool((SC.scores(c, torch.float32)[c.fam_of('lse') == c.fams.index('tie')][:, t1]
                 == SC.scores(c, torch.float32)[c.fam_of('lse') == c.fams.index('tie')][:, t2]).all())
    assert (top2(r)[:, 0] - r.topk(3, -1).values[:, 2]).min().item() > SC.TIE - 10
    if c.mask is None:
        assert 'masked_max' not in c.fams and 'single_visible' not in c.fams
        return
    r, b = _rows(c, s, 'masked_max')
    assert bool(b.gather(1, r.argmax(-1, keepdim=True)).all())                  # the largest score is on a blocked key
    assert (r.amax(-1) - vis('masked_max').amax(-1)).min().item() > SC.BLOCKED_MAX - 10
    r, b = _rows(c, s, 'single_visible')
    assert bool(((~b).sum(-1) == 1).all()) and bool((~b)[:, S - 1].all())
    assert (r[:, S - 1] + SC.SHIFT).abs().max().item() < 7
    # A bounds every |score| of the row
    assert bool((c.A[..., None] >= s.abs() - 1e-9).all())


def test_families_discriminate():
    """an f32 softmax without the subtraction of the maximum is non-finite on shift_pos and underflow (and fine on the control); a
    maximum taken before masking is wrong on masked_max"""
    c, _, want, _ = _case(SHAPES[0])
    s = SC.scores(c, torch.float32)
    blocked = c.mask[:, None].expand_as(s)
    e = s.exp().masked_fill(blocked, 0.0)
    naive = e / e.sum(-1, keepdim=True)
    fam = c.fam_of('lse')
    bad = lambda name: bool((~torch.isfinite(naive[fam == c.fams.index(name)])).any())      # noqa: E731
    assert bad('shift_pos') and bad('underflow') and not bad('unit') and not bad('spike_mid')
    # one pass with the maximum of ALL keys, masked ones included
    m = s.amax(-1, keepdim=True)
    p = (s - m).exp().masked_fill(blocked, 0.0)
    vh = c.v.view(c.B, c.S, H, SC.D_HEAD).transpose(1, 2)
    out = ((p / p.sum(-1, keepdim=True)) @ vh).transpose(1, 2).reshape(c.B, c.Q, -1)
    r = SC.ratios('out', out, want['out'], SC.attention_refs(c, None, torch.float32)['out'], c.fam_of('rows'), c.fams, None, SC.U_F32)
    assert not r['masked_max'][2] <= 1.0 and r['unit'][2] <= 1.0


@pytest.mark.parametrize('form', ['f32', 'x3', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES)
def test_bound_is_achievable(shape, form):
    """the emulated kernel (softmax_cases.emulate) is within the bound in every family, for every output"""
    c, go, want, ref32 = _case(shape, form == 'bf16')
    got = SC.emulate(c, go, x3=form == 'x3', bf16=form == 'bf16')
    u = dict(f32=SC.U_F32, x3=SC.U_X3, bf16=SC.U_BF16)[form]
    for name, r in SC.attention_ratios(c, got, want, ref32, u).items():
        SC.assert_within(f'emulated {form} {shape} {name}', r)


WINDOW_CASES = [(7, (14, 21), 0), (7, (14, 21), 3), (12, (24, 36), 6)]


@pytest.mark.parametrize('ws,hw,shift', WINDOW_CASES)
def test_window_bound_is_achievable_with_the_row_term(ws, hw, shift):
    """The window attention cases of the GPU test against softmax_cases.emulate_window, a correct f32 kernel of that design
    (lse stored in f32, P recomputed from it). Every output is within the bound. For grad_k of the unshifted 7 x 7 case the
    bound as first stated, S = (1 + max A) max |want|, is NOT achievable: an `underflow` row has P = 1 on its last key up to
    the rounding of an lse of size 300, |delta| = 18 and |scale q| = 300 there, which leaves 0.1 on a gradient of size 370 --
    1.3 times that bound. With S_rows (softmax_cases.ratios) the same emulation stands at 0.14."""
    from test_window_attn_gpu import _coords, dense_ref
    heads, B, L = 2, 2, hw[0] * hw[1]
    C = heads * SC.D_HEAD
    win, reg, ly, lx = _coords(hw[0], hw[1], ws, shift)
    qkv, fams, fam = SC.window_qkv(B, heads, win, reg, ly * ws + lx, ws * ws, seed=100 * ws + shift, shifted=shift > 0)
    g = torch.Generator().manual_seed(ws + shift)
    table, go = torch.randn((2 * ws - 1) ** 2, heads, generator=g), torch.randn(B, L, C, generator=g)

    def run(dt):
        qd, td = qkv.to(dt).requires_grad_(), table.to(dt).requires_grad_()
        out, lse = dense_ref(qd, td, hw, ws, shift, heads)
        gq, gt = torch.autograd.grad(out, (qd, td), go.to(dt))
        return dict(out=out.detach(), lse=lse.detach(), grad_qkv=gq, grad_table=gt)
    w, r = run(torch.float64), run(torch.float32)
    A, S_rows = SC.window_scales(qkv, table, go, win, reg, ly, lx, ws, heads)
    e = SC.emulate_window(qkv, table, go, win, reg, ly, lx, ws, heads)
    part = lambda t, i: t[..., i * C:(i + 1) * C]                           # noqa: E731
    fam_rows, fam_lse = fam[:, :, None].expand(B, L, C), fam[:, None, :].expand(B, heads, L)
    tag = f'emulated window ws={ws} shift={shift}'
    SC.assert_within(f'{tag} out', SC.ratios('out', e['out'], w['out'], r['out'], fam_rows, fams, None, SC.U_F32))
    SC.assert_within(f'{tag} lse', SC.ratios('lse', e['lse'], w['lse'], r['lse'], fam_lse, fams, A, SC.U_F32))
    SC.assert_within(f'{tag} grad_q', SC.ratios('grad_rows', part(e['grad_qkv'], 0), part(w['grad_qkv'], 0), part(r['grad_qkv'], 0),
                                                fam_rows, fams, (A, fam_lse), SC.U_F32))
    for i, name in ((1, 'grad_k'), (2, 'grad_v')):
        args = ('grad_sum', part(e['grad_qkv'], i), part(w['grad_qkv'], i), part(r['grad_qkv'], i), None, fams, A, SC.U_F32)
        SC.assert_within(f'{tag} {name}', SC.ratios(*args, S_rows=S_rows[i - 1]))
        if (ws, shift, name) == (7, 0, 'grad_k'):
            first = SC.ratios(*args)['all']
            print(f'{tag} grad_k without S_rows: {first}')
            assert first[2] > 1.0
    SC.assert_within(f'{tag} grad_table', SC.ratios('grad_sum', e['grad_table'], w['grad_table'], r['grad_table'], None, fams, A,
                                                    SC.U_F32, S_rows=S_rows[2]))


@pytest.mark.parametrize('N', [8, 134, 1000, 4104])
def test_logit_rows(N):
    lg = SC.logit_rows(23, N, seed=N)
    x = lg.x.double()
    assert torch.isfinite(x).all() and set(lg.fam.tolist()) == set(range(len(lg.fams)))
    row = lambda name: x[lg.fam == lg.fams.index(name)]                 # noqa: E731
    for name, col in (('spike_first', 0), ('spike_mid', SC.mid_key(N)), ('spike_last', N - 1)):
        assert bool((row(name).argmax(-1) == col).all())
    t1, t2 = SC.tie_keys(N)
    r = row('tie')
    assert t1 != t2 and bool((r[:, t1] == r[:, t2]).all()) and bool((r.amax(-1) == SC.TIE).all()) and bool((r.argmax(-1) == t1).all())
    assert row('underflow').amax(-1).min().item() == SC.UNDERFLOW and row('shift_neg').amax(-1).max().item() < -SC.SHIFT + 7
    naive = lg.x.exp() / lg.x.exp().sum(-1, keepdim=True)
    assert not torch.isfinite(naive[lg.fam == lg.fams.index('shift_pos')]).all()
    assert bool((lg.A == x.abs().amax(1)).all())
