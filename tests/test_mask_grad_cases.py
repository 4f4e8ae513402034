"""tests/mask_grad_cases.py before it meets a kernel. CPU only.

EXACT -- every operand is an odd integer that survives bf16 with an empty low piece; both references are f32 values whose sums of
magnitudes stay below 2^24, so they are THE result in either mode and under any summation order.

TABLE -- the plan of csrc/mask_logits_bwd.hip, restated in `MG.plan`, is pinned at the shapes the issue names, and the set of cases
covers every edge it claims: row tiles, row groups, half-wave rows, half steps, chunk tails, the tile wrap, the batch stride.

TEETH -- each of the eight seeded faults changes the reference of every case that has its edge; none applies nowhere.

HOST -- `LazyMasks.select`, `preselect` + `select` and `select_by_weights` on the CPU (where `_contract` is torch.bmm) equal the
dense float64 formulation, outputs and gradients, bit for bit."""
import pytest
import torch

import mask_grad_cases as MG
from cgg_amd.mask2former_head import LazyMasks

SHAPES = sorted({(c.B, c.Q, c.h, c.w) for c in MG.CASES})


# ------------------------------------------------------------------------------------------------
# EXACT
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,Q,h,w', SHAPES, ids=lambda v: str(v))
def test_operands_and_references_are_exact(B, Q, h, w):
    o = MG.operands(B, Q, h, w)
    for name, t in (('embed', o.embed), ('feat', o.feat), ('grad_out', o.grad_out)):
        assert t.dtype == torch.float32 and t.is_contiguous()
        assert torch.equal(t.bfloat16().float(), t), f'{name}: not a bf16 value'
        assert not (t - t.bfloat16().float()).bfloat16().any(), f'{name}: a low piece'            # the (hi, lo) pair of split mode
        assert ((t.abs() == 1) | (t.abs() == 3)).all(), f'{name}: outside the odd integers of {MG.VALUES}'
        if t.numel() >= 64:
            assert {float(v) for v in t.unique()} == {float(v) for v in MG.VALUES}, f'{name}: a value never drawn'
    ge, gf = MG._reference(B, Q, h, w)
    assert tuple(ge.shape) == (B, Q, MG.C) and tuple(gf.shape) == (B, MG.C, h, w) and ge.dtype == gf.dtype == torch.float64
    for name, r in (('grad_embed', ge), ('grad_feat', gf)):
        assert torch.equal(r.float().double(), r), f'{name}: the reference is not an f32'
        assert torch.equal(r, r.round()), f'{name}: not an integer'
    # sums of magnitudes: no partial sum, in any order, leaves the integers below 2^24
    top_f = torch.einsum('bqc,bqp->bcp', o.embed.abs().double(), o.grad_out.flatten(2).abs().double()).max().item()
    top_e = torch.einsum('bqp,bcp->bqc', o.grad_out.flatten(2).abs().double(), o.feat.flatten(2).abs().double()).max().item()
    assert top_f <= 9 * Q <= 9 * 520 < 2 ** 24 and top_e <= 9 * h * w <= 9 * 66808 < 2 ** 24
    # parity: n odd terms
    assert ((ge.abs() % 2) == (h * w) % 2).all() and ((gf.abs() % 2) == Q % 2).all()


def test_references_equal_f32_sums_in_two_orders():
    """the float64 einsum against f32 sums taken front to back and back to front in blocks of 16, at the deepest contractions of the table"""
    for B, Q, h, w in ((3, 513, 4, 8), (1, 33, 8, 134)):
        o = MG.operands(B, Q, h, w)
        ge, gf = MG._reference(B, Q, h, w)
        E, F_, G = o.embed, o.feat.flatten(2), o.grad_out.flatten(2)
        for order in (range(0, Q, 16), reversed(range(0, Q, 16))):
            acc = torch.zeros(B, MG.C, h * w)
            for q0 in order:
                acc = acc + torch.einsum('bqc,bqp->bcp', E[:, q0:q0 + 16], G[:, q0:q0 + 16])
            assert torch.equal(acc.double(), gf.flatten(2))
        for order in (range(0, h * w, 16), reversed(range(0, h * w, 16))):
            acc = torch.zeros(B, Q, MG.C)
            for p0 in order:
                acc = acc + torch.einsum('bqp,bcp->bqc', G[..., p0:p0 + 16], F_[..., p0:p0 + 16])
            assert torch.equal(acc.double(), ge)


# ------------------------------------------------------------------------------------------------
# TABLE
# ------------------------------------------------------------------------------------------------
def test_plan_at_the_shapes_the_issue_names():
    p = MG.plan(1, 33, 1032, True)
    assert (p.nsteps, p.steps_per_chunk, p.nchunks, p.last_chunk, p.half_step) == (65, 64, 2, 1, True)
    p = MG.plan(3, 129, 1056, True)
    assert (p.nsteps, p.steps_per_chunk, p.nchunks, p.last_chunk, p.half_step) == (66, 64, 2, 2, False)
    p = MG.plan(1, 33, 1072, False)
    assert (p.nsteps, p.steps_per_chunk, p.nchunks, p.last_chunk, p.half_step) == (67, 64, 2, 3, False)
    p = MG.plan(512, 2, 264, True)                                  # the wrap: one workgroup of 8 waves, 9 tiles, the ninth ragged
    assert (p.cap, p.T, p.gx, p.wraps, p.ragged_tile, p.nchunks, p.half_step) == (1, 9, 1, True, True, 1, True)
    p = MG.plan(2, 100, 256 * 256, False)                           # the largest case of test_mask_logits_backward_vs_float64: T = 8 cap
    assert (p.T, p.cap, p.gx, p.wraps) == (2048, 256, 256, False)
    p = MG.plan(2, 100, 200 * 334, False)                           # a 1333 x 800 training image at B = 2 wraps
    assert (p.T, p.gx, p.wraps) == (2088, 256, True)
    assert MG.plan(511, 2, 264, True).wraps is False                # one image less: cap = 2, no wrap -- 512 is the smallest batch
    assert MG.plan(512, 2, 256, True).wraps is False                # one tile less: T = 8
    assert MG.plan(1, 1, 1 << 20, True).steps_per_chunk == 128      # steps_per_chunk > 64 needs B npix > 2^20: left out
    assert max(MG.case_plan(c).steps_per_chunk for c in MG.CASES) == 64
    p = MG.plan(3, 513, 56, False)
    assert p.feat_groups == [(0, 256, 16), (256, 256, 16), (512, 1, 1)]
    assert p.embed_groups == [(0, 128, 4), (128, 128, 4), (256, 128, 4), (384, 128, 4), (512, 1, 1)]
    p = MG.plan(3, 136, 32, True)
    assert p.feat_groups == [(0, 128, 8), (128, 8, 1)] and p.embed_groups == [(0, 128, 4), (128, 8, 1)]
    assert MG.plan(3, 136, 32, False).feat_groups == [(0, 136, 9)]
    assert p.ws_floats == 3 * 1 * 128 * 256


def test_table_holds_the_rows_and_pixels_the_issue_lists():
    split_q = {c.Q for c in MG.CASES if c.split}
    plain_q = {c.Q for c in MG.CASES if not c.split}
    assert split_q >= {1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, 136, 255, 256, 257}
    assert plain_q >= {255, 256, 257, 264, 272, 513}
    npix = {c.h * c.w for c in MG.CASES}
    assert npix >= {8, 16, 24, 32, 40, 56, 264, 1032, 1056, 1072}
    for hw in MG.CHUNKED_HW:
        assert {(c.Q, c.split) for c in MG.CASES if (c.h, c.w) == hw} >= {(33, True), (129, True)}
    for hw in MG.SMALL_HW:                                          # small pixel counts meet few rows and a second row group
        qs = {c.Q for c in MG.CASES if (c.h, c.w) == hw and c.split}
        assert min(qs) <= 31 and max(qs) > 128, hw
    # the batch stride: every Q above a group limit of either kernel runs with B = 3; elsewhere both B = 1 and B = 3 occur
    for c in MG.CASES:
        if c.Q > 128 and c.edge != 'tile wrap':
            assert c.B == 3, c
    assert {c.B for c in MG.CASES if c.Q <= 128 and c.edge != 'tile wrap'} == {1, 3}
    wraps = [c for c in MG.CASES if MG.case_plan(c).wraps]
    assert sorted(c.split for c in wraps) == [False, True] and all((c.B, c.Q, c.h, c.w) == MG.WRAP for c in wraps)
    one = [c for c in MG.CASES if not (c.need_embed and c.need_feat)]
    assert {(c.need_embed, c.need_feat, c.split) for c in one} == {(False, True, True), (False, True, False), (True, False, True),
                                                                  (True, False, False)}
    assert all(len(MG.case_plan(c).embed_groups) > 1 for c in one)
    # the large case is the wrap alone
    assert all(c.B * MG.C * c.h * c.w * 4 <= 4 << 20 for c in MG.CASES if c.edge != 'tile wrap')
    assert MG.WRAP[0] * MG.C * MG.WRAP[2] * MG.WRAP[3] * 4 < 140e6


@pytest.mark.parametrize('split', [True, False], ids=['split', 'plain'])
def test_table_crosses_what_it_claims(split):
    cases = [c for c in MG.CASES if c.split == split]
    plans = [MG.case_plan(c) for c in cases]
    embed_last = [p.embed_groups[-1] for c, p in zip(cases, plans) if c.need_embed]
    feat_last = [p.feat_groups[-1] for c, p in zip(cases, plans) if c.need_feat]
    assert {mt for _, _, mt in embed_last} == {1, 2, 3, 4}                              # every <SPLIT, MT> template as a LAST group
    assert {rows for _, rows, _ in embed_last} >= {1, 8} and {rows for _, rows, _ in feat_last} >= {1, 8}
    assert max(len(p.embed_groups) for p in plans) >= 3 and max(len(p.feat_groups) for p in plans) >= 3
    ks = {k for _, _, k in feat_last} | {k for p in plans for _, _, k in p.feat_groups}
    assert ks >= ({1, 2, 3, 4, 5, 6, 7, 8} if split else {1, 9, 16})
    # the upper half-wave without a row of its own in the last k-step (rows % 16 in 1..8), and with one (9..15 and 0)
    rem = {rows % 16 for _, rows, _ in feat_last}
    assert rem >= {1, 8, 0} and (rem & set(range(9, 16)))
    # exact group limits and one past them
    lim = 128 if split else 256
    qs = {c.Q for c in cases}
    assert {lim - 1, lim, lim + 1, lim + 8} <= qs
    # pixels
    assert any(p.half_step for p in plans) and any(not p.half_step for p in plans)
    assert any(p.ragged_tile for p in plans) and any(not p.ragged_tile for p in plans)
    assert any(p.T == 1 and c.h * c.w == 8 for c, p in zip(cases, plans))                # one half step: the clamp fix of this change
    assert any(p.T > 1 and not p.wraps for p in plans) and any(p.wraps for p in plans)
    tails = {(p.last_chunk, p.half_step) for c, p in zip(cases, plans) if p.nchunks > 1 and c.need_embed}
    assert tails == {(1, True), (2, False), (3, False)}                                 # both loop exits at a chunk's end; a half step alone
    assert {p.nsteps % 2 for p in plans if p.nchunks == 1} == {0, 1}                      # ... and at the end of a single chunk
    assert any(p.nsteps == 1 for p in plans) and any(p.nsteps == 2 for p in plans)


# ------------------------------------------------------------------------------------------------
# TEETH
# ------------------------------------------------------------------------------------------------
# cases that MUST have the edge a fault names (by the words of the table), besides whatever else `fault_outputs` finds
NAMED = {'leak_first_row_of_next_group': lambda c: c.need_feat and c.Q > (128 if c.split else 256),
         'drop_tail_half_step': lambda c: c.need_embed and (c.h * c.w) % 16 == 8,
         'skip_wrapped_tiles': lambda c: c.edge == 'tile wrap',
         'drop_last_chunk': lambda c: c.need_embed and c.edge.startswith('chunks')}


@pytest.mark.parametrize('kind', MG.FAULTS)
def test_every_fault_is_detected(kind):
    hits = 0
    for c in MG.CASES:
        outs = MG.fault_outputs(c, kind)
        if kind in NAMED:
            assert bool(outs) == bool(NAMED[kind](c)), (kind, c)
        else:
            touched = {'first_group_adds_to_old_contents': {'grad_feat'}, 'double_last_step': {'grad_embed'}}.get(kind, {'grad_embed', 'grad_feat'})
            asked = {n for n, need in (('grad_embed', c.need_embed), ('grad_feat', c.need_feat)) if need}
            assert set(outs) == touched & asked, (kind, c)                              # every case that asks for a touched output
        if not outs:
            continue
        ref = dict(zip(('grad_embed', 'grad_feat'), MG.reference(c)))
        bad = dict(zip(('grad_embed', 'grad_feat'), MG.faulty_reference(c, kind)))
        for name in ('grad_embed', 'grad_feat'):
            if name in outs:
                with pytest.raises(AssertionError, match='elements differ'):
                    MG.assert_equal(bad[name].float(), ref[name], f'{kind} {MG.case_id(c)} {name}')
                hits += 1
            else:
                assert bad[name] is ref[name]
    assert hits > 0, f'{kind} applies to no case'


def test_one_missing_term_flips_the_parity():
    """the structural guarantee: whatever the values, a dropped or doubled term cannot leave an element unchanged"""
    one = next(c for c in MG.CASES if c.Q == 7)                                           # one row group: one term dropped
    assert (MG.faulty_reference(one, 'drop_last_row_of_group')[1] != MG.reference(one)[1]).all()
    two = next(c for c in MG.CASES if c.Q == 129 and c.split and c.need_embed and c.need_feat)
    ge, gf = MG.reference(two)
    assert (MG.faulty_reference(two, 'leak_first_row_of_next_group')[1] != gf).all()       # one term counted twice
    assert (MG.faulty_reference(two, 'drop_last_pixel')[0] != ge).all()


def test_assert_equal_reports_count_and_first_index():
    want = torch.arange(12.0, dtype=torch.float64).view(3, 4)
    got = want.float()
    MG.assert_equal(got, want, 'same')
    got[1, 2] = 7.0
    got[2, 3] = float('nan')
    with pytest.raises(AssertionError, match=r'2 of 12 elements differ, first at \(1, 2\): 7\.0 != 6\.0'):
        MG.assert_equal(got, want, 'two')
    with pytest.raises(AssertionError, match='not an f32'):
        MG.assert_equal(want.float(), want + 2.0 ** -40, 'no f32')


# ------------------------------------------------------------------------------------------------
# HOST: LazyMasks
# ------------------------------------------------------------------------------------------------
def test_lazy_scenarios_have_the_shapes_they_claim():
    sums = {n: MG.lazy_scenario(n).sum_pm for n in MG.LAZY_SPECS}
    assert sums['below_8'] < 8 and sums['crosses_128'] > 128 and 8 <= sums['mid'] <= 128
    for name in MG.LAZY_SPECS:
        s = MG.lazy_scenario(name)
        assert 3 <= len(s.counts) <= 10 and (s.h * s.w) % 8 == 0
        assert any(not any(row) for row in s.counts), f'{name}: no layer with pm == 0'
        assert any(any(row) and not all(row) for row in s.counts), f'{name}: no image without positives in a live layer'
        pos = [MG.positions(wm) for wm in s.weights]
        assert [p['pm'] for p in pos] == [max(row) for row in s.counts]
        # positives of one image sit in different slots across layers: the last query, in slot counts - 1
        slots = {}
        for p in pos:
            for b, q, r in zip(p['b'].tolist(), p['q'].tolist(), p['r'].tolist()):
                slots.setdefault((b, q), set()).add(r)
        assert any(len(v) > 1 for v in slots.values()), name
        for wm in s.weights:
            assert (wm < 0).any() and (wm == 0).any()                                     # `> 0` is the rule, not `!= 0`
        outs, ges, gf = MG.lazy_dense(name)
        for t in outs + ges + [gf]:
            assert torch.equal(t.float().double(), t) and not (t.abs() >= 2 ** 24).any()


@pytest.mark.parametrize('how', MG.LAZY_HOW)
@pytest.mark.parametrize('name', list(MG.LAZY_SPECS))
def test_lazy_masks_equal_the_dense_formulation(name, how):
    got = MG.run_lazy(LazyMasks, name, how)
    MG.assert_lazy_equal(got, name, f'{name} {how}')


def test_lazy_masks_without_positives():
    s = MG.lazy_scenario('below_8')
    e, f = s.embeds[0].clone().requires_grad_(True), s.feat.clone().requires_grad_(True)
    out = LazyMasks(e, f).select_by_weights(torch.zeros(s.B, s.Q))
    assert tuple(out.shape) == (0, s.h, s.w)
    ge, gf = torch.autograd.grad(out.sum(), (e, f))
    assert not ge.any() and not gf.any()
    lazies = [LazyMasks(e, f), LazyMasks(e, f)]
    pos = [MG.positions(torch.zeros(s.B, s.Q)) for _ in lazies]
    LazyMasks.preselect(lazies, pos)                                                     # nothing to contract: no `_pre`, `select` still answers
    assert all(getattr(lz, '_pre', None) is None for lz in lazies)
    assert tuple(lazies[1].select(pos[1]).shape) == (0, s.h, s.w)
