"""Exact operands for the mask-logit backward, cgg_mask_logits_backward (csrc/mask_logits_bwd.hip), and for `LazyMasks`, the host logic
in front of it (mask2former_head.py). Host only: builders, float64 references, seeded faults, the kernel's plan restated. No kernel.

    grad_feat [b][c][p] = sum_q embed[b][q][c] grad_out[b][q][p]      cgg_mask_logits_grad_feat_kernel<SPLIT>
    grad_embed[b][q][c] = sum_p grad_out[b][q][p] feat[b][c][p]       cgg_mask_logits_grad_embed_kernel<SPLIT, MT> + _reduce

tests/test_mask_grad_cases.py proves on the CPU what is derived here; tests/test_mask_grad_edges_gpu.py then asserts every bit.

OPERANDS. embed, feat and grad_out hold ODD integers drawn from {-3, -1, 1, 3}. Each is an exact bf16 value, so the (hi, lo) pair of
split mode has a zero low piece and the plain mode's single bf16 piece is the value itself: both modes multiply the same numbers.

SUMS. Every product is an odd integer of magnitude <= 9, every partial sum an integer: |grad_feat| <= 9 Q <= 9 x 513 and
|grad_embed| <= 9 npix <= 9 x 1072 for the table below, far below 2^24, where every integer is an f32. So in both modes and under any
summation order -- MFMA blocks, row groups added into the first group's store, pixel chunks summed by the second kernel -- both
gradients ARE the float64 einsum. Every comparison is `torch.equal`; no tolerance appears anywhere, plain bf16 mode included. (The
randn claim of test_kernels_gpu.py::test_mask_logits_backward_vs_float64 -- 2e-5 split, 1e-2 plain -- is what integers cannot hold.)

PARITY. A sum of n odd integers has the parity of n. An element that misses one term, or counts one twice, has the wrong parity,
whatever the seed: such a fault cannot hide behind a zero operand. Faults that move an even number of terms (a whole 16-pixel step,
a whole chunk) or misplace terms are caught by the random values, and the CPU test asserts that each one is, case by case.

PLAN (restated from csrc/mask_logits_bwd.hip in `plan`). grad_feat: row groups of 128 (split) or 256 (plain), KS = ceil(rows / 16)
k-steps each; a group after the first ADDS into the first group's store. T = ceil(npix / 32) pixel tiles, 8 per workgroup,
min(ceil(T / 8), cap) workgroups per image with cap = ceil(512 / B): T > 8 cap makes a wave wrap to a second tile. grad_embed: row
groups of 128 in both modes, MT = ceil(rows / 32) row tiles; nsteps = ceil(npix / 16) steps of 16 pixels (npix % 16 == 8: the last
one is a half step), split into chunks of steps_per_chunk (64 at these sizes), each chunk one workgroup whose two-deep load
pipeline leaves its loop at one of two places according to the parity of the chunk's length.

LEFT OUT ON PURPOSE. steps_per_chunk > 64 needs ceil(nsteps / cap) > 64, i.e. B npix > 2^19 x 2: a `feat` of 0.5 GB and more. The
wrap is the one large case (B npix must exceed 512 x 256 whatever B is: about 140 MB for `feat` and for `grad_feat`)."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import torch

C = 256
SENTINEL = -12345.5             # no integer: an output element that still holds it, or had it added, equals no reference value
VALUES = (-3, -1, 1, 3)

Case = namedtuple('Case', 'B Q h w split need_embed need_feat edge')


def case_id(c):
    tail = '' if c.need_embed and c.need_feat else ('_feat_only' if c.need_feat else '_embed_only')
    return f'b{c.B}_q{c.Q}_{c.h}x{c.w}_{"split" if c.split else "plain"}{tail}'


# ------------------------------------------------------------------------------------------------
# the plan of csrc/mask_logits_bwd.hip
# ------------------------------------------------------------------------------------------------
def plan(B, Q, npix, split):
    lim = 128 if split else 256
    feat_groups = [(q0, min(lim, Q - q0), (min(lim, Q - q0) + 15) // 16) for q0 in range(0, Q, lim)]            # (q0, rows, KS)
    embed_groups = [(q0, min(128, Q - q0), (min(128, Q - q0) + 31) // 32) for q0 in range(0, Q, 128)]           # (q0, rows, MT)
    T = (npix + 31) // 32
    cap = (512 + B - 1) // B
    gx = min((T + 7) // 8, cap)
    nsteps = (npix + 15) // 16
    spc = (nsteps + cap - 1) // cap                       # mlb_plan: want = cap
    if spc < 64:
        spc = min(nsteps, 64)
    nchunks = (nsteps + spc - 1) // spc
    return SimpleNamespace(feat_groups=feat_groups, embed_groups=embed_groups, T=T, cap=cap, gx=gx, wraps=T > 8 * gx,
                           ragged_tile=npix % 32 != 0, nsteps=nsteps, steps_per_chunk=spc, nchunks=nchunks,
                           last_chunk=nsteps - (nchunks - 1) * spc, half_step=npix % 16 == 8,
                           ws_floats=B * nchunks * min(Q, 128) * C)


def case_plan(c):
    return plan(c.B, c.Q, c.h * c.w, c.split)


# ------------------------------------------------------------------------------------------------
# the table: one entry per edge, not a product
# ------------------------------------------------------------------------------------------------
ROWS_SPLIT = (1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, 136, 255, 256, 257)
# plain adds 136 (KS = 9: the second half of the k-steps begins, with 8 rows) and 200 (a last grad_embed group of 3 row tiles)
ROWS_PLAIN = (136, 200, 255, 256, 257, 264, 272, 513)
ROW_HW = ((4, 8), (5, 8), (3, 88), (7, 8))                # 32, 40, 264, 56 pixels: a full tile, ragged tiles, a half step
SMALL_HW = ((1, 8), (2, 8), (3, 8), (4, 8), (5, 8), (7, 8), (3, 88))          # 8 (one half step, upper half-wave idle) .. 264
CHUNKED_HW = ((24, 43), (24, 44), (8, 134))              # 1032, 1056, 1072 pixels: chunks of 64 + 1 (a half step), 64 + 2, 64 + 3 steps
SMALL_Q = (1, 7, 9, 17, 8, 31, 2)
WRAP = (512, 2, 8, 33)                                   # cap = 1: one workgroup owns T = 9 tiles, wave 0 wraps into the ragged tile


def _table():
    t = []
    add = lambda B, Q, hw, split, edge, ne=True, nf=True: t.append(Case(B, Q, hw[0], hw[1], split, ne, nf, edge))      # noqa: E731
    for i, Q in enumerate(ROWS_SPLIT):                    # B = 3 above a group limit (the batch stride is Qtot), else 1, 3, 1, ...
        add(3 if Q > 128 else (1, 3)[i % 2], Q, ROW_HW[i % 4], True, f'rows, split: Q = {Q}')
    for i, Q in enumerate(ROWS_PLAIN):                    # every one is above grad_embed's limit of 128
        add(3, Q, ROW_HW[(i + 1) % 4], False, f'rows, plain: Q = {Q}')
    for i, hw in enumerate(SMALL_HW):
        add((3, 1)[i % 2], SMALL_Q[i], hw, True, f'pixels: {hw[0] * hw[1]}, few rows')
        add(3, (129, 130, 136)[i % 3], hw, True, f'pixels: {hw[0] * hw[1]}, second row group (split)')
        if hw in ((1, 8), (3, 8), (3, 88)):
            add(3, 257, hw, False, f'pixels: {hw[0] * hw[1]}, second row group (plain)')
            add(1, SMALL_Q[i] + 1, hw, False, f'pixels: {hw[0] * hw[1]}, few rows (plain)')
    for hw in CHUNKED_HW:
        add(1, 33, hw, True, f'chunks: {hw[0] * hw[1]} pixels, Q = 33')
        add(3, 129, hw, True, f'chunks: {hw[0] * hw[1]} pixels, Q = 129')
        add(1, 33, hw, False, f'chunks: {hw[0] * hw[1]} pixels, Q = 33 (plain)')
    for split in (False, True):
        add(WRAP[0], WRAP[1], WRAP[2:], split, 'tile wrap')
    add(3, 129, (5, 8), True, 'grad_feat only', ne=False)
    add(3, 257, (7, 8), False, 'grad_feat only (plain)', ne=False)
    add(3, 129, (7, 8), True, 'grad_embed only', nf=False)
    add(3, 257, (5, 8), False, 'grad_embed only (plain)', nf=False)
    assert len({case_id(c) for c in t}) == len(t)
    return tuple(t)


CASES = _table()
CASE_IDS = tuple(case_id(c) for c in CASES)


# ------------------------------------------------------------------------------------------------
# operands and references
# ------------------------------------------------------------------------------------------------
def odd_ints(shape, gen):
    return (2 * torch.randint(0, 4, shape, generator=gen) - 3).float()


@functools.lru_cache(maxsize=None)
def operands(B, Q, h, w):
    """embed (B, Q, 256), feat (B, 256, h, w), grad_out (B, Q, h, w): odd integers of {-3, -1, 1, 3}, one seed per shape"""
    gen = torch.Generator().manual_seed(((B * 1009 + Q) * 1013 + h) * 1019 + w)
    return SimpleNamespace(embed=odd_ints((B, Q, C), gen), feat=odd_ints((B, C, h, w), gen), grad_out=odd_ints((B, Q, h, w), gen))


def _embed_terms(o, p0, p1):
    """the terms of grad_embed that pixels [p0, p1) contribute (float64)"""
    return torch.einsum('bqp,bcp->bqc', o.grad_out.flatten(2)[..., p0:p1].double(), o.feat.flatten(2)[..., p0:p1].double())


def _feat_term(o, r):
    """the term of grad_feat that query row r contributes (float64, (B, 256, npix))"""
    return torch.einsum('bc,bp->bcp', o.embed[:, r].double(), o.grad_out.flatten(2)[:, r].double())


@functools.lru_cache(maxsize=None)
def _reference(B, Q, h, w):
    o = operands(B, Q, h, w)
    ge = _embed_terms(o, 0, h * w)
    gf = torch.einsum('bqc,bqp->bcp', o.embed.double(), o.grad_out.flatten(2).double()).view(B, C, h, w)
    return ge, gf


def reference(c):
    """float64 (grad_embed (B, Q, 256), grad_feat (B, 256, h, w)); shared between the tests, never written to"""
    return _reference(c.B, c.Q, c.h, c.w)


def forward_reference(B, Q, h, w):
    o = operands(B, Q, h, w)
    return torch.einsum('bqc,bchw->bqhw', o.embed.double(), o.feat.double())


def assert_equal(got, want64, what):
    want = want64.float()
    assert torch.equal(want.double(), want64), f'{what}: the reference is not an f32'
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == want.shape, f'{what}: {got.dtype} {tuple(got.shape)} for {tuple(want.shape)}'
    if not torch.equal(got, want):
        bad = (got != want) | (got != got)
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {i}: {got[i].item()!r} != {want[i].item()!r}')


# ------------------------------------------------------------------------------------------------
# seeded faults: what a wrong clamp, select, loop bound or accumulate flag would compute
# ------------------------------------------------------------------------------------------------
FAULTS = ('drop_last_row_of_group', 'leak_first_row_of_next_group', 'drop_last_pixel', 'drop_tail_half_step',
          'first_group_adds_to_old_contents', 'skip_wrapped_tiles', 'drop_last_chunk', 'double_last_step')


def fault_outputs(c, kind):
    """the outputs ('grad_embed', 'grad_feat') of case c that the fault changes: empty where the case does not have the edge"""
    p = case_plan(c)
    both = ('grad_embed', 'grad_feat')
    hit = {'drop_last_row_of_group': both,
           'leak_first_row_of_next_group': ('grad_feat',) if len(p.feat_groups) > 1 else (),
           'drop_last_pixel': both,
           'drop_tail_half_step': ('grad_embed',) if p.half_step else (),
           'first_group_adds_to_old_contents': ('grad_feat',),
           'skip_wrapped_tiles': ('grad_feat',) if p.wraps else (),
           'drop_last_chunk': ('grad_embed',) if p.nchunks > 1 else (),
           'double_last_step': ('grad_embed',)}[kind]
    return tuple(n for n in hit if (c.need_embed if n == 'grad_embed' else c.need_feat))


def faulty_reference(c, kind):
    """(grad_embed, grad_feat) in float64 with one fault; an output the fault does not touch is the reference itself
      drop_last_row_of_group             the last row of every row group counts for nothing (grad_feat: its term is missing; grad_embed:
                                         its row is zero)
      leak_first_row_of_next_group       a grad_feat group also counts the row behind its last one (live data: the next group's first)
      drop_last_pixel                    pixel npix - 1 is taken for out of range: no grad_feat column, no term in grad_embed
      drop_tail_half_step                the 8 pixels of a last half step are missing from grad_embed
      first_group_adds_to_old_contents   the first grad_feat group adds into what the buffer held (the sentinel), as later groups do
      skip_wrapped_tiles                 the pixel-tile loop runs once: tiles from 8 gridDim.x on keep what the buffer held
      drop_last_chunk                    the last pixel chunk is missing from the sum over chunks
      double_last_step                   the pipeline runs the last step of every chunk twice"""
    assert kind in FAULTS
    o, p, npix = operands(c.B, c.Q, c.h, c.w), case_plan(c), c.h * c.w
    ge, gf = reference(c)
    hit = fault_outputs(c, kind)
    ge = ge.clone() if 'grad_embed' in hit else ge
    gf = gf.clone().flatten(2) if 'grad_feat' in hit else gf
    if kind == 'drop_last_row_of_group':
        if 'grad_feat' in hit:
            for q0, rows, _ in p.feat_groups:
                gf -= _feat_term(o, q0 + rows - 1)
        if 'grad_embed' in hit:
            for q0, rows, _ in p.embed_groups:
                ge[:, q0 + rows - 1] = 0
    elif kind == 'leak_first_row_of_next_group' and hit:
        for q0, rows, _ in p.feat_groups[:-1]:
            gf += _feat_term(o, q0 + rows)
    elif kind == 'drop_last_pixel':
        if 'grad_feat' in hit:
            gf[..., npix - 1] = 0
        if 'grad_embed' in hit:
            ge -= _embed_terms(o, npix - 1, npix)
    elif kind == 'drop_tail_half_step' and hit:
        ge -= _embed_terms(o, npix - 8, npix)
    elif kind == 'first_group_adds_to_old_contents' and hit:
        gf += SENTINEL
    elif kind == 'skip_wrapped_tiles' and hit:
        gf[..., 32 * 8 * p.gx:] = SENTINEL
    elif kind == 'drop_last_chunk' and hit:
        ge -= _embed_terms(o, 16 * p.steps_per_chunk * (p.nchunks - 1), npix)
    elif kind == 'double_last_step' and hit:
        for k in range(p.nchunks):
            s = min(p.nsteps, (k + 1) * p.steps_per_chunk) - 1
            ge += _embed_terms(o, 16 * s, min(16 * s + 16, npix))
    return ge, (gf.view(c.B, C, c.h, c.w) if 'grad_feat' in hit else gf)


# ------------------------------------------------------------------------------------------------
# LazyMasks scenarios
# ------------------------------------------------------------------------------------------------
# counts[l][b] = positives of image b in decoder layer l; pm_l = max_b counts[l][b] slots per image, sum_l pm_l rows in the one
# contraction of `preselect`. Every scenario has a layer without any positive and an image without positives in a live layer.
LAZY_SPECS = {
    'below_8': dict(B=2, Q=20, h=3, w=8, counts=((2, 0), (0, 0), (3, 1))),                                        # sum pm = 5
    'mid': dict(B=3, Q=50, h=5, w=8, counts=((5, 0, 2), (0, 0, 0), (1, 7, 3), (4, 4, 0))),                         # sum pm = 16
    'crosses_128': dict(B=2, Q=100, h=7, w=8, counts=((14, 9), (13, 0), (0, 0), (15, 15), (12, 14), (0, 16), (14, 13), (13, 13),
                                                      (15, 2), (14, 15))),                                       # sum pm = 129
}


def positions(weights):
    """the index set `Mask2FormerHeadOpen` hands to `LazyMasks.select` for a (B, Q) weight map: image b, query q, slot r = rank of
    the query among its image's positives, pm = most positives of one image"""
    sel = weights > 0
    b, q = torch.nonzero(sel, as_tuple=True)
    r = (torch.cumsum(sel.long(), 1) - 1)[b, q]
    return dict(b=b, q=q, r=r, pm=int(sel.sum(1).max()))


@functools.lru_cache(maxsize=None)
def lazy_scenario(name):
    """embeds: one (B, Q, 256) per layer; feat (B, 256, h, w); weights: one (B, Q) map per layer, positive at the positives (the
    last query is one wherever an image has any, so it sits in slot counts - 1, which differs between layers), zero or negative
    elsewhere; G: the integer upstream gradient of each layer's selection, (n_pos, h, w)"""
    s = LAZY_SPECS[name]
    B, Q, h, w = s['B'], s['Q'], s['h'], s['w']
    gen = torch.Generator().manual_seed(4000 + Q)
    embeds, weights, G = [], [], []
    for row in s['counts']:
        embeds.append(odd_ints((B, Q, C), gen))
        wm = -(torch.arange(B * Q).view(B, Q) % 2).float()                     # non-positives: 0 and -1
        for b, n in enumerate(row):
            if n:
                wm[b, torch.randperm(Q - 1, generator=gen)[:n - 1]] = 0.5
                wm[b, Q - 1] = 2.0
        assert tuple(int(v) for v in (wm > 0).sum(1)) == tuple(row)
        weights.append(wm)
        G.append(odd_ints((sum(row), h, w), gen))
    return SimpleNamespace(name=name, B=B, Q=Q, h=h, w=w, counts=s['counts'], embeds=embeds, feat=odd_ints((B, C, h, w), gen),
                           weights=weights, G=G, sum_pm=sum(max(row) for row in s['counts']))


@functools.lru_cache(maxsize=None)
def lazy_dense(name):
    """the dense formulation in float64: outs[l] = einsum('bqc,bchw->bqhw', E_l, F)[weights_l > 0], loss = sum_l (outs[l] G_l).sum(),
    and autograd's gradients of it -> (outs, grad_embeds, grad_feat)"""
    s = lazy_scenario(name)
    embeds = [e.double().requires_grad_(True) for e in s.embeds]
    feat = s.feat.double().requires_grad_(True)
    outs = [torch.einsum('bqc,bchw->bqhw', e, feat)[wm > 0] for e, wm in zip(embeds, s.weights)]
    loss = sum((o * g.double()).sum() for o, g in zip(outs, s.G))
    grads = torch.autograd.grad(loss, embeds + [feat])
    return [o.detach() for o in outs], list(grads[:-1]), grads[-1]


LAZY_HOW = ('select', 'preselect', 'select_by_weights')


def run_lazy(LazyMasks, name, how, device='cpu', pack=None):
    """the scenario through `LazyMasks` (the class is handed in: this file imports no product code) -> (outs, grad_embeds, grad_feat)
    how: 'select' per layer | 'preselect' of all layers, then 'select' | 'select_by_weights' per layer. pack: feat -> PackedFeature"""
    s = lazy_scenario(name)
    embeds = [e.clone().to(device).requires_grad_(True) for e in s.embeds]
    feat = s.feat.clone().to(device).requires_grad_(True)
    packed = pack(feat.detach()) if pack is not None else None
    lazies = [LazyMasks(e, feat, packed) for e in embeds]
    if how == 'select_by_weights':
        outs = [lz.select_by_weights(wm.to(device)) for lz, wm in zip(lazies, s.weights)]
    else:
        pos = [positions(wm.to(device)) for wm in s.weights]
        if how == 'preselect':
            LazyMasks.preselect(lazies, pos)
            assert [getattr(lz, '_pre', None) is not None for lz in lazies] == [max(row) > 0 for row in s.counts]
        outs = [lz.select(p) for lz, p in zip(lazies, pos)]
    loss = sum((o * g.to(device)).sum() for o, g in zip(outs, s.G))
    grads = torch.autograd.grad(loss, embeds + [feat])
    return outs, list(grads[:-1]), grads[-1]


def assert_lazy_equal(got, name, what):
    outs, ges, gf = got
    want_outs, want_ges, want_gf = lazy_dense(name)
    s = lazy_scenario(name)
    for l, (o, wo, g, wg, row) in enumerate(zip(outs, want_outs, ges, want_ges, s.counts)):
        assert tuple(o.shape) == (sum(row), s.h, s.w), f'{what} layer {l}: shape {tuple(o.shape)}'
        assert_equal(o, wo, f'{what} layer {l}: selected logits')
        assert_equal(g, wg, f'{what} layer {l}: grad mask_embed')
        if not any(row):
            assert not g.any(), f'{what} layer {l}: no positive, but a gradient'
    assert_equal(gf, want_gf, f'{what}: grad mask_feature')
