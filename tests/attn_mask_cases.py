"""The attention-mask chain on exact operands: cases, float64 references, expected words and visible sets. Plain torch on the CPU;
tests/test_attn_mask_cases.py proves the cases (exactness, seeded faults), tests/test_attn_mask_edges_gpu.py runs the kernels on them.

The interface between the mask producers (cgg_pack_mask_feature*, cgg_mask_logits*, cgg_attn_mask_from_logits,
cgg_attn_mask_fix_full_rows) and the consumers (cgg_masked_xattn_*) is one bit per (query, key): "this key is blocked for this
query", bit p % 32 of word p / 32, set where the (resized) logit is < 0 (open_set/models/mask2former_head.py:749-759, :825-826).
Nothing here has a tolerance on that bit.

A. Producers. `embed` holds integers in [-4, 4] (channels >= 16 kept with probability 0.1), `feat` integers in [-8, 8]; the 2 x 2 mean
of a pooled level is a multiple of 1/4 with |value| <= 8. Every operand is exact in bf16 and in the f16 (hi, lo) pair, every product
and every partial sum is a multiple of 1/4 far below 2^24: the f32, f16 x 3 and bf16 contractions all reproduce the float64 einsum
BIT FOR BIT, exact zeros included (0.2 - 0.8 % of the logits of a pooled level), so `<` and `<=` differ on the operands and the words
are compared raw, tail bits and all. Planted in every case (as far as Q has room, see `lattice`): an all-zero query, a query and its
negation, a pixel at which every ordinary query has logit 0, a query with a positive and one with a negative logit at every pixel.
Channel 0 is the handle of the last two: the feature holds 8 there, ordinary queries hold 0, the two planted rows hold +-4 and
nothing else -- so the "zero pixel" is zero in the 255 channels that ordinary queries read.

B. Consumers. q = 0: every score is 0 in every operand format, every probability exp(0) = 1, chunk sums are integers and the combine
rescales by exactly 1. v is one-hot, v[s, e] = [e == column(s)], so out[q, e] n_q = the number of visible keys of row q in column e:
the visible set is read off the output. What is left is one division (and one log for the lse), hence
    |out - want| <= FACTOR U_F32 want          |lse - log n| <= FACTOR U_F32 max(1, log n)
with softmax_cases' constants. The backward's probabilities are exp(0 - lse): they inherit the lse's allowance and add the
exponential's own (an argument of size log n), so grad_v is held to 2 FACTOR u max(1, log n) / n with u of the operand format
(U_X3 for the f16 x 3 form, whose operands carry 22 bits), blocked pairs to exactly 0, grad_k to exactly 0 (q = 0), grad_q to
the bound of test_kernels_gpu.check_masked_xattn_backward against float64."""
import functools
import math

import torch
import torch.nn.functional as F

import softmax_cases as SC
from oracle import ops as ref

C = 256
E, HEADS, D = 256, 8, 32
FACTOR, U_F32, U_X3 = SC.FACTOR, SC.U_F32, SC.U_X3
_SHIFT = torch.arange(32, dtype=torch.int64)


# ------------------------------------------------------------------------------------------------
# words
# ------------------------------------------------------------------------------------------------
def pack_words(mask, tail=False):
    """bool (..., n) -> int32 (..., ceil(n / 32)), bit p % 32 of word p / 32; the unused bits of the last word are `tail`"""
    n = mask.shape[-1]
    W = (n + 31) // 32
    fill = torch.full((*mask.shape[:-1], W * 32 - n), bool(tail))
    w = (torch.cat([mask, fill], -1).reshape(*mask.shape[:-1], W, 32).to(torch.int64) << _SHIFT).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_words(words, n=None):
    """int32 (..., W) -> bool (..., 32 W), or its first n"""
    b = ((words.cpu().to(torch.int64).unsqueeze(-1) >> _SHIFT) & 1).bool().flatten(-2)
    return b if n is None else b[..., :n]


def assert_words(got, want, what):
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == torch.int32, (what, got.shape, want.shape, got.dtype)
    bad = (got != want).nonzero()
    assert len(bad) == 0, (f'{what}: {len(bad)} of {want.numel()} words differ, first at {bad[0].tolist()}: got '
                           f'{got[tuple(bad[0])].item() & 0xFFFFFFFF:#010x} want {want[tuple(bad[0])].item() & 0xFFFFFFFF:#010x}')


# ------------------------------------------------------------------------------------------------
# A. producers
# ------------------------------------------------------------------------------------------------
PLANTED = ('neg_all', 'zero', 'a', 'minus_a', 'pos_all')


def lattice(B, Q, H, W, pools, seed):
    """(embed (B, Q, C), feat (B, C, H, W), planted {kind: [(b, q)]}, zero_pixel). Q >= 5: rows 0, 1, Q - 3, Q - 2, Q - 1 of every
    image are zero, a, pos_all, minus_a, neg_all -- the last rows sit in the ragged query tile / the last row group. Q < 5: image b
    plants kinds b, b + 1, ... as far as rows go (`minus_a` is then the negation of a vector that is no row). zero_pixel: the last
    pixel of every level of `pools` is zero in channels 1 .. 255 (not where a level is that one pixel)."""
    g = torch.Generator().manual_seed(seed)
    embed = torch.randint(-4, 5, (B, Q, C), generator=g).float()
    keep = torch.rand(B, Q, C, generator=g) < 0.1
    keep[..., :16] = True
    embed = embed * keep
    embed[..., 0] = 0.0
    feat = torch.randint(-8, 9, (B, C, H, W), generator=g).float()
    feat[:, 0] = 8.0
    P = max(pools)
    zero_pixel = (H // P) * (W // P) > 1
    if zero_pixel:
        feat[:, 1:, H - P:, W - P:] = 0.0
    a = torch.randint(-4, 5, (B, C), generator=g).float()
    a[:, 0] = 0.0
    planted = {k: [] for k in PLANTED}
    for b in range(B):
        if Q >= 5:
            rows = dict(zero=0, a=1, pos_all=Q - 3, minus_a=Q - 2, neg_all=Q - 1)
        else:
            rows = {PLANTED[(b + i) % 5]: i for i in range(Q)}
        for kind, q in rows.items():
            embed[b, q] = 0.0
            if kind == 'a':
                embed[b, q] = a[b]
            elif kind == 'minus_a':
                embed[b, q] = -a[b]
            elif kind in ('pos_all', 'neg_all'):
                embed[b, q, 0] = 4.0 if kind == 'pos_all' else -4.0
            planted[kind].append((b, q))
    return embed, feat, planted, zero_pixel


def pooled(feat, pool):
    """the 2 x 2 mean that bilinear (align_corners=False) down-sampling by `pool` reads, in feat's dtype"""
    if pool == 1:
        return feat
    o = pool // 2 - 1
    return ((feat[..., o::pool, o::pool] + feat[..., o::pool, o + 1::pool])
            + (feat[..., o + 1::pool, o::pool] + feat[..., o + 1::pool, o + 1::pool])) * 0.25


class Level:
    """one pooled level of a ProducerCase: the float64 references and the expected words"""

    def __init__(self, case, pool):
        self.pool, self.h, self.w = pool, case.H // pool, case.W // pool
        self.npix = self.h * self.w
        self.nwords = (self.npix + 31) // 32
        self.feat64 = pooled(case.feat.double(), pool)                                   # (B, C, h, w)
        self.logits64 = ref.mask_logits(case.embed.double(), self.feat64)                # (B, Q, h, w)
        self.blocked = self.logits64.flatten(2) < 0                                      # (B, Q, npix)
        self.words = pack_words(self.blocked)                                            # tail bits 0


class ProducerCase:
    def __init__(self, name, B, Q, H, W, pools, seed):
        self.name, self.B, self.Q, self.H, self.W, self.pools = name, B, Q, H, W, tuple(pools)
        self.embed, self.feat, self.planted, self.zero_pixel = lattice(B, Q, H, W, pools, seed)
        self._levels = {}

    def level(self, pool):
        if pool not in self._levels:
            self._levels[pool] = Level(self, pool)
        return self._levels[pool]

    def nhwc(self):
        return self.feat.permute(0, 2, 3, 1).contiguous()


# Every Q meets every npix: Q in {1, 31, 32, 33, 128, 129, 256} (one row, ragged / full query tile, full row group, second group)
# and 257 (three row groups; split mode only, with a one-tile and a nine-tile level) x npix in {1, 31, 32, 33, 35 (5 x 7), 257, 288}
# (one pixel, ragged / full tile, 8 tiles + 1 pixel, 9 full tiles = one more than the 8 tiles of a workgroup slot). Of the pools and
# batch sizes, case (i, j) takes pool (1, 2, 4, 8)[(i + j) % 4] and B = 3 where (i + 2 j) % 3 == 0, else 1 -- so every Q and every
# npix meets every pool and both B, but not every (Q, npix) pair does: the pooling is the pack kernels' alone (they never see Q) and
# the image is a grid dimension of every kernel, so the pairs left out cross no edge that these do not.
QS = (1, 31, 32, 33, 128, 129, 256)
LEVEL_HW = {1: (1, 1), 31: (1, 31), 32: (4, 8), 33: (3, 11), 35: (5, 7), 257: (1, 257), 288: (12, 24)}
POOLS = (1, 2, 4, 8)
SPLIT_ONLY_Q = 257


def _specs():
    """{name: (B, Q, H, W of the full map, pools)}"""
    specs = {}
    for i, Q in enumerate(QS + (SPLIT_ONLY_Q,)):
        for j, (npix, (h, w)) in enumerate(LEVEL_HW.items()):
            if Q == SPLIT_ONLY_Q and npix not in (33, 288):
                continue
            pool, B = POOLS[(i + j) % 4], 3 if (i + 2 * j) % 3 == 0 else 1
            if Q == SPLIT_ONLY_Q:
                B = 3 if npix == 288 else 1
            specs[f'q{Q}_pix{npix}_pool{pool}_b{B}'] = (B, Q, h * pool, w * pool, (pool,))
    return specs


PRODUCER_SPECS = _specs()


def find_case(Q, npix, specs=None):
    """the name of the case with these Q and npix"""
    return next(n for n in (PRODUCER_SPECS if specs is None else specs) if n.startswith(f'q{Q}_pix{npix}_'))


# channel-last maps: all pools of a map from ONE launch (npix 384 / 96 / 24 / 6 and 2240 / 560 / 140 / 35)
NHWC_SPECS = {
    'nhwc_16x24_q33_b3': (3, 33, 16, 24, (1, 2, 4, 8)),
    'nhwc_40x56_q129': (1, 129, 40, 56, (1, 2, 4, 8)),
}
CHAIN_SPEC = ('chain_20x28_pool4_q33', 1, 33, 20, 28, (4,))


@functools.lru_cache(maxsize=None)
def producer_case(name):
    if name == CHAIN_SPEC[0]:
        return ProducerCase(*CHAIN_SPEC, seed=777)
    spec = PRODUCER_SPECS.get(name) or NHWC_SPECS[name]
    names = list(PRODUCER_SPECS) + list(NHWC_SPECS)
    return ProducerCase(name, *spec, seed=1000 + names.index(name))


def producer_levels(specs=None):
    """(case name, pool) of every level"""
    specs = PRODUCER_SPECS if specs is None else specs
    return [(name, pool) for name, spec in specs.items() for pool in spec[4]]


def check_logits(lv, logits, what):
    got = logits.cpu()
    assert got.shape == lv.logits64.shape and got.dtype == torch.float32, (what, got.shape, got.dtype)
    bad = (got.double() != lv.logits64).nonzero()
    assert len(bad) == 0, (f'{what}: {len(bad)} of {got.numel()} logits differ from float64, first at {bad[0].tolist()}: got '
                           f'{got[tuple(bad[0])].item()!r} want {lv.logits64[tuple(bad[0])].item()!r}')


def check_planted(case, lv, words, what):
    """what the planted rows and the zero pixel must show, read from the raw words"""
    bits = unpack_words(words)
    valid, tail = bits[..., :lv.npix], bits[..., lv.npix:]
    nz = lv.logits64.flatten(2) != 0
    at = {k: v for k, v in case.planted.items() if v}
    for b, q in at.get('zero', []):
        assert not bits[b, q].any(), f'{what}: all-zero query ({b}, {q}) has bits set'
    for b, q in at.get('pos_all', []):
        assert not bits[b, q].any(), f'{what}: positive query ({b}, {q}) has bits set'
    for b, q in at.get('neg_all', []):
        assert valid[b, q].all(), f'{what}: negative query ({b}, {q}) misses valid bits'
        assert not tail[b, q].any(), f'{what}: negative query ({b}, {q}) has tail bits set'
    if 'a' in at and 'minus_a' in at:
        for (b, qa), (b2, qm) in zip(at['a'], at['minus_a']):
            assert b == b2
            assert not (valid[b, qa] & valid[b, qm]).any(), f'{what}: a and -a share a bit in image {b}'
            assert torch.equal(valid[b, qa] | valid[b, qm], nz[b, qa]), f'{what}: a | -a is not (logit != 0) in image {b}'
    if case.zero_pixel:
        ordinary = torch.ones(case.B, case.Q, dtype=torch.bool)
        for k in ('pos_all', 'neg_all'):
            for b, q in at.get(k, []):
                ordinary[b, q] = False
        assert not valid[..., lv.npix - 1][ordinary].any(), f'{what}: the zero pixel is blocked'
    assert not tail.any(), f'{what}: tail bits set'


def check_words(case, lv, words, what):
    assert_words(words, lv.words, what)
    check_planted(case, lv, words, what)


# ---- cgg_attn_mask_from_logits ----
# (H, W, h, w, exact): exact = integer scale factors (every tap weight 1/4 or 1: no element left out)
RESIZE_SPECS = {
    '16x24_to_8x12': (16, 24, 8, 12, True),
    '16x24_to_4x6': (16, 24, 4, 6, True),
    '16x24_to_1x1': (16, 24, 1, 1, True),                    # npix 1
    '16x24_to_5x7': (16, 24, 5, 7, False),
    '20x28_to_25x42': (20, 28, 25, 42, False),               # 1050 pixels, 33 words
    '8x8_to_3x11': (8, 8, 3, 11, False),
    '8x8_to_15x17': (8, 8, 15, 17, False),                   # npix 255: the kernel writes 8 words per block
    '16x24_to_16x16': (16, 24, 16, 16, False),               # npix 256
    '8x8_to_1x257': (8, 8, 1, 257, False),                   # npix 257
}
RESIZE_CAP = 0.01          # largest share of a case that may be left out
TRUE_ZERO = 2.0 ** -20


class ResizeCase:
    """integer logits (2, 3, H, W) in [-8, 8] with a zero half plane and a zero plane. Reference: float64 F.interpolate, then < 0.
    `excluded`: the float64 value is a true zero (an f32 evaluation may land on either side) and its taps are not all zero;
    `taps_zero`: every tap with a non-zero weight is zero -- the bit must be 0."""

    def __init__(self, name, H, W, h, w, exact):
        self.name, self.H, self.W, self.h, self.w, self.exact = name, H, W, h, w, exact
        g = torch.Generator().manual_seed(2000 + list(RESIZE_SPECS).index(name))
        self.logits = torch.randint(-8, 9, (2, 3, H, W), generator=g).float()
        self.logits[0, 0, :H // 2] = 0.0
        self.logits[1, 2] = 0.0
        self.npix = h * w
        self.ref64 = F.interpolate(self.logits.double(), (h, w), mode='bilinear', align_corners=False).flatten(2)
        self.ref32 = F.interpolate(self.logits, (h, w), mode='bilinear', align_corners=False).flatten(2)
        self.want = self.ref64 < 0
        self.taps_zero = F.interpolate((self.logits != 0).double(), (h, w), mode='bilinear', align_corners=False).flatten(2) == 0
        self.excluded = (self.ref64.abs() < TRUE_ZERO) & ~self.taps_zero
        if exact:
            self.excluded = torch.zeros_like(self.excluded)


@functools.lru_cache(maxsize=None)
def resize_case(name):
    return ResizeCase(name, *RESIZE_SPECS[name])


def check_resize(case, words, what):
    bits = unpack_words(words)
    assert bits.shape[-1] == (case.npix + 31) // 32 * 32, (what, bits.shape)
    got, tail = bits[..., :case.npix], bits[..., case.npix:]
    keep = ~case.excluded
    bad = (got != case.want) & keep
    assert not bad.any(), f'{what}: {int(bad.sum())} bits differ from (float64 interpolate < 0), first at {bad.nonzero()[0].tolist()}'
    assert not got[case.taps_zero].any(), f'{what}: a bit is set where all four taps are zero'
    assert not tail.any(), f'{what}: tail bits set'


# ---- cgg_attn_mask_fix_full_rows ----
FIX_ROWS = (1, 5, 7)                                          # four rows per workgroup
FIX_NPIX = (1, 31, 32, 33, 2048, 2049, 2081)                  # 64 and 65 words (the lane stride); 1 or 33 % 32 valid bits in the last
FIX_KINDS = ('empty', 'full', 'full_but_bit0', 'full_but_last', 'full_but_far', 'full_valid_tail0', 'full_valid_tail1')


class FixCase:
    """rows x ceil(npix / 32) words; row r is kind (r + first) % 7 -- 7 rows hold every kind, 5 rows the last five, 1 row
    `full_valid_tail0` (the row a kernel that compares whole words would miss). `full_but_far` clears bit 0 of word 64 where
    there is one (else the middle bit). Rows that stay hold tail bits (all 1, all 0 or alternating) that must survive."""

    def __init__(self, rows, npix):
        self.rows, self.npix = rows, npix
        W = (npix + 31) // 32
        first = {7: 0, 5: 2, 1: 5}[rows]
        self.kinds = [FIX_KINDS[(r + first) % 7] for r in range(rows)]
        bits = torch.zeros(rows, W * 32, dtype=torch.bool)
        for r, kind in enumerate(self.kinds):
            if kind == 'empty':
                bits[r, npix:] = True
                continue
            bits[r] = True
            if kind == 'full_but_bit0':
                bits[r, 0] = False
            elif kind == 'full_but_last':
                bits[r, npix - 1:] = False
            elif kind == 'full_but_far':
                bits[r, 64 * 32 if npix > 64 * 32 else npix // 2] = False
                bits[r, npix + 1::2] = False
            elif kind == 'full_valid_tail0':
                bits[r, npix:] = False
        self.bits = bits
        self.words = pack_words(bits)
        valid = ref.fix_full_rows(bits[:, :npix].clone())
        cleared = bits[:, :npix].all(1)
        self.cleared = cleared
        want = torch.cat([valid, bits[:, npix:]], 1)
        want[cleared] = False                                  # a cleared row is zero words: producers leave the tail bits 0
        self.want_valid = valid
        self.want = pack_words(want)


@functools.lru_cache(maxsize=None)
def fix_case(rows, npix):
    return FixCase(rows, npix)


def check_fix(case, words, what):
    got = unpack_words(words)
    assert torch.equal(got[:, :case.npix], case.want_valid), f'{what}: valid bits differ from oracle.ops.fix_full_rows'
    keep = ~case.cleared
    assert torch.equal(got[keep][:, case.npix:], case.bits[keep][:, case.npix:]), f'{what}: tail bits of a kept row changed'
    assert_words(words, case.want, what)


# ------------------------------------------------------------------------------------------------
# B. consumers
# ------------------------------------------------------------------------------------------------
F32_S = (1, 33, 64, 65, 321)                                  # f32-row kernels
BF16_S = (8, 36, 64, 68, 324)                                 # cgg_masked_xattn_forward_bf16: S % 4 == 0, S >= 8
TILE = 64                                                     # XA_TK: keys per tile, and per chunk above 256 keys at B H = 8


def chunk_keys(S):
    """keys per workgroup chunk of csrc/xattn.hip's xattn_plan at B = 1, H = 8: one chunk up to 4 tiles, else one tile per chunk"""
    tiles = (S + TILE - 1) // TILE
    return tiles * TILE if tiles <= 4 else TILE


def mask_rows(S):
    """[(name, blocked bool (S,))]: the rows of one launch. Rows that would block every key by accident (S = 1) are dropped."""
    def row(fn):
        m = torch.zeros(S, dtype=torch.bool)
        fn(m)
        return m

    def only(m, lo, hi):
        m[:] = True
        m[lo:hi] = False
    T = (S + TILE - 1) // TILE
    rows = [('open', row(lambda m: None)),
            ('only_key0', row(lambda m: only(m, 0, 1))),
            ('only_last_key', row(lambda m: only(m, S - 1, S)))]
    if S > 32:
        rows.append(('word1_blocked', row(lambda m: m.__setitem__(slice(32, 64), True))))
        rows.append(('word0_blocked', row(lambda m: m.__setitem__(slice(0, 32), True))))
    if T >= 2:
        rows.append(('first_chunk_blocked', row(lambda m: m.__setitem__(slice(0, TILE), True))))
        rows.append(('last_chunk_blocked', row(lambda m: m.__setitem__(slice((T - 1) * TILE, S), True))))
        rows.append(('only_last_chunk', row(lambda m: only(m, (T - 1) * TILE, S))))
    if T >= 3:
        rows.append(('middle_chunk_blocked', row(lambda m: m.__setitem__(slice(T // 2 * TILE, T // 2 * TILE + TILE), True))))
        rows.append(('first_chunks_blocked', row(lambda m: m.__setitem__(slice(0, 2 * TILE), True))))
    rows.append(('even_blocked', row(lambda m: m.__setitem__(slice(0, S, 2), True))))
    rows.append(('odd_blocked', row(lambda m: m.__setitem__(slice(1, S, 2), True))))
    rows = [(n, m) for n, m in rows if not m.all()]
    rows.append(('full', torch.ones(S, dtype=torch.bool)))
    return rows


class ConsumerCase:
    """B = 1, q = 0 (1, Q, E), k random, v one-hot. Row i of the launch is pattern (i + first) % len(patterns) of `mask_rows(S)`
    (without 'full' unless `full`). launch 0: column(s) = s % 256; launch 1 (S > 256): column(s) = (s + s // 256) % 256 -- two keys
    that share a column in one launch do not in the other. grad_out[q, e] = [e == q] for the backward."""

    def __init__(self, Q, S, launch=0, full=False, first=0, bf16=False, blocked=None):
        self.Q, self.S, self.launch, self.full = Q, S, launch, full
        pats = [(n, m) for n, m in mask_rows(S) if full or n != 'full']
        self.names = [pats[(i + first) % len(pats)][0] for i in range(Q)]
        self.blocked = torch.stack([pats[(i + first) % len(pats)][1] for i in range(Q)])[None]            # (1, Q, S)
        if blocked is not None:                                # the chained case: the mask is the producers'
            self.names = [f'row{i}' for i in range(Q)]
            self.blocked = blocked
        g = torch.Generator().manual_seed(3000 + S)
        self.k = torch.randn(1, S, E, generator=g)
        if bf16:
            self.k = self.k.bfloat16().float()
        s = torch.arange(S)
        self.col = (s + (s // 256 if launch else 0)) % 256
        self.v = F.one_hot(self.col, E).float()[None]
        self.q = torch.zeros(1, Q, E)
        self.kv = torch.cat([self.k, self.v], -1).contiguous()
        self.go = torch.eye(E)[:Q][None].contiguous()
        assert Q <= E

    def words(self, tail):
        return pack_words(self.blocked, tail)

    def visible(self, full):
        """(visible bool (Q, S), n (Q,)): full = 'mean' -> an all-blocked row sees every key (mask2former_head.py:825-826)"""
        vis = ~self.blocked[0]
        if full == 'mean':
            vis = vis.clone()
            vis[vis.sum(1) == 0] = True
        return vis, vis.sum(1)

    def rows(self, name):
        return [i for i, n in enumerate(self.names) if n == name]


@functools.lru_cache(maxsize=None)
def consumer_case(Q, S, launch=0, full=False, first=0, bf16=False):
    return ConsumerCase(Q, S, launch, full, first, bf16)


def same_or_both_nan(a, b):
    a, b = a.cpu(), b.cpu()
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def check_forward(case, out, lse=None, full=None, what=''):
    """full: None = the case has no all-blocked row; 'nan' = such rows are NaN (include/cgg_hip.h); 'mean' = they see every key"""
    out = out.cpu()
    assert out.shape == (1, case.Q, E), (what, out.shape)
    vis, n = case.visible(full)
    live = n > 0
    if full == 'nan':
        assert not live.all(), f'{what}: the case has no all-blocked row'
        assert torch.isnan(out[0, ~live]).all(), f'{what}: an all-blocked row is not NaN'
    else:
        assert live.all(), f'{what}: an all-blocked row without a contract'
    nl = n[live].double()[:, None]
    count = vis[live].double() @ case.v[0].double()                                  # visible keys of the row per column
    want = count / nl
    got = out[0, live].double()
    bad = (got > 0.5 / nl) != (count > 0)
    assert not bad.any(), (f'{what}: rows {sorted({case.names[i] for i in live.nonzero()[bad.any(1)].flatten().tolist()})} '
                           f'attend to the wrong keys ({int(bad.sum())} columns)')
    err = (got - want).abs()
    assert bool((err <= FACTOR * U_F32 * want).all()), f'{what}: out off by {(err / want.clamp_min(1e-30)).max().item():.3g} relative'
    if lse is not None:
        lse = lse.cpu()
        assert lse.shape == (1, HEADS, case.Q), (what, lse.shape)
        wl = torch.log(n[live].double())
        el = (lse[0][:, live].double() - wl).abs()
        assert bool((el <= FACTOR * U_F32 * wl.clamp_min(1.0)).all()), f'{what}: lse off by {el.max().item():.3g}'


def backward_ref(case, vis, dtype=torch.float64):
    """(grad_q (Q, E), grad_k (S, E), grad_v (S, E)) of the attention over `vis` with q = 0: P = vis / n for every head"""
    Q, S = vis.shape
    P = vis.to(dtype) / vis.sum(1).to(dtype)[:, None]
    heads = lambda t, n: t[0].to(dtype).view(n, HEADS, D).transpose(0, 1)            # noqa: E731  (H, n, D)
    dP = heads(case.go, Q) @ heads(case.v, S).transpose(1, 2)                        # (H, Q, S)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    gq = ((dS @ heads(case.k, S)) * D ** -0.5).transpose(0, 1).reshape(Q, E)
    return gq, torch.zeros(S, E, dtype=dtype), P.t() @ case.go[0].to(dtype)


def check_backward(case, grad_q, grad_kv, u, what=''):
    grad_q, grad_kv = grad_q.cpu(), grad_kv.cpu()
    assert grad_q.shape == (1, case.Q, E) and grad_kv.shape == (1, case.S, 2 * E), (what, grad_q.shape, grad_kv.shape)
    vis, n = case.visible(None)
    assert (n > 0).all()
    wq, _, wv = backward_ref(case, vis)
    gk, gv = grad_kv[0, :, :E], grad_kv[0, :, E:].double()
    assert bool((gk == 0).all()), f'{what}: grad_k is not 0 ({int((gk != 0).sum())} elements)'
    bad = (gv != 0) != (wv != 0)
    assert not bad.any(), f'{what}: grad_v is non-zero at {int((bad & (wv == 0)).sum())} blocked pairs, zero at {int((bad & (wv != 0)).sum())} visible'
    bound = torch.zeros(E, dtype=torch.float64)
    bound[:case.Q] = 2 * FACTOR * u * torch.log(n.double()).clamp_min(1.0)
    err = (gv - wv).abs()
    assert bool((err <= bound * wv).all()), f'{what}: grad_v off by {(err / wv.clamp_min(1e-30)).max().item():.3g} relative'
    scale = wq.abs().max().item()
    eq = (grad_q[0].double() - wq).abs().max().item()
    assert eq <= 2e-5 * scale + 1e-6, (what, 'grad_q', eq, scale)


# (Q, S, launch, first) of every consumer case: Q = 130 crosses the wrappers' 128-query split (4 query tiles + 2 rows), S > 256 runs
# both column assignments, and one S runs a single query whose row is 'only_last_key'
def consumer_shapes(bf16=False):
    shapes = []
    for S in (BF16_S if bf16 else F32_S):
        for launch in ((0, 1) if S > 256 else (0,)):
            shapes.append((130, S, launch, 0))
    shapes.append((1, 68 if bf16 else 65, 0, 2))
    return shapes


def forward_twice(case, fwd, full, what):
    """fwd(words (1, Q, W) int32) -> (out, lse | None), run with the unused bits of the last word cleared and set: equal outputs,
    and the first within `check_forward`"""
    out0, lse0 = fwd(case.words(False))
    out1, lse1 = fwd(case.words(True))
    assert same_or_both_nan(out0, out1), f'{what}: the output depends on the tail bits of the last word'
    assert lse0 is None or same_or_both_nan(lse0, lse1), f'{what}: the lse depends on the tail bits of the last word'
    check_forward(case, out0, lse0, full, what)


def backward_twice(case, bwd, u, what):
    """bwd(words) -> (out, lse, grad_q, grad_kv), as `forward_twice`"""
    r0, r1 = bwd(case.words(False)), bwd(case.words(True))
    for a, b, name in zip(r0, r1, ('out', 'lse', 'grad_q', 'grad_kv')):
        assert same_or_both_nan(a, b), f'{what}: {name} depends on the tail bits of the last word'
    check_forward(case, r0[0], r0[1], None, what)
    check_backward(case, r0[2], r0[3], u, what)


# ------------------------------------------------------------------------------------------------
# C. the chain
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_case():
    """(producer case, consumer case): the 5 x 7 level of a 20 x 28 map at pool 4, Q = 33. The consumer case's mask is
    fix_full_rows(attn_mask_from_logits(mask_logits(embed, feat))) of oracle/ops.py -- pixel p = i w + j of the producer is key p of
    the consumer. The planted negative query is the row that fix_full_rows clears."""
    case = producer_case(CHAIN_SPEC[0])
    blocked = ref.fix_full_rows(ref.attn_mask_from_logits(ref.mask_logits(case.embed, case.feat), (5, 7)).clone())
    assert blocked.shape == (1, 33, 35) and blocked.any() and not blocked.all(-1).any()
    assert not blocked[0, 32].any() and case.level(4).blocked[0, 32].all()
    return case, ConsumerCase(33, 35, blocked=blocked)
