"""tests/attn_mask_cases.py before it meets a kernel. CPU only.

EXACT -- on every level of every case the f32 and float64 einsums are equal, F.interpolate in f32 equals its float64 result, the
pooled feature survives .bfloat16() and .half() unchanged, `embed x pooled feature` equals `interpolate(embed x feat)`, the logits stay
far inside the exact range and exact zeros occur; the resize cases leave out at most 1 % and have no other element near a tie.

ROOM and TEETH -- a torch emulation of the rule (`emu_*` below: f32, the kernels' row groups / pixel tiles / key chunks) passes every
assertion that tests/test_attn_mask_edges_gpu.py makes, and each of its seeded FAULTS trips at least one named case."""
import functools

import pytest
import torch
import torch.nn.functional as F

import attn_mask_cases as AM
from oracle import ops as ref

PRODUCER_FAULTS = ('le_zero', 'tail_bits_set', 'word_index_off_by_one', 'pool_origin_off_by_one', 'row_group_reads_group_0',
                   'ragged_tile_dropped')
CONSUMER_FAULTS = ('last_key_lost', 'blocked_chunk_kept', 'blocked_prefix_unmasks_row', 'tail_bits_honoured')
FAULTS = PRODUCER_FAULTS + CONSUMER_FAULTS
ALL_LEVELS = AM.producer_levels() + AM.producer_levels(AM.NHWC_SPECS) + [(AM.CHAIN_SPEC[0], 4)]


# ------------------------------------------------------------------------------------------------
# EXACT
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,pool', ALL_LEVELS)
def test_lattice_is_exact(name, pool):
    case = AM.producer_case(name)
    lv = case.level(pool)
    full64 = ref.mask_logits(case.embed.double(), case.feat.double())
    assert torch.equal(ref.mask_logits(case.embed, case.feat).double(), full64)                   # f32 einsum == float64 einsum
    p32 = AM.pooled(case.feat, pool)
    assert torch.equal(p32.double(), lv.feat64)
    assert torch.equal(p32.bfloat16().float(), p32) and torch.equal(p32.half().float(), p32)      # exact in bf16 and in f16
    assert torch.equal(case.embed.bfloat16().float(), case.embed) and torch.equal(case.embed.half().float(), case.embed)
    assert torch.equal(ref.mask_logits(case.embed, p32).double(), lv.logits64)
    size = (lv.h, lv.w)
    i64 = F.interpolate(full64, size, mode='bilinear', align_corners=False)
    i32 = F.interpolate(full64.float(), size, mode='bilinear', align_corners=False)
    assert torch.equal(i32.double(), i64)                                                         # interpolate f32 == float64
    assert torch.equal(i64, lv.logits64)                                        # embed x pooled feature == interpolate(embed x feat)
    assert torch.equal(ref.attn_mask_from_logits(full64.float(), size), lv.blocked)               # the reference rule, literally
    top = lv.logits64.abs().max().item()
    zeros = (lv.logits64 == 0).float().mean().item()
    print(f'{name} pool {pool}: npix {lv.npix} max |logit| {top:g} exact zeros {100 * zeros:.2f} %')
    assert top <= 1024.0           # quarter units below 2^12: every partial sum of an f32 accumulator is exact (2^24)
    assert (lv.logits64 * 4 == (lv.logits64 * 4).round()).all()
    if case.Q >= 5:
        assert (lv.logits64 == 0).any() and lv.blocked.any() and (lv.logits64 > 0).any()
    AM.check_planted(case, lv, lv.words, f'{name} reference')


def test_exact_zeros_occur_unplanted():
    """0.2 - 0.8 % of the logits of the pooled levels are exact zeros apart from the planted rows and pixel (measured 0.3 - 0.7 %)"""
    shares = []
    for name, pool in AM.producer_levels():             # one level per map: the zero block is that level's last pixel alone
        case = AM.producer_case(name)
        lv = case.level(pool)
        if pool == 1 or case.Q < 31 or lv.npix < 31:
            continue
        keep = torch.ones(case.B, case.Q, lv.npix, dtype=torch.bool)
        for rows in case.planted.values():
            for b, q in rows:
                keep[b, q] = False
        keep[..., lv.npix - 1] = False
        shares.append(((lv.logits64.flatten(2)[keep] == 0).float().mean().item(), int(keep.sum())))
    print('share of exact zeros per pooled level:', [round(100 * s, 2) for s, _ in shares])
    assert shares and 0.001 <= sum(s for s, _ in shares) / len(shares) <= 0.01
    assert all(s > 0.0 for s, n in shares if n >= 4096)


@pytest.mark.parametrize('name', list(AM.RESIZE_SPECS))
def test_resize_case_numbers(name):
    c = AM.resize_case(name)
    share = c.excluded.float().mean().item()
    nz = c.ref64.abs()[c.ref64.abs() >= AM.TRUE_ZERO]
    e32 = (c.ref32.double() - c.ref64).abs().max().item()
    print(f'{name}: excluded {100 * share:.2f} %  smallest non-zero |value| {nz.min().item():.3g}  torch f32 error {e32:.3g}')
    assert share <= AM.RESIZE_CAP
    # tap weights are multiples of 1 / (2 h) x 1 / (2 w) and the taps integers: no value lies strictly between 0 and 1 / (4 h w)
    assert nz.min().item() >= (1.0 - 1e-9) / (4 * c.h * c.w)
    assert e32 <= 3e-5 and e32 < 0.25 * nz.min().item()
    assert c.taps_zero.any() and not c.want[c.taps_zero].any()
    if c.exact:
        assert torch.equal(c.ref32.double(), c.ref64)


@pytest.mark.parametrize('rows', AM.FIX_ROWS)
@pytest.mark.parametrize('npix', AM.FIX_NPIX)
def test_fix_case_kinds(rows, npix):
    c = AM.fix_case(rows, npix)
    assert c.words.shape == (rows, (npix + 31) // 32)
    for r, kind in enumerate(c.kinds):
        assert bool(c.cleared[r]) == (kind in ('full', 'full_valid_tail0', 'full_valid_tail1')), (r, kind)
    if npix > 2048:
        assert c.words.shape[1] > 64 and ('full_but_far' not in c.kinds or not c.bits[c.kinds.index('full_but_far'), 64 * 32])


# ------------------------------------------------------------------------------------------------
# the emulation
# ------------------------------------------------------------------------------------------------
def emu_producer(case, pool, fault=None):
    """(logits f32 (B, Q, h, w), words): 2 x 2 mean -> f32 contraction per row group of 128 queries -> (< 0) per 32-pixel tile"""
    lv = case.level(pool)
    f = case.feat
    if pool > 1:
        o = pool // 2 - 1 + (1 if fault == 'pool_origin_off_by_one' else 0)
        fp = F.pad(f, (0, 1, 0, 1), mode='replicate')
        cut = lambda t: t[..., :lv.h, :lv.w]                                              # noqa: E731
        f = ((cut(fp[..., o::pool, o::pool]) + cut(fp[..., o::pool, o + 1::pool]))
             + (cut(fp[..., o + 1::pool, o::pool]) + cut(fp[..., o + 1::pool, o + 1::pool]))) * 0.25
    x = f.flatten(2)
    logits = torch.zeros(case.B, case.Q, lv.npix)
    for q0 in range(0, case.Q, 128):
        e = case.embed[:, q0:q0 + 128]
        if fault == 'row_group_reads_group_0':
            e = case.embed[:, :e.shape[1]]
        logits[:, q0:q0 + 128] = e @ x
    neg = logits <= 0 if fault == 'le_zero' else logits < 0
    if fault == 'ragged_tile_dropped' and lv.npix % 32:
        logits[..., lv.npix // 32 * 32:] = 0.0
        neg[..., lv.npix // 32 * 32:] = False
    words = AM.pack_words(neg, tail=fault == 'tail_bits_set')
    if fault == 'word_index_off_by_one':
        words = torch.roll(words, 1, -1)
    return logits.view(case.B, case.Q, lv.h, lv.w), words


def emu_resize(case, fault=None):
    neg = case.ref32 <= 0 if fault == 'le_zero' else case.ref32 < 0
    words = AM.pack_words(neg, tail=fault == 'tail_bits_set')
    return torch.roll(words, 1, -1) if fault == 'word_index_off_by_one' else words


def emu_fix(words, npix, fault=None):
    """rows whose valid bits are all set become zero words (`tail_bits_honoured`: whose every bit is set)"""
    bits = AM.unpack_words(words)
    full = bits.all(-1) if fault == 'tail_bits_honoured' else bits[..., :npix].all(-1)
    out = words.clone()
    out[full] = 0
    return out


def emu_visible(case, words, fix=False, fault=None):
    """(Q, S) float: the keys each row of `words` (1, Q, W) attends to, chunk by chunk as csrc/xattn.hip splits them"""
    S = case.S
    raw = AM.unpack_words(words[0])
    valid = torch.arange(raw.shape[1]) < (S - 1 if fault == 'last_key_lost' else S)
    vis = ~raw & valid
    KC = AM.chunk_keys(S)
    chunks = [slice(c, min(c + KC, raw.shape[1])) for c in range(0, S, KC)]
    if fix:
        if fault == 'tail_bits_honoured':
            full = raw.all(1)
        elif fault == 'blocked_prefix_unmasks_row':
            full = vis[:, chunks[0]].sum(1) == 0
        else:
            full = vis.sum(1) == 0
        vis[full] = valid
    if fault == 'blocked_chunk_kept':
        for sl in chunks:
            dead = vis[:, sl].sum(1) == 0
            vis[dead, sl] = valid[sl]
    return vis[:, :S].float()


def emu_forward(case, words, fix=False, fault=None, lse=True):
    vis = emu_visible(case, words, fix, fault)
    n = vis.sum(1)
    out = (vis @ case.v[0]) / n[:, None]
    return out[None], (torch.log(n)[None, None].expand(1, AM.HEADS, case.Q) if lse else None)


def emu_backward(case, words, fault=None):
    vis = emu_visible(case, words, False, fault)
    out, lse = emu_forward(case, words, False, fault)
    gq, gk, gv = AM.backward_ref(case, vis, torch.float32)
    return out, lse, gq[None], torch.cat([gk, gv], -1)[None]


@functools.lru_cache(maxsize=None)
def run_grid(fault=None):
    """every assertion of the GPU file on the emulation: {case label: the assertion's message} of those that fail"""
    failed = {}

    def attempt(label, fn):
        try:
            fn()
        except AssertionError as e:
            failed[label] = str(e)[:200]

    def producer(name, pool):
        case = AM.producer_case(name)
        lv = case.level(pool)
        logits, words = emu_producer(case, pool, fault)
        AM.check_logits(lv, logits, name)
        AM.check_words(case, lv, words, name)
    for name, pool in ALL_LEVELS:
        attempt(f'producer {name} pool {pool}', lambda: producer(name, pool))
    for name in AM.RESIZE_SPECS:
        attempt(f'resize {name}', lambda: AM.check_resize(AM.resize_case(name), emu_resize(AM.resize_case(name), fault), name))
    for rows in AM.FIX_ROWS:
        for npix in AM.FIX_NPIX:
            c = AM.fix_case(rows, npix)
            attempt(f'fix rows {rows} npix {npix}', lambda: AM.check_fix(c, emu_fix(c.words, npix, fault), 'fix'))
    for bf16 in (False, True):
        tag = 'bf16' if bf16 else 'f32'
        for Q, S, launch, first in AM.consumer_shapes(bf16):
            label = f'{tag} Q{Q} S{S} launch {launch}'
            plain = AM.consumer_case(Q, S, launch, False, first, bf16)
            full = AM.consumer_case(Q, S, launch, True, first, bf16)
            attempt(f'forward {label}', lambda: AM.forward_twice(plain, lambda w: emu_forward(plain, w, False, fault), None, label))
            if Q == 1:                                          # the single row is 'only_last_key'
                continue
            attempt(f'forward full=nan {label}', lambda: AM.forward_twice(full, lambda w: emu_forward(full, w, False, fault), 'nan', label))
            attempt(f'forward full=mean in-kernel {label}',
                    lambda: AM.forward_twice(full, lambda w: emu_forward(full, w, True, fault), 'mean', label))
            attempt(f'forward full=mean fix_full_rows {label}',
                    lambda: AM.forward_twice(full, lambda w: emu_forward(full, emu_fix(w, S, fault), False, fault), 'mean', label))
            if not bf16:
                attempt(f'backward {label}', lambda: AM.backward_twice(plain, lambda w: emu_backward(plain, w, fault), AM.U_F32, label))
    attempt('chain', lambda: chain(fault))
    return failed


def chain(fault=None):
    case, cons = AM.chain_case()
    _, words = emu_producer(case, 4, fault)
    words = emu_fix(words, 35, fault)
    out, lse = emu_forward(cons, words, False, fault)
    AM.check_forward(cons, out, lse, None, 'chain')


def test_room():
    failed = run_grid()
    assert not failed, failed


@pytest.mark.parametrize('fault', FAULTS)
def test_teeth(fault):
    failed = run_grid(fault)
    print(f'{fault}: caught by {len(failed)} cases:')
    for k, v in failed.items():
        print(f'  {k}: {v}')
    assert failed, f'{fault}: every case passes'
    kind = ('producer', 'resize', 'fix', 'chain') if fault in PRODUCER_FAULTS else ('forward', 'backward', 'fix', 'chain')
    assert all(k.split()[0] in kind for k in failed), f'{fault} trips cases of the other side: {list(failed)}'


def test_teeth_are_named():
    """the case each fault is meant for does catch it"""
    def producer(Q, npix):
        name = AM.find_case(Q, npix)
        return f'producer {name} pool {AM.PRODUCER_SPECS[name][4][0]}'
    meant = {
        'le_zero': producer(33, 35),                           # exact zeros of a pooled level
        'tail_bits_set': producer(1, 1),                       # 31 unused bits
        'word_index_off_by_one': producer(129, 288),           # nine words
        'pool_origin_off_by_one': producer(32, 35),            # pool 4
        'row_group_reads_group_0': producer(257, 33),          # rows 128 .. 256 of the split-mode launch
        'ragged_tile_dropped': producer(128, 257),             # 8 tiles + 1 pixel
        'last_key_lost': 'forward f32 Q1 S65 launch 0',
        'blocked_chunk_kept': 'forward f32 Q130 S321 launch 0',
        'blocked_prefix_unmasks_row': 'forward full=mean in-kernel bf16 Q130 S324 launch 1',
        'tail_bits_honoured': 'forward full=mean in-kernel bf16 Q130 S36 launch 0',
    }
    assert set(meant) == set(FAULTS)
    for fault, label in meant.items():
        assert label in run_grid(fault), (fault, label)
