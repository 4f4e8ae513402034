"""The attention-mask chain bit for bit on the exact operands of tests/attn_mask_cases.py (whose docstring derives every bound; the
cases are proven on the CPU by tests/test_attn_mask_cases.py). No tolerance on a bit anywhere. Kernels reached, per test:

  test_mask_logits_lattice       split: cgg_pack_mask_feature (hi + lo) -> cgg_mask_logits (f16 x 3, row groups of 128 in one launch)
                                 bf16:  cgg_pack_mask_feature (hi) -> cgg_mask_logits (bf16)
                                 f32:   cgg_mask_logits_f32 (through the Q > 128 split of ops.mask_logits)
                                 astat: cgg_pack_mask_feature (hi) -> cgg_mask_logits_bits_astat (register and LDS-ring kernels)
  test_mask_logits_channel_last  cgg_pack_mask_feature_nhwc, cgg_pack_mask_feature_nhwc_multi, cgg_pack_mask_feature_nhwc_f32_x3
                                 (all pools of a map from one launch) -> cgg_mask_logits / cgg_mask_logits_bits_astat
  test_attn_mask_from_logits     cgg_attn_mask_from_logits
  test_fix_full_rows_edges       cgg_attn_mask_fix_full_rows
  test_forward_visible_sets      cgg_masked_xattn_forward, _forward_strided, _forward_x3, _forward_lse (CGG_F32, CGG_F32_X3,
                                 CGG_F32_BF16MFMA), cgg_xattn_combine_wave; cgg_attn_mask_fix_full_rows in front of each
  test_forward_bf16_visible_sets cgg_masked_xattn_forward_bf16 with its in-kernel full-row test off and on
  test_backward_visible_sets     cgg_masked_xattn_forward_lse -> cgg_masked_xattn_backward / cgg_masked_xattn_backward_x3
  test_chain                     cgg_pack_mask_feature -> cgg_mask_logits -> cgg_attn_mask_fix_full_rows -> cgg_masked_xattn_forward(_x3)"""
import pytest
import torch

import attn_mask_cases as AM
from cgg_amd import ops, runtime

pytestmark = pytest.mark.gpu
H = AM.HEADS


# ------------------------------------------------------------------------------------------------
# A. producers
# ------------------------------------------------------------------------------------------------
PATHS = ('split', 'bf16', 'f32', 'astat')
LATTICE = [(path, name, pool) for path in PATHS for name, pool in AM.producer_levels()
           if path == 'split' or AM.PRODUCER_SPECS[name][1] < AM.SPLIT_ONLY_Q]


def _logits_and_words(case, lv, embed, packed, what):
    """want_logits + want_bits, and want_bits alone: the same words; both against the float64 reference"""
    logits, words = ops.mask_logits(embed, packed, want_logits=True, want_bits=True)
    none, alone = ops.mask_logits(embed, packed, want_logits=False, want_bits=True)
    assert none is None
    AM.check_logits(lv, logits, what)
    AM.check_words(case, lv, words, what)
    AM.assert_words(alone, lv.words, f'{what} want_bits alone')


@pytest.mark.parametrize('path,name,pool', LATTICE)
def test_mask_logits_lattice(dev, path, name, pool, monkeypatch):
    case = AM.producer_case(name)
    lv = case.level(pool)
    embed, feat = case.embed.to(dev), case.feat.to(dev)
    what = f'{path} {name} pool {pool}'
    if path == 'f32':
        monkeypatch.setattr(runtime, '_X3', False)       # read once at import: the test flips the module switch, not the environment
    with runtime.precision_scope('fp32'):
        packed = ops.pack_mask_feature(feat, pool=pool, split=path in ('split', 'f32'))
        assert (packed.h, packed.w, packed.words) == (lv.h, lv.w, lv.nwords)
        if path == 'f32':
            assert packed.f32 is not None
            assert torch.equal(packed.f32.cpu().double(), lv.feat64)
        elif path == 'split':
            assert runtime.x3_enabled() and packed.f32 is None and packed.lo is not None
        else:
            assert packed.f32 is None and packed.lo is None
        if path == 'astat':
            words = ops.mask_logits_bits_astat(embed, packed)
            AM.check_words(case, lv, words, what)
        else:
            _logits_and_words(case, lv, embed, packed, what)


@pytest.mark.parametrize('name', list(AM.NHWC_SPECS))
def test_mask_logits_channel_last(dev, name):
    """the same map channel-last: every level through the one-pool packer, all levels from one launch of the bf16 and the f32 -> x3
    packers; then the same kernels and the same words as from the channel-first packer"""
    case = AM.producer_case(name)
    embed = case.embed.to(dev)
    f32 = case.nhwc().to(dev)
    b16 = f32.bfloat16()
    pools = list(case.pools)
    with runtime.precision_scope('fp32'):
        assert runtime.x3_enabled()
        multi = ops.pack_mask_feature_nhwc_multi(b16, pools)
        x3 = ops.pack_mask_feature_nhwc_x3(f32, pools)
        for i, pool in enumerate(pools):
            lv = case.level(pool)
            one = ops.pack_mask_feature_nhwc(b16, pool)
            first = ops.pack_mask_feature(case.feat.to(dev), pool=pool, split=True)
            for tag, packed in (('nhwc', one), ('nhwc_multi', multi[i]), ('nhwc_x3', x3[i])):
                what = f'{tag} {name} pool {pool}'
                assert (packed.h, packed.w, packed.words) == (lv.h, lv.w, lv.nwords) and (packed.lo is not None) == (tag == 'nhwc_x3')
                _logits_and_words(case, lv, embed, packed, what)
                if packed.lo is None:
                    AM.check_words(case, lv, ops.mask_logits_bits_astat(embed, packed), f'{what} astat')
                else:               # the images themselves: the channel-first packer's, pad pixels of the last tile included
                    assert torch.equal(packed.hi, first.hi) and torch.equal(packed.lo, first.lo), f'{what}: packed images differ'


@pytest.mark.parametrize('name', list(AM.RESIZE_SPECS))
def test_attn_mask_from_logits(dev, name):
    case = AM.resize_case(name)
    words = ops.attn_mask_from_logits(case.logits.to(dev), (case.h, case.w))
    assert words.shape == (2, 3, (case.npix + 31) // 32) and words.dtype == torch.int32
    AM.check_resize(case, words, name)


@pytest.mark.parametrize('npix', AM.FIX_NPIX)
@pytest.mark.parametrize('rows', AM.FIX_ROWS)
def test_fix_full_rows_edges(dev, rows, npix):
    case = AM.fix_case(rows, npix)
    words = case.words.to(dev)
    out = ops.attn_mask_fix_full_rows(words, npix)
    AM.check_fix(case, out, f'rows {rows} npix {npix}')
    # a batch of rows in one launch: (2, rows, words)
    both = torch.stack([case.words, case.words.flip(0)]).to(dev)
    ops.attn_mask_fix_full_rows(both, npix)
    AM.assert_words(both, torch.stack([case.want, case.want.flip(0)]), f'rows 2 x {rows} npix {npix}')


# ------------------------------------------------------------------------------------------------
# B. consumers
# ------------------------------------------------------------------------------------------------
FORWARDS = ('f32', 'strided', 'x3', 'lse_f32', 'lse_x3', 'lse_bf16')
_shape_id = lambda s: f'Q{s[0]}S{s[1]}launch{s[2]}'         # noqa: E731


def _forward(variant, case, dev, monkeypatch):
    """fwd(words on the CPU) -> (out, lse | None) of one variant of `ops.masked_xattn`, its mode asserted"""
    monkeypatch.setattr(ops, 'XATTN_X3', variant not in ('f32', 'strided', 'lse_f32'))
    monkeypatch.setattr(ops, 'XATTN_X3_TRAIN', variant == 'lse_x3')
    q, kv = case.q.to(dev), case.kv.to(dev)
    if variant == 'strided':
        wide = torch.randn(1, case.S, 2 * AM.E + 64, device=dev)
        wide[..., 32:32 + 2 * AM.E] = kv
        kv = wide[..., 32:32 + 2 * AM.E]
        assert kv.is_contiguous() == (case.S == 1)              # a single row has no stride: it runs the dense kernel
    scope = 'bf16' if variant == 'lse_bf16' else 'fp32'
    with runtime.precision_scope(scope):
        if variant.startswith('lse'):
            want = dict(lse_f32=0, lse_x3=ops.CGG_F32_X3, lse_bf16=ops.CGG_F32_BF16MFMA)[variant]
            assert ops._xattn_train_dtype(forward=True) == want
        elif variant == 'x3':
            assert runtime.x3_enabled()

    def fwd(words, fix=False):
        bits = words.to(dev)
        if fix:
            ops.attn_mask_fix_full_rows(bits, case.S)
        with runtime.precision_scope(scope):
            r = ops.masked_xattn(q, kv, bits, H, return_lse=variant.startswith('lse'))
        return r if variant.startswith('lse') else (r, None)
    return fwd


@pytest.mark.parametrize('shape', AM.consumer_shapes(), ids=_shape_id)
@pytest.mark.parametrize('variant', FORWARDS)
def test_forward_visible_sets(dev, variant, shape, monkeypatch):
    Q, S, launch, first = shape
    what = f'{variant} {_shape_id(shape)}'
    plain = AM.consumer_case(Q, S, launch, False, first)
    AM.forward_twice(plain, _forward(variant, plain, dev, monkeypatch), None, what)
    if Q == 1:                                                  # the single row is 'only_last_key'
        return
    full = AM.consumer_case(Q, S, launch, True, first)
    fwd = _forward(variant, full, dev, monkeypatch)
    AM.forward_twice(full, fwd, 'nan', f'{what} full=nan')
    AM.forward_twice(full, lambda w: fwd(w, fix=True), 'mean', f'{what} full=mean after fix_full_rows')


@pytest.mark.parametrize('shape', AM.consumer_shapes(bf16=True), ids=_shape_id)
def test_forward_bf16_visible_sets(dev, shape):
    Q, S, launch, first = shape
    what = f'bf16 {_shape_id(shape)}'

    def forward(case, fix_in_kernel, fix_before=False):
        q, k = case.q.to(dev), case.k.bfloat16().to(dev)
        vt = case.v.bfloat16().transpose(1, 2).contiguous().to(dev)

        def fwd(words):
            bits = words.to(dev)
            if fix_before:
                ops.attn_mask_fix_full_rows(bits, S)
            kept = bits.clone()
            out = ops.masked_xattn_bf16(q, k, vt, bits, H, fix_full_rows=fix_in_kernel)
            assert torch.equal(bits, kept)                      # `bits` itself is not modified
            return out, None
        return fwd
    plain = AM.consumer_case(Q, S, launch, False, first, True)
    AM.forward_twice(plain, forward(plain, False), None, what)
    AM.forward_twice(plain, forward(plain, True), None, f'{what} in-kernel test, no full row')
    if Q == 1:
        return
    full = AM.consumer_case(Q, S, launch, True, first, True)
    AM.forward_twice(full, forward(full, False), 'nan', f'{what} full=nan')
    AM.forward_twice(full, forward(full, True), 'mean', f'{what} full=mean in-kernel')
    AM.forward_twice(full, forward(full, False, fix_before=True), 'mean', f'{what} full=mean after fix_full_rows')


@pytest.mark.parametrize('shape', AM.consumer_shapes(), ids=_shape_id)
@pytest.mark.parametrize('form', ['x3', 'f32'])
def test_backward_visible_sets(dev, form, shape, monkeypatch):
    Q, S, launch, first = shape
    x3 = form == 'x3'
    monkeypatch.setattr(ops, 'XATTN_X3', True)
    monkeypatch.setattr(ops, 'XATTN_X3_TRAIN', x3)
    monkeypatch.setattr(ops, 'XATTN_X3_BWD', x3)
    case = AM.consumer_case(Q, S, launch, False, first)
    q, kv, go = case.q.to(dev), case.kv.to(dev), case.go.to(dev)

    def bwd(words):
        bits = words.to(dev)
        with runtime.precision_scope('fp32'):
            assert runtime.x3_enabled() and ops._xattn_train_dtype(forward=True) == (ops.CGG_F32_X3 if x3 else 0)
            out, lse = ops.masked_xattn(q, kv, bits, H, return_lse=True)
            gq, gkv = ops.masked_xattn_backward(q, kv, bits, out, lse, go, H)
        return out, lse, gq, gkv
    AM.backward_twice(case, bwd, AM.U_X3 if x3 else AM.U_F32, f'backward {form} {_shape_id(shape)}')


# ------------------------------------------------------------------------------------------------
# C. the chain
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('x3', [True, False], ids=['x3', 'f32'])
def test_chain(dev, x3, monkeypatch):
    """lattice embed and feat -> mask_logits(want_bits) -> attn_mask_fix_full_rows -> masked_xattn: the rows see the keys that
    oracle/ops.py's fix_full_rows(attn_mask_from_logits(mask_logits(...))) leaves visible -- pixel i w + j is key i w + j"""
    monkeypatch.setattr(ops, 'XATTN_X3', x3)
    case, cons = AM.chain_case()
    lv = case.level(4)
    with runtime.precision_scope('fp32'):
        packed = ops.pack_mask_feature(case.feat.to(dev), pool=4, split=True)
        _, bits = ops.mask_logits(case.embed.to(dev), packed, want_logits=False, want_bits=True)
        AM.assert_words(bits, lv.words, 'chain mask_logits')
        ops.attn_mask_fix_full_rows(bits, lv.npix)
        AM.assert_words(bits, cons.words(False), 'chain fix_full_rows')
        out = ops.masked_xattn(cons.q.to(dev), cons.kv.to(dev), bits, H)
    AM.check_forward(cons, out, None, None, 'chain')
