"""The mask-logit backward on the exact operands of tests/mask_grad_cases.py (whose docstring derives why both modes and every
summation order give the float64 einsum; the cases, their plan and the seeded faults are proven on the CPU by
tests/test_mask_grad_cases.py). Every comparison is `torch.equal`: plain bf16 mode is held to equality here, not to the 1e-2 of
test_kernels_gpu.py::test_mask_logits_backward_vs_float64, which keeps the randn accuracy claim. Kernels reached, per test:

  test_backward_owned_buffers   cgg_mask_logits_backward through `ops._call`, over the whole table, into caller-owned views of
                                sentinel-filled buffers with guards in front and behind, workspace sentinel-filled as well:
                                cgg_mask_logits_grad_feat_kernel<true> with KS = 1 .. 8 and 1 .. 3 row groups, <false> with KS = 1, 3,
                                9, 13, 16 and 1 .. 3 row groups (a group after the first adds into the first one's store);
                                cgg_mask_logits_grad_embed_kernel<SPLIT, MT> for MT = 1 .. 4 in both modes, 1 .. 5 row groups, one
                                and two pixel chunks with a last chunk of 1 (a half step), 2 and 3 steps;
                                cgg_mask_logits_grad_embed_reduce; 8 pixels (one half step, the upper half-wave's clamp) to 1072;
                                the tile wrap at B = 512; grad_embed alone and grad_feat alone
  test_backward_wrapper         ops.mask_logits_backward (its own outputs and the shared workspace) on one case per edge family,
                                the need_embed / need_feat forms, twice for equal bits
  test_autograd_function_chain  mask2former_head._MaskLogitsFn: cgg_pack_mask_feature, the forward (cgg_mask_logits_f32 or
                                cgg_mask_logits, in slices of 256 rows at Q = 513) and the backward above, Q = 1, 129, 257, 513
  test_lazy_masks_on_device     LazyMasks.select / preselect / select_by_weights with `packed` set: the index_put packing, ONE
                                _MaskLogitsFn call per contraction, the gather and its scatter backward, layers without positives"""
import pytest
import torch

import mask_grad_cases as MG
from cgg_amd import ops
from cgg_amd import mask2former_head as M2F

pytestmark = pytest.mark.gpu
GUARD = 4096                    # floats in front of and behind every owned output (a multiple of 4: the views stay 16-B aligned)


def _owned(shape, dev):
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((GUARD + n + GUARD,), MG.SENTINEL, device=dev)
    view = buf[GUARD:GUARD + n].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return buf, view


def _assert_guards(buf, what):
    assert (buf[:GUARD] == MG.SENTINEL).all(), f'{what}: stored in front of the buffer'
    assert (buf[-GUARD:] == MG.SENTINEL).all(), f'{what}: stored behind the buffer'


@pytest.mark.parametrize('case', MG.CASES, ids=MG.CASE_IDS)
def test_backward_owned_buffers(dev, case):
    """The library entry as `ops.mask_logits_backward` calls it, but into memory this test owns: a skipped store leaves the sentinel
    (never an earlier call's right answer in a recycled block), a first row group that adds into old contents adds to the sentinel,
    a store outside the output meets a guard. The rows behind a row group are the next group's live operands -- a leak flips a parity."""
    c, p = case, MG.case_plan(case)
    o = MG.operands(c.B, c.Q, c.h, c.w)
    npix = c.h * c.w
    embed, feat, gout = o.embed.to(dev), o.feat.to(dev), o.grad_out.to(dev)
    ws_bytes = ops._lib_().cgg_mask_logits_backward_workspace_bytes(c.B, min(c.Q, 128), MG.C, npix)
    assert ws_bytes == 4 * p.ws_floats, (ws_bytes, p.ws_floats)                      # the plan restated in MG.plan is the library's
    ws_buf, ws = _owned((p.ws_floats,), dev)
    ge_buf, ge = _owned((c.B, c.Q, MG.C), dev) if c.need_embed else (None, None)
    gf_buf, gf = _owned((c.B, MG.C, c.h, c.w), dev) if c.need_feat else (None, None)
    ops._call('cgg_mask_logits_backward', ops.dev_ptr(embed, 'embed', torch.float32), ops.dev_ptr(feat, 'feat', torch.float32),
              ops.dev_ptr(gout, 'grad_out', torch.float32), ops.dev_ptr(ge), ops.dev_ptr(gf), ops.dev_ptr(ws), c.B, c.Q, MG.C, npix,
              int(c.split), ops.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    what = MG.case_id(c)
    want_e, want_f = MG.reference(c)
    if c.need_embed:
        assert not (ge == MG.SENTINEL).any(), f'{what}: grad_embed has elements that were never stored'
        MG.assert_equal(ge, want_e, f'{what} grad_embed')
        _assert_guards(ge_buf, f'{what} grad_embed')
    if c.need_feat:
        assert not (gf == MG.SENTINEL).any(), f'{what}: grad_feat has elements that were never stored'
        MG.assert_equal(gf, want_f, f'{what} grad_feat')
        _assert_guards(gf_buf, f'{what} grad_feat')
    _assert_guards(ws_buf, f'{what} workspace')
    if not c.need_embed:
        assert (ws == MG.SENTINEL).all(), f'{what}: the workspace was written without grad_embed'
    for t, src, name in ((embed, o.embed, 'embed'), (feat, o.feat, 'feat'), (gout, o.grad_out, 'grad_out')):
        assert torch.equal(t.cpu(), src), f'{what}: operand {name} changed'


def _one_per_family():
    """one case per edge family: rows in one group and across groups (both modes), 8 pixels, a half step, each chunk tail, the wrap,
    each single-output form"""
    want = ['b1_q1_4x8_split', 'b3_q8_5x8_split', 'b1_q33_3x88_split', 'b3_q129_5x8_split', 'b3_q257_5x8_split',
            'b3_q136_5x8_plain', 'b3_q257_5x8_plain', 'b3_q513_4x8_plain', 'b3_q1_1x8_split', 'b3_q257_1x8_plain',
            'b1_q33_24x43_split', 'b3_q129_24x44_split', 'b1_q33_8x134_plain', 'b512_q2_8x33_plain',
            'b3_q129_5x8_split_feat_only', 'b3_q257_7x8_plain_feat_only', 'b3_q129_7x8_split_embed_only',
            'b3_q257_5x8_plain_embed_only']
    by_id = dict(zip(MG.CASE_IDS, MG.CASES))
    return [by_id[n] for n in want]


@pytest.mark.parametrize('case', _one_per_family(), ids=MG.case_id)
def test_backward_wrapper(dev, case):
    c = case
    o = MG.operands(c.B, c.Q, c.h, c.w)
    embed, feat, gout = o.embed.to(dev), o.feat.to(dev), o.grad_out.to(dev)
    assert ops.mask_logits_backward_ok(embed, feat)
    want_e, want_f = MG.reference(c)
    what = MG.case_id(c)
    runs = []
    for _ in range(2):
        ge, gf = ops.mask_logits_backward(embed, feat, gout, c.split, need_embed=c.need_embed, need_feat=c.need_feat)
        assert (ge is None) == (not c.need_embed) and (gf is None) == (not c.need_feat), f'{what}: an output that was not asked for'
        if c.need_embed:
            assert tuple(ge.shape) == (c.B, c.Q, MG.C)
            MG.assert_equal(ge, want_e, f'{what} grad_embed (wrapper)')
        if c.need_feat:
            assert tuple(gf.shape) == (c.B, MG.C, c.h, c.w)
            MG.assert_equal(gf, want_f, f'{what} grad_feat (wrapper)')
        runs.append((ge, gf))
    for a, b in zip(*runs):
        assert (a is None and b is None) or (a.data_ptr() != b.data_ptr() and torch.equal(a, b)), f'{what}: two calls differ'


@pytest.mark.parametrize('split', [True, False], ids=['split', 'plain'])
@pytest.mark.parametrize('Q', [1, 129, 257, 513])
def test_autograd_function_chain(dev, Q, split):
    """`_MaskLogitsFn.apply` on packed features: the forward is the float64 einsum (|logit| <= 9 x 256), `torch.autograd.grad` with the
    integer upstream the references; 513 rows take the forward's slices of 256 and three to five row groups in the backward"""
    B, h, w = 3, 7, 8
    o = MG.operands(B, Q, h, w)
    embed, feat = o.embed.to(dev).requires_grad_(True), o.feat.to(dev).requires_grad_(True)
    packed = ops.pack_mask_feature(feat.detach(), 1, split)
    assert (packed.lo is not None) == split and ops.mask_logits_ok(embed, packed) and ops.mask_logits_backward_ok(embed, feat)
    out = M2F._MaskLogitsFn.apply(embed, feat, packed)
    what = f'_MaskLogitsFn Q={Q} {"split" if split else "plain"}'
    MG.assert_equal(out, MG.forward_reference(B, Q, h, w), f'{what} forward')
    ge, gf = torch.autograd.grad(out, (embed, feat), o.grad_out.to(dev))
    want_e, want_f = MG._reference(B, Q, h, w)
    MG.assert_equal(ge, want_e, f'{what} grad_embed')
    MG.assert_equal(gf, want_f, f'{what} grad_feat')
    # one input alone: the other output is not computed
    out = M2F._MaskLogitsFn.apply(embed, feat.detach(), packed)
    MG.assert_equal(torch.autograd.grad(out, embed, o.grad_out.to(dev))[0], want_e, f'{what} grad_embed alone')
    out = M2F._MaskLogitsFn.apply(embed.detach(), feat, packed)
    MG.assert_equal(torch.autograd.grad(out, feat, o.grad_out.to(dev))[0], want_f, f'{what} grad_feat alone')


@pytest.mark.parametrize('split', [True, False], ids=['split', 'plain'])
@pytest.mark.parametrize('how', MG.LAZY_HOW)
@pytest.mark.parametrize('name', list(MG.LAZY_SPECS))
def test_lazy_masks_on_device(dev, name, how, split, monkeypatch):
    """the scenarios of tests/test_mask_grad_cases.py with `packed` set: `_contract` runs `_MaskLogitsFn`, whose backward must be the
    HIP one -- once per contraction (one for all layers after `preselect`, one per live layer otherwise), never the einsum pair"""
    s = MG.lazy_scenario(name)
    calls = []
    real = ops.mask_logits_backward

    def counted(embed, feat, grad_out, split_, *a, **k):
        calls.append((tuple(embed.shape), bool(split_)))
        return real(embed, feat, grad_out, split_, *a, **k)
    monkeypatch.setattr(ops, 'mask_logits_backward', counted)
    got = MG.run_lazy(M2F.LazyMasks, name, how, dev, pack=lambda f: ops.pack_mask_feature(f, 1, split))
    MG.assert_lazy_equal(got, name, f'{name} {how} {"split" if split else "plain"}')
    live = [max(row) for row in s.counts if max(row)]
    want_calls = [(s.B, s.sum_pm, MG.C)] if how == 'preselect' else [(s.B, pm, MG.C) for pm in live]
    assert sorted(c[0] for c in calls) == sorted(want_calls) and all(c[1] == split for c in calls), calls
    # a layer without positives: shape (0, h, w), zero gradients, no kernel call
    for l, row in enumerate(s.counts):
        if not any(row):
            assert tuple(got[0][l].shape) == (0, s.h, s.w) and got[0][l].is_cuda and not got[1][l].any()


def test_lazy_masks_pm_zero_call_on_device(dev):
    s = MG.lazy_scenario('below_8')
    e, f = s.embeds[0].to(dev).requires_grad_(True), s.feat.to(dev).requires_grad_(True)
    lz = M2F.LazyMasks(e, f, ops.pack_mask_feature(f.detach(), 1, True))
    out = lz.select(MG.positions(torch.zeros(s.B, s.Q, device=dev)))
    assert tuple(out.shape) == (0, s.h, s.w) and out.is_cuda
    ge, gf = torch.autograd.grad(out.sum(), (e, f))
    assert tuple(ge.shape) == tuple(e.shape) and tuple(gf.shape) == tuple(f.shape) and not ge.any() and not gf.any()
