"""-m gpu: the inference-tail kernels of csrc/postproc.hip against the float64 references of tests/postproc_cases.py, at the geometry
edges of every branch of instance_masks_dispatch, with ops.panoptic_argmax / panoptic_paint called directly and the softmax / top-k
kernels held to a float64 bound. Thresholded outputs are compared with torch.equal outside the exclusion band of the inputs
(tests/test_postproc_cases.py shows that the band holds at most 1e-3 of the pixels); every assertion message carries the excluded
count. Each test prints its worst ratio to the bound it asserts.

Measured on an MI355X (excluded pixels over all 16 planes; worst mask-score error / bound over instance_masks, multi, picks, bitpack):
  generic_noninteger 3 of 56 000, 0.008     scale4_cropped_w70 0, 0.006     two_stage_up 1 of 132 000, 0.007
  two_stage_down 1 of 41 328, 0.008         scale3 2 of 69 120, 0.008       fast_w96 0, 0.006      generic_w100 0, 0.008
  clamp_4x4_s2 / s4 / s8 0, 0.010 / 0.011 / 0.018       row_1x8_s2 / s4 / s8 0, 0.012 / 0.013 / 0.021
  fast_many_tiles 0, 0.007     down_32_to_16 0, 0.011     down_20x28_to_13x9 0, 0.007     picks_generic 6e-5, 0.007     picks_fast 0, 0.008
  panoptic n1 / n7 / n7_twins / n40 / n1024: no pixel excluded, every id, win_half and count equal to the rule
  softmax (prob and maxv): rows 1 / 5 / 37 at 0.385 / 0.401 / 0.408 of the bound (torch's own f32 softmax on the CPU: 0.39)
  class_topk scores: three_types 0.195, wide_300 0.157, k1 0.180, k_all 0.260, k1024 0.252, window 0.148 of the bound
  upsample_bilinear: 0.040, 0.058, 0.141, 0.141 of the band, in the order of UPSAMPLE_CASES (torch f32 on the CPU: 0.040, 0.051, 0.141, 0.141)
clamp_4x4_s2 has out_w = 8 and so runs the generic kernel; S = 2 with both column clamps inside one thread of the fast path is
row_1x8_s2."""
import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import ops

import postproc_cases as PC

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ A. instance masks
def _check_masks(label, masks, idx, ref):
    """masks (n, oh, ow) bool of the planes idx against the rule, outside the band"""
    masks = masks.cpu()
    want, inside = ref.mask[idx], ref.inside[idx]
    assert masks.shape == want.shape, (label, masks.shape, want.shape)
    bad = (masks != want) & ~inside
    assert torch.equal(masks[~inside], want[~inside]), \
        f'{label}: {int(bad.sum())} pixels differ from the rule outside the band ({int(inside.sum())} of {inside.numel()} excluded); ' \
        f'first at {bad.nonzero()[:4].tolist()}'


def _check_scores_boxes(label, score, box, idx, ref):
    """per-detection mask score (within 1e-5 + pixels in the band / count) and box (exact when no pixel is in the band)"""
    score, box = score.cpu().double(), box.cpu()
    err = (score - ref.score[idx]).abs()
    ratio = (err / ref.score_bound[idx]).max().item()
    print(f'{label}: mask score at {ratio:.3f} of its bound (worst |error| {err.max().item():.2e})')
    assert bool((err <= ref.score_bound[idx]).all()), f'{label}: score error {err.tolist()} against {ref.score_bound[idx].tolist()}'
    clean = ref.n_inside[idx] == 0
    assert torch.equal(box[clean], ref.box[idx][clean]), f'{label}: boxes {box[clean].tolist()} != {ref.box[idx][clean].tolist()}'
    for j, q in enumerate(idx.tolist()):
        if ref.count[q] == 0:                               # empty mask: score exactly 0, box (0, 0, 0, 0)
            assert score[j].item() == 0.0 and box[j].tolist() == [0, 0, 0, 0], (label, q, score[j].item(), box[j].tolist())


def _picks_of(ref, g):
    """the selection, twice over in another order, with class scores"""
    sel = torch.tensor(PC.SEL)
    qidx = torch.cat([sel, sel.flip(0)[:7]])
    return qidx, torch.rand(qidx.numel(), generator=g) * 0.9 + 0.1


def _check_picks(label, masks, bboxes, qidx, cls, ref):
    _check_masks(label, masks, qidx, ref)
    bboxes = bboxes.cpu()
    clean = ref.n_inside[qidx] == 0
    assert torch.equal(bboxes[:, :4][clean], ref.box[qidx][clean]), f'{label}: boxes'
    want = cls.double() * ref.score[qidx]
    bound = cls.double() * ref.score_bound[qidx] + 2.0 ** -23 * want              # the product's own rounding
    err = (bboxes[:, 4].double() - want).abs()
    print(f'{label}: class score x mask score at {(err / bound).max().item():.3f} of its bound')
    assert bool((err <= bound).all()), f'{label}: {err.tolist()} against {bound.tolist()}'


@pytest.mark.parametrize('name', list(PC.INSTANCE_GEOMS))
def test_instance_masks_match_the_rule(dev, name):
    """instance_masks, instance_masks_multi and instance_masks_picks on one geometry: masks, mask scores and boxes against the rule"""
    ref = PC.instance_case(name)
    hw, up, crop, out = PC.INSTANCE_GEOMS[name]
    logits = ref.logits.to(dev)
    sel = torch.tensor(PC.SEL)
    assert ops.instance_masks_bitpack_ok(hw, up, crop, out) == PC.bitpack_expected(name)
    masks, score, box = ops.instance_masks(logits, sel.to(torch.int32).to(dev), up, crop, out)
    _check_masks(f'{name} instance_masks', masks, sel, ref)
    _check_scores_boxes(f'{name} instance_masks', score, box, sel, ref)
    full = ref.count[PC.FULL].item() == out[0] * out[1]
    assert full and box[sel.tolist().index(PC.FULL)].tolist() == [0, 0, out[1], out[0]]
    # the copied query and the repeated index compute the same bits
    m = masks.cpu()
    s = sel.tolist()
    assert torch.equal(m[s.index(PC.COPY)], m[s.index(PC.COPY_OF)]) and torch.equal(m[2], m[3])

    lists = [sel[:4], sel[4:], sel[:0], torch.tensor([PC.CORNER, 5, 5, PC.EMPTY])]
    masks_l, qscore, qbox = ops.instance_masks_multi(logits, [ix.to(dev) for ix in lists], up, crop, out)
    for t, (ix, mt) in enumerate(zip(lists, masks_l)):
        assert mt.shape[0] == ix.numel()
        if ix.numel():
            _check_masks(f'{name} multi[{t}]', mt, ix, ref)
    picked = torch.cat(lists).unique()
    _check_scores_boxes(f'{name} multi', qscore[picked.to(dev)], qbox[picked.to(dev)], picked, ref)

    g = torch.Generator().manual_seed(7)
    qidx, cls = _picks_of(ref, g)
    pm, pb = ops.instance_masks_picks(logits, qidx.to(dev), cls.to(dev), up, crop, out)
    _check_picks(f'{name} picks', pm, pb, qidx, cls, ref)


def test_fast_path_and_generic_kernel_agree(dev):
    """the same logits at width 96 (integer fast path) and width 100 (generic kernel): equal masks on the shared columns"""
    a, b = PC.instance_case('fast_w96'), PC.instance_case('generic_w100')
    sel = torch.tensor(PC.SEL)
    got = []
    for name, ref in (('fast_w96', a), ('generic_w100', b)):
        hw, up, crop, out = PC.INSTANCE_GEOMS[name]
        got.append(ops.instance_masks(ref.logits.to(dev), sel.to(torch.int32).to(dev), up, crop, out)[0].cpu())
    inside = a.inside[sel]
    ma, mb = got[0], got[1][:, :, :96]
    assert torch.equal(ma[~inside], mb[~inside]), f'{int(((ma != mb) & ~inside).sum())} pixels differ ({int(inside.sum())} excluded)'


@pytest.mark.parametrize('name', list(PC.PICKS_GEOMS))
def test_instance_masks_picks_plan(dev, name):
    """300 picks over 5 queries, one of them never picked: the plan kernel's strided loops and its rank among duplicates"""
    ref, qidx, cls = PC.picks_case(name)
    hw, up, crop, out = PC.PICKS_GEOMS[name]
    masks, bboxes = ops.instance_masks_picks(ref.logits.to(dev), qidx.to(dev), cls.to(dev), up, crop, out)
    _check_picks(name, masks, bboxes, qidx, cls, ref)


@pytest.mark.parametrize('name', list(PC.PICKS_GEOMS))
def test_instance_masks_picks_invalid_queries(dev, name):
    """picks with qidx = -1 and qidx = Q: their bboxes rows are zero and every other row is what it is without them"""
    ref, qidx, cls = PC.picks_case(name)
    hw, up, crop, out = PC.PICKS_GEOMS[name]
    qidx, cls = qidx[:40].clone(), cls[:40].clone()
    bad = torch.tensor([0, 17, 18, 39])
    valid = torch.ones(40, dtype=torch.bool)
    valid[bad] = False
    logits = ref.logits.to(dev)
    qbad = qidx.clone()
    qbad[bad] = torch.tensor([-1, PC.PICKS_Q, -1, PC.PICKS_Q])
    masks, bboxes = ops.instance_masks_picks(logits, qbad.to(dev), cls.to(dev), up, crop, out)
    masks, bboxes = masks.cpu(), bboxes.cpu()
    assert bool((bboxes[bad] == 0).all()), bboxes[bad].tolist()
    _check_picks(name, masks[valid], bboxes[valid], qidx[valid], cls[valid], ref)
    m0, b0 = ops.instance_masks_picks(logits, qidx[valid].to(dev), cls[valid].to(dev), up, crop, out)
    assert torch.equal(masks[valid], m0.cpu()) and torch.equal(bboxes[valid], b0.cpu())


@pytest.mark.parametrize('name', PC.FAST_GEOMS)
def test_instance_masks_bitpacked_match_the_rule(dev, name):
    ref = PC.instance_case(name)
    hw, up, crop, out = PC.INSTANCE_GEOMS[name]
    assert ops.instance_masks_bitpack_ok(hw, up, crop, out)
    g = torch.Generator().manual_seed(8)
    qidx, cls = _picks_of(ref, g)
    packed, bboxes = ops.instance_masks_picks(ref.logits.to(dev), qidx.to(dev), cls.to(dev), up, crop, out, bitpack=True)
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (qidx.numel(), out[0], out[1] // 8)
    masks = torch.from_numpy(np.unpackbits(packed.cpu().numpy(), axis=-1, bitorder='little')).bool()
    _check_picks(f'{name} bitpack', masks, bboxes, qidx, cls, ref)


@pytest.mark.parametrize('name', [n for n in PC.INSTANCE_GEOMS if n not in PC.FAST_GEOMS])
def test_bitpack_is_refused_off_the_fast_path(dev, name):
    ref = PC.instance_case(name)
    hw, up, crop, out = PC.INSTANCE_GEOMS[name]
    assert not ops.instance_masks_bitpack_ok(hw, up, crop, out)
    qidx, cls = _picks_of(ref, torch.Generator().manual_seed(9))
    with pytest.raises(ops.CggError):
        ops.instance_masks_picks(ref.logits.to(dev), qidx.to(dev), cls.to(dev), up, crop, out, bitpack=True)


# ------------------------------------------------------------------------------------------------ B. panoptic
@pytest.mark.parametrize('name', list(PC.PANOPTIC_CASES))
def test_panoptic_argmax_matches_the_rule(dev, name):
    ref = PC.panoptic_case(name)
    ids, half, counts = ops.panoptic_argmax(ref.logits.to(dev), ref.keep.to(dev), ref.score.to(dev), ref.up, ref.crop, ref.out)
    ids, half, counts = ids.cpu().long(), half.cpu().bool(), counts.cpu().long()
    assert tuple(ids.shape) == tuple(ref.out) and bool(((ids >= 0) & (ids < ref.n)).all())
    ex_i, ex_h = ref.ids_excluded, ref.half_excluded
    assert torch.equal(ids[~ex_i], ref.ids[~ex_i]), \
        f'{name}: {int(((ids != ref.ids) & ~ex_i).sum())} ids differ from the rule ({int(ex_i.sum())} of {ex_i.numel()} excluded)'
    assert torch.equal(half[~ex_h], ref.win_half[~ex_h]), \
        f'{name}: {int(((half != ref.win_half) & ~ex_h).sum())} win_half differ from the rule ({int(ex_h.sum())} excluded)'
    diff = (counts - ref.counts).abs()
    assert bool((diff <= ref.slack).all()), f'{name}: counts off by {diff.tolist()} where {ref.slack.tolist()} pixels are excluded'
    # the counts are those of the kernel's own maps
    onehot = torch.nn.functional.one_hot(ids, ref.n).permute(2, 0, 1).bool()
    assert torch.equal(counts[:, 0], onehot.flatten(1).sum(1)) and torch.equal(counts[:, 2], (onehot & half).flatten(1).sum(1))
    if name == 'n7_twins':                                  # equal values: the first maximum, exactly, with no band
        assert int((ids == 5).sum()) == 0 and int((ids == 3).sum()) >= int(((ref.ids == 3) & ~ex_i).sum()) > 0
    print(f'{name}: {int(ex_i.sum())} + {int(ex_h.sum())} pixels excluded, largest count difference {int(diff.max())}')


def test_panoptic_paint_exact(dev):
    ids, win_half, lut_val, lut_half, void, want = PC.paint_case()
    got = ops.panoptic_paint(ids.to(dev), win_half.to(dev), lut_val.to(dev), lut_half.to(dev), void)
    assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------------------ C. softmax, class_topk
@pytest.mark.parametrize('rows', PC.SOFTMAX_ROWS)
def test_rowwise_softmax_argmax_vs_float64(dev, rows):
    worst = 0.0
    for n in PC.SOFTMAX_N:
        x, ties = PC.softmax_rows(rows, n)
        p64, bound = PC.softmax_ref(x)
        prob, maxv, arg = ops.rowwise_softmax_argmax(x.to(dev))
        prob, maxv, arg = prob.cpu().double(), maxv.cpu().double(), arg.cpu()
        ratio = ((prob - p64).abs() / bound).max().item()
        top, first = p64.max(1)
        rmax = ((maxv - top).abs() / bound.gather(1, first[:, None])[:, 0]).max().item()
        worst = max(worst, ratio, rmax)
        assert ratio <= 1.0, f'rows {rows} n {n}: prob at {ratio:.3g} of the bound'
        assert rmax <= 1.0, f'rows {rows} n {n}: maxv at {rmax:.3g} of the bound'
        assert torch.equal(arg, x.double().argmax(1)), f'rows {rows} n {n}: argmax {arg.tolist()}'      # first maximum of the row
        for r, a in ties.items():
            assert arg[r].item() == a, f'rows {rows} n {n}: tie in row {r} -> {arg[r].item()}, first index {a}'
        _, maxv2, arg2 = ops.rowwise_softmax_argmax(x.to(dev), want_prob=False)
        assert torch.equal(maxv2.cpu().double(), maxv) and torch.equal(arg2.cpu(), arg)
    print(f'rows {rows}: softmax at {worst:.3f} of the bound')


def test_rowwise_softmax_argmax_nan_row(dev):
    """a row of nothing but NaN returns an argmax inside the row, and the rows of its workgroup are unaffected"""
    n = 65
    x, _ = PC.softmax_rows(6, n)
    clean = ops.rowwise_softmax_argmax(x.to(dev))
    xn = x.clone()
    xn[1] = float('nan')
    xn[5] = float('nan')
    prob, maxv, arg = ops.rowwise_softmax_argmax(xn.to(dev))
    arg = arg.cpu()
    assert bool(((arg >= 0) & (arg < n)).all()), arg.tolist()
    assert bool(torch.isnan(prob[1]).all()) and bool(torch.isnan(prob[5]).all()) and bool(torch.isnan(maxv[[1, 5]]).all())
    keep = [0, 2, 3, 4]
    assert torch.equal(prob[keep], clean[0][keep]) and torch.equal(maxv[keep], clean[1][keep]) and torch.equal(arg[keep], clean[2].cpu()[keep])
    assert torch.equal(arg[keep], x.double().argmax(1)[keep])


@pytest.mark.parametrize('name', list(PC.TOPK_CASES))
def test_class_topk_vs_float64(dev, name):
    B, Q, ld, col0, ncols, k, _ = PC.TOPK_CASES[name]
    dots = PC.topk_dots(name)
    assert ops.class_topk_supported(Q, ncols, k)
    labels, scores, qidx = ops.class_topk(dots.to(dev), B, col0, ncols, k)
    labels, scores, qidx = labels.cpu(), scores.cpu(), qidx.cpu()
    assert tuple(labels.shape) == tuple(scores.shape) == tuple(qidx.shape) == (B, len(col0), k)
    worst = 0.0
    for b in range(B):
        for t, (c0, nc) in enumerate(zip(col0, ncols)):
            p64, bound = PC.topk_ref(dots, b, Q, c0, nc)
            worst = max(worst, PC.check_topk(labels[b, t], scores[b, t], qidx[b, t], p64, bound, Q, nc, k))
    print(f'{name}: scores at {worst:.3f} of the bound')


def test_class_topk_cuts_a_tie_group_at_the_lowest_indices(dev):
    """8 identical rows: k ends inside a group of 8 bitwise-equal probabilities, which yields its lowest flat indices"""
    dots = PC.tie_dots()
    Q, nc, k = PC.TIE_Q, PC.TIE_NC, PC.TIE_K
    labels, scores, qidx = ops.class_topk(dots.to(dev), 1, [0], [nc], k)
    labels, scores, qidx = labels.cpu()[0, 0], scores.cpu()[0, 0], qidx.cpu()[0, 0]
    p64, bound = PC.topk_ref(dots, 0, Q, 0, nc)
    PC.check_topk(labels, scores, qidx, p64, bound, Q, nc, k)
    want = p64.sort(descending=True, stable=True).indices[:k]
    assert torch.equal(qidx * (nc - 1) + labels, want), f'{(qidx * (nc - 1) + labels).tolist()} != {want.tolist()}'
    assert scores[k - 1] == scores[k - 3] and scores.unique().numel() == 3            # the groups are bitwise equal


# ------------------------------------------------------------------------------------------------ D. upsample_bilinear
@pytest.mark.parametrize('hw,size', PC.UPSAMPLE_CASES)
def test_upsample_bilinear_vs_rule(dev, hw, size):
    x, want, bound = PC.upsample_case(hw, size)
    got = ops.upsample_bilinear(x.to(dev), size).cpu().double()
    assert tuple(got.shape) == (3,) + tuple(size)
    ratio = ((got - want).abs() / bound).max().item()
    print(f'{hw} -> {size}: at {ratio:.3f} of the band')
    assert ratio <= 1.0
