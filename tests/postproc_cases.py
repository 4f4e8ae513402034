"""Inputs and references for the inference-tail kernels of csrc/postproc.hip. Plain numpy / torch on the CPU: no GPU, no project kernel.

The resize reference ("the rule") restates torch's upsample_bilinear2d(align_corners=False): the source coordinate and the taps in
float32, exactly as torch and the kernels form them, and the four-sample blend in float64. A float64 F.interpolate is no reference
for a scale that is not a power of two: its coordinates differ from the float32 ones by about 1e-6, which moves values by about 2e-5.

Outputs that come from a threshold (masks, boxes, ids, win_half) are compared exactly, outside an exclusion band that is a condition
on the inputs and not a tolerance on the kernel: a pixel whose reference value lies within the band of the threshold is left out.
The band of a pixel (`band`) has two terms per resize stage (two stages when out != crop):

  blend        8 * 2^-24 * max |plane|: the f32 blend is 4 products and 3 sums of values no larger than max |plane|, with weights
               that carry one rounding each (1 - l1).
  coordinate   2^-22 * max(H, W, crop_h, crop_w) * |plane[i] - plane[neighbour]| (horizontal and vertical neighbours): one ulp of
               the source coordinate per axis, which is what contracting scale * (o + 0.5) - 0.5 into one fma can move it by; the
               value is continuous and piecewise linear in the coordinate, with slope at most the neighbour difference. Absent for a
               stage that resizes both axes by a power of two: those coordinates are exact in float32.

The blend maximum is taken per plane, since a pixel of plane q depends on plane q alone, and the neighbour difference locally, over the
pairs around the pixel's taps (`local_diff`); the second stage carries the first stage's band at its taps along."""
import functools

import numpy as np
import torch

U = 2.0 ** -24                  # one f32 rounding
BLEND_ROUNDINGS = 8
SHARE_CAP = 1e-3                # largest share of pixels that a case may exclude


# ------------------------------------------------------------------------------------------------ the rule
def taps(n_in, n_out):
    """(i0, i1 int64 tensors, l1 float64 tensor) of every output index; the arithmetic up to l1 is float32"""
    scale = np.float32(n_in) / np.float32(n_out)
    o = np.arange(n_out, dtype=np.float32)
    src = np.maximum(scale * (o + np.float32(0.5)) - np.float32(0.5), np.float32(0.0))
    assert src.dtype == np.float32
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(np.float32)
    assert l1.dtype == np.float32
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l1.astype(np.float64))


def resize_rule(x, size):
    """x (..., H, W) -> (..., h, w) float64"""
    x = x.double()
    H, W = x.shape[-2:]
    y0, y1, ly = taps(H, int(size[0]))
    x0, x1, lx = taps(W, int(size[1]))
    ly = ly[:, None]

    def row(r):
        return (1.0 - lx) * r[..., x0] + lx * r[..., x1]

    return (1.0 - ly) * row(x[..., y0, :]) + ly * row(x[..., y1, :])


def resized(logits, up, crop, out):
    """the rule to `up`, the crop, then the rule again to `out` if out != crop; float64"""
    v = resize_rule(logits, up)[..., :crop[0], :crop[1]]
    if tuple(out) != tuple(crop):
        v = resize_rule(v, out)
    return v


def torch_f32_resized(logits, up, crop, out):
    """the same chain by torch's own f32 operator"""
    F = torch.nn.functional
    x = logits.float().reshape((-1, 1) + tuple(logits.shape[-2:]))
    v = F.interpolate(x, tuple(up), mode='bilinear', align_corners=False)[..., :crop[0], :crop[1]]
    if tuple(out) != tuple(crop):
        v = F.interpolate(v, tuple(out), mode='bilinear', align_corners=False)
    return v.reshape(tuple(logits.shape[:-2]) + tuple(out))


def _pow2_ratio(a, b):
    lo, hi = min(a, b), max(a, b)
    return hi % lo == 0 and ((hi // lo) & (hi // lo - 1)) == 0


def exact_coordinates(hw, up, crop, out):
    ok = _pow2_ratio(hw[0], up[0]) and _pow2_ratio(hw[1], up[1])
    if tuple(out) != tuple(crop):
        ok = ok and _pow2_ratio(crop[0], out[0]) and _pow2_ratio(crop[1], out[1])
    return ok


def _pool3(m):
    """3 x 3 running maximum of every plane of m (Q, H, W), borders clamped"""
    return torch.nn.functional.max_pool2d(m[:, None], 3, 1, 1)[:, 0]


def local_diff(p):
    """(Q, H, W): for every element, the largest |difference| of a horizontally or vertically adjacent pair that touches it or one
    of its eight neighbours. It bounds the slope of the interpolant in every cell next to the element, so a coordinate that an ulp
    carries across a cell border is covered."""
    m = torch.zeros_like(p)
    if p.shape[-1] > 1:
        d = (p[..., :, 1:] - p[..., :, :-1]).abs()
        m[..., :, 1:] = torch.maximum(m[..., :, 1:], d)
        m[..., :, :-1] = torch.maximum(m[..., :, :-1], d)
    if p.shape[-2] > 1:
        d = (p[..., 1:, :] - p[..., :-1, :]).abs()
        m[..., 1:, :] = torch.maximum(m[..., 1:, :], d)
        m[..., :-1, :] = torch.maximum(m[..., :-1, :], d)
    return _pool3(m)


def _at_taps(m, y0, y1, x0, x1):
    """the larger of m at the two diagonal taps of every output pixel (m is already a 3 x 3 maximum)"""
    return torch.maximum(m[:, y0][:, :, x0], m[:, y1][:, :, x1])


def _stage_band(p, err_in, size, n_coord):
    """per-pixel band (Q, h, w) of one resize of the planes p (Q, H, W) float64, whose elements carry the error err_in already"""
    H, W = p.shape[-2:]
    y0, y1, _ = taps(H, int(size[0]))
    x0, x1, _ = taps(W, int(size[1]))
    e = (BLEND_ROUNDINGS * U * p.abs().flatten(1).max(1).values)[:, None, None].expand(-1, int(size[0]), int(size[1])).clone()
    if not (_pow2_ratio(H, size[0]) and _pow2_ratio(W, size[1])):
        e = e + 2.0 ** -22 * n_coord * _at_taps(local_diff(p), y0, y1, x0, x1)
    if err_in is not None:
        e = e + _at_taps(_pool3(err_in), y0, y1, x0, x1)
    return e


def band(planes, up, crop, out):
    """(Q, oh, ow) float64: the exclusion band of every output pixel of `planes` (Q, H, W) for this geometry. Per stage: the blend
    term of the plane plus, where the stage's coordinates are inexact, 2^-22 * max(H, W, crop_h, crop_w) * the local neighbour
    difference at the pixel's taps; the second stage adds the first stage's band at its own taps."""
    p = planes.double()
    H, W = p.shape[-2:]
    n_coord = max(H, W, crop[0], crop[1])
    e = _stage_band(p, None, up, n_coord)[:, :crop[0], :crop[1]]
    if tuple(out) != tuple(crop):
        e = _stage_band(resize_rule(p, up)[:, :crop[0], :crop[1]], e, out, n_coord)
    return e


# ------------------------------------------------------------------------------------------------ A. instance masks
Q_RANDOM = 12
EMPTY, FULL, CORNER, COPY = 12, 13, 14, 15       # the planted queries
COPY_OF = 3
SEL = (3, 0, 7, 7, 11, 2, EMPTY, FULL, CORNER, COPY)

# name: (low-res (H, W), up, crop, out)
INSTANCE_GEOMS = {
    'generic_noninteger':   ((13, 19), (50, 70), (50, 70), (50, 70)),          # npix = 3500, not a multiple of 16
    'scale4_cropped_w70':   ((13, 19), (52, 76), (47, 70), (47, 70)),          # integer scale, out_w % 16 != 0 -> generic kernel
    'two_stage_up':         ((16, 24), (64, 96), (60, 90), (75, 110)),
    'two_stage_down':       ((16, 24), (64, 96), (60, 90), (41, 63)),
    'scale3':               ((24, 20), (72, 60), (72, 60), (72, 60)),
    'fast_w96':             ((25, 42), (100, 168), (97, 96), (97, 96)),        # the same logits on the fast path ...
    'generic_w100':         ((25, 42), (100, 168), (97, 100), (97, 100)),      # ... and on the generic kernel
    'clamp_4x4_s2':         ((4, 4), (8, 8), (8, 8), (8, 8)),                  # out_w = 8: the generic kernel
    'clamp_4x4_s4':         ((4, 4), (16, 16), (16, 16), (16, 16)),            # fast path, both column clamps in one thread
    'clamp_4x4_s8':         ((4, 4), (32, 32), (32, 32), (32, 32)),
    'row_1x8_s2':           ((1, 8), (2, 16), (2, 16), (2, 16)),               # H == 1: rm == m == rp
    'row_1x8_s4':           ((1, 8), (4, 32), (4, 32), (4, 32)),
    'row_1x8_s8':           ((1, 8), (8, 64), (8, 64), (8, 64)),
    'fast_many_tiles':      ((40, 40), (160, 160), (150, 160), (150, 160)),    # 380 tiles per detection, out_h % S != 0
    'down_32_to_16':        ((32, 32), (16, 16), (16, 16), (16, 16)),          # target smaller than the logits
    'down_20x28_to_13x9':   ((20, 28), (13, 9), (13, 9), (13, 9)),
}
# the geometries that reach the integer fast path (bit-packed output is possible on these alone)
FAST_GEOMS = ('fast_w96', 'clamp_4x4_s4', 'clamp_4x4_s8', 'row_1x8_s2', 'row_1x8_s4', 'row_1x8_s8', 'fast_many_tiles')
_SEEDS = {'fast_w96': 143, 'generic_w100': 143}       # the pair shares its logits


def _seed(name):
    return _SEEDS.get(name, 100 + sorted(INSTANCE_GEOMS).index(name))


def instance_logits(H, W, seed, q_random=Q_RANDOM, planted=True):
    """(q_random [+ 4], H, W) f32: randn * 3 and the planted queries"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(q_random, H, W, generator=g) * 3
    if not planted:
        return x
    empty = -(torch.randn(1, H, W, generator=g).abs() * 3 + 0.1)           # all negative: empty mask
    full = torch.randn(1, H, W, generator=g).abs() * 3 + 0.1               # all positive: full mask
    corner = -(torch.rand(1, H, W, generator=g) + 1.0)                     # negative but for the low-res bottom-right element
    corner[0, H - 1, W - 1] = 40.0
    return torch.cat([x, empty, full, corner, x[COPY_OF:COPY_OF + 1].clone()])


class MaskRef:
    """of every plane of `logits` for one geometry: v (Q, oh, ow) float64 by the rule, band (Q, oh, ow), inside (Q, oh, ow) bool
    (|v| <= band), mask = v > 0, count, n_inside (Q,), score (Q,) float64, box (Q, 4) f32 (mmdet's mask2bbox)"""

    def __init__(self, logits, up, crop, out):
        from oracle.head import mask2bbox
        self.logits, self.up, self.crop, self.out = logits, tuple(up), tuple(crop), tuple(out)
        self.v = resized(logits, up, crop, out)
        self.band = band(logits, up, crop, out)
        self.inside = self.v.abs() <= self.band
        self.mask = self.v > 0
        self.count = self.mask.flatten(1).sum(1)
        self.n_inside = self.inside.flatten(1).sum(1)
        self.score = (torch.sigmoid(self.v) * self.mask).flatten(1).sum(1) / (self.count.double() + 1e-6)
        self.box = mask2bbox(self.mask)
        self.score_bound = 1e-5 + self.n_inside.double() / self.count.clamp(min=1).double()

    @property
    def share(self):
        return self.inside.double().mean().item()


@functools.lru_cache(maxsize=None)
def instance_case(name):
    hw, up, crop, out = INSTANCE_GEOMS[name]
    return MaskRef(instance_logits(hw[0], hw[1], _seed(name)), up, crop, out)


def bitpack_expected(name):
    """what ops.instance_masks_bitpack_ok must say"""
    return name in FAST_GEOMS


# the picks of the plan kernel's case: 300 picks over 5 queries, query 3 never picked
PICKS_Q, PICKS_N, PICKS_UNPICKED = 5, 300, 3
PICKS_GEOMS = {'picks_generic': ((13, 19), (52, 76), (47, 70), (47, 70)), 'picks_fast': ((16, 24), (64, 96), (64, 96), (64, 96))}


@functools.lru_cache(maxsize=None)
def picks_case(name):
    """(MaskRef over 5 planes, qidx (300,) int64, cls_scores (300,) f32)"""
    hw, up, crop, out = PICKS_GEOMS[name]
    g = torch.Generator().manual_seed(170)
    ref = MaskRef(instance_logits(hw[0], hw[1], 171, q_random=PICKS_Q, planted=False), up, crop, out)
    qidx = torch.tensor([0, 1, 2, 4])[torch.randint(0, 4, (PICKS_N,), generator=g)]
    return ref, qidx, torch.rand(PICKS_N, generator=g)


# ------------------------------------------------------------------------------------------------ B. panoptic
PAN_Q = 50
PAN_GEOM = ((13, 19), (52, 76), (47, 70), (59, 81))       # two-stage, 4779 pixels
PAN_GEOM_1024 = ((8, 8), (16, 16), (16, 16), (16, 16))
# name: (geometry, n, seed, duplicate pair)
PANOPTIC_CASES = {
    'n1':         (PAN_GEOM, 1, 201, False),
    'n7':         (PAN_GEOM, 7, 202, False),
    'n7_twins':   (PAN_GEOM, 7, 203, True),               # keep[3] == keep[5] with equal scores
    'n40':        (PAN_GEOM, 40, 204, False),
    'n1024':      (PAN_GEOM_1024, 1024, 205, False),
}


class PanopticRef:
    """logits (Q, H, W) f32, keep (n,) int32, score (n,) f32 and, by the rule in float64: ids (first argmax of score * sigmoid(v)),
    win_half (v of the winner >= 0), counts (n, 3); ids_excluded / half_excluded (oh, ow) bool; slack (n, 3): how far each count
    may differ, the excluded pixels that involve k"""

    def __init__(self, geom, n, seed, twins):
        hw, self.up, self.crop, self.out = geom
        g = torch.Generator().manual_seed(seed)
        self.logits = torch.randn(PAN_Q, hw[0], hw[1], generator=g) * 3
        if n <= PAN_Q:
            keep = torch.randperm(PAN_Q, generator=g)[:n]
        else:
            keep = torch.randint(0, PAN_Q, (n,), generator=g)
        score = torch.rand(n, generator=g) * 0.7 + 0.3
        if twins:
            keep[5], score[5] = keep[3], score[3]
        self.keep, self.score, self.n = keep.to(torch.int32), score, n
        v = resized(self.logits[keep], self.up, self.crop, self.out)                # (n, oh, ow)
        bnd = band(self.logits[keep], self.up, self.crop, self.out)                 # (n, oh, ow)
        pv = score.double()[:, None, None] * torch.sigmoid(v)
        # an entry that repeats an earlier one (same plane, same score) computes the same bits and never wins: first maximum
        self.shadowed = torch.zeros(n, dtype=torch.bool)
        seen = {}
        for k in range(n):
            key = (int(keep[k]), float(score[k]))
            self.shadowed[k] = key in seen
            seen.setdefault(key, k)
        pv_live = pv.clone()
        pv_live[self.shadowed] = -1.0
        self.ids = pv_live.argmax(0)
        onehot = torch.nn.functional.one_hot(self.ids, n).permute(2, 0, 1).bool()
        pick = lambda t: t.gather(0, self.ids[None])[0]                             # noqa: E731  the winner's entry of t (n, oh, ow)
        # sigmoid's slope is at most 1/4; 2^-22 covers the rounding of sigmoid and of the product. The band is the pixel's own:
        # the larger of the two planes compared
        self.gap_thr = 0.25 * score.max().item() * torch.maximum(bnd, pick(bnd)[None]) + 2.0 ** -22
        contender = (pick(pv_live)[None] - pv_live < self.gap_thr) & ~onehot & ~self.shadowed[:, None, None]
        self.ids_excluded = contender.any(0)
        self.win_half = pick(v) >= 0
        near_half = v.abs() <= bnd                                                  # (n, oh, ow): v_k >= 0 undecided
        self.half_excluded = pick(near_half) | self.ids_excluded
        half = v >= 0
        self.counts = torch.stack([onehot.flatten(1).sum(1), half.flatten(1).sum(1), (onehot & half).flatten(1).sum(1)], 1)
        involved = contender | (onehot & self.ids_excluded)                         # k may win an excluded pixel, or lose it
        s0 = involved.flatten(1).sum(1)
        s1 = near_half.flatten(1).sum(1)
        s2 = (involved | (near_half & onehot)).flatten(1).sum(1)
        self.slack = torch.stack([s0, s1, s2], 1)
        self.band = bnd

    @property
    def share(self):
        return (self.ids_excluded | self.half_excluded).double().mean().item()


@functools.lru_cache(maxsize=None)
def panoptic_case(name):
    return PanopticRef(*PANOPTIC_CASES[name])


def paint_case(seed=210, npix=1000, n=9, void=255):
    """random ids / win_half / look-up tables with a negative value and a lut_half entry; -> inputs and the expected map"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, n, (npix,), generator=g).to(torch.int32)
    win_half = (torch.rand(npix, generator=g) < 0.5).to(torch.uint8)
    lut_val = torch.randint(0, 2000, (n,), generator=g).to(torch.int32)
    lut_half = torch.zeros(n, dtype=torch.int32)
    lut_val[2], lut_val[6] = -1, 0
    lut_half[4], lut_half[2], lut_half[7] = 1, 1, 3
    k = ids.long()
    want = torch.where((lut_val[k] >= 0) & ((lut_half[k] == 0) | (win_half != 0)), lut_val[k], torch.full_like(ids, void))
    return ids, win_half, lut_val, lut_half, void, want


# ------------------------------------------------------------------------------------------------ C. softmax, class_topk
SOFTMAX_ROWS = (1, 5, 37)
SOFTMAX_N = (1, 63, 64, 65, 257, 300)
ROW_KINDS = ('plain', 'plus80', 'minus80', 'times5', 'neg_inf')


def softmax_rows(rows, n, seed=300):
    """x (rows, n) f32: row r is of kind ROW_KINDS[r % 5]; exact ties at the row maximum are planted in row 0 (two lanes) and, when
    there is more than one row and n >= 65, in the last row (one lane: i and i + 64). -> (x, {row: first index of the tie})"""
    g = torch.Generator().manual_seed(seed + 1000 * rows + n)
    x = torch.randn(rows, n, generator=g) * 6
    for r in range(rows):
        kind = ROW_KINDS[r % len(ROW_KINDS)]
        if kind == 'plus80':
            x[r] += 80
        elif kind == 'minus80':
            x[r] -= 80
        elif kind == 'times5':
            x[r] *= 5
        elif kind == 'neg_inf':
            x[r, 1::3] = float('-inf')
    ties = {}
    if n >= 2:
        a, b = n // 3, n - 1
        x[0, a] = x[0, b] = x[0].max() + 1
        ties[0] = a
    if rows > 1 and n >= 65:
        a, b = n - 65, n - 1
        top = x[rows - 1][torch.isfinite(x[rows - 1])].max() + 1
        x[rows - 1, a] = x[rows - 1, b] = top
        ties[rows - 1] = a
    return x, ties


def softmax_ref(x):
    """(p64, bound): float64 softmax of the f32 values and |p - p64| <= 2^-23 * (8 + (max - x)) * p64 + 1e-30. The argument x - max
    carries half an ulp of |x - max|; expf, the tree sum and the reciprocal account for the 8."""
    x = x.double()
    m = x.max(-1, keepdim=True).values
    p = torch.softmax(x, -1)
    d = torch.where(torch.isfinite(x), m - x, torch.zeros_like(x))              # -inf entries: p64 = 0, the bound is 1e-30
    return p, 2.0 ** -23 * (8.0 + d) * p + 1e-30


# name: (B, Q, ld, col0, ncols, k, seed)
TOPK_CASES = {
    'three_types':  (2, 100, 134, [0, 66, 84], [66, 18, 50], 100, 401),
    'wide_300':     (1, 40, 300, [0], [300], 64, 402),                  # the nc > 256 branch
    'k1':           (2, 17, 30, [0], [30], 1, 403),
    'k_all':        (1, 10, 12, [0], [12], 110, 404),                   # k == Q * (nc - 1)
    'k1024':        (1, 100, 66, [0], [66], 1024, 405),
    'window':       (2, 23, 100, [7, 40], [20, 33], 50, 406),           # col0 > 0, ld > sum(ncols)
}
TIE_Q, TIE_NC, TIE_K = 8, 10, 8 * 2 + 3                                 # k cuts the third group of 8 equal probabilities


def topk_dots(name):
    B, Q, ld, col0, ncols, k, seed = TOPK_CASES[name]
    g = torch.Generator().manual_seed(seed)
    dots = torch.randn(B * Q, ld, generator=g) * 3
    if name == 'window':                                                # columns outside every window must not matter
        own = torch.zeros(ld, dtype=torch.bool)
        for c0, nc in zip(col0, ncols):
            own[c0:c0 + nc] = True
        dots[:, ~own] = 1e4
    return dots


def tie_dots(seed=407):
    """8 identical rows: every probability occurs 8 times, bitwise"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, TIE_NC, generator=g) * 3).repeat(TIE_Q, 1).contiguous()


def topk_ref(dots, b, Q, c0, nc):
    """(p64 flat (Q * (nc - 1),), bound flat) of image b, one type"""
    p, bound = softmax_ref(dots[b * Q:(b + 1) * Q, c0:c0 + nc])
    return p[:, :-1].reshape(-1), bound[:, :-1].reshape(-1)


def check_topk(labels, scores, qidx, p64, bound, Q, nc, k):
    """the properties of one (image, type) result against float64; returns the worst score error / bound"""
    n = nc - 1
    labels, qidx, scores = labels.long(), qidx.long(), scores.double()
    assert labels.shape == qidx.shape == scores.shape == (k,)
    assert bool(((labels >= 0) & (labels < n) & (qidx >= 0) & (qidx < Q)).all()), 'pair out of range'
    flat = qidx * n + labels
    assert flat.unique().numel() == k, 'a pair was returned twice'
    err = (scores - p64[flat]).abs() / bound[flat]
    assert bool((err <= 1.0).all()), f'score off by {err.max().item():.3g} of the bound'
    ds, df = scores[1:] - scores[:-1], flat[1:] - flat[:-1]
    assert bool((ds <= 0).all()), 'scores increase'
    assert bool((df[ds == 0] > 0).all()), 'equal scores out of flat-index order'
    left = torch.ones(Q * n, dtype=torch.bool)
    left[flat] = False
    over = p64[left] - bound[left] - scores.min()
    assert not bool((over > 0).any()), f'a pair left out beats the smallest returned score by {over.max().item():.3g} more than its bound'
    return err.max().item()


# ------------------------------------------------------------------------------------------------ D. upsample_bilinear
UPSAMPLE_CASES = (((20, 28), (50, 97)), ((20, 28), (13, 9)), ((1, 8), (4, 32)), ((8, 1), (32, 4)))


def upsample_case(hw, size, seed=500):
    """(x (3, H, W) f32, want (3, h, w) float64 by the rule, bound (3, h, w))"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(3, hw[0], hw[1], generator=g) * 3
    return x, resize_rule(x, size), band(x, size, size, size)
