"""The reference's training pipeline (large-scale jitter), from raw uint8 images and instance masks to `forward_train`'s arguments.

Every reference training config runs the same [3P] mmdet steps in front of the model (configs/instance/coco_b48n17.py:195-218):

    LoadImageFromFile(to_float32=True) | Load*Annotations | RandomFlip(0.5) |
    Resize(img_scale=(1024, 1024), ratio_range=(0.1, 2.0), multiscale_mode='range', keep_ratio=True) |
    RandomCrop(crop_size=(1024, 1024), crop_type='absolute', recompute_bbox=True, allow_negative_crop=True) |
    FilterAnnotations(min_gt_bbox_wh=(1e-5, 1e-5), by_mask=True) | Pad(size=(1024, 1024), pad_val=dict(img=..., masks=0, seg=255)) |
    Normalize(to_rgb=True) | OpenFormatBundle | Collect

This module restates that chain as ONE gather per output pixel -- flip, resize and crop compose into index arithmetic, so the resized
image (2048^2 floats at ratio 2.0, three quarters of which the crop throws away) never exists:

    spec = parse_train_pipeline(cfg.data.train.pipeline)     # the steps as one small record (anything else raises)
    params = [draw_train_params(rng, s['img'].shape[:2], spec) for s in samples]   # the random decisions as explicit values
    kwargs, kept = prepare_train_host(samples, params, spec)  # numpy: the rule written down, and the host way to prepare
    kwargs, kept = TrainPrep(spec, device).prep(samples, params)   # csrc/train_prep.hip: one H2D copy + two launches per batch

THE RULE (`prepare_train_host` is its definition, the kernel equals it bit for bit). With (nh, nw) = image_prep.rescale_size(hw,
params.scale), (oy, ox) = params.crop_yx, (ch, cw) = spec.crop_size and (H, W) = spec.size, for an output pixel (y, x) of the H x W plane:

1. geometry: Y = y + oy, X = x + ox. The pixel is inside the image iff y < min(nh - oy, ch) and x < min(nw - ox, cw); that extent is
   `img_shape`. Outside it the image planes hold (pad_val - mean) * rstd (`image_prep.norm_constants` with pad_before_norm=True: a
   per-channel pad_val is in source channel order), masks hold 0 and the semantic map holds pad_val['seg'].
2. image: taps (i0, i1) and the fraction fx of `image_prep.resize_coefficients` (its rule 2, clamps at both ends included) for Y with
   h -> nh and for X with w -> nw. No 11-bit rounding here -- the image is float32 from the loader on -- the weights are the float32
   values 1 - fx and fx. Under `flip` source column c is read at w - 1 - c. Per source row r: R_r = f32(f32(p[r][i0] a0) + f32(p[r][i1]
   a1)); v = f32(f32(R_0 b0) + f32(R_1 b1)); then to_rgb and f32(f32(v - mean) rstd). Every product and sum is rounded on its own.
3. masks and the semantic map (nearest): source row min(floor(Y sy), h - 1) with sy = 1 / (nh / h) in double; columns likewise, then
   mirrored under `flip`. A mask pixel is set where the source is non-zero.
4. per instance, over the image extent: the area and bbox = (xmin, ymin, xmax + 1, ymax + 1) as float32. An instance is kept iff its
   area >= 1; kept instances keep their order, gt_labels is filtered alike. With recompute_bbox the boxes enclose their masks, so the
   [3P] box tests of RandomCrop (a box of positive width and height inside the window) and of FilterAnnotations (w, h > 1e-5,
   by_mask) hold exactly for the instances with one pixel or more: "area >= 1" is both tests.

This restates the [3P] steps (mmdet RandomFlip / Resize / RandomCrop / FilterAnnotations / Pad / Normalize over mmcv's imflip /
imrescale bilinear on float32 / nearest for masks) from their published behaviour. mmdet, mmcv and cv2 are not available offline,
so equality with a particular build is NOT claimed; what is pinned is this rule (tests/test_train_prep.py). Nor is equality claimed
with mmdet's use of the global `np.random` stream: the random decisions are drawn by `draw_train_params` in a documented order and
are an argument of the rule, so a caller may supply its own. PhotoMetricDistortion and multi-scale value lists are not restated and
are refused by name; so is poly2mask=False (polygon-form gt_masks through the pipeline). Polygons that the loader rasterises
(poly2mask=True, the reference's setting) are rule 6 below.

PANOPTIC SAMPLES. The panoptic configs start from `LoadOpenPanopticAnnotations(with_mask=True, with_seg=True)`, which turns the
panoptic PNG into one bitmap per thing and a semantic map on the host (open_set/datasets/pipelines/loading.py:317-341). A raw
panoptic sample carries the id map itself instead: `pan_seg`, (h, w) int32 ids >= 0 or (h, w, 3) uint8 in RGB order as the loader
reads the PNG (id = R + 256 G + 65536 B, `rgb2id`), `segments` = the `ann_info['masks']` records (dicts with id, category,
is_thing) and `gt_labels`, one per record with is_thing true. `load_panoptic_host` is the loader's rule:

5. the semantic map starts at 255 -- the loader's constant, not Pad's pad_val['seg'] -- and every record, crowd things (is_thing
   false) and stuff included, writes its category where pan == id; a pixel whose id no record lists stays 255. Every is_thing
   record yields the bitmap pan == id, in record order.

`prepare_train_host` of panoptic samples is DEFINED as `prepare_train_host` of the bitmap samples rule 5 makes. Rule 3 is a nearest
gather, which commutes with "compare the id": (pan[ry, rx] == id) is the resized bitmap and category_of(pan[ry, rx]) the resized
semantic map, so `TrainPrep` stages the id map (3 or 4 bytes per pixel, against 1 + n_things bytes for the planes) and a table of
the records, and one gather per output pixel yields every plane, bit for bit. With with_seg=False only the thing planes are made.

POLYGON SAMPLES. The instance configs start from `LoadOpenAnnotations(with_mask=True, poly2mask=True)`: the dataset hands over the raw
`segmentation` lists and the loader rasterises them on the host with pycocotools (`frPyObjects` -> `merge` -> `decode`,
open_set/datasets/pipelines/loading.py:105-129). A raw polygon sample carries the lists themselves: `gt_polygons`, a list over
instances of lists over parts of flat x0, y0, x1, y1, ... sequences (`ann_info['masks']`), and `gt_labels`, one per instance.
`polygon_mask_host(parts, h, w)` is the loader's rule, restated from the published maskApi.c (rleFrPoly):

6. per part with k vertices, in double precision, every product and sum rounded on its own (no fused multiply-add), (int) = C
   truncation: X[j] = (int)(5 x_j + 0.5), Y[j] likewise, vertex k = vertex 0. Edge j with dx = |X[j+1] - X[j]|, dy = |Y[j] - Y[j+1]|:
   flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye) swaps its ends; s = (ye - ys) / dx if dx >= dy else (xe - xs) / dy; its
   points are d = 0 .. max(dx, dy) with t = max - d under flip, else d: (u, v) = (t + xs, (int)(ys + s t + 0.5)), x and y exchanged when
   dx < dy; dx == dy == 0 gives the one point (xs, ys). All edges' points form one sequence. Every point i >= 1 with u[i] != u[i-1]
   is a crossing when xd = ((u[i] if u[i] < u[i-1] else u[i] - 1) + 0.5) / 5 - 0.5 is an integer in [0, w - 1]: with yd =
   ceil(clamp((min(v[i], v[i-1]) + 0.5) / 5 - 0.5, 0, h)) it lies at the COLUMN-MAJOR index a = xd h + yd (yd == h is legal: row 0 of
   the next column). Pixel p = x h + y is set iff the number of crossings <= p is odd -- ONE prefix parity over the whole plane,
   carried across columns (crossings per column are not always even in number). `_polygon_mask_literal` spells the same out as
   rleFrPoly does: sorted crossings, h w appended, differences, zero-length runs merged, runs alternating 0, 1. An instance is the OR
   of its parts (`merge`, intersect = 0); one without parts is empty and falls to "area >= 1".

pycocotools is not available offline, so equality with a particular build is NOT claimed; what is pinned is this rule
(tests/test_train_prep_polygons.py holds the two forms equal). `prepare_train_host` of polygon samples is DEFINED as
`prepare_train_host` of the bitmap samples rule 6 makes (`polygons_to_bitmap_sample`). `TrainPrep` stages the coordinates as float64
(a few hundred bytes per instance against h w) and three small tables; `cgg_train_prep_polygons_u8` rasterises every instance into a
column-major bit plane at source resolution (crossings as atomic XORs into a toggle plane, then a prefix XOR), and the plane kernel
of the bitmap route gathers from those bits: rule 3 and rule 4 are the same code. Refused by name: an RLE dict (a crowd; the
reference dataset sends those to bboxes_ignore), an odd coordinate count, an empty part, non-finite coordinates, |coordinate| >
CGG_IMAGE_PREP_MAX_DIM (it bounds the edge walk), gt_masks next to gt_polygons, a pipeline with with_seg.
"""
import functools
from dataclasses import dataclass
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import ops
from ._lib import CggError
from .image_prep import PrepSpec, _StagingRing, _as_hwc_u8, norm_constants, rescale_size
from .ops import (TRAIN_PREP_IMG_COLS, TRAIN_PREP_INST_COLS, TRAIN_PREP_MAX_SEGMENTS, TRAIN_PREP_PAN_COLS, TRAIN_PREP_POLY_INST_COLS,
                  TRAIN_PREP_POLY_PART_COLS, TRAIN_PREP_SEG_COLS, three_floats)

CAPTION_FIELDS = ('gt_caption_ids', 'gt_caption_mask', 'gt_caption_nouns_ids', 'gt_caption_nouns_mask')


@dataclass(frozen=True)
class TrainPrepSpec:
    """One reference training pipeline. `img_scale` is (w, h) as in the configs, `crop_size` and `size` (Pad) are (h, w); `pad_val`
    holds (img (3 floats, source channel order), masks, seg); mean / std in the channel order AFTER `to_rgb`."""
    img_scale: Tuple[int, int] = (1024, 1024)
    ratio_range: Tuple[float, float] = (0.1, 2.0)
    flip_ratio: float = 0.5
    crop_size: Tuple[int, int] = (1024, 1024)
    size: Tuple[int, int] = (1024, 1024)
    pad_val: Tuple[Tuple[float, float, float], int, int] = ((0.0, 0.0, 0.0), 0, 255)
    mean: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    std: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    to_rgb: bool = False
    with_seg: bool = False


class TrainParams(NamedTuple):
    """The random decisions of one sample: flip (bool), scale = the (w, h) box `rescale_size` fits the image into, crop_yx = (oy, ox)."""
    flip: bool
    scale: Tuple[int, int]
    crop_yx: Tuple[int, int]


_LOADERS = ('LoadImageFromFile',)
_ANNOTATIONS = ('LoadAnnotations', 'LoadOpenAnnotations', 'LoadPanopticAnnotations', 'LoadOpenPanopticAnnotations')
_PASSIVE = ('OpenFormatBundle', 'DefaultFormatBundle', 'Collect')
_ORDER = ('RandomFlip', 'Resize', 'RandomCrop', 'FilterAnnotations', 'Pad', 'Normalize')


def _unsupported(step, why):
    return CggError(f'train pipeline: {step}: {why} (train_prep restates LoadImageFromFile(to_float32) / RandomFlip(horizontal) / '
                    'Resize(ratio_range, keep_ratio) / RandomCrop(absolute, recompute_bbox) / FilterAnnotations(by_mask) / Pad(size) / '
                    'Normalize, in that order)')


def _pair(v, step, name):
    if not isinstance(v, (list, tuple)) or len(v) != 2:
        raise _unsupported(step, f'{name}={v!r}')
    return v[0], v[1]


def parse_train_pipeline(pipeline):
    """A reference-style `cfg.data.train.pipeline` (list of dicts with a `type`) -> TrainPrepSpec. Raises CggError naming the
    transform for anything this build does not restate."""
    if not isinstance(pipeline, (list, tuple)) or not pipeline:
        raise CggError('train pipeline: expected a non-empty list of transform dicts')
    kw, seen = {}, []
    for step in pipeline:
        t = step.get('type') if hasattr(step, 'get') else None
        if t in seen and t not in _PASSIVE:
            raise _unsupported(str(t), 'appears twice')
        if t in _ORDER and any(_ORDER.index(s) > _ORDER.index(t) for s in seen if s in _ORDER):
            later = next(s for s in seen if s in _ORDER and _ORDER.index(s) > _ORDER.index(t))
            raise _unsupported(t, f'follows {later}' + (' (Normalize before Pad)' if (t, later) == ('Pad', 'Normalize') else ''))
        seen.append(t)
        if t in _LOADERS:
            if not step.get('to_float32', False):
                raise _unsupported(t, 'to_float32 is missing or false (the 8-bit resize is the test pipeline\'s rule, image_prep.py)')
        elif t in _ANNOTATIONS:
            if step.get('poly2mask', True) is False:
                raise _unsupported(t, 'poly2mask=False (polygons are rasterised, rule 6: polygon-form gt_masks are out of scope)')
            if not step.get('with_mask', t != 'LoadAnnotations'):
                raise _unsupported(t, 'with_mask=False' + (' (the thing masks are what the panoptic rule yields)' if 'Panoptic' in t else ''))
            # the panoptic loaders' with_mask_based_bbox (either value) and with_seg=False are accepted: neither makes the result differ
            # from the rule -- the boxes are those of the cropped masks whatever boxes the loader made (recompute_bbox is required),
            # and without with_seg only the thing planes are produced
            kw['with_seg'] = bool(step.get('with_seg', 'Panoptic' in t))
        elif t == 'RandomFlip':
            if step.get('direction', 'horizontal') != 'horizontal':
                raise _unsupported(t, f'direction={step.get("direction")!r}')
            fr = step.get('flip_ratio')
            if fr is None or isinstance(fr, (list, tuple)) or not 0.0 <= float(fr) <= 1.0:
                raise _unsupported(t, f'flip_ratio={fr!r}')
            kw['flip_ratio'] = float(fr)
        elif t == 'Resize':
            if step.get('multiscale_mode', 'range') != 'range':
                raise _unsupported(t, f'multiscale_mode={step.get("multiscale_mode")!r} (multi-scale value lists are out of scope)')
            if not step.get('keep_ratio', True):
                raise _unsupported(t, 'keep_ratio=False')
            if step.get('interpolation', 'bilinear') != 'bilinear' or step.get('backend', 'cv2') != 'cv2':
                raise _unsupported(t, f'interpolation={step.get("interpolation")!r}, backend={step.get("backend")!r}')
            scale = step.get('img_scale')
            if isinstance(scale, (list, tuple)) and len(scale) == 1 and isinstance(scale[0], (list, tuple)):
                scale = scale[0]
            w, h = _pair(scale, t, 'img_scale')
            if isinstance(w, (list, tuple)) or min(w, h) < 1:
                raise _unsupported(t, f'img_scale={step.get("img_scale")!r} (multi-scale value lists are out of scope)')
            lo, hi = _pair(step.get('ratio_range'), t, 'ratio_range')
            if not 0.0 < float(lo) <= float(hi):
                raise _unsupported(t, f'ratio_range={step.get("ratio_range")!r}')
            kw['img_scale'], kw['ratio_range'] = (int(w), int(h)), (float(lo), float(hi))
        elif t == 'RandomCrop':
            if step.get('crop_type', 'absolute') != 'absolute':
                raise _unsupported(t, f'crop_type={step.get("crop_type")!r}')
            if not step.get('recompute_bbox', False):
                raise _unsupported(t, 'recompute_bbox=False (the boxes here are those of the cropped masks)')
            if not step.get('allow_negative_crop', False):
                raise _unsupported(t, 'allow_negative_crop=False')
            ch, cw = _pair(step.get('crop_size'), t, 'crop_size')
            if min(ch, cw) < 1:
                raise _unsupported(t, f'crop_size={step.get("crop_size")!r}')
            kw['crop_size'] = (int(ch), int(cw))
        elif t == 'FilterAnnotations':
            if not step.get('by_mask', False) or not step.get('by_box', True) or not step.get('keep_empty', True):
                raise _unsupported(t, 'by_mask=True, by_box=True, keep_empty=True expected')
            mw, mh = _pair(step.get('min_gt_bbox_wh', (1.0, 1.0)), t, 'min_gt_bbox_wh')
            if not (0.0 <= float(mw) < 1.0 and 0.0 <= float(mh) < 1.0 and step.get('min_gt_mask_area', 1) <= 1):
                raise _unsupported(t, 'thresholds other than "one pixel or more"')
        elif t == 'Pad':
            if step.get('pad_to_square', False) or step.get('size_divisor') is not None:
                raise _unsupported(t, 'pad_to_square / size_divisor (a fixed size is expected)')
            if step.get('size') is None:
                raise _unsupported(t, 'size is missing')
            ph, pw = _pair(step.get('size'), t, 'size')
            kw['size'] = (int(ph), int(pw))
            pv = step.get('pad_val', 0)
            if hasattr(pv, 'get'):
                img, masks, seg = pv.get('img', 0), pv.get('masks', 0), pv.get('seg', 255)
            else:
                img, masks, seg = pv, 0, 255
            if masks != 0 or not 0 <= int(seg) <= 255 or int(seg) != seg:
                raise _unsupported(t, f'pad_val masks={masks!r} / seg={seg!r}')
            kw['pad_val'] = (three_floats(img, 'train pipeline: Pad.pad_val.img'), 0, int(seg))
        elif t == 'Normalize':
            kw['mean'] = three_floats(step.get('mean', 0.0), 'train pipeline: Normalize.mean')
            kw['std'] = three_floats(step.get('std', 1.0), 'train pipeline: Normalize.std')
            if any(s == 0.0 for s in kw['std']):
                raise _unsupported(t, 'std == 0')
            kw['to_rgb'] = bool(step.get('to_rgb', True))
        elif t in _PASSIVE:
            pass
        else:
            raise _unsupported(str(t), 'unknown transform')
    for t in _LOADERS[:1] + _ORDER:
        if t not in seen:
            raise _unsupported(t, 'missing')
    if not any(t in seen for t in _ANNOTATIONS):
        raise _unsupported('Load*Annotations', 'missing')
    if kw['size'][0] < kw['crop_size'][0] or kw['size'][1] < kw['crop_size'][1]:
        raise _unsupported('Pad', f'size {kw["size"]} is smaller than crop_size {kw["crop_size"]}')
    return TrainPrepSpec(**kw)


# ---- the random decisions ----------------------------------------------------------------------------------------------------------
def draw_train_params(rng, hw, spec):
    """The random decisions of one sample from a `numpy.random.Generator`, in this order (four draws, always):
        flip = rng.random() < flip_ratio
        ratio = rng.random() * (hi - lo) + lo;  scale = (int(W * ratio), int(H * ratio))  with (W, H) = img_scale
        (nh, nw) = image_prep.rescale_size(hw, scale)
        oy = rng.integers(0, max(nh - ch, 0) + 1);  ox = rng.integers(0, max(nw - cw, 0) + 1)
    A scale with a zero entry raises CggError."""
    flip = bool(rng.random() < spec.flip_ratio)
    lo, hi = spec.ratio_range
    ratio = rng.random() * (hi - lo) + lo
    scale = (int(spec.img_scale[0] * ratio), int(spec.img_scale[1] * ratio))
    nh, nw = resized_hw(hw, scale)
    oy = int(rng.integers(0, max(nh - spec.crop_size[0], 0) + 1))
    ox = int(rng.integers(0, max(nw - spec.crop_size[1], 0) + 1))
    return TrainParams(flip, scale, (oy, ox))


def resized_hw(hw, scale):
    """(nh, nw) of a source of (h, w) fitted into the (w, h) box `scale`, keeping the ratio; a zero anywhere raises."""
    if not isinstance(scale, (list, tuple)) or len(scale) != 2 or min(int(scale[0]), int(scale[1])) < 1:
        raise CggError(f'train_prep: a scale with a zero entry ({scale!r})')
    nh, nw = rescale_size(hw, (int(scale[0]), int(scale[1])))
    if nh < 1 or nw < 1:
        raise CggError(f'train_prep: scale {tuple(scale)} resizes a {int(hw[0])} x {int(hw[1])} image to {nh} x {nw}')
    return nh, nw


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def bilinear_taps(s, d):
    """Rule 2 for one axis with float32 weights: (i0, i1, a0, a1) of length d -- `image_prep.resize_coefficients`' taps (equal to
    them, clamps included) with a0 = float32(1 - fx), a1 = fx instead of the 11-bit integers."""
    scale = 1.0 / (float(d) / float(s))
    k = np.arange(d, dtype=np.float64)
    fx = ((k + 0.5) * scale - 0.5).astype(np.float32)           # numpy rounds the product and the difference separately
    fl = np.floor(fx)
    i = fl.astype(np.int64)
    fx = (fx - fl).astype(np.float32)
    lo, hi = i < 0, i >= s - 1
    i = np.where(lo, 0, np.where(hi, s - 1, i))
    fx = np.where(lo | hi, np.float32(0), fx).astype(np.float32)
    return i.astype(np.int32), np.minimum(i + 1, s - 1).astype(np.int32), (np.float32(1) - fx).astype(np.float32), fx


def nearest_index(s, d):
    """Rule 3 for one axis: the source index of each of the d target positions, min(floor(k * (1 / (d / s))), s - 1)."""
    scale = 1.0 / (float(d) / float(s))
    return np.minimum(np.floor(np.arange(d, dtype=np.float64) * scale).astype(np.int64), s - 1)


def sample_geometry(hw, p, spec):
    """(nh, nw, oy, ox, eh, ew) of one sample: the resized size, the window's corner and the image extent inside the output plane."""
    nh, nw = resized_hw(hw, p.scale)
    oy, ox = int(p.crop_yx[0]), int(p.crop_yx[1])
    ch, cw = spec.crop_size
    if not (0 <= oy <= max(nh - ch, 0) and 0 <= ox <= max(nw - cw, 0)):
        raise CggError(f'train_prep: crop offset ({oy}, {ox}) outside the margins ({max(nh - ch, 0)}, {max(nw - cw, 0)}) of the '
                       f'{nh} x {nw} resized image')
    return nh, nw, oy, ox, min(nh - oy, ch), min(nw - ox, cw)


def _norm_spec(spec):
    return PrepSpec(pad_val=tuple(spec.pad_val[0]), mean=spec.mean, std=spec.std, to_rgb=spec.to_rgb, pad_before_norm=True)


def train_meta(sample, hw, p, geom, spec):
    h, w = int(hw[0]), int(hw[1])
    nh, nw, _, _, eh, ew = geom
    return dict(filename=sample.get('filename'), ori_filename=sample.get('ori_filename', sample.get('filename')),
                ori_shape=(h, w, 3), img_shape=(eh, ew, 3), pad_shape=(spec.size[0], spec.size[1], 3),
                scale_factor=np.array([nw / w, nh / h, nw / w, nh / h], dtype=np.float32), flip=bool(p.flip),
                flip_direction='horizontal' if p.flip else None,
                img_norm_cfg=dict(mean=np.asarray(spec.mean, dtype=np.float32), std=np.asarray(spec.std, dtype=np.float32),
                                  to_rgb=spec.to_rgb), batch_input_shape=tuple(spec.size))


def _check_sample(s, spec):
    """(img, masks (n, h, w) uint8 view, labels, seg or None) of one raw sample"""
    if not hasattr(s, 'get') or s.get('img') is None:
        raise CggError('train_prep: a sample is a dict with img, gt_masks, gt_labels')
    img = _as_hwc_u8(s['img'])
    h, w = img.shape[:2]
    if h < 1 or w < 1:
        raise CggError(f'train_prep: a zero-sized image ({h} x {w})')
    masks = s.get('gt_masks')
    masks = masks.cpu().numpy() if torch.is_tensor(masks) else np.asarray(getattr(masks, 'masks', masks))
    if masks.dtype == np.bool_:
        masks = masks.view(np.uint8)
    if masks.dtype != np.uint8 or masks.ndim != 3 or (masks.shape[0] and masks.shape[1:] != (h, w)):
        raise CggError(f'train_prep: gt_masks must be (n, {h}, {w}) uint8 or bool bitmaps (got {masks.dtype}, shape {masks.shape}; '
                       'polygons go in gt_polygons, rule 6)')
    labels = s.get('gt_labels')
    labels = labels.cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if labels.shape != (masks.shape[0],):
        raise CggError(f'train_prep: gt_labels must be ({masks.shape[0]},) (got shape {labels.shape})')
    seg = None
    if spec.with_seg:
        seg = s.get('gt_semantic_seg')
        if seg is None:
            raise CggError('train_prep: the pipeline loads a semantic map (with_seg) and the sample has no gt_semantic_seg')
        seg = seg.cpu().numpy() if torch.is_tensor(seg) else np.asarray(seg)
        if seg.dtype != np.uint8 or seg.shape != (h, w):
            raise CggError(f'train_prep: gt_semantic_seg must be ({h}, {w}) uint8 (got {seg.dtype}, shape {seg.shape})')
    return img, masks, labels, seg


def _check_pan_seg(pan, hw=None):
    """(array, format) of an id map: (h, w) int32 -> 0, (h, w, 3) uint8 RGB -> 1; anything else raises naming pan_seg"""
    pan = pan.cpu().numpy() if torch.is_tensor(pan) else np.asarray(pan)
    fmt = 0 if (pan.dtype == np.int32 and pan.ndim == 2) else 1 if (pan.dtype == np.uint8 and pan.ndim == 3 and pan.shape[2] == 3) else -1
    if fmt < 0 or (hw is not None and tuple(pan.shape[:2]) != (int(hw[0]), int(hw[1]))):
        want = '(h, w)' if hw is None else f'({int(hw[0])}, {int(hw[1])})'
        raise CggError(f'train_prep: pan_seg must be {want} int32 ids or {want[:-1]}, 3) uint8 RGB (got {pan.dtype}, shape {pan.shape})')
    if fmt == 0 and pan.size and int(pan.min()) < 0:
        raise CggError(f'train_prep: pan_seg holds a negative id ({int(pan.min())}); ids are 0 .. 2^31 - 1')
    return pan, fmt


def _check_segments(segments, fmt):
    """[(id, category, is_thing)] of the `ann_info['masks']` records, in record order; anything outside rule 5 raises naming segments"""
    if segments is None or isinstance(segments, (str, bytes)) or not hasattr(segments, '__iter__'):
        raise CggError("train_prep: segments must be a sequence of dicts with id, category, is_thing (ann_info['masks'])")
    recs, seen = [], set()
    top = 2**24 - 1 if fmt == 1 else 2**31 - 1
    for i, r in enumerate(segments):
        if not hasattr(r, 'get') or r.get('id') is None or r.get('category') is None:
            raise CggError(f'train_prep: segments[{i}] must be a dict with id, category, is_thing (got {r!r})')
        sid, cat = int(r['id']), int(r['category'])
        if sid != r['id'] or not 0 <= sid <= top:
            raise CggError(f'train_prep: segments[{i}]: id {r["id"]!r} outside 0 .. {top}' + (' (an RGB id map holds 24 bits)' if fmt == 1 else ''))
        if cat != r['category'] or not 0 <= cat <= 254:
            raise CggError(f'train_prep: segments[{i}]: category {r["category"]!r} outside 0 .. 254 (255 is the ignore label)')
        if sid in seen:
            raise CggError(f'train_prep: segments[{i}]: id {sid} appears twice')
        seen.add(sid)
        recs.append((sid, cat, bool(r.get('is_thing'))))
    if len(recs) > TRAIN_PREP_MAX_SEGMENTS:
        raise CggError(f'train_prep: segments: {len(recs)} records for one image, more than {TRAIN_PREP_MAX_SEGMENTS}')
    return recs


def _pan_ids(pan, fmt):
    """the (h, w) int32 ids of an id map: rgb2id for the RGB form"""
    if fmt == 0:
        return pan
    p = pan.astype(np.int32)
    return p[:, :, 0] + 256 * p[:, :, 1] + 65536 * p[:, :, 2]


def _load_panoptic(pan, fmt, recs):
    ids = _pan_ids(pan, fmt)
    seg = np.full(ids.shape, 255, dtype=np.uint8)            # 255 as ignore: the loader's constant
    masks = []
    for sid, cat, is_thing in recs:
        m = ids == sid
        seg = np.where(m, np.uint8(cat), seg)
        if is_thing:                                         # the legal thing masks
            masks.append(m.astype(np.uint8))
    masks = np.stack(masks) if masks else np.zeros((0,) + ids.shape, dtype=np.uint8)
    return masks, seg


def load_panoptic_host(pan_seg, segments):
    """Rule 5, the reference's LoadOpenPanopticAnnotations._load_masks_and_semantic_segs (loading.py:317-341) in numpy: the id map
    ((h, w) int32, or (h, w, 3) uint8 RGB) and the `ann_info['masks']` records -> (gt_masks (n_things, h, w) uint8, one bitmap per
    is_thing record in record order; gt_semantic_seg (h, w) uint8, each record's category where pan == id, 255 elsewhere)."""
    pan, fmt = _check_pan_seg(pan_seg)
    return _load_panoptic(pan, fmt, _check_segments(segments, fmt))


def _check_pan_sample(s):
    """(img, id map, format, records, labels) of one raw panoptic sample"""
    if not hasattr(s, 'get') or s.get('img') is None:
        raise CggError('train_prep: a panoptic sample is a dict with img, pan_seg, segments, gt_labels')
    if s.get('gt_masks') is not None:
        raise CggError('train_prep: a sample with both gt_masks and pan_seg (bitmaps or the id map, not both)')
    img = _as_hwc_u8(s['img'])
    h, w = img.shape[:2]
    if h < 1 or w < 1:
        raise CggError(f'train_prep: a zero-sized image ({h} x {w})')
    pan, fmt = _check_pan_seg(s['pan_seg'], (h, w))
    recs = _check_segments(s.get('segments'), fmt)
    things = sum(1 for r in recs if r[2])
    labels = s.get('gt_labels')
    labels = labels.cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if labels.shape != (things,):
        raise CggError(f'train_prep: gt_labels must be ({things},), one per is_thing record of segments (got shape {labels.shape})')
    return img, pan, fmt, recs, labels


def _is_panoptic(s):
    return hasattr(s, 'get') and s.get('pan_seg') is not None


def _batch_is_panoptic(samples):
    pan = [_is_panoptic(s) for s in samples]
    if any(pan) and not all(pan):
        raise CggError('train_prep: a batch that mixes bitmap samples (gt_masks) and panoptic samples (pan_seg)')
    return pan[0]


def panoptic_to_bitmap_sample(s):
    """the bitmap sample rule 5 makes of a raw panoptic one: pan_seg / segments replaced by gt_masks and gt_semantic_seg"""
    _, pan, fmt, recs, _ = _check_pan_sample(s)
    out = {k: v for k, v in s.items() if k not in ('pan_seg', 'segments')}
    out['gt_masks'], out['gt_semantic_seg'] = _load_panoptic(pan, fmt, recs)
    return out


# ---- rule 6: COCO polygons -> bitmaps ---------------------------------------------------------------------------------------------
POLY_SCALE = 5                                               # rleFrPoly walks the outline on a grid of 1 / 5 pixel


def _as_part(part):
    """one part as a float64 array x0, y0, x1, y1, ... (no checks: `_check_polygons` is the checked door)"""
    return np.asarray(part, dtype=np.float64).reshape(-1)


def _polygon_mask_literal(parts, h, w):
    """Rule 6 in its LITERAL form, plain loops over Python floats (IEEE doubles, every operation rounded on its own; int() truncates
    toward zero like a C cast): per part the vertices, the edge walk, the crossings, then the sorted crossings as run lengths with
    zero-length runs merged as rleFrPoly does, decoded column-major; the parts OR-ed (`merge` with intersect = 0). Test-facing: it is
    what `polygon_mask_host` is held equal to."""
    h, w = int(h), int(w)
    out = np.zeros(h * w, dtype=np.uint8)
    for part in parts:
        xy = [float(c) for c in _as_part(part)]
        k = len(xy) // 2
        X = [int(POLY_SCALE * xy[2 * j] + 0.5) for j in range(k)]
        Y = [int(POLY_SCALE * xy[2 * j + 1] + 0.5) for j in range(k)]
        X.append(X[0])
        Y.append(Y[0])
        u, v = [], []
        for j in range(k):
            xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
            dx, dy = abs(xe - xs), abs(ys - ye)
            flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
            if flip:
                xs, xe, ys, ye = xe, xs, ye, ys
            if dx == 0 and dy == 0:                          # one point; the slope 0 / 0 is never used
                u.append(xs)
                v.append(ys)
            elif dx >= dy:
                s = float(ye - ys) / dx
                for d in range(dx + 1):
                    t = dx - d if flip else d
                    u.append(t + xs)
                    v.append(int(ys + s * t + 0.5))
            else:
                s = float(xe - xs) / dy
                for d in range(dy + 1):
                    t = dy - d if flip else d
                    v.append(t + ys)
                    u.append(int(xs + s * t + 0.5))
        a = []
        for i in range(1, len(u)):
            if u[i] == u[i - 1]:
                continue
            xd = float(u[i] if u[i] < u[i - 1] else u[i] - 1)
            xd = (xd + 0.5) / POLY_SCALE - 0.5
            if np.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(min(v[i], v[i - 1]))
            yd = (yd + 0.5) / POLY_SCALE - 0.5
            yd = 0.0 if yd < 0 else float(h) if yd > h else yd
            a.append(int(xd) * h + int(np.ceil(yd)))
        a.sort()
        a.append(h * w)
        p = 0
        for j in range(len(a)):                              # differences
            a[j], p = a[j] - p, a[j]
        runs = [a[0]]
        j = 1
        while j < len(a):                                    # zero-length runs merge their neighbours
            if a[j] > 0:
                runs.append(a[j])
                j += 1
            else:
                j += 1
                if j < len(a):
                    runs[-1] += a[j]
                    j += 1
        pos, val = 0, 0
        for r in runs:                                       # the runs alternate 0, 1, ... over the column-major pixels
            if val:
                out[pos:pos + r] = 1
            pos += r
            val ^= 1
    return np.ascontiguousarray(out.reshape(w, h).T)


def _part_crossings(part, h, w):
    """steps 1 to 3 of rule 6 for one part, vectorised per edge: the column-major indices of its crossings (int64, unsorted)"""
    xy = _as_part(part)
    X = (POLY_SCALE * xy[0::2] + 0.5).astype(np.int64)       # the cast truncates toward zero
    Y = (POLY_SCALE * xy[1::2] + 0.5).astype(np.int64)
    k = X.size
    us, vs = [], []
    for j in range(k):
        xs, xe, ys, ye = int(X[j]), int(X[(j + 1) % k]), int(Y[j]), int(Y[(j + 1) % k])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        m = max(dx, dy)
        if m == 0:
            us.append(np.array([xs], dtype=np.int64))
            vs.append(np.array([ys], dtype=np.int64))
            continue
        t = np.arange(m, -1, -1, dtype=np.int64) if flip else np.arange(m + 1, dtype=np.int64)
        tf = t.astype(np.float64)
        if dx >= dy:
            s = np.float64(ye - ys) / np.float64(dx)
            us.append(t + xs)
            vs.append(((np.float64(ys) + s * tf) + 0.5).astype(np.int64))
        else:
            s = np.float64(xe - xs) / np.float64(dy)
            vs.append(t + ys)
            us.append(((np.float64(xs) + s * tf) + 0.5).astype(np.int64))
    u, v = np.concatenate(us), np.concatenate(vs)
    u0, u1, v0, v1 = u[:-1], u[1:], v[:-1], v[1:]
    xd = (np.where(u1 < u0, u1, u1 - 1).astype(np.float64) + 0.5) / POLY_SCALE - 0.5
    ok = (u1 != u0) & (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = (np.minimum(v0, v1).astype(np.float64) + 0.5) / POLY_SCALE - 0.5
    yd = np.ceil(np.clip(yd, 0.0, float(h)))
    return xd[ok].astype(np.int64) * h + yd[ok].astype(np.int64)


def polygon_mask_host(parts, h, w):
    """Rule 6: the (h, w) uint8 bitmap of one instance given as a list of polygons (`parts`, each a flat x0, y0, x1, y1, ...
    sequence) -- what pycocotools' `frPyObjects` -> `merge` -> `decode` is published to yield, restated from maskApi.c (rleFrPoly):
    vertices on a grid of 1 / 5 pixel, the outline walked point by point, a crossing at every change of column, and a pixel set iff
    the number of crossings at or before its column-major index is odd (one prefix parity over the whole plane: it does not restart
    at a column); the parts OR-ed. This is the PARITY form, the one csrc/train_prep.hip computes; `_polygon_mask_literal` is the
    run-length form the C code spells out, and tests/test_train_prep_polygons.py holds the two equal. pycocotools is not available
    offline, so equality with a particular build is NOT claimed; what is pinned is this rule. No input checks here."""
    h, w = int(h), int(w)
    out = np.zeros((h, w), dtype=np.uint8)
    for part in parts:
        a = _part_crossings(part, h, w)
        tog = np.bincount(a, minlength=h * w + 1)[:h * w] & 1        # a == h * w lies past the last pixel
        out |= (np.cumsum(tog) & 1).astype(np.uint8).reshape(w, h).T
    return out


def _check_polygons(polys, where='gt_polygons'):
    """`ann_info['masks']` of one image -> [[float64 array per part] per instance]; anything outside rule 6 raises naming it"""
    from .ops import TRAIN_PREP_MAX_COORD
    if polys is None or isinstance(polys, (str, bytes, dict)) or not hasattr(polys, '__iter__'):
        raise CggError(f"train_prep: {where} must be a list over instances of lists of polygons (ann_info['masks'])")
    out = []
    for i, inst in enumerate(polys):
        if isinstance(inst, dict):
            raise CggError(f'train_prep: {where}[{i}] is an RLE dict segmentation (a crowd; the dataset sends those to bboxes_ignore): '
                           'only polygon lists are rasterised')
        if isinstance(inst, (str, bytes)) or not hasattr(inst, '__iter__'):
            raise CggError(f'train_prep: {where}[{i}] must be a list of polygons (got {type(inst).__name__})')
        parts = []
        for j, part in enumerate(inst):
            try:
                xy = np.asarray(part, dtype=np.float64)
            except (TypeError, ValueError):
                raise CggError(f'train_prep: {where}[{i}][{j}] must be a flat sequence of numbers x0, y0, x1, y1, ...') from None
            if xy.ndim != 1:
                raise CggError(f'train_prep: {where}[{i}][{j}] must be a flat sequence x0, y0, x1, y1, ... (got shape {xy.shape})')
            if xy.size == 0:
                raise CggError(f'train_prep: {where}[{i}][{j}] is an empty part')
            if xy.size % 2:
                raise CggError(f'train_prep: {where}[{i}][{j}] has an odd coordinate count ({xy.size})')
            if not np.isfinite(xy).all():
                raise CggError(f'train_prep: {where}[{i}][{j}] holds non-finite coordinates')
            if np.abs(xy).max() > TRAIN_PREP_MAX_COORD:
                raise CggError(f'train_prep: {where}[{i}][{j}] holds a coordinate beyond +-{TRAIN_PREP_MAX_COORD} '
                               f'({xy[np.abs(xy).argmax()]!r}); CGG_IMAGE_PREP_MAX_DIM bounds the edge walk')
            parts.append(np.ascontiguousarray(xy))
        out.append(parts)
    return out


def _check_poly_sample(s, spec):
    """(img, [[part arrays] per instance], labels) of one raw polygon sample"""
    if not hasattr(s, 'get') or s.get('img') is None:
        raise CggError('train_prep: a polygon sample is a dict with img, gt_polygons, gt_labels')
    if s.get('gt_masks') is not None:
        raise CggError('train_prep: a sample with both gt_masks and gt_polygons (bitmaps or polygons, not both)')
    if spec is not None and spec.with_seg:
        raise CggError('train_prep: the pipeline loads a semantic map (with_seg) and gt_polygons samples have none')
    img = _as_hwc_u8(s['img'])
    h, w = img.shape[:2]
    if h < 1 or w < 1:
        raise CggError(f'train_prep: a zero-sized image ({h} x {w})')
    polys = _check_polygons(s['gt_polygons'])
    labels = s.get('gt_labels')
    labels = labels.cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if labels.shape != (len(polys),):
        raise CggError(f'train_prep: gt_labels must be ({len(polys)},), one per instance of gt_polygons (got shape {labels.shape})')
    return img, polys, labels


def _is_polygons(s):
    return hasattr(s, 'get') and s.get('gt_polygons') is not None


def _batch_is_polygons(samples):
    poly = [_is_polygons(s) for s in samples]
    if any(poly) and not all(poly):
        raise CggError('train_prep: a batch that mixes polygon samples (gt_polygons) with bitmap or panoptic samples')
    return poly[0]


def polygons_to_bitmap_sample(s, spec=None):
    """the bitmap sample rule 6 makes of a raw polygon one: gt_polygons replaced by gt_masks (n, h, w) uint8 (with `spec`, a
    pipeline that loads a semantic map is refused: polygon samples have none)"""
    img, polys, _ = _check_poly_sample(s, spec)
    h, w = img.shape[:2]
    out = {k: v for k, v in s.items() if k != 'gt_polygons'}
    out['gt_masks'] = (np.stack([polygon_mask_host(parts, h, w) for parts in polys]) if polys
                       else np.zeros((0, h, w), dtype=np.uint8))
    return out


def _check_batch(samples, params):
    if not isinstance(samples, (list, tuple)) or not samples:
        raise CggError('train_prep: expected a non-empty list of samples')
    if not isinstance(params, (list, tuple)) or len(params) != len(samples):
        raise CggError('train_prep: one TrainParams per sample expected')


def stats_to_boxes(stats):
    """(n, 5) int32 rows of area, xmin, ymin, xmax, ymax -> (n, 4) float32 boxes (xmin, ymin, xmax + 1, ymax + 1)"""
    st = np.asarray(stats, dtype=np.int64).reshape(-1, 5)
    return np.stack([st[:, 1], st[:, 2], st[:, 3] + 1, st[:, 4] + 1], axis=1).astype(np.float32)


def mask_stats(m, eh, ew):
    """area, xmin, ymin, xmax, ymax of one (H, W) mask over its image extent (an empty one: 0, INT32_MAX twice, -1 twice)"""
    ys, xs = np.nonzero(m[:eh, :ew])
    if ys.size == 0:
        return (0, 2**31 - 1, 2**31 - 1, -1, -1)
    return (int(ys.size), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def prepare_train_host(samples, params, spec):
    """The rule in numpy. samples: dicts with img (h, w, 3) uint8 BGR, gt_masks (n, h, w) uint8 / bool, gt_labels (n,), optionally
    gt_semantic_seg (h, w) uint8, the caption fields and filename / ori_filename (passed through) -- or raw panoptic samples with
    pan_seg and segments in place of gt_masks / gt_semantic_seg (rule 5; all of a batch or none), or raw polygon samples with
    gt_polygons in place of gt_masks (rule 6; likewise); params: one TrainParams each.
    -> (kwargs, kept): kwargs holds img (B, 3, H, W) float32, img_metas, gt_masks (list of (k_b, H, W) uint8), gt_bboxes (list of
    (k_b, 4) float32), gt_labels, gt_semantic_seg (B, 1, H, W) uint8 when the pipeline loads one, and the caption fields as lists --
    numpy arrays, named as `forward_train` names them (`to_device` uploads them); kept = [k_b], the surviving instances per sample."""
    _check_batch(samples, params)
    if _batch_is_panoptic(samples):                          # by definition: the rule on the bitmap samples rule 5 makes
        return prepare_train_host([panoptic_to_bitmap_sample(s) for s in samples], params, spec)
    if _batch_is_polygons(samples):                          # likewise: the rule on the bitmap samples rule 6 makes
        return prepare_train_host([polygons_to_bitmap_sample(s, spec) for s in samples], params, spec)
    H, W = spec.size
    mean, rstd, pad = norm_constants(_norm_spec(spec))
    B = len(samples)
    batch = np.empty((B, 3, H, W), dtype=np.float32)
    segs = np.full((B, 1, H, W), spec.pad_val[2], dtype=np.uint8) if spec.with_seg else None
    out = dict(img=batch, img_metas=[], gt_bboxes=[], gt_labels=[], gt_masks=[])
    kept = []
    for b, (s, p) in enumerate(zip(samples, params)):
        img, masks, labels, seg = _check_sample(s, spec)
        h, w = img.shape[:2]
        geom = sample_geometry((h, w), p, spec)
        nh, nw, oy, ox, eh, ew = geom
        # ---- image: rule 2 on the window's rows and columns only
        yi0, yi1, yb0, yb1 = (a[oy:oy + eh] for a in bilinear_taps(h, nh))
        xi0, xi1, xa0, xa1 = (a[ox:ox + ew] for a in bilinear_taps(w, nw))
        if p.flip:
            xi0, xi1 = w - 1 - xi0, w - 1 - xi1
        src = img.astype(np.float32)
        R0 = src[yi0][:, xi0] * xa0[None, :, None] + src[yi0][:, xi1] * xa1[None, :, None]
        R1 = src[yi1][:, xi0] * xa0[None, :, None] + src[yi1][:, xi1] * xa1[None, :, None]
        v = R0 * yb0[:, None, None] + R1 * yb1[:, None, None]
        assert v.dtype == np.float32
        if spec.to_rgb:
            v = v[:, :, ::-1]
        batch[b] = pad[:, None, None]
        batch[b, :, :eh, :ew] = ((v - mean) * rstd).astype(np.float32).transpose(2, 0, 1)
        # ---- masks and the semantic map: rule 3
        ry = nearest_index(h, nh)[oy:oy + eh]
        rx = nearest_index(w, nw)[ox:ox + ew]
        if p.flip:
            rx = w - 1 - rx
        m = np.zeros((masks.shape[0], H, W), dtype=np.uint8)
        m[:, :eh, :ew] = masks[:, ry][:, :, rx] != 0
        if seg is not None:
            segs[b, 0, :eh, :ew] = seg[ry][:, rx]
        stats = np.array([mask_stats(mi, eh, ew) for mi in m], dtype=np.int32).reshape(-1, 5)
        keep = np.nonzero(stats[:, 0] >= 1)[0]
        out['gt_masks'].append(np.ascontiguousarray(m[keep]))
        out['gt_bboxes'].append(stats_to_boxes(stats[keep]))
        out['gt_labels'].append(labels[keep])
        out['img_metas'].append(train_meta(s, (h, w), p, geom, spec))
        kept.append(int(keep.size))
    if segs is not None:
        out['gt_semantic_seg'] = segs
    for k in CAPTION_FIELDS:
        if all(k in s for s in samples):
            out[k] = [s[k].cpu().numpy() if torch.is_tensor(s[k]) else np.asarray(s[k]) for s in samples]
    return out, kept


def to_device(kwargs, device):
    """`prepare_train_host`'s kwargs with every array as a tensor on `device` (img_metas stay on the host)."""
    def up(v):
        if isinstance(v, list):
            return [up(x) for x in v]
        return torch.as_tensor(v).to(device) if isinstance(v, (np.ndarray, torch.Tensor)) else v
    return {k: (v if k == 'img_metas' else up(v)) for k, v in kwargs.items()}


# ---- the device side -------------------------------------------------------------------------------------------------------------
class TrainPrep:
    """Device-side training pipeline: `prep(samples, params) -> (kwargs, kept)`, equal to `prepare_train_host` with every array a
    tensor on `device`; `forward_train(**kwargs)` takes it as it is.

    One call = one host copy into a pinned staging slot (the two descriptor tables, then the raw images, instance masks and semantic
    maps back to back), ONE asynchronous H2D copy and at most TWO launches of `cgg_train_prep_u8` on the current stream (image
    planes; mask and semantic planes with the per-instance area / box reduction), then ONE small D2H copy of the (N, 5) int32
    statistics. A batch of raw panoptic samples (pan_seg + segments) stages three tables, the images and the id maps -- no bitmap, no
    semantic map -- and runs `cgg_train_prep_panoptic_u8` instead (image planes; every thing mask, the semantic plane and the
    statistics from one gather of the id map per pixel); the rest is the same. A batch of raw polygon samples (gt_polygons) stages
    three tables, the images and the float64 coordinates -- no bitmap -- and runs `cgg_train_prep_polygons_u8`: three launches (image
    planes; the instances' bit planes into a grow-only device workspace kept next to the staging slots; the plane kernel over those
    bits). So, every way: ONE small D2H copy of the
    statistics. Waiting for that copy is the SINGLE synchronisation per batch: which instances survive decides the shapes of
    gt_masks / gt_bboxes / gt_labels, and the host has to know them. gt_masks[b] is a zero-copy slice of the masks tensor when every
    instance of image b survived, an index_select otherwise; gt_bboxes come from the statistics. A sample without a surviving
    instance is returned as it is, with a (0, H, W) mask tensor, and reported as kept[b] == 0 -- re-sampling is the caller's
    decision (tools/train.py follows [3P] mmdet and draws another sample). There is no CPU path: a non-ROCm device raises (use
    `prepare_train_host` to prepare on the host, explicitly)."""

    def __init__(self, spec, device, slots=3):
        device = torch.device(device)
        if device.type != 'cuda' or not torch.cuda.is_available():
            raise CggError(f'TrainPrep needs a ROCm device (got {device}); prepare_train_host is the host-side form of the same rule')
        if not isinstance(spec, TrainPrepSpec):
            spec = parse_train_pipeline(spec)
        self.spec, self.device = spec, device
        self._ring = _StagingRing(device, slots, 'TrainPrep')
        self._workspace = self._workspace_used = None           # the polygon route's device workspace, grow-only
        self.last_staged_bytes = 0

    # A layout lays out the staged bytes of one batch -- the tables back to back from byte 0 (the default offsets of the ops), then the
    # planes -- and answers (n bytes, [int32 rows of each table], [(byte offset, array)] to copy, launch). `launch(slot, tables, img,
    # masks, seg, stats, n, stream)` runs the batch's kernels on the uploaded slot.
    @staticmethod
    def _image_rows(parsed, params, geoms, counts, n, copies, planes=None):
        """The image table of every layout, the images staged from byte `n` on. `planes(b, q, h, w, n) -> (n, semantic-map offset)`
        stages what else belongs to image b right behind it. Returns (n, rows)."""
        rows, first = [], 0
        for b, (q, p, (nh, nw, oy, ox, _, _)) in enumerate(zip(parsed, params, geoms)):
            h, w = int(q[0].shape[0]), int(q[0].shape[1])
            off, seg_off = n, -1
            copies.append((off, q[0]))
            n += h * w * 3
            if planes is not None:
                n, seg_off = planes(b, q, h, w, n)
            rows.append((off, h, w, 3 * w, nh, nw, oy, ox, int(bool(p.flip)), first, counts[b], seg_off))
            first += counts[b]
        return n, rows

    @staticmethod
    def _table_bytes(shapes):
        """bytes of the int32 tables of these (rows, cols), back to back: where the planes start"""
        return 4 * sum(rows * cols for rows, cols in shapes)

    @staticmethod
    def _tables(shapes, *rows):
        """the row lists of the tables as int32 arrays of their (rows, cols)"""
        return [np.asarray(r, dtype=np.int32).reshape(shape) for r, shape in zip(rows, shapes)]

    def _layout_bitmaps(self, parsed, params, geoms, counts):
        """image and instance (image index, byte offset, row pitch) tables, then per sample the image, its instance bitmaps and its
        semantic map"""
        B, N = len(parsed), sum(counts)
        inst_rows, copies = [], []

        def planes(b, q, h, w, n):
            for i in range(counts[b]):
                inst_rows.append((b, n, w))
                copies.append((n, q[1][i]))
                n += h * w
            if q[3] is None:
                return n, -1
            copies.append((n, q[3]))
            return n + h * w, n
        shapes = (B, TRAIN_PREP_IMG_COLS), (N, TRAIN_PREP_INST_COLS)
        n, img_rows = self._image_rows(parsed, params, geoms, counts, self._table_bytes(shapes), copies, planes)
        return n, self._tables(shapes, img_rows, inst_rows), copies, functools.partial(self._launch, ops.train_prep_u8)

    def _layout_panoptic(self, parsed, params, geoms, counts):
        """image, panoptic and segment tables, then per sample the image and the id map (an int32 map on a 4-byte boundary). No
        bitmap and no semantic map is staged."""
        B, S = len(parsed), sum(len(q[3]) for q in parsed)
        pan_rows, seg_rows, copies = [], [], []

        def planes(b, q, h, w, n):
            _, pan, fmt, recs, _ = q
            if fmt == 0:
                n = (n + 3) & ~3
            bpp = 3 if fmt else 4
            pan_rows.append((n, bpp * w, fmt, len(seg_rows), len(recs)))
            copies.append((n, pan))
            slot, rows = 0, []
            for sid, cat, is_thing in recs:                  # slot t + 1 = the image's thing t, in record order; 0 = no thing
                slot += int(is_thing)
                rows.append((sid, ((slot if is_thing else 0) << 8) | cat))
            seg_rows.extend(sorted(rows))                    # the kernel searches them by id
            return n + h * w * bpp, -1
        shapes = (B, TRAIN_PREP_IMG_COLS), (B, TRAIN_PREP_PAN_COLS), (S, TRAIN_PREP_SEG_COLS)
        n, img_rows = self._image_rows(parsed, params, geoms, counts, self._table_bytes(shapes), copies, planes)
        return n, self._tables(shapes, img_rows, pan_rows, seg_rows), copies, functools.partial(self._launch, ops.train_prep_panoptic_u8)

    def _layout_polygons(self, parsed, params, geoms, counts):
        """image, instance (image index, first part, parts) and part (byte offset, vertices) tables, the images, then every part's
        coordinates as float64 from an 8-byte boundary on. No bitmap is staged."""
        B, N = len(parsed), sum(counts)
        P = sum(len(parts) for q in parsed for parts in q[1])
        inst_rows, part_rows, copies = [], [], []
        shapes = (B, TRAIN_PREP_IMG_COLS), (N, TRAIN_PREP_POLY_INST_COLS), (P, TRAIN_PREP_POLY_PART_COLS)
        n, img_rows = self._image_rows(parsed, params, geoms, counts, self._table_bytes(shapes), copies)
        n = (n + 7) & ~7
        for b, q in enumerate(parsed):
            for parts in q[1]:
                inst_rows.append((b, len(part_rows), len(parts)))
                for xy in parts:
                    part_rows.append((n, xy.size // 2))
                    copies.append((n, xy))
                    n += xy.nbytes
        return n, self._tables(shapes, img_rows, inst_rows, part_rows), copies, self._launch_polygons

    def _launch(self, op, slot, tables, img, masks, seg, stats, n, stream):
        spec = self.spec
        op(slot.dev, *tables, img, masks, seg, stats, spec.mean, spec.std, spec.pad_val[0], to_rgb=spec.to_rgb,
           crop_size=spec.crop_size, seg_pad=spec.pad_val[2], staged_bytes=n)

    def _launch_polygons(self, slot, tables, img, masks, seg, stats, n, stream):
        """the polygon route keeps a grow-only device workspace (bit planes, toggle planes) next to the staging slots: the kernels
        clear what they read, and an event says when the last batch's kernels have left it"""
        spec = self.spec
        nbytes = ops.train_prep_polygons_workspace_bytes(tables[0], masks.shape[0])
        if self._workspace is None or self._workspace.numel() * 4 < nbytes:
            self._workspace = torch.empty((max(1 << 14, 1 << max(nbytes - 1, 1).bit_length()) // 4,), dtype=torch.int32, device=self.device)
        if self._workspace_used is not None:
            stream.wait_event(self._workspace_used)           # device: the last batch's kernels have left the workspace (another stream)
        ops.train_prep_polygons_u8(slot.dev, *tables, slot.pinned, img, masks, stats, self._workspace, spec.mean, spec.std,
                                   spec.pad_val[0], to_rgb=spec.to_rgb, crop_size=spec.crop_size, staged_bytes=n)
        self._workspace_used = torch.cuda.Event()
        self._workspace_used.record(stream)

    def prep(self, samples, params):
        spec = self.spec
        _check_batch(samples, params)
        H, W = spec.size
        B = len(samples)
        if _batch_is_panoptic(samples):
            parsed = [_check_pan_sample(s) for s in samples]
            labels_all = [q[4] for q in parsed]
            counts = [int(q[4].shape[0]) for q in parsed]
            layout = self._layout_panoptic
        elif _batch_is_polygons(samples):
            parsed = [_check_poly_sample(s, spec) for s in samples]
            labels_all = [q[2] for q in parsed]
            counts = [len(q[1]) for q in parsed]
            layout = self._layout_polygons
        else:
            parsed = [_check_sample(s, spec) for s in samples]
            labels_all = [q[2] for q in parsed]
            counts = [int(q[1].shape[0]) for q in parsed]
            layout = self._layout_bitmaps
        geoms = [sample_geometry(q[0].shape[:2], p, spec) for q, p in zip(parsed, params)]
        N = sum(counts)
        n, tables, copies, launch = layout(parsed, params, geoms, counts)
        self.last_staged_bytes = n                            # tables + raw planes of this call (what the one H2D copy moves)
        img_out = torch.empty((B, 3, H, W), dtype=torch.float32, device=self.device)
        masks_out = torch.empty((N, H, W), dtype=torch.uint8, device=self.device)
        seg_out = torch.empty((B, 1, H, W), dtype=torch.uint8, device=self.device) if spec.with_seg else None
        stats = torch.empty((N, 5), dtype=torch.int32, device=self.device)
        stats_host = torch.empty((N, 5), dtype=torch.int32).pin_memory()
        with torch.cuda.device(self.device):
            slot = self._ring.acquire(n)
            stream = torch.cuda.current_stream(self.device)
            host_tables, off = [], 0
            for rows in tables:                              # written into the slot; the views are the host copies the op validates
                t = slot.pinned[off:off + 4 * rows.size].view(torch.int32).view(rows.shape)
                if rows.size:
                    t.numpy()[:] = rows
                host_tables.append(t)
                off += 4 * rows.size
            for off, a in copies:
                np.copyto(slot.host[off:off + a.nbytes].view(a.dtype).reshape(a.shape), a)
            self._ring.upload(slot, n, stream)
            launch(slot, host_tables, img_out, masks_out, seg_out, stats, n, stream)
            self._ring.release(slot, stream)
            stats_host.copy_(stats, non_blocking=True)
            done = torch.cuda.Event()
            done.record(stream)
            done.synchronize()                               # the one synchronisation of the batch
            st = stats_host.numpy()
            keep = st[:, 0] >= 1
            keep_idx = torch.from_numpy(np.nonzero(keep)[0]).to(self.device) if not keep.all() else None
            boxes = (stats[:, 1:5] + torch.tensor([0, 0, 1, 1], dtype=torch.int32, device=self.device)).float()
            labels_np = [lab[keep[f:f + c]] for lab, f, c in zip(labels_all, np.cumsum([0] + counts[:-1]).tolist(), counts)]
            out = dict(img=img_out, img_metas=[], gt_bboxes=[], gt_labels=[], gt_masks=[])
            kept, first, kfirst = [], 0, 0
            for b, (s, p, q, g) in enumerate(zip(samples, params, parsed, geoms)):
                c = counts[b]
                k = int(keep[first:first + c].sum())
                if k == c:
                    out['gt_masks'].append(masks_out[first:first + c])
                    out['gt_bboxes'].append(boxes[first:first + c])
                else:
                    idx = keep_idx[kfirst:kfirst + k]
                    out['gt_masks'].append(masks_out.index_select(0, idx))
                    out['gt_bboxes'].append(boxes.index_select(0, idx))
                out['gt_labels'].append(torch.as_tensor(labels_np[b]).to(self.device, non_blocking=True))
                out['img_metas'].append(train_meta(s, q[0].shape[:2], p, g, spec))
                kept.append(k)
                first += c
                kfirst += k
            if seg_out is not None:
                out['gt_semantic_seg'] = seg_out
            for key in CAPTION_FIELDS:
                if all(key in s for s in samples):
                    out[key] = [torch.as_tensor(s[key]).to(self.device, non_blocking=True) for s in samples]
        return out, kept

    __call__ = prep
