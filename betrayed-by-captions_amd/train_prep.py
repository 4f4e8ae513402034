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
are an argument of the rule, so a caller may supply its own. PhotoMetricDistortion, multi-scale value lists and polygon masks are
not restated and are refused by name.

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
"""
from dataclasses import dataclass
from typing import NamedTuple, Tuple

import numpy as np
import torch

from ._lib import CggError
from .image_prep import ImagePrep, PrepSpec, _as_hwc_u8, norm_constants, rescale_size
from .ops import (TRAIN_PREP_IMG_COLS, TRAIN_PREP_INST_COLS, TRAIN_PREP_MAX_SEGMENTS, TRAIN_PREP_PAN_COLS, TRAIN_PREP_SEG_COLS,
                  three_floats)

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
                raise _unsupported(t, 'poly2mask=False (polygon masks are out of scope)')
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
                       'polygon masks are out of scope)')
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
    pan_seg and segments in place of gt_masks / gt_semantic_seg (rule 5; all of a batch or none); params: one TrainParams each.
    -> (kwargs, kept): kwargs holds img (B, 3, H, W) float32, img_metas, gt_masks (list of (k_b, H, W) uint8), gt_bboxes (list of
    (k_b, 4) float32), gt_labels, gt_semantic_seg (B, 1, H, W) uint8 when the pipeline loads one, and the caption fields as lists --
    numpy arrays, named as `forward_train` names them (`to_device` uploads them); kept = [k_b], the surviving instances per sample."""
    _check_batch(samples, params)
    if _batch_is_panoptic(samples):                          # by definition: the rule on the bitmap samples rule 5 makes
        return prepare_train_host([panoptic_to_bitmap_sample(s) for s in samples], params, spec)
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
    statistics from one gather of the id map per pixel); the rest is the same. So, either way: ONE small D2H copy of the
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
        if slots < 1:
            raise CggError('TrainPrep: slots must be >= 1')
        self.spec, self.device = spec, device
        self._slots = [None] * slots
        self._n = 0
        self.last_staged_bytes = 0

    _slot = ImagePrep._slot                                  # the same rotation of pinned staging slots

    def _layout_bitmaps(self, parsed, params, geoms, counts):
        """the staged bytes of a bitmap batch: (n, [(byte offset, int32 rows)] image table first, [(byte offset, array)], op)"""
        B, N = len(parsed), sum(counts)
        img_rows, inst_rows, copies = [], [], []
        inst_off = 4 * TRAIN_PREP_IMG_COLS * B
        n = inst_off + 4 * TRAIN_PREP_INST_COLS * N
        first = 0
        for b, ((img, masks, _, seg), p, (nh, nw, oy, ox, _, _)) in enumerate(zip(parsed, params, geoms)):
            h, w = int(img.shape[0]), int(img.shape[1])
            off = n
            copies.append((off, img))
            n += h * w * 3
            for i in range(counts[b]):
                inst_rows.append((b, n, w))
                copies.append((n, masks[i]))
                n += h * w
            seg_off = -1
            if seg is not None:
                seg_off = n
                copies.append((n, seg))
                n += h * w
            img_rows.append((off, h, w, 3 * w, nh, nw, oy, ox, int(bool(p.flip)), first, counts[b], seg_off))
            first += counts[b]
        tables = [(0, np.asarray(img_rows, dtype=np.int32).reshape(B, TRAIN_PREP_IMG_COLS)),
                  (inst_off, np.asarray(inst_rows, dtype=np.int32).reshape(N, TRAIN_PREP_INST_COLS))]
        return n, tables, copies, 'train_prep_u8'

    def _layout_panoptic(self, parsed, params, geoms, counts):
        """the staged bytes of a panoptic batch: the image, panoptic and segment tables, then per sample the image and the id map (an
        int32 map on a 4-byte boundary). No bitmap and no semantic map is staged."""
        B = len(parsed)
        S = sum(len(q[3]) for q in parsed)
        pan_off = 4 * TRAIN_PREP_IMG_COLS * B
        seg_off = pan_off + 4 * TRAIN_PREP_PAN_COLS * B
        n = seg_off + 4 * TRAIN_PREP_SEG_COLS * S
        img_rows, pan_rows, seg_rows, copies = [], [], [], []
        first = sfirst = 0
        for b, ((img, pan, fmt, recs, _), p, (nh, nw, oy, ox, _, _)) in enumerate(zip(parsed, params, geoms)):
            h, w = int(img.shape[0]), int(img.shape[1])
            img_rows.append((n, h, w, 3 * w, nh, nw, oy, ox, int(bool(p.flip)), first, counts[b], -1))
            copies.append((n, img))
            n += h * w * 3
            if fmt == 0:
                n = (n + 3) & ~3
            bpp = 3 if fmt else 4
            pan_rows.append((n, bpp * w, fmt, sfirst, len(recs)))
            copies.append((n, pan))
            n += h * w * bpp
            slot, rows = 0, []
            for sid, cat, is_thing in recs:                  # slot t + 1 = the image's thing t, in record order; 0 = no thing
                slot += int(is_thing)
                rows.append((sid, ((slot if is_thing else 0) << 8) | cat))
            seg_rows += sorted(rows)                         # the kernel searches them by id
            first += counts[b]
            sfirst += len(recs)
        tables = [(0, np.asarray(img_rows, dtype=np.int32).reshape(B, TRAIN_PREP_IMG_COLS)),
                  (pan_off, np.asarray(pan_rows, dtype=np.int32).reshape(B, TRAIN_PREP_PAN_COLS)),
                  (seg_off, np.asarray(seg_rows, dtype=np.int32).reshape(S, TRAIN_PREP_SEG_COLS))]
        return n, tables, copies, 'train_prep_panoptic_u8'

    def prep(self, samples, params):
        from . import ops
        spec = self.spec
        _check_batch(samples, params)
        H, W = spec.size
        B = len(samples)
        if _batch_is_panoptic(samples):
            parsed = [_check_pan_sample(s) for s in samples]
            labels_all = [q[4] for q in parsed]
            counts = [int(q[4].shape[0]) for q in parsed]
            layout = self._layout_panoptic
        else:
            parsed = [_check_sample(s, spec) for s in samples]
            labels_all = [q[2] for q in parsed]
            counts = [int(q[1].shape[0]) for q in parsed]
            layout = self._layout_bitmaps
        geoms = [sample_geometry(q[0].shape[:2], p, spec) for q, p in zip(parsed, params)]
        N = sum(counts)
        n, tables, copies, op = layout(parsed, params, geoms, counts)
        self.last_staged_bytes = n                            # tables + raw planes of this call (what the one H2D copy moves)
        img_out = torch.empty((B, 3, H, W), dtype=torch.float32, device=self.device)
        masks_out = torch.empty((N, H, W), dtype=torch.uint8, device=self.device)
        seg_out = torch.empty((B, 1, H, W), dtype=torch.uint8, device=self.device) if spec.with_seg else None
        stats = torch.empty((N, 5), dtype=torch.int32, device=self.device)
        stats_host = torch.empty((N, 5), dtype=torch.int32).pin_memory()
        with torch.cuda.device(self.device):
            slot = self._slot(n)
            stream = torch.cuda.current_stream(self.device)
            host_tables = []
            for off, rows in tables:                         # written into the slot; the views are the host copies the op validates
                t = slot.pinned[off:off + 4 * rows.size].view(torch.int32).view(rows.shape)
                if rows.size:
                    t.numpy()[:] = rows
                host_tables.append(t)
            for off, a in copies:
                np.copyto(slot.host[off:off + a.nbytes].view(a.dtype).reshape(a.shape), a)
            if slot.consumed is not None:
                stream.wait_event(slot.consumed)             # device: the kernels that read this slot last are done (another stream)
            slot.dev[:n].copy_(slot.pinned[:n], non_blocking=True)
            slot.copied = torch.cuda.Event()
            slot.copied.record(stream)
            offsets = [off for off, _ in tables]
            common = dict(to_rgb=spec.to_rgb, crop_size=spec.crop_size, seg_pad=spec.pad_val[2], img_table_offset=offsets[0], staged_bytes=n)
            if op == 'train_prep_panoptic_u8':
                ops.train_prep_panoptic_u8(slot.dev, *host_tables, img_out, masks_out, seg_out, stats, spec.mean, spec.std, spec.pad_val[0],
                                           pan_table_offset=offsets[1], seg_table_offset=offsets[2], **common)
            else:
                ops.train_prep_u8(slot.dev, *host_tables, img_out, masks_out, seg_out, stats, spec.mean, spec.std, spec.pad_val[0],
                                  inst_table_offset=offsets[1], **common)
            slot.consumed = torch.cuda.Event()
            slot.consumed.record(stream)
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
