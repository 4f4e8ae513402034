"""The reference's test pipeline, from raw uint8 images to the float batch the stem reads.

Every reference config prepares a test image with the same [3P] mmdet steps:

    LoadImageFromFile | LoadImageFromWebcam
    MultiScaleFlipAug(img_scale=(1333, 800), flip=False, transforms=[
        Resize(keep_ratio=True), RandomFlip, Pad(size_divisor=32, pad_val=...), Normalize(mean, std, to_rgb=True),
        ImageToTensor, Collect])

followed by the collation of the samples into one batch. This module restates those steps:

    spec = parse_test_pipeline(cfg.data.test.pipeline)      # the steps as one small record (anything else raises)
    batch, img_metas = prepare_host(imgs, spec)             # numpy: the rule written down, and the host way to prepare
    batch, img_metas = ImagePrep(spec, device)(imgs)        # csrc/image_prep.hip: one H2D copy + one launch per batch

THE RULE (what both sides compute; `prepare_host` is its definition, the kernel equals it bit for bit):

1. target size (keep_ratio): f = min(L / max(h, w), S / min(h, w)) with L, S = max / min of img_scale; new = int(x * f + 0.5).
2. per-axis taps for source length s, target length d: scale = 1 / (d / s) in double; fx = float32((k + 0.5) * scale - 0.5) (two
   separately rounded double operations); i = floor(fx), fx -= i; i < 0 -> (0, 0); i >= s - 1 -> (s - 1, 0);
   a0 = rint(float32(1 - fx) * 2048), a1 = rint(fx * 2048) (int16); second tap min(i + 1, s - 1).
3. pixel: R[y][k] = src[y][i] a0 + src[y][i + 1] a1 (int32); out = (((b0 (R[j] >> 4)) >> 16) + ((b1 (R[j + 1] >> 4)) >> 16) + 2) >> 2.
4. BGR -> RGB when to_rgb; v = float32(float32(x - mean_c) * float32(1 / std_c)); Pad at the bottom / right, before Normalize (the
   pad region holds the normalised pad value, a per-channel pad_val is in source channel order) or after it (pad_val itself).
5. collate: the batch has the largest padded shape; beyond an image's own pad_shape the plane is 0.0.

Rules 2 and 3 restate [3P] mmcv `imrescale` on OpenCV's 8-bit INTER_LINEAR from their published description. No cv2 build exists
offline to compare with, so equality with a particular cv2 build is NOT claimed; what is pinned is this rule (tests/test_image_prep.py).
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from ._lib import CggError
from .ops import IMAGE_PREP_TABLE_COLS, three_floats

INTER_BITS = 11            # coefficient fixed point: 2048 = 1.0
TABLE_COLS = IMAGE_PREP_TABLE_COLS   # descriptor row: byte offset, h, w, row pitch, new_h, new_w, pad_h, pad_w (int32)


@dataclass(frozen=True)
class PrepSpec:
    """One reference test pipeline. `img_scale` is (w, h) as in the configs; `size_divisor` / `size` as [3P] mmdet Pad takes them (both
    None: no Pad step); `pad_val` a number or three of them; mean / std in the channel order AFTER `to_rgb`."""
    img_scale: Tuple[int, int] = (1333, 800)
    keep_ratio: bool = True
    size_divisor: Optional[int] = 32
    size: Optional[Tuple[int, int]] = None
    pad_val: object = 0
    mean: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    std: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    to_rgb: bool = False
    pad_before_norm: bool = True


_LOADERS = ('LoadImageFromFile', 'LoadImageFromWebcam')
_PASSIVE = ('ImageToTensor', 'DefaultFormatBundle', 'Collect')


def _unsupported(step, why):
    return CggError(f'test pipeline: {step}: {why} (image_prep restates Resize / RandomFlip(no flip) / Pad / Normalize under one '
                    'MultiScaleFlipAug with one scale)')


def parse_test_pipeline(pipeline):
    """A reference-style `cfg.data.test.pipeline` (list of dicts with a `type`) -> PrepSpec. Raises CggError naming the transform
    for anything this build does not restate: more than one scale, flip=True, an interpolation other than bilinear, an unknown step."""
    if not isinstance(pipeline, (list, tuple)) or not pipeline:
        raise CggError('test pipeline: expected a non-empty list of transform dicts')
    aug = None
    for step in pipeline:
        t = step.get('type') if hasattr(step, 'get') else None
        if t in _LOADERS:
            continue
        if t == 'MultiScaleFlipAug':
            if aug is not None:
                raise _unsupported(t, 'appears twice')
            aug = step
            continue
        raise _unsupported(str(t), 'unknown top-level transform')
    if aug is None:
        raise _unsupported('MultiScaleFlipAug', 'missing')
    if aug.get('scale_factor') is not None:
        raise _unsupported('MultiScaleFlipAug', 'scale_factor is not restated, give img_scale')
    scale = aug.get('img_scale')
    if isinstance(scale, (list, tuple)) and scale and isinstance(scale[0], (list, tuple)):
        if len(scale) != 1:
            raise _unsupported('MultiScaleFlipAug', f'{len(scale)} scales (test-time augmentation is out of scope)')
        scale = scale[0]
    if not isinstance(scale, (list, tuple)) or len(scale) != 2 or min(scale) < 1:
        raise _unsupported('MultiScaleFlipAug', f'img_scale={scale!r}')
    if aug.get('flip', False):
        raise _unsupported('MultiScaleFlipAug', 'flip=True (test-time augmentation is out of scope)')
    kw = dict(img_scale=(int(scale[0]), int(scale[1])), size_divisor=None, size=None)
    seen = []
    for step in aug.get('transforms', []):
        t = step.get('type') if hasattr(step, 'get') else None
        if t in seen and t not in _PASSIVE:
            raise _unsupported(str(t), 'appears twice')
        seen.append(t)
        if t == 'Resize':
            interp = step.get('interpolation', 'bilinear')
            if interp != 'bilinear':
                raise _unsupported('Resize', f'interpolation={interp!r}')
            if step.get('img_scale') is not None or step.get('ratio_range') is not None or step.get('multiscale_mode', 'range') != 'range':
                raise _unsupported('Resize', 'a scale of its own (training-time jitter is out of scope)')
            if step.get('backend', 'cv2') != 'cv2':
                raise _unsupported('Resize', f'backend={step.get("backend")!r}')
            kw['keep_ratio'] = bool(step.get('keep_ratio', True))
        elif t == 'RandomFlip':
            pass                       # under MultiScaleFlipAug the flip is the aug's decision, and flip=True was refused above
        elif t == 'Pad':
            if 'Resize' not in seen:
                raise _unsupported('Pad', 'precedes Resize')
            if step.get('pad_to_square', False):
                raise _unsupported('Pad', 'pad_to_square')
            size, div = step.get('size'), step.get('size_divisor')
            if (size is None) == (div is None):
                raise _unsupported('Pad', 'exactly one of size / size_divisor is required')
            kw['size'] = None if size is None else (int(size[0]), int(size[1]))
            kw['size_divisor'] = None if div is None else int(div)
            pv = step.get('pad_val', 0)
            pv = pv.get('img', 0) if hasattr(pv, 'get') else pv
            kw['pad_val'] = tuple(float(x) for x in pv) if isinstance(pv, (list, tuple)) else float(pv)
            kw['pad_before_norm'] = 'Normalize' not in seen
        elif t == 'Normalize':
            if 'Resize' not in seen:
                raise _unsupported('Normalize', 'precedes Resize')
            kw['mean'] = three_floats(step.get('mean', 0.0), 'test pipeline: Normalize.mean')
            kw['std'] = three_floats(step.get('std', 1.0), 'test pipeline: Normalize.std')
            kw['to_rgb'] = bool(step.get('to_rgb', True))
        elif t in _PASSIVE:
            pass
        else:
            raise _unsupported(str(t), 'unknown transform')
    if 'Resize' not in seen:
        raise _unsupported('Resize', 'missing')
    if not isinstance(kw.get('pad_val', 0), tuple):
        kw['pad_val'] = float(kw.get('pad_val', 0))
    elif len(kw['pad_val']) != 3:
        raise _unsupported('Pad', f'pad_val with {len(kw["pad_val"])} entries')
    return PrepSpec(**kw)


# ---- rules 1-3 -------------------------------------------------------------------------------------------------------------------
def rescale_size(hw, img_scale, keep_ratio=True):
    """(h, w) of the source -> (new_h, new_w) ([3P] mmcv rescale_size; img_scale is (w, h) when the ratio is not kept)."""
    h, w = int(hw[0]), int(hw[1])
    if h < 1 or w < 1:
        raise CggError(f'image_prep: a zero-sized image ({h} x {w})')
    if not keep_ratio:
        return int(img_scale[1]), int(img_scale[0])
    L, S = max(img_scale), min(img_scale)
    f = min(L / max(h, w), S / min(h, w))
    return int(h * f + 0.5), int(w * f + 0.5)


def resize_coefficients(s, d):
    """Rule 2 for one axis: (i0, i1, a0, a1), int32 arrays of length d -- the two taps and their 11-bit weights."""
    scale = 1.0 / (float(d) / float(s))
    k = np.arange(d, dtype=np.float64)
    fx = ((k + 0.5) * scale - 0.5).astype(np.float32)           # numpy rounds the product and the difference separately
    fl = np.floor(fx)
    i = fl.astype(np.int64)
    fx = (fx - fl).astype(np.float32)
    lo, hi = i < 0, i >= s - 1
    i = np.where(lo, 0, np.where(hi, s - 1, i))
    fx = np.where(lo | hi, np.float32(0), fx).astype(np.float32)
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int16)
    a1 = np.rint(fx * np.float32(2048)).astype(np.int16)
    return i.astype(np.int32), np.minimum(i + 1, s - 1).astype(np.int32), a0.astype(np.int32), a1.astype(np.int32)


def resize_u8(img, new_h, new_w):
    """Rules 2 and 3: (h, w, C) uint8 -> (new_h, new_w, C) uint8."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise CggError(f'image_prep: expected an (h, w, C) uint8 image (got {img.dtype}, shape {img.shape})')
    h, w = img.shape[:2]
    xi0, xi1, xa0, xa1 = resize_coefficients(w, new_w)
    yi0, yi1, yb0, yb1 = resize_coefficients(h, new_h)
    s = img.astype(np.int32)
    R = (s[:, xi0] * xa0[None, :, None] + s[:, xi1] * xa1[None, :, None]) >> 4
    out = (((yb0[:, None, None] * R[yi0]) >> 16) + ((yb1[:, None, None] * R[yi1]) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255, 'rule 3 left the 8-bit range'
    return out.astype(np.uint8)


# ---- rules 4-5 -------------------------------------------------------------------------------------------------------------------
def norm_constants(spec):
    """float32 (mean, 1 / std, value of the pad region) per OUTPUT plane: the constants both sides use."""
    mean = np.asarray(spec.mean, dtype=np.float32)
    rstd = (1.0 / np.asarray(spec.std, dtype=np.float64)).astype(np.float32)
    pad = np.asarray(spec.pad_val if isinstance(spec.pad_val, tuple) else (spec.pad_val,) * 3, dtype=np.float32)
    if spec.pad_before_norm:
        if spec.to_rgb:
            pad = pad[::-1]
        pad = ((pad - mean) * rstd).astype(np.float32)
    return mean, rstd, pad


def image_geometry(hw, spec):
    """(new_h, new_w, pad_h, pad_w) of one image."""
    nh, nw = rescale_size(hw, spec.img_scale, spec.keep_ratio)
    if spec.size is not None:
        ph, pw = spec.size
        if ph < nh or pw < nw:
            raise CggError(f'image_prep: Pad size {spec.size} is smaller than the resized image ({nh}, {nw})')
    elif spec.size_divisor is not None:
        dv = spec.size_divisor
        ph, pw = -(-nh // dv) * dv, -(-nw // dv) * dv
    else:
        ph, pw = nh, nw
    return nh, nw, ph, pw


def image_meta(hw, spec, geom=None):
    """The meta keys the reference's `Collect` carries (data_contract.META_KEYS), for an image given as an array."""
    h, w = int(hw[0]), int(hw[1])
    nh, nw, ph, pw = geom or image_geometry(hw, spec)
    return dict(filename=None, ori_filename=None, ori_shape=(h, w, 3), img_shape=(nh, nw, 3), pad_shape=(ph, pw, 3),
                scale_factor=np.array([nw / w, nh / h, nw / w, nh / h], dtype=np.float32), flip=False, flip_direction=None,
                img_norm_cfg=dict(mean=np.asarray(spec.mean, dtype=np.float32), std=np.asarray(spec.std, dtype=np.float32),
                                  to_rgb=spec.to_rgb))


def _as_hwc_u8(img, keep_device=False):
    """numpy view of one source image; with `keep_device` a device tensor comes back as it is (ImagePrep copies it on the device)."""
    if torch.is_tensor(img):
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise CggError(f'image_prep: expected an (h, w, 3) uint8 image (got {img.dtype}, shape {tuple(img.shape)})')
        if keep_device and img.is_cuda:
            return img
        return img.cpu().numpy()
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise CggError(f'image_prep: expected an (h, w, 3) uint8 image (got {img.dtype}, shape {img.shape})')
    return img


def prepare_host(imgs, spec):
    """Rules 1-5 in numpy: list of (h, w, 3) uint8 images -> ((B, 3, Hb, Wb) float32 array, img_metas)."""
    if not isinstance(imgs, (list, tuple)) or not imgs:
        raise CggError('image_prep: expected a non-empty list of images')
    imgs = [_as_hwc_u8(i) for i in imgs]
    geoms = [image_geometry(i.shape[:2], spec) for i in imgs]
    Hb, Wb = max(g[2] for g in geoms), max(g[3] for g in geoms)
    mean, rstd, pad = norm_constants(spec)
    batch = np.zeros((len(imgs), 3, Hb, Wb), dtype=np.float32)
    metas = []
    for b, (img, (nh, nw, ph, pw)) in enumerate(zip(imgs, geoms)):
        r = resize_u8(img, nh, nw)
        if spec.to_rgb:
            r = r[:, :, ::-1]
        v = ((r.astype(np.float32) - mean) * rstd).astype(np.float32)
        batch[b, :, :ph, :pw] = pad[:, None, None]
        batch[b, :, :nh, :nw] = v.transpose(2, 0, 1)
        metas.append(image_meta(img.shape[:2], spec, (nh, nw, ph, pw)))
    return batch, metas


# ---- the device side -------------------------------------------------------------------------------------------------------------
class _Slot:
    __slots__ = ('pinned', 'host', 'dev', 'copied', 'consumed')

    def __init__(self, nbytes, device):
        self.pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.host = self.pinned.numpy()
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.copied = None          # event behind the slot's last H2D copy: the pinned bytes may be overwritten after it
        self.consumed = None        # event behind the slot's last kernel: the device bytes may be overwritten after it


class _StagingRing:
    """`slots` staging slots used in rotation, and the events that let a slot be used again without a synchronisation. Per batch:
    `acquire` a slot, fill its pinned bytes, `upload` them, launch what reads the device bytes, `release`."""

    def __init__(self, device, slots, who):
        if slots < 1:
            raise CggError(f'{who}: slots must be >= 1')
        self.device = device
        self.slots = [None] * slots
        self.n = 0                  # batches so far: batch i takes slot i % len(slots)

    def acquire(self, nbytes):
        """the next slot, of at least `nbytes`, its pinned bytes free to be overwritten"""
        k = self.n % len(self.slots)
        self.n += 1
        slot = self.slots[k]
        if slot is not None and slot.copied is not None:
            slot.copied.synchronize()                        # host: the pinned bytes have left
        if slot is None or slot.pinned.numel() < nbytes:
            if slot is not None and slot.consumed is not None:
                torch.cuda.current_stream(self.device).wait_event(slot.consumed)
            slot = self.slots[k] = _Slot(max(1 << 16, 1 << (nbytes - 1).bit_length()), self.device)
        return slot

    def upload(self, slot, n, stream):
        """the ONE H2D copy of the batch: the slot's first `n` pinned bytes to its device bytes, on `stream`"""
        if slot.consumed is not None:
            stream.wait_event(slot.consumed)                 # device: the kernels that read this slot last are done (another stream)
        slot.dev[:n].copy_(slot.pinned[:n], non_blocking=True)
        slot.copied = torch.cuda.Event()
        slot.copied.record(stream)

    def release(self, slot, stream):
        """after the last launch that reads the slot's device bytes"""
        slot.consumed = torch.cuda.Event()
        slot.consumed.record(stream)


class ImagePrep:
    """Device-side test pipeline: `prep(imgs) -> (batch (B, 3, Hb, Wb) float32 on `device`, img_metas)`, equal to `prepare_host`.

    `imgs`: (h, w, 3) uint8 numpy arrays or CPU / device uint8 tensors (BGR, as cv2 / the reference's loaders give them). One call =
    one host copy into a pinned staging slot (descriptor table + the raw images back to back), ONE asynchronous H2D copy and ONE
    kernel launch on the current stream; nothing synchronises unless all `slots` staging buffers are still in flight. (An image that
    is already a device tensor is copied into the device buffer on the device instead of being staged.) There is no CPU path: a
    non-ROCm device raises (use `prepare_host` to prepare on the host, explicitly)."""

    def __init__(self, spec, device, slots=3):
        device = torch.device(device)
        if device.type != 'cuda' or not torch.cuda.is_available():
            raise CggError(f'ImagePrep needs a ROCm device (got {device}); prepare_host is the host-side form of the same rule')
        if not isinstance(spec, PrepSpec):
            spec = parse_test_pipeline(spec)
        self.spec, self.device = spec, device
        self._ring = _StagingRing(device, slots, 'ImagePrep')

    def describe(self, imgs):
        """((B, 3, Hb, Wb), img_metas) of the batch `self(imgs)` would return; no device work."""
        srcs, geoms = self._plan(imgs)
        shape = (len(srcs), 3, max(g[2] for g in geoms), max(g[3] for g in geoms))
        return shape, [image_meta(s.shape[:2], self.spec, g) for s, g in zip(srcs, geoms)]

    def _plan(self, imgs):
        if not isinstance(imgs, (list, tuple)) or not imgs:
            raise CggError('ImagePrep: expected a non-empty list of images')
        srcs = [_as_hwc_u8(i, keep_device=True) for i in imgs]
        return srcs, [image_geometry(s.shape[:2], self.spec) for s in srcs]

    def __call__(self, imgs, out=None):
        from . import ops
        spec = self.spec
        srcs, geoms = self._plan(imgs)
        B = len(srcs)
        Hb, Wb = max(g[2] for g in geoms), max(g[3] for g in geoms)
        table_bytes = 4 * TABLE_COLS * B
        offs, n = [], table_bytes
        for s in srcs:
            offs.append(n)
            n += int(s.shape[0]) * int(s.shape[1]) * 3
        if out is None:
            out = torch.empty((B, 3, Hb, Wb), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (B, 3, Hb, Wb):
            raise CggError(f'ImagePrep: out must be {(B, 3, Hb, Wb)} for this batch (got {tuple(out.shape)})')
        with torch.cuda.device(self.device):
            slot = self._ring.acquire(n)
            stream = torch.cuda.current_stream(self.device)
            table = slot.host[:table_bytes].view(np.int32).reshape(B, TABLE_COLS)
            on_device = []
            for b, (s, off, (nh, nw, ph, pw)) in enumerate(zip(srcs, offs, geoms)):
                h, w = int(s.shape[0]), int(s.shape[1])
                table[b] = (off, h, w, 3 * w, nh, nw, ph, pw)
                if torch.is_tensor(s):
                    on_device.append((s, off, h, w))
                else:
                    np.copyto(slot.host[off:off + h * w * 3].reshape(h, w, 3), s)
            self._ring.upload(slot, n, stream)
            for s, off, h, w in on_device:
                slot.dev[off:off + h * w * 3].view(h, w, 3).copy_(s, non_blocking=True)
            ops.image_prep_u8(slot.dev, slot.pinned[:table_bytes].view(torch.int32).view(B, TABLE_COLS), out, spec.mean, spec.std,
                              spec.pad_val, to_rgb=spec.to_rgb, pad_before_norm=spec.pad_before_norm, table_offset=0, staged_bytes=n)
            self._ring.release(slot, stream)
        metas = [image_meta(s.shape[:2], spec, g) for s, g in zip(srcs, geoms)]
        return out, metas
