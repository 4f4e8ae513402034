"""Drawing a result over its image: `MaskFormerOpen.show_result` / `_show_pan_result` ([3P] open_set/models/maskformer.py:228-382,
open_set/core/visualization/image.py) without mmcv, cv2 or pycocotools, and with the masks never leaving the device.

The `*_host` functions are plain numpy. They are the specification of the kernels of csrc/paint.hip (which equal them bit for
bit), the route taken outside the kernels' gates, and the comparison side of the tests.

Three rules:
  fill    the reference's one numpy line (image.py:199), `img[mask] = img[mask] * (1 - alpha) + color * alpha`: uint8 through
          float64 and truncated back, mask after mask, so the order decides the value where masks overlap. Matched exactly
          (tests/golden/g12_paint.npz comes from the reference's own `draw_masks`).
  edges   THIS BUILD'S RULE (the reference rasterises matplotlib contour polygons with anti-aliasing, which no pixel rule
          reproduces): a pixel of a kept mask with a four-neighbour outside that mask (outside the image counts as outside the
          mask) is blended once, after all fills, with white at alpha 0.8.
  boxes   THIS BUILD'S RULE: the pixels of the truncated box x0..x1, y0..y1 nearer than `thickness` to one of its sides are
          blended once with the box colour at alpha 0.8, box after box. Pixels outside the image are not drawn.
Text is drawn on the host with PIL and is outside any parity claim.
"""
import numpy as np
import torch

from ._lib import CggError

INSTANCE_OFFSET = 1000      # [3P] mmdet.core.evaluation.panoptic_utils.INSTANCE_OFFSET
EDGE_ALPHA = 0.8
COMPONENT_CAPACITY = 4096   # records the device labelling may return before the host rule takes over

_COLOR_NAMES = dict(red=(0, 0, 255), green=(0, 255, 0), blue=(255, 0, 0), cyan=(255, 255, 0), yellow=(0, 255, 255),
                    magenta=(255, 0, 255), white=(255, 255, 255), black=(0, 0, 0))      # [3P] mmcv.Color (BGR)


# ---- colours ---------------------------------------------------------------------------------------------------------------------
def get_palette(palette, num_classes):
    """[3P] mmdet.core.visualization.get_palette for the forms `show_result` takes: None (the seeded random palette), one colour
    (a triplet or an mmcv colour name) for every class, or a list of colours, one per class -> (num_classes, 3) uint8."""
    n = int(num_classes)
    if palette is None:
        return np.random.RandomState(42).randint(0, 256, size=(n, 3)).astype(np.uint8)
    if isinstance(palette, str):
        if palette not in _COLOR_NAMES:
            raise CggError(f'get_palette: unknown colour name {palette!r} (known: {sorted(_COLOR_NAMES)})')
        palette = _COLOR_NAMES[palette]
    arr = np.asarray(palette)
    if arr.ndim == 1 and arr.size == 3:
        arr = np.tile(arr[None], (n, 1))
    if arr.ndim != 2 or arr.shape[1] != 3 or arr.shape[0] < n:
        raise CggError(f'get_palette: one colour or a list of at least {n} colours expected (got shape {arr.shape})')
    return arr[:n].astype(np.uint8)


def instance_colors_host(labels, palette=None, seed=0):
    """The reference's colour choice for masks (image.py:63-78, 193-196): the class colour `palette[label]`; a colour already taken
    is moved by clip(c + randint(-30, 31, 3), 0, 255) until it is free. The reference draws from numpy's global unseeded state;
    here the draws come from RandomState(seed), one of its possible outcomes. -> (n, 3) uint8, applied to the image's channels
    in stored order."""
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    if palette is None or not (isinstance(palette, np.ndarray) and palette.ndim == 2):
        palette = get_palette(palette, int(labels.max()) + 1 if labels.size else 0)
    rs = np.random.RandomState(seed)
    taken = set()
    out = np.zeros((labels.size, 3), np.uint8)
    for i, label in enumerate(labels.tolist()):
        c = palette[label].astype(np.int64)
        while tuple(c.tolist()) in taken:
            c = np.clip(c + rs.randint(-30, 31, size=3), 0, 255)
        taken.add(tuple(c.tolist()))
        out[i] = c
    return out


def adaptive_scales(areas, min_area=800, max_area=30000):
    """`_get_adaptive_scales` (image.py:40-60): the text scale, 0.5 at `min_area` and below, 1.0 at `max_area` and above."""
    areas = np.asarray(areas)
    return np.clip(0.5 + (areas - min_area) / (max_area - min_area), 0.5, 1.0)


# ---- the pixel rules ----------------------------------------------------------------------------------------------------------
def _blend(img, sel, color, alpha):
    """the reference line; `sel` indexes pixels, `color` is a uint8 triplet"""
    img[sel] = img[sel] * (1 - alpha) + np.asarray(color, dtype=np.uint8) * alpha


def unpack_masks_host(masks, width):
    """(n, H, W) bool, or the bit-packed (n, H, row_bytes) uint8 of `mask_bits=True` (pixel x = bit x & 7 of byte x >> 3; bits
    past `width` are undefined and ignored) -> (n, H, width) bool."""
    masks = np.asarray(masks)
    if masks.dtype == np.uint8 and masks.ndim == 3 and masks.shape[2] * 8 >= width:        # the dtype decides: uint8 is packed
        return np.unpackbits(masks, axis=-1, bitorder='little')[:, :, :width].astype(bool)
    if masks.ndim != 3 or masks.shape[2] != width:
        raise CggError(f'masks: (n, H, {width}) bool or (n, H, >= {(width + 7) // 8}) bit-packed uint8 expected, got {masks.shape} '
                       f'{masks.dtype}')
    return masks.astype(bool)


def truncate_boxes(boxes):
    """(n, 4 or 5) floats -> (n, 4) int32, truncated as `draw_bboxes` does (`astype(np.int32)`)"""
    b = np.asarray(boxes, dtype=np.float64)
    b = b.reshape(-1, b.shape[-1] if b.ndim == 2 else 4)[:, :4]
    return np.clip(np.nan_to_num(b), -2.0**30, 2.0**30).astype(np.int32)


def _edge_of(m):
    p = np.pad(m, 1)
    return m & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def paint_instances_host(img, masks, colors, keep=None, boxes=None, box_colors=None, alpha=0.8, thickness=2, edges=True):
    """img (H, W, 3) uint8; masks (n, H, W) bool or bit-packed (n, H, row_bytes) uint8; colors (n, 3) uint8; keep (n) or None = all;
    boxes (n, 4 or 5) with box_colors (n, 3), or None -> the painted copy: fills in index order, then the edge pixels once, then
    the box frames in index order (the module docstring states the three rules)."""
    img = np.array(img, dtype=np.uint8, copy=True)
    if img.ndim != 3 or img.shape[2] != 3:
        raise CggError(f'paint_instances_host: (H, W, 3) uint8 image expected, got {img.shape}')
    H, W, _ = img.shape
    masks = np.asarray(masks)
    n = masks.shape[0]
    masks = unpack_masks_host(masks, W) if n else np.zeros((0, H, W), bool)
    colors = np.asarray(colors, dtype=np.uint8).reshape(n, 3)
    keep = np.ones(n, bool) if keep is None else np.asarray(keep).astype(bool).reshape(n)
    edge = np.zeros((H, W), bool)
    for i in range(n):
        if not keep[i]:
            continue
        _blend(img, masks[i], colors[i], alpha)
        if edges:
            edge |= _edge_of(masks[i])
    if edges:
        _blend(img, edge, (255, 255, 255), EDGE_ALPHA)
    if boxes is not None and n:
        ib = truncate_boxes(boxes).astype(np.int64)
        box_colors = np.asarray(box_colors, dtype=np.uint8).reshape(n, 3)
        t = int(thickness)
        for i in range(n):
            if not keep[i]:
                continue
            x0, y0, x1, y1 = ib[i].tolist()
            xa, xb, ya, yb = max(x0, 0), min(x1, W - 1), max(y0, 0), min(y1, H - 1)
            if xa > xb or ya > yb:
                continue
            yy, xx = np.mgrid[ya:yb + 1, xa:xb + 1]
            sel = (xx - x0 < t) | (x1 - xx < t) | (yy - y0 < t) | (y1 - yy < t)
            region = img[ya:yb + 1, xa:xb + 1]
            _blend(region, sel, box_colors[i], EDGE_ALPHA)
    return img


def components_host(pan, void):
    """The 8-connected components of equal non-void id in an (H, W) integer map -> int64 (k, 5) records
    [root, id, area, sum_x, sum_y], sorted by root = the smallest linear index y * W + x of the component. (Row runs joined by
    union-find; no scipy.)"""
    pan = np.asarray(pan)
    if pan.ndim != 2:
        raise CggError(f'components_host: (H, W) map expected, got {pan.shape}')
    H, W = pan.shape
    parent, r_y, r_s, r_e, r_id = [], [], [], [], []

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    prev = []                       # run indices of the row above
    for y in range(H):
        row = pan[y]
        cuts = np.flatnonzero(row[1:] != row[:-1]) + 1
        starts = np.concatenate(([0], cuts)).tolist()
        ends = np.concatenate((cuts, [W])).tolist()
        ids = row[starts].tolist()
        cur = []
        j = 0
        for s, e, v in zip(starts, ends, ids):
            if v == void:
                continue
            k = len(parent)
            parent.append(k)
            r_y.append(y), r_s.append(s), r_e.append(e), r_id.append(v)
            cur.append(k)
            while j < len(prev) and r_e[prev[j]] < s:          # ends left of s - 1: not even diagonal
                j += 1
            q = j
            while q < len(prev) and r_s[prev[q]] <= e:         # starts at e at the latest (diagonal)
                if r_id[prev[q]] == v:
                    a, b = find(k), find(prev[q])
                    if a != b:
                        parent[max(a, b)] = min(a, b)          # runs are in raster order: the smallest run holds the root pixel
                q += 1
        prev = cur
    acc = {}
    for k in range(len(parent)):
        r = find(k)
        n = r_e[k] - r_s[k]
        a = acc.setdefault(r, [r_y[r] * W + r_s[r], r_id[r], 0, 0, 0])
        a[2] += n
        a[3] += (r_s[k] + r_e[k] - 1) * n // 2
        a[4] += r_y[k] * n
    rec = np.array(sorted(acc.values()), dtype=np.int64).reshape(-1, 5)
    return rec


def largest_components(records):
    """One record per id: its component of largest area, ties to the smallest root -- what np.argmax over
    cv2.connectedComponentsWithStats' raster-ordered labels picks (image.py:335-339). Sorted by id. The centroid of a record
    is (sum_x / area, sum_y / area) in float64."""
    rec = np.asarray(records, dtype=np.int64).reshape(-1, 5)
    order = np.lexsort((rec[:, 0], -rec[:, 2], rec[:, 1]))           # by id, then area descending, then root
    rec = rec[order]
    first = np.ones(len(rec), bool)
    first[1:] = rec[1:, 1] != rec[:-1, 1]
    return rec[first]


def paint_panoptic_host(img, pan, ids, colors, void, alpha=0.8, edges=True):
    """img (H, W, 3) uint8, pan (H, W) integer map: every pixel whose id is in `ids` (never `void`) is blended once with its id's
    colour; a painted pixel with a four-neighbour of another id, or on the frame, is then blended once with white at 0.8."""
    img = np.array(img, dtype=np.uint8, copy=True)
    pan = np.asarray(pan).astype(np.int64)
    ids = np.asarray(ids).astype(np.int64).reshape(-1)
    colors = np.asarray(colors, dtype=np.uint8).reshape(ids.size, 3)
    painted = np.zeros(pan.shape, bool)
    for k, v in enumerate(ids.tolist()):
        if v == void:
            continue
        m = pan == v
        _blend(img, m, colors[k], alpha)
        painted |= m
    if edges:
        p = np.pad(pan, 1, constant_values=-(1 << 62))
        same = (p[:-2, 1:-1] == pan) & (p[2:, 1:-1] == pan) & (p[1:-1, :-2] == pan) & (p[1:-1, 2:] == pan)
        _blend(img, painted & ~same, (255, 255, 255), EDGE_ALPHA)
    return img


# ---- results -> what to draw ------------------------------------------------------------------------------------------------------
def _load_image(img):
    """file name | (h, w, 3) uint8 array | tensor -> the image as the caller holds it (numpy or tensor), uint8 (h, w, 3)"""
    if isinstance(img, str):
        from .apis import _read_image
        img = _read_image(img)
    if torch.is_tensor(img):
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise CggError(f'show_result: (h, w, 3) uint8 image expected, got {tuple(img.shape)} {img.dtype}')
        return img
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise CggError(f'show_result: (h, w, 3) uint8 image expected, got {img.shape} {img.dtype}')
    return img


def _model_device(model):
    try:
        dev = next(model.parameters()).device
    except StopIteration:
        return None
    return dev if dev.type == 'cuda' else None


def _fits_int32(pan):
    """whether every id of the map survives the conversion to the kernels' int32 (asked BEFORE the conversion; a device map of a
    wider type costs one small read, the fusion head's own maps are int32 and cost none)"""
    if torch.is_tensor(pan):
        if pan.dtype in (torch.int32, torch.int16, torch.int8, torch.uint8) or pan.numel() == 0:
            return True
        lo, hi = torch.aminmax(pan)
        return bool(lo >= -(1 << 31)) and bool(hi < (1 << 31))
    pan = np.asarray(pan)
    if pan.dtype.kind not in 'iu':
        return False
    return pan.size == 0 or (int(pan.min()) >= -(1 << 31) and int(pan.max()) < (1 << 31))


def _host_image(img):
    return img.cpu().numpy() if torch.is_tensor(img) else img


def _device_image(img, dev):
    t = img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img))
    return t.to(dev).contiguous()


def instance_draw_list(result, score_thr):
    """`result['all_results']` in the host form (per-class lists) or the device form (labels, boxes (n, 5), masks) ->
    (labels (n) int64, boxes (n, 5) float, masks, order, keep): `masks` as the result holds them (a list of host arrays, or the
    device tensor, untouched), `order` the position in `masks` of every drawn instance in the reference's order (by class, within
    a class in result order), `keep` the reference's filter (`scores > score_thr` when score_thr > 0) in that order."""
    all_result = result['all_results']
    if len(all_result) == 3 and torch.is_tensor(all_result[0]):
        labels_t, boxes_t, masks = all_result
        n = labels_t.numel()
        # labels, scores and boxes in ONE small copy through a pinned buffer (labels are small integers: exact in float64)
        small = torch.cat([labels_t.reshape(n, 1).to(torch.float64), boxes_t.reshape(n, boxes_t.shape[-1]).to(torch.float64)], dim=1)
        host = torch.empty(small.shape, dtype=torch.float64, pin_memory=small.is_cuda)
        host.copy_(small)
        host = host.numpy()
        labels, boxes = host[:, 0].astype(np.int64), host[:, 1:].astype(np.float32)
        order = np.argsort(labels, kind='stable')
    else:
        bbox_result, segm_result = all_result
        boxes = np.vstack(bbox_result) if len(bbox_result) else np.zeros((0, 5), np.float32)
        labels = np.concatenate([np.full(b.shape[0], i, dtype=np.int64) for i, b in enumerate(bbox_result)]) \
            if len(bbox_result) else np.zeros(0, np.int64)
        masks = [m for per_class in segm_result for m in per_class] if segm_result is not None else []
        order = np.arange(len(labels))
        if len(masks) != len(labels):
            raise CggError(f'show_result: {len(labels)} boxes but {len(masks)} masks')
    labels, boxes = labels[order], boxes[order]
    if score_thr > 0:
        if boxes.shape[1] != 5:
            raise CggError('show_result: score_thr > 0 needs (n, 5) boxes')
        keep = boxes[:, 4] > score_thr
    else:
        keep = np.ones(len(labels), bool)
    return labels, boxes, masks, order, keep


def draw_labels(img, texts, positions, colors, font_size, scales, center=False):
    """Text on the host with PIL, each label on a black box; (h, w, 3) uint8 -> a new array. Outside the parity claim."""
    try:
        from PIL import Image, ImageDraw, ImageFont
    except ImportError:
        raise CggError('show_result: drawing labels needs PIL, which is not importable here; pass show_labels=False')
    pil = Image.fromarray(np.ascontiguousarray(img))
    draw = ImageDraw.Draw(pil)
    for text, pos, color, scale in zip(texts, positions, colors, scales):
        size = max(float(font_size) * float(scale), 1.0)
        try:
            font = ImageFont.load_default(size=size)
        except TypeError:                                     # an older Pillow: one bitmap size only
            font = ImageFont.load_default()
        x, y = float(pos[0]), float(pos[1])
        l, t, r, b = draw.textbbox((x, y), text, font=font)
        if center:
            dx = (r - l) / 2
            x, l, r = x - dx, l - dx, r - dx
        draw.rectangle((l - 1, t - 1, r + 1, b + 1), fill=(0, 0, 0))
        draw.text((x, y), text, fill=tuple(int(c) for c in color), font=font)
    return np.asarray(pil).copy()


def _finish(img, show, wait_time, out_file, win_name):
    if out_file is not None:
        try:
            from PIL import Image
        except ImportError:
            raise CggError('show_result: writing out_file needs PIL, which is not importable here')
        import os
        d = os.path.dirname(os.path.abspath(out_file))
        os.makedirs(d, exist_ok=True)
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(out_file)     # stored channel order BGR -> the file's RGB
        show = False
    if show:
        try:
            import matplotlib.pyplot as plt
        except ImportError:
            raise CggError('show_result: show=True needs matplotlib, which is not importable here; use out_file, or take the '
                           'returned array')
        plt.figure(win_name)
        plt.imshow(img)
        plt.axis('off')
        if wait_time == 0:
            plt.show()
        else:
            plt.show(block=False)
            plt.pause(wait_time)
        plt.close()
    if not (show or out_file):
        return img
    return None


def _class_text(model, label):
    names = getattr(model, 'CLASSES', None)
    return str(names[label]) if names is not None else f'class {label}'


def show_instances(model, img, result, score_thr=0.3, bbox_color=(72, 101, 241), text_color=(72, 101, 241), mask_color=None,
                   thickness=2, font_size=13, win_name='', show=False, wait_time=0, out_file=None, show_labels=True, seed=0):
    """`MaskFormerOpen.show_result` (maskformer.py:228-309 -> imshow_det_bboxes): see the method's docstring."""
    from . import ops
    img = _load_image(img)
    labels, boxes, masks, order, keep = instance_draw_list(result, score_thr)
    n = len(labels)
    max_label = int(labels.max()) if n else 0
    mask_colors = np.zeros((n, 3), np.uint8)
    # the reference colours the instances that passed the filter, in order: the draws of dropped ones never happen
    mask_colors[keep] = instance_colors_host(labels[keep], get_palette(mask_color, max_label + 1), seed=seed)
    box_colors = get_palette(bbox_color, max_label + 1)[labels] if n else np.zeros((0, 3), np.uint8)
    dev = _model_device(model)
    if torch.is_tensor(masks) and masks.is_cuda:
        dev = masks.device
    H, W = img.shape[:2]
    painted = None
    if dev is not None and n <= ops.PAINT_MAX_MASKS and H * W * 3 <= ops.PAINT_MAX_IMAGE_BYTES:
        if torch.is_tensor(masks):
            m = masks.to(dev)
        else:
            m = torch.from_numpy(np.stack(masks).astype(bool) if n else np.zeros((0, H, W), bool)).to(dev)
        if tuple(m.shape[:2]) != (n, H):
            raise CggError(f'show_result: masks of shape {tuple(m.shape)} for {n} instances on a {H} x {W} image')
        bits = ops.pack_bool_masks(m) if m.dtype == torch.bool else m
        if n and not np.array_equal(order, np.arange(n)):
            bits = bits.index_select(0, torch.from_numpy(order).to(dev))
        dimg = _device_image(img, dev)
        if ops.paint_instances_ok(dimg, bits):
            small = np.concatenate([keep.astype(np.uint8).reshape(n, 1), mask_colors, box_colors], axis=1)      # one upload
            small = torch.from_numpy(np.ascontiguousarray(small)).to(dev)
            dboxes = torch.from_numpy(truncate_boxes(boxes) if n else np.zeros((0, 4), np.int32)).to(dev)
            painted = ops.paint_instances(dimg, bits, small[:, 0].contiguous(), small[:, 1:4].contiguous(), dboxes,
                                          small[:, 4:7].contiguous(), alpha=0.8, thickness=thickness).cpu().numpy()
    if painted is None:                                       # outside the kernel's gate, or no device: the host rule
        if torch.is_tensor(masks):
            hm = masks.cpu().numpy()[order]
        else:
            hm = np.stack(masks) if n else np.zeros((0, H, W), bool)
        painted = paint_instances_host(_host_image(img), hm, mask_colors, keep, boxes if n else None, box_colors,
                                       alpha=0.8, thickness=thickness)
    if show_labels and keep.any():
        text_palette = get_palette(text_color, max_label + 1)
        kb = boxes[keep]
        texts = [_class_text(model, int(l)) + (f'|{b[4]:.02f}' if kb.shape[1] == 5 else '') for l, b in zip(labels[keep], kb)]
        areas = (kb[:, 3] - kb[:, 1]) * (kb[:, 2] - kb[:, 0])
        painted = draw_labels(painted, texts, truncate_boxes(kb)[:, :2] + int(thickness), text_palette[labels[keep]], font_size,
                              adaptive_scales(areas))
    return _finish(painted, show, wait_time, out_file, win_name)


def show_panoptic(model, img, result, score_thr=0.3, bbox_color=(72, 101, 241), text_color=(72, 101, 241), mask_color=None,
                  thickness=2, font_size=20, win_name='', show=False, wait_time=0, out_file=None, show_labels=True, seed=0,
                  capacity=COMPONENT_CAPACITY):
    """`MaskFormerOpen._show_pan_result` (maskformer.py:311-382): see the method's docstring."""
    from . import ops
    img = _load_image(img)
    pan = result['panoptic_all_results']
    void = int(model.num_classes)
    H, W = img.shape[:2]
    if tuple(pan.shape) != (H, W):
        raise CggError(f'show_result: panoptic map of shape {tuple(pan.shape)} for a {H} x {W} image')
    dev = pan.device if torch.is_tensor(pan) and pan.is_cuda else _model_device(model)
    records, dpan = None, None
    if dev is not None and not _fits_int32(pan):              # a wider map with ids the kernels' int32 cannot hold: the host rule
        dev = None
    if dev is not None:
        dpan = (pan if torch.is_tensor(pan) else torch.from_numpy(np.ascontiguousarray(pan))).to(dev).to(torch.int32).contiguous()
        if ops.label_components_ok(dpan):
            rec, status = ops.label_components(dpan, void, capacity=capacity)
            host = torch.cat([status.to(torch.int64), rec.reshape(-1)]).cpu().numpy()           # ONE small copy
            count, flags = int(host[0]), int(host[1])
            if flags == 0 and count <= capacity:
                rec = host[2:].reshape(-1, 5)[:count]
                records = rec[np.argsort(rec[:, 0])]
    if records is None:                                       # overflow, outside the gate, or no device: the host rule
        records = components_host(pan.cpu().numpy() if torch.is_tensor(pan) else np.asarray(pan), void)
    ids = np.unique(records[:, 1])[::-1]                      # "keep objects ahead": descending, void is in no record
    labels = ids % INSTANCE_OFFSET
    max_label = int(labels.max()) if len(ids) else 0
    colors = instance_colors_host(labels, get_palette(mask_color, max_label + 1), seed=seed)
    painted = None
    if dpan is not None:
        dimg = _device_image(img, dev)
        if ops.paint_panoptic_ok(dimg, dpan, len(ids)) and (len(ids) == 0 or (ids.min() >= -(1 << 31) and ids.max() < (1 << 31))):
            asc = ids[::-1].astype(np.int32).copy()              # (a copy: torch takes no negative strides)
            painted = ops.paint_panoptic(dimg, dpan, torch.from_numpy(asc).to(dev),
                                         torch.from_numpy(colors[::-1].copy()).to(dev), alpha=0.8).cpu().numpy()
    if painted is None:
        painted = paint_panoptic_host(_host_image(img), pan.cpu().numpy() if torch.is_tensor(pan) else pan, ids, colors, void,
                                      alpha=0.8)
    if show_labels and len(ids):
        big = largest_components(records)                     # sorted by id ascending
        big = big[::-1]                                       # the order of `ids`
        text_palette = get_palette(text_color, max_label + 1)
        pos = np.stack([big[:, 3] / big[:, 2], big[:, 4] / big[:, 2]], axis=1)
        painted = draw_labels(painted, [_class_text(model, int(l)) for l in labels], pos, text_palette[labels], font_size,
                              adaptive_scales(big[:, 2]), center=True)
    return _finish(painted, show, wait_time, out_file, win_name)
