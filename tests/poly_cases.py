"""Seeded polygon cases shared by test_train_prep_polygons.py (host: the literal form against the parity form of rule 6) and
test_train_prep_polygons_gpu.py (the fill kernel against the parity form). A case is (name, parts, h, w): `parts` = one instance,
a list of flat x0, y0, x1, y1, ... lists. Nothing here touches a device."""
import numpy as np

from cgg_amd import train_prep as tp

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
PLANES = [(1, 1), (1, 9), (9, 1), (6, 7), (37, 45)]          # (h, w)
OVER_LDS = (601, 655)                                        # (h, w): 393655 pixels, the first plane of this shape past 393216 bits

RECT_A = ([1, 1, 3, 1, 3, 3, 1, 3], (slice(1, 3), slice(1, 3)))             # in a 6 x 7 plane: rows 1-2 x columns 1-2
RECT_B = ([1.5, 1.5, 4.5, 1.5, 4.5, 3.5, 1.5, 3.5], (slice(2, 4), slice(2, 5)))   # rows 2-3 x columns 2-4


def _random_part(r, h, w, k, simple):
    """k vertices up to 5 px outside the h x w plane on every side; `simple`: sorted by angle round the centre (star-shaped)"""
    if simple:
        ang = np.sort(r.uniform(0, 2 * np.pi, size=k))
        rad = r.uniform(0.3, 1.0, size=k)
        x = (w / 2) + rad * (w / 2 + 5) * np.cos(ang)
        y = (h / 2) + rad * (h / 2 + 5) * np.sin(ang)
    else:
        x, y = r.uniform(-5, w + 5, size=k), r.uniform(-5, h + 5, size=k)
    q = r.integers(0, 3)                                     # whole pixels, halves, or arbitrary fractions
    if q == 0:
        x, y = np.round(x), np.round(y)
    elif q == 1:
        x, y = np.round(2 * x) / 2, np.round(2 * y) / 2
    return np.stack([x, y], axis=1).reshape(-1).tolist()


def cases():
    """the case list of the issue, seeded: every plane x (random simple, random self-intersecting, axis-aligned, 45 degrees,
    repeated vertices, k = 1, k = 2, a part outside the plane, a vertex below the plane)"""
    out = []
    for h, w in PLANES:
        r = np.random.default_rng(1000 * h + w)
        for i in range(4):
            out.append((f'simple{i}', [_random_part(r, h, w, int(r.integers(3, 12)), True)], h, w))
            out.append((f'selfx{i}', [_random_part(r, h, w, int(r.integers(3, 12)), False)], h, w))
        x0, y0 = float(r.integers(-2, max(w // 2, 1))), float(r.integers(-2, max(h // 2, 1)))
        x1, y1 = x0 + float(r.integers(1, w + 3)), y0 + float(r.integers(1, h + 3))
        out.append(('axis', [[x0, y0, x1, y0, x1, y1, x0, y1]], h, w))
        out.append(('axis_half', [[x0 + .5, y0 + .5, x1 + .5, y0 + .5, x1 + .5, y1 + .5, x0 + .5, y1 + .5]], h, w))
        d = float(max(min(h, w) // 2, 1))
        cx, cy = w / 2.0, h / 2.0
        out.append(('diamond45', [[cx, cy - d, cx + d, cy, cx, cy + d, cx - d, cy]], h, w))
        out.append(('diamond45_ccw', [[cx, cy - d, cx - d, cy, cx, cy + d, cx + d, cy]], h, w))
        p = _random_part(r, h, w, 5, True)
        out.append(('repeated', [p[:4] + p[2:4] + p[4:] + p[-2:] + p[-2:]], h, w))
        out.append(('k1', [[w / 2.0, h / 2.0]], h, w))
        out.append(('k1_outside', [[-3.0, -2.0]], h, w))
        out.append(('k2', [[0.0, 0.0, float(w), float(h)]], h, w))
        out.append(('k2_steep', [[w / 3.0, -1.0, w / 2.0, h + 2.0]], h, w))
        out.append(('outside_right', [[w + 2.0, 1.0, w + 6.0, 1.0, w + 6.0, h + 1.0, w + 2.0, h + 1.0]], h, w))
        out.append(('outside_left', [[-6.0, 0.0, -1.0, 0.0, -1.0, float(h), -6.0, float(h)]], h, w))
        out.append(('below', [[0.0, 0.0, float(w), 0.0, w / 2.0, h + 4.0]], h, w))          # a vertex below: the yd == h clamp
        out.append(('below_last_column', [[w - 1.0, h - 0.5, float(w), h + 3.0, w + 2.0, h - 0.5]], h, w))
        out.append(('whole_plane', [[-1.0, -1.0, w + 1.0, -1.0, w + 1.0, h + 1.0, -1.0, h + 1.0]], h, w))
        out.append(('two_parts', [_random_part(r, h, w, 6, True), _random_part(r, h, w, 4, False)], h, w))
    return out


CASES = cases()


def circle(cx, cy, rad, k=200):
    a = 2 * np.pi * np.arange(k) / k
    return np.stack([cx + rad * np.cos(a), cy + rad * np.sin(a)], axis=1).reshape(-1).tolist()


def layout(images, pixels=None, dirty=0xCC):
    """the staged bytes of the polygon ABI for `images` = [(h, w, [instance parts, ...]) ...]: (buf uint8, img_table, inst_table,
    part_table) as numpy arrays, tables first, back to back, then the (h, w, 3) uint8 `pixels` of every image when given (without
    them every image row points at byte 0: `cgg_polygon_fill_bits` reads no pixel), then the coordinates. The image rows describe
    the identity geometry: no flip, no resize, the window at the origin."""
    B = len(images)
    N = sum(len(insts) for _, _, insts in images)
    P = sum(len(parts) for _, _, insts in images for parts in insts)
    n = 48 * B + 12 * N + 8 * P
    offs = []
    for b in range(B):
        offs.append(n if pixels is not None else 0)
        n += pixels[b].size if pixels is not None else 0
    n = (n + 7) & ~7
    img_rows, inst_rows, part_rows, coords = [], [], [], []
    first = pfirst = 0
    for b, (h, w, insts) in enumerate(images):
        img_rows.append((offs[b], h, w, 3 * w, h, w, 0, 0, 0, first, len(insts), -1))
        first += len(insts)
        for parts in insts:
            inst_rows.append((b, pfirst, len(parts)))
            pfirst += len(parts)
            for part in parts:
                xy = np.asarray(part, dtype=np.float64)
                part_rows.append((n, xy.size // 2))
                coords.append((n, xy))
                n += xy.nbytes
    buf = np.full(max(n, 8), dirty, dtype=np.uint8)
    tables = [np.asarray(t, dtype=np.int32).reshape(-1, c) for t, c in ((img_rows, 12), (inst_rows, 3), (part_rows, 2))]
    off = 0
    for t in tables:
        buf[off:off + t.nbytes] = t.reshape(-1).view(np.uint8)
        off += t.nbytes
    for b in range(B if pixels is not None else 0):
        buf[offs[b]:offs[b] + pixels[b].size] = pixels[b].reshape(-1)
    for o, xy in coords:
        buf[o:o + xy.nbytes] = xy.view(np.uint8)
    return buf, tables[0], tables[1], tables[2]


def spec_for(crop, size):
    return tp.TrainPrepSpec(img_scale=(64, 64), crop_size=crop, size=size, pad_val=((128.0, 64.0, 32.0), 0, 255), mean=MEAN, std=STD,
                            to_rgb=True, with_seg=False)


def poly_sample(h, w, seed, insts, captions=True):
    r = np.random.default_rng(seed)
    s = dict(img=r.integers(0, 256, size=(h, w, 3), dtype=np.uint8), gt_polygons=insts,
             gt_labels=r.integers(0, 80, size=len(insts)).astype(np.int64), filename=f'poly_{seed}.jpg')
    if captions:
        s['gt_caption_ids'] = r.integers(0, 1000, size=8).astype(np.int64)
        s['gt_caption_mask'] = np.ones(8, dtype=np.int64)
        s['gt_caption_nouns_ids'] = r.integers(0, 1000, size=8).astype(np.int64)
        s['gt_caption_nouns_mask'] = np.ones(8, dtype=np.int64)
    return s


def prep_batch(flip_first, scale_up):
    """B = 3 samples of 48 x 64 into a 64 x 64 plane: image 0 with five instances (multi-part, partly outside, a two-vertex part, one
    in the top-left corner, one wholly outside), image 1 with zero instances, image 2 whose instances all lie in the top rows, which
    its window at the far margin does not see. scale_up: image 0 at 2.0 (96 x 128 resized, a non-zero crop corner), else below 1."""
    h, w = 48, 64
    r = np.random.default_rng(7)
    a = poly_sample(h, w, 1, [
        [_random_part(r, h, w, 7, True), _random_part(r, h // 2, w // 2, 5, True)],
        [[50.5, 10.0, 70.0, 12.0, 69.0, 40.25, 52.0, 30.0]],
        [[20.0, 20.0, 40.0, 22.0, 38.0, 40.0, 18.0, 36.0], [5.0, 5.0, 30.0, 44.0]],
        [[0.0, 0.0, 6.0, 0.0, 6.0, 5.0, 0.0, 5.0]],
        [[70.0, 5.0, 90.0, 5.0, 80.0, 30.0]],
    ])
    b = poly_sample(h, w, 2, [])
    c = poly_sample(h, w, 3, [[[2.0, 0.0, 30.0, 0.0, 30.0, 3.0, 2.0, 3.0]], [[40.0, 0.5, 60.0, 0.5, 50.0, 2.5]]])
    spec = spec_for((64, 64), (64, 64))
    if scale_up:
        pa = tp.TrainParams(flip_first, (128, 128), (20, 37))            # 96 x 128 resized; margins (32, 64)
    else:
        pa = tp.TrainParams(flip_first, (40, 40), (0, 0))                # 30 x 40 resized
    pb = tp.TrainParams(not flip_first, (64, 64), (0, 0))
    nh, nw = tp.resized_hw((h, w), (128, 128))
    pc_ = tp.TrainParams(flip_first, (128, 128), (max(nh - 64, 0), max(nw - 64, 0)))
    return [a, b, c], [pa, pb, pc_], spec
