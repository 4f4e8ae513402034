"""Shared cases of the paint tests (test_paint.py, test_paint_gpu.py).

Instances: images of 1 x 1, 19 x 37 (5 mask bytes per row, the 3 pad bits of the last byte set), 8 x 64 (8 full bytes), 33 x 130
(17 bytes, 6 pad bits) and 8 x 1032 (129 bytes) with n in {0, 1, 3, 70} masks cycling through the kinds below, `keep` mixing 0 and
1 (at n = 70 every kind of mask and of box is drawn at least once: `instance_case` asserts it), and one box per mask cycling through
the box kinds. The kernel's tile is 4 rows x 64 mask bytes (512 pixels): 33 rows cross it
nine times with a ragged last tile, 1032 columns make three column tiles, the last one byte wide.

Components: maps of 1 x 1, 7 x 300, 300 x 7 and 65 x 129 (the kernels work on 64-pixel row segments: 300 and 129 cross them with a
ragged end, 7 stays inside one).

Every host reference is computed once per case (lru_cache) and never modified by a test.
"""
import functools

import numpy as np

INSTANCE_SIZES = [(1, 1), (19, 37), (8, 64), (33, 130), (8, 1032)]
INSTANCE_COUNTS = [0, 1, 3, 70]
ALPHA_THICKNESS = [(0.8, 2), (0.5, 1), (1.0, 5)]
MASK_KINDS = ['nested_outer', 'nested_mid', 'nested_inner', 'empty', 'full', 'corners', 'hline', 'vline', 'touch_left', 'touch_right',
              'touch_top', 'touch_bottom', 'noise']
BOX_KINDS = ['inside', 'degenerate_x', 'degenerate_y', 'partly_outside', 'wholly_outside', 'tiny', 'inverted', 'whole_image']
VOID = 80
COMPONENT_SIZES = [(1, 1), (7, 300), (300, 7), (65, 129)]
COMPONENT_KINDS = ['spiral', 'comb', 'checker_one_id', 'checker_two_ids', 'ties', 'void_regions', 'extreme_ids', 'blobs']
PANOPTIC_TABLES = ['all_but_void', 'one_id', 'table_1024']


def pack(px, row_bytes, pad_ones=False):
    """(n, H, W) bool -> (n, H, row_bytes) uint8, pixel x in bit (x & 7) of byte (x >> 3); pad bits zero, or all ones"""
    n, H, W = px.shape
    full = np.full((n, H, row_bytes * 8), 1 if pad_ones else 0, np.uint8)
    full[:, :, :W] = px
    return np.packbits(full, axis=-1, bitorder='little')


def _mask(kind, H, W, rng):
    m = np.zeros((H, W), bool)
    if kind == 'nested_outer':
        m[H // 8:H - H // 8, W // 8:W - W // 8] = True
    elif kind == 'nested_mid':
        m[H // 4:H - H // 4, W // 4:W - W // 4] = True
    elif kind == 'nested_inner':
        m[H // 2 - H // 8:H // 2 + H // 8 + 1, W // 2 - W // 8:W // 2 + W // 8 + 1] = True
    elif kind == 'full':
        m[:] = True
    elif kind == 'corners':
        m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = True
    elif kind == 'hline':
        m[H // 2, :] = True
    elif kind == 'vline':
        m[:, W // 3] = True
    elif kind == 'touch_left':
        m[H // 4:H // 2 + 1, 0:max(W // 5, 1)] = True
    elif kind == 'touch_right':
        m[H // 3:H // 2 + 2, W - max(W // 5, 1):] = True
    elif kind == 'touch_top':
        m[0:max(H // 4, 1), W // 3:W // 2 + 1] = True
    elif kind == 'touch_bottom':
        m[H - max(H // 4, 1):, W // 2:W - W // 4 + 1] = True
    elif kind == 'noise':
        m = rng.random((H, W)) < 0.4
    return m


def _box(kind, H, W, rng):
    if kind == 'inside':
        return [W * 0.2 + 0.7, H * 0.2 + 0.3, W * 0.8 + 0.9, H * 0.8 + 0.2]
    if kind == 'degenerate_x':
        return [W // 2 + 0.5, 0.2, W // 2 + 0.9, H - 0.5]
    if kind == 'degenerate_y':
        return [1.0, H // 2, W - 1.0, H // 2 + 0.99]
    if kind == 'partly_outside':
        return [-3.5, -2.5, W * 0.6, H + 4.0]
    if kind == 'wholly_outside':
        return [W + 2.0, H + 3.0, W + 9.0, H + 8.0]
    if kind == 'tiny':                      # thinner than any thickness above 1
        return [W // 3, H // 3, W // 3 + 2.5, H // 3 + 1.5]
    if kind == 'inverted':
        return [W * 0.7, H * 0.7, W * 0.3, H * 0.3]
    return [0.0, 0.0, W - 1.0, H - 1.0]


@functools.lru_cache(maxsize=None)
def instance_case(size, n, at):
    """-> dict(img, masks (n, H, W) bool, bits (packed, pad bits set to ones), keep, colors, boxes (n, 5), box_colors, alpha, thickness,
    want, want_fill_only: without edges and boxes)"""
    from cgg_amd.paint import paint_instances_host
    H, W = size
    alpha, thickness = at
    rng = np.random.default_rng(1000 * H + 10 * W + n)
    img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    masks = np.stack([_mask(MASK_KINDS[i % len(MASK_KINDS)], H, W, rng) for i in range(n)]) if n else np.zeros((0, H, W), bool)
    # every fifth instance is dropped; 5 is coprime to the 13 mask kinds and the 8 box kinds, so at n = 70 every kind is drawn (and
    # every kind is dropped) at least once. The dropped residue moves with the (alpha, thickness) variant: at n = 3 the three nested
    # masks are all kept in two variants (the order is visible three deep) and the middle one is dropped in the third.
    drop = {0: 3, 1: 1, 2: 4}[ALPHA_THICKNESS.index(at)]
    keep = np.array([0 if i % 5 == drop else 1 for i in range(n)], np.uint8) if n > 1 else np.ones(n, np.uint8)
    if n >= 5 * max(len(MASK_KINDS), len(BOX_KINDS)):
        for kinds in (MASK_KINDS, BOX_KINDS):
            for k in range(len(kinds)):
                assert keep[k::len(kinds)].any() and not keep[k::len(kinds)].all(), f'{kinds[k]} is never kept, or never dropped'
    colors = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    if n > 2:
        colors[0], colors[2] = (0, 255, 0), (255, 0, 255)
    boxes = np.array([_box(BOX_KINDS[i % len(BOX_KINDS)], H, W, rng) + [0.5] for i in range(n)], np.float32).reshape(n, 5)
    box_colors = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    rb = (W + 7) // 8
    c = dict(img=img, masks=masks, bits=pack(masks, rb, pad_ones=True), keep=keep, colors=colors, boxes=boxes, box_colors=box_colors,
             alpha=alpha, thickness=thickness)
    c['want'] = paint_instances_host(img, masks, colors, keep, boxes, box_colors, alpha=alpha, thickness=thickness)
    c['want_fill_only'] = paint_instances_host(img, masks, colors, keep, alpha=alpha, edges=False)
    return c


@functools.lru_cache(maxsize=None)
def all_pairs_case(alpha):
    """256 x 256 image whose channel values equal x, 256 one-row masks, mask y with colour (y, y, y): every (value, colour) pair"""
    from cgg_amd.paint import paint_instances_host
    img = np.tile(np.arange(256, dtype=np.uint8)[None, :, None], (256, 1, 3))
    masks = np.zeros((256, 256, 256), bool)
    masks[np.arange(256), np.arange(256), :] = True
    colors = np.tile(np.arange(256, dtype=np.uint8)[:, None], (1, 3))
    want = paint_instances_host(img, masks, colors, alpha=alpha, edges=False)
    return dict(img=img, masks=masks, bits=pack(masks, 32), colors=colors, want=want)


# ---- id maps ---------------------------------------------------------------------------------------------------------------------
def _spiral(H, W):
    """a one-pixel corridor winding inwards from (0, 0): walk ahead while the cell after the next is free, else turn right"""
    m = np.zeros((H, W), bool)
    y = x = 0
    m[0, 0] = True
    dy, dx, turns = 0, 1, 0
    while turns < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
            y, x, turns = ny, nx, 0
            m[y, x] = True
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return m


def id_map(kind, H, W):
    rng = np.random.default_rng(7 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    pan = np.full((H, W), VOID, np.int32)
    if kind == 'spiral':
        pan[_spiral(H, W)] = 5
    elif kind == 'comb':
        pan[0, :] = 9
        pan[:, ::2] = 9                     # teeth hanging from the top row
        pan[H - 1, 1::2] = 1009             # one-pixel components of another id between the teeth
    elif kind == 'checker_one_id':
        pan[(yy + xx) % 2 == 0] = 3
    elif kind == 'checker_two_ids':
        pan[:] = np.where((yy + xx) % 2 == 0, 3, 4)
    elif kind == 'ties':
        h, w = max(H // 4, 1), max(W // 4, 1)
        pan[0:h, 0:w] = 12
        pan[H - h:H, W - w:W] = 12          # same id, same area: the smaller root wins
        if H > 2 * h or W > 2 * w:
            pan[H // 2, W // 2] = 2012
    elif kind == 'void_regions':
        pan[:] = rng.integers(0, 3, size=(H, W)) + 20
        pan[rng.random((H, W)) < 0.35] = VOID
    elif kind == 'extreme_ids':
        pan[:, :max(W // 2, 1)] = 0
        pan[:, max(W // 2, 1):] = 2**31 - 1
        pan[H // 2, :] = np.where(xx[0] % 3 == 0, VOID, pan[H // 2, :])
    elif kind == 'blobs':
        ids = np.array([1, 17, 1001, 2001, 64 + 15, 3017], np.int32)
        coarse = ids[rng.integers(0, 6, size=((H + 7) // 8 + 1, (W + 7) // 8 + 1))]
        pan[:] = np.kron(coarse, np.ones((8, 8), np.int32))[3:3 + H, 5:5 + W]
    return pan


@functools.lru_cache(maxsize=None)
def component_case(size, kind):
    from cgg_amd.paint import components_host
    pan = id_map(kind, *size)
    rec = components_host(pan, VOID)
    return dict(pan=pan, records=rec)


@functools.lru_cache(maxsize=None)
def panoptic_case(size, table):
    from cgg_amd.paint import paint_panoptic_host
    H, W = size
    rng = np.random.default_rng(31 * H + W)
    img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    if table == 'table_1024':
        pool = np.sort(rng.choice(60000, size=1100, replace=False)).astype(np.int32)
        pool = pool[pool != VOID]
        pan = pool[rng.integers(0, len(pool), size=(H, W))].astype(np.int32)
        pan[rng.random((H, W)) < 0.1] = VOID
        ids = pool[rng.permutation(len(pool))[:1024]]
    else:
        pan = id_map('blobs', H, W).copy()
        pan[rng.random((H, W)) < 0.2] = VOID
        present = np.unique(pan)
        ids = present[present != VOID] if table == 'all_but_void' else np.array([1001], np.int32)
    ids = np.sort(ids)[::-1].astype(np.int32)                 # descending, as the reference walks them
    colors = rng.integers(0, 256, size=(len(ids), 3), dtype=np.uint8)
    want = paint_panoptic_host(img, pan, ids, colors, VOID)
    return dict(img=img, pan=pan, ids=ids, colors=colors, want=want)
