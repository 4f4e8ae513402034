"""Shared cases of the device-side RLE tests (test_rle_device.py, test_rle_device_gpu.py): bit-packed planes at the sizes where
the kernels take another path (one pixel, less than a byte, exactly one 64 x 64 block, one row / column more or less than a
block, several strips and block-rows with set pad bits, a plane stride with a gap), each with the planes that exercise a rule
of the stream (empty, full, first / last pixel, a run across or broken at a column border, a disk, the checkerboard with its
maximal number of transitions, noise), and one 512 x 512 bar whose counts need several 5-bit groups and negative deltas.
The expected strings come from `ops.rle_encode_bitmasks`, which test_host_logic.py pins to the published COCO algorithm;
they are computed once per case."""
import functools

import numpy as np

# (H, W, row_bytes, pad bits of every plane set to ones, rows between planes beyond H)
SIZES = [
    (1, 1, 1, False, 0),
    (7, 5, 1, False, 0),
    (64, 64, 8, False, 0),
    (65, 63, 8, False, 0),
    (63, 65, 9, False, 0),
    (130, 200, 26, True, 0),
    (128, 136, 20, False, 3),
]
PLANES = ['empty', 'full', 'first_pixel', 'last_pixel', 'run_across_border', 'run_broken_at_border', 'disk', 'checkerboard', 'noise']


def pack(px, row_bytes):
    """(n, H, W) bool -> (n, H, row_bytes) uint8, pixel x in bit (x & 7) of byte (x >> 3), pad bits zero"""
    n, H, W = px.shape
    full = np.zeros((n, H, row_bytes * 8), np.uint8)
    full[:, :, :W] = px
    return np.packbits(full, axis=-1, bitorder='little')


def pixels(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    px = np.zeros((len(PLANES), H, W), bool)
    px[1] = True
    px[2, 0, 0] = True
    px[3, H - 1, W - 1] = True
    xb = 63 if W > 64 else W - 2          # the border between columns xb and xb + 1 (63 / 64 wherever the mask has a column 64)
    if xb >= 0:
        px[4, H - 1, xb] = True           # column xb ends in 1 and column xb + 1 starts with 1: one run across the border
        px[4, 0, xb + 1] = True
        px[5, H - 1, xb] = True           # column xb ends in 1, column xb + 1 starts with 0: the run ends with the column
        if H > 1:
            px[5, 1, xb + 1] = True
    px[6] = (yy - 0.45 * H) ** 2 + (xx - 0.55 * W) ** 2 <= (0.3 * min(H, W) + 0.5) ** 2
    px[7] = (yy + xx) % 2 == 1
    px[8] = rng.random((H, W)) < 0.5
    return px


@functools.lru_cache(maxsize=None)
def case(idx):
    """-> dict(H, W, row_bytes, px (n, H, W) bool, bits (n, H, row_bytes) uint8 -- a view with a plane stride > H * row_bytes in
    the strided case --, base (the array `bits` views), names)"""
    if idx == len(SIZES):
        # one 512 x 512 plane of full-height bars: counts 51200, 102400, 25600, 5120, 77824 -> strings of several 5-bit groups
        # (a count above 2^15) and negative deltas against counts[i - 2]
        px = np.zeros((1, 512, 512), bool)
        px[0, :, 100:300] = True
        px[0, :, 350:360] = True
        bits = pack(px, 64)
        return dict(H=512, W=512, row_bytes=64, px=px, bits=bits, base=bits, names=['bar'])
    H, W, rb, pad_ones, gap = SIZES[idx]
    px = pixels(H, W, seed=100 + idx)
    packed = pack(px, rb)
    rng = np.random.default_rng(200 + idx)
    pad = np.ones((H, rb * 8), np.uint8)
    pad[:, :W] = 0
    pad = np.packbits(pad, axis=-1, bitorder='little')              # the pad bits of a row
    if pad_ones:
        packed |= pad[None]
    else:
        packed[8] |= pad & rng.integers(0, 256, (H, rb), dtype=np.uint8)     # pad bits may hold anything
    base = rng.integers(0, 256, (len(PLANES), H + gap, rb), dtype=np.uint8)  # the gap rows hold anything too
    base[:, :H] = packed
    bits = base[:, :H]
    return dict(H=H, W=W, row_bytes=rb, px=px, bits=bits, base=base, names=list(PLANES))


CASE_IDS = list(range(len(SIZES) + 1))


def case_name(idx):
    c = case(idx)
    return f"{c['H']}x{c['W']}"


@functools.lru_cache(maxsize=None)
def expected_rles(idx):
    """the comparison side: `ops.rle_encode_bitmasks` on the (contiguous) planes"""
    from cgg_amd import ops
    c = case(idx)
    return ops.rle_encode_bitmasks(np.ascontiguousarray(c['bits']), c['W'], threads=1)


def cols_host(px):
    """numpy transpose into the workspace layout of cgg_rle_transitions: (n, H, W) bool -> (n, 64 * ceil(W / 64), ceil(H / 64))
    uint64, bit r of [i, x, by] = pixel (by * 64 + r, x), zeros beyond H and W"""
    n, H, W = px.shape
    Hb, Wp = (H + 63) // 64, 64 * ((W + 63) // 64)
    full = np.zeros((n, Hb * 64, Wp), np.uint64)
    full[:, :H, :W] = px
    words = (full.reshape(n, Hb, 64, Wp) << np.arange(64, dtype=np.uint64)[None, None, :, None]).sum(axis=2, dtype=np.uint64)
    return np.ascontiguousarray(words.transpose(0, 2, 1))
