"""CPU tests of the host half of the device-side RLE: the numpy rule (`host_results.rle_transitions_host`) followed by
`ops.rle_strings_from_transitions`, and `ops.rle_encode_colmajor` on numpy-built column planes, both byte-equal to
`ops.rle_encode_bitmasks` on every shared case; argument validation of the three C entry points without a device."""
import ctypes

import numpy as np
import pytest

import rle_cases as RC
from cgg_amd import _lib, ops
from cgg_amd.host_results import rle_to_mask, rle_transitions_host


@pytest.mark.parametrize('idx', RC.CASE_IDS, ids=RC.case_name)
def test_rule_then_strings_equal_the_bitmask_encoder(idx):
    c = RC.case(idx)
    pos, offs = rle_transitions_host(c['bits'], c['W'])
    assert pos.dtype == np.uint32 and offs.dtype == np.int64 and offs.shape == (len(c['names']) + 1,)
    got = ops.rle_strings_from_transitions(pos, offs, c['H'], c['W'])
    want = RC.expected_rles(idx)
    assert len(got) == len(want) == len(c['names'])
    for name, g, w, px in zip(c['names'], got, want, c['px']):
        assert g == w, name
        assert np.array_equal(rle_to_mask(g), px), name                # and both mean the mask
    hw = c['H'] * c['W']
    for i, name in enumerate(c['names']):                               # the rule itself, on the planes whose answer is known
        t = pos[offs[i]:offs[i + 1]].tolist()
        if name == 'empty':
            assert t == []
        elif name == 'full':
            assert t == [0]
        elif name == 'first_pixel':
            assert t == ([0, 1] if hw > 1 else [0])
        elif name == 'last_pixel':
            assert t == [hw - 1]
        elif name == 'run_across_border' and c['W'] > 1:
            xb = 63 if c['W'] > 64 else c['W'] - 2
            p = (xb + 1) * c['H'] - 1
            assert t == [p, p + 2]                                       # ONE run of two pixels across the column border
        elif name == 'checkerboard':
            assert len(t) == hw - 1 - (c['W'] - 1 if c['H'] % 2 == 0 else 0)       # all but p = 0 and, for even H, the column tops
        elif name == 'bar':
            assert np.diff([0] + t + [hw]).max() > 2 ** 15


@pytest.mark.parametrize('idx', RC.CASE_IDS, ids=RC.case_name)
def test_encode_colmajor_equals_the_bitmask_encoder(idx):
    c = RC.case(idx)
    cols = RC.cols_host(c['px'])
    assert cols.shape[1:] == ops.rle_cols_shape(c['H'], c['W'])
    for threads in (1, 3):
        assert ops.rle_encode_colmajor(cols, c['H'], c['W'], threads=threads) == RC.expected_rles(idx)
    assert ops.rle_encode_colmajor(cols.view(np.int64)[1:], c['H'], c['W']) == RC.expected_rles(idx)[1:]


def test_no_masks():
    pos, offs = rle_transitions_host(np.zeros((0, 8, 2), np.uint8), 16)
    assert pos.shape == (0,) and offs.tolist() == [0]
    assert ops.rle_strings_from_transitions(pos, offs, 8, 16) == []
    assert ops.rle_encode_colmajor(np.zeros((0, 64, 1), np.uint64), 8, 16) == []


def test_strings_from_transitions_take_a_prefix_of_the_masks():
    """what the collector does after an overflow: the first k masks from the positions, whatever follows them in the buffer"""
    c = RC.case(3)
    pos, offs = rle_transitions_host(c['bits'], c['W'])
    k = c['names'].index('checkerboard')
    got = ops.rle_strings_from_transitions(pos, np.ascontiguousarray(offs[:k + 1]), c['H'], c['W'])
    assert got == RC.expected_rles(3)[:k]


def test_argument_validation_error_codes_without_a_device():
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    einval = -1
    T = lib.cgg_rle_transitions
    assert lib.cgg_rle_transitions_workspace_bytes(2, 65, 63) == 2 * 64 * 2 * 8 + 2 * 4 + 2 * 8
    assert lib.cgg_rle_transitions_workspace_bytes(3, 64, 65) == 3 * 128 * 8 + 6 * 4 + 6 * 8
    assert T(null, 1, 8, 8, 8, 1, p, p, 4, p, null) == einval                    # bits
    assert b'null' in lib.cgg_last_error_string()
    assert T(p, 1, 8, 8, 8, 1, null, p, 4, p, null) == einval                    # ws
    assert T(p, 1, 8, 8, 8, 1, p, null, 4, p, null) == einval                    # positions with capacity > 0
    assert T(p, 1, 8, 8, 8, 1, p, p, 4, null, null) == einval                    # offsets
    assert T(p, -1, 8, 8, 8, 1, p, p, 4, p, null) == einval                      # n < 0
    assert T(p, 1, 0, 8, 8, 1, p, p, 4, p, null) == einval                       # H < 1
    assert T(p, 1, 8, 0, 8, 1, p, p, 4, p, null) == einval                       # W < 1
    assert T(p, 1, 8, 9, 8, 1, p, p, 4, p, null) == einval                       # row_bytes * 8 < W
    assert T(p, 1, 8, 8, 7, 1, p, p, 4, p, null) == einval                       # mask stride < H * row_bytes
    assert T(p, 1, 8, 8, 8, 1, p, p, -1, p, null) == einval                      # capacity < 0
    assert T(p, 1, 1 << 16, 1 << 15, 1 << 28, 1 << 12, p, p, 4, p, null) == einval      # H * W = 2^31
    assert b'31 bits' in lib.cgg_last_error_string()
    assert T(p, 1, 8, 8, 8, 1, odd, p, 4, p, null) == einval                     # misaligned ws
    assert T(p, 1, 8, 8, 8, 1, p, p, 4, odd, null) == einval                     # misaligned offsets
    S = lib.cgg_rle_strings_from_transitions
    offs = (ctypes.c_int64 * 3)(0, 2, 3)
    pos = (ctypes.c_uint32 * 3)(1, 5, 0)
    out = (ctypes.c_uint8 * 64)()
    oo = (ctypes.c_int64 * 3)()
    assert S(pos, offs, 2, 4, 4, out, 64, oo) == 6 and list(oo) == [0, 3, 6]      # counts [1, 4, 11] and [0, 16]
    assert bytes(out[:6]) == b'14;0`0'                                            # 16 = groups 16 | continue, 0
    assert S(pos, offs, 2, 4, 4, out, 2, oo) == 6                                 # too small: the size, nothing copied
    assert S(pos, null, 2, 4, 4, out, 64, oo) == einval
    assert S(pos, offs, 2, 4, 4, out, 64, null) == einval
    assert S(pos, offs, -1, 4, 4, out, 64, oo) == einval
    assert S(pos, offs, 2, 0, 4, out, 64, oo) == einval
    assert S(pos, offs, 2, 1 << 16, 1 << 15, out, 64, oo) == einval
    assert S(pos, offs, 2, 2, 2, out, 64, oo) == einval                           # position 5 >= H * W
    assert S((ctypes.c_uint32 * 3)(5, 5, 0), offs, 2, 4, 4, out, 64, oo) == einval        # not ascending
    assert S(pos, (ctypes.c_int64 * 3)(0, 2, 1), 2, 4, 4, out, 64, oo) == einval  # offsets decrease
    assert S(null, offs, 2, 4, 4, out, 64, oo) == einval                          # positions missing
    C = lib.cgg_rle_encode_colmajor
    cols = (ctypes.c_uint64 * 64)()
    assert C(cols, 1, 4, 4, 1, out, 64, oo) == 2 and bytes(out[:2]) == b'`0'      # empty 4 x 4 mask: counts [16]
    assert C(null, 1, 4, 4, 1, out, 64, oo) == einval
    assert C(cols, 1, 4, 4, 1, out, 64, null) == einval
    assert C(cols, -1, 4, 4, 1, out, 64, oo) == einval
    assert C(cols, 1, 0, 4, 1, out, 64, oo) == einval
    assert C(cols, 1, 4, 0, 1, out, 64, oo) == einval
    assert C(cols, 1, 1 << 16, 1 << 15, 1, out, 64, oo) == einval
    assert b'cgg_rle_encode_colmajor' in lib.cgg_last_error_string()


def test_wrappers_refuse_what_the_library_cannot_read():
    import torch
    with pytest.raises(_lib.CggError, match='ROCm device'):
        ops.rle_transitions(torch.zeros(1, 8, 1, dtype=torch.uint8), 8, capacity=4)
    with pytest.raises(_lib.CggError):
        ops.rle_strings_from_transitions(np.zeros(2, np.uint32), np.array([0, 3], np.int64), 4, 4)     # offsets past the positions
    with pytest.raises(_lib.CggError):
        ops.rle_encode_colmajor(np.zeros((1, 64, 2), np.uint64), 4, 4)                                 # Hb of another H
    with pytest.raises(_lib.CggError, match='position'):
        ops.rle_strings_from_transitions(np.array([3, 2], np.uint32), np.array([0, 2], np.int64), 4, 4)


def test_collector_arguments_default_to_the_host_path():
    import inspect
    from cgg_amd.host_results import RleCollector
    sig = inspect.signature(RleCollector.__init__)
    assert sig.parameters['device_rle'].default is False and sig.parameters['run_capacity'].default is None
