"""Rule 6 of train_prep.py on the host: COCO polygons -> bitmaps as the published maskApi.c (rleFrPoly, merge) is restated. The
literal run-length form and the parity form (the one the kernel computes) are held equal bit for bit on the seeded cases of
tests/poly_cases.py; polygon samples through `prepare_train_host`; the refusals; the synthetic stream; the ABI's declarations."""
import ctypes

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import _lib, ops, synthetic, train_prep as tp
from cgg_amd._lib import CggError

import poly_cases as pc

CASES = pc.CASES


def test_known_rectangles():
    for xy, (rows, cols) in (pc.RECT_A, pc.RECT_B):
        want = np.zeros((6, 7), dtype=np.uint8)
        want[rows, cols] = 1
        for fn in (tp.polygon_mask_host, tp._polygon_mask_literal):
            got = fn([xy], 6, 7)
            assert got.dtype == np.uint8 and got.shape == (6, 7) and np.array_equal(got, want), (fn.__name__, xy, got)


def test_literal_form_equals_parity_form():
    names, filled, clamp = set(), 0, 0
    for name, parts, h, w in CASES:
        a, b = tp._polygon_mask_literal(parts, h, w), tp.polygon_mask_host(parts, h, w)
        assert a.shape == (h, w) and np.array_equal(a, b), (name, h, w, parts)
        names.add(name)
        filled += int(b.any())
        if name.startswith('outside'):
            assert not b.any(), (name, h, w)
        if name == 'whole_plane':
            assert b.all(), (h, w)
        if name.startswith('below'):
            clamp += int(any((tp._part_crossings(p, h, w) % h == 0).any() for p in parts))
    assert {'simple3', 'selfx3', 'axis','diamond45', 'repeated', 'k1', 'k2', 'outside_right', 'below', 'two_parts'} <= names
    assert {(h, w) for _, _, h, w in CASES} == set(pc.PLANES)
    assert filled >= len(CASES) // 3 and clamp >= 3


def test_parity_is_carried_across_columns():
    """a polygon whose crossings per column are not all even in number: restarting the parity at each column would differ"""
    odd = 0
    for name, parts, h, w in CASES:
        for p in parts:
            a = tp._part_crossings(p, h, w)
            a = a[a < h * w]
            odd += int((np.bincount(a // h, minlength=w) % 2).any())
    assert odd >= 5


def test_union_of_parts():
    h, w = 37, 45
    p, q = [5.0, 5.0, 30.0, 6.0, 28.0, 30.0, 4.0, 25.0], [20.0, 10.0, 44.0, 12.0, 40.0, 36.0, 18.0, 33.0]
    a, b = tp.polygon_mask_host([p], h, w), tp.polygon_mask_host([q], h, w)
    assert (a & b).any() and (a & ~b & 1).any() and (b & ~a & 1).any()
    for fn in (tp.polygon_mask_host, tp._polygon_mask_literal):
        assert np.array_equal(fn([p, q], h, w), a | b)
    assert not tp.polygon_mask_host([], h, w).any()


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('scale_up', [False, True])
def test_prepare_train_host_of_polygon_samples(flip, scale_up):
    samples, params, spec = pc.prep_batch(flip, scale_up)
    bitmaps = [tp.polygons_to_bitmap_sample(s) for s in samples]
    for s, m in zip(samples, bitmaps):
        assert 'gt_polygons' not in m and m['gt_masks'].shape == (len(s['gt_polygons']),) + s['img'].shape[:2]
    got, kept = tp.prepare_train_host(samples, params, spec)
    want, want_kept = tp.prepare_train_host(bitmaps, params, spec)
    assert kept == want_kept and set(got) == set(want)
    assert kept[1] == 0 and kept[2] == 0 and 1 <= kept[0] < 5
    for k in want:
        if k == 'img_metas':
            assert [sorted(m) for m in got[k]] == [sorted(m) for m in want[k]]
            for a, b in zip(got[k], want[k]):
                assert a['img_shape'] == b['img_shape'] and a['flip'] == b['flip'] and np.array_equal(a['scale_factor'], b['scale_factor'])
            continue
        gs, ws = (got[k], want[k]) if isinstance(want[k], list) else ([got[k]], [want[k]])
        assert len(gs) == len(ws)
        for a, b in zip(gs, ws):
            assert a.dtype == b.dtype and np.array_equal(a, b), k


def test_refusals_name_the_offender():
    spec = pc.spec_for((16, 16), (16, 16))
    params = [tp.TrainParams(False, (16, 16), (0, 0))]
    ok = [[[1.0, 1.0, 9.0, 1.0, 9.0, 9.0]]]

    def sample(polys, **kw):
        s = pc.poly_sample(12, 16, 0, polys)
        s.update(kw)
        return s

    rle = dict(size=[12, 16], counts=[3, 4, 185])
    big = float(ops.TRAIN_PREP_MAX_COORD) + 1.0
    for polys, pat in (([rle], r'gt_polygons\[0\].*RLE'),
                       ([ok[0], [[1.0, 2.0, 3.0]]], r'gt_polygons\[1\]\[0\].*odd coordinate count'),
                       ([[[]]], r'gt_polygons\[0\]\[0\].*empty part'),
                       ([[[1.0, float('nan'), 2.0, 2.0]]], r'gt_polygons\[0\]\[0\].*non-finite'),
                       ([[[1.0, float('inf'), 2.0, 2.0]]], r'gt_polygons\[0\]\[0\].*non-finite'),
                       ([[[1.0, 1.0, -big, 2.0]]], r'gt_polygons\[0\]\[0\].*CGG_IMAGE_PREP_MAX_DIM')):
        for fn in (lambda s: tp.prepare_train_host([s], params, spec), tp.polygons_to_bitmap_sample):
            with pytest.raises(CggError, match=pat):
                fn(sample(polys))
    with pytest.raises(CggError, match='both gt_masks and gt_polygons'):
        tp.prepare_train_host([sample(ok, gt_masks=np.zeros((1, 12, 16), dtype=np.uint8))], params, spec)
    seg_spec = tp.TrainPrepSpec(img_scale=(64, 64), crop_size=(16, 16), size=(16, 16), with_seg=True)
    with pytest.raises(CggError, match='with_seg.*gt_polygons'):
        tp.prepare_train_host([sample(ok)], params, seg_spec)
    with pytest.raises(CggError, match='gt_labels.*gt_polygons'):
        tp.prepare_train_host([sample(ok, gt_labels=np.zeros(2, dtype=np.int64))], params, spec)
    with pytest.raises(CggError, match='mixes polygon samples'):
        tp.prepare_train_host([sample(ok), dict(sample(ok), gt_polygons=None, gt_masks=np.zeros((1, 12, 16), dtype=np.uint8))],
                              params * 2, spec)
    # an instance without parts is legal: an empty mask, filtered by "area >= 1"
    got, kept = tp.prepare_train_host([sample([[], ok[0]])], params, spec)
    assert kept == [1] and got['gt_masks'][0].shape == (1, 16, 16)
    # the coordinate bound itself is legal
    assert tp._check_polygons([[[1.0, 1.0, float(ops.TRAIN_PREP_MAX_COORD), 2.0]]])


def test_synthetic_polygon_stream():
    hw = (48, 64)
    a = [s for s, _ in zip(synthetic.polygon_samples(hw, 10, seed=5), range(3))]
    b = [s for s, _ in zip(synthetic.polygon_samples(hw, 10, seed=5), range(3))]
    assert [s['gt_polygons'] for s in a] == [s['gt_polygons'] for s in b] and all(np.array_equal(x['img'], y['img']) for x, y in zip(a, b))
    assert a[0]['gt_polygons'] != a[1]['gt_polygons']
    assert synthetic.POLYGON_KINDS == ('multi_part', 'partly_outside', 'two_vertex_part', 'never_kept')
    for s in a:
        assert s['img'].dtype == np.uint8 and s['img'].shape == hw + (3,)
        polys = tp._check_polygons(s['gt_polygons'])
        assert len(polys) == len(s['gt_labels']) >= 5 and all(k in s for k in tp.CAPTION_FIELDS)
        masks = tp.polygons_to_bitmap_sample(s)['gt_masks']
        assert len(polys[0]) == 3 and masks[0].any()                                             # multi-part
        xs = np.concatenate([p[0::2] for p in polys[1]])
        assert xs.max() > hw[1] and xs.min() < hw[1] and masks[1].any()                          # partly outside
        assert any(p.size == 4 for p in polys[2]) and masks[2].any()                             # a two-vertex part
        assert not masks[3].any()                                                                # no crop keeps it
    spec = pc.spec_for((64, 64), (64, 64))
    rng = np.random.default_rng(0)
    params = [tp.draw_train_params(rng, hw, spec) for _ in a]
    _, kept = tp.prepare_train_host(a, params, spec)
    assert all(k < len(s['gt_labels']) for k, s in zip(kept, a))


def test_abi_is_declared_and_exported():
    lib = _lib.load()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert _lib.PROTOTYPES['cgg_train_prep_polygons_workspace_bytes'] == (i64, [vp, i32, i32, i32])
    assert _lib.PROTOTYPES['cgg_polygon_fill_bits'] == (i32, [vp, i64, i64, i64, i64, vp, vp, vp, vp, i32, i32, i32, vp, i64, i32, vp])
    res, args = _lib.PROTOTYPES['cgg_train_prep_polygons_u8']
    assert res is i32 and len(args) == 27 and args[:5] == [vp, i64, i64, i64, i64] and args[-4:] == [vp, i64, i32, vp]
    for name in ('cgg_train_prep_polygons_u8', 'cgg_polygon_fill_bits', 'cgg_train_prep_polygons_workspace_bytes'):
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert ops.POLY_SCAN_BITS == 8192 and ops.POLY_LDS_BITS % ops.POLY_SCAN_BITS == 0
    # the workspace: one bit plane per instance, the largest image's words apart; twice that on the workspace route
    rows = torch.tensor([[0, 48, 64, 192, 48, 64, 0, 0, 0, 0, 2, -1], [0, 5, 7, 21, 5, 7, 0, 0, 0, 2, 1, -1]], dtype=torch.int32)
    assert ops.train_prep_polygons_workspace_bytes(rows, 3) == 3 * (48 * 64 // 32) * 4
    assert ops.train_prep_polygons_workspace_bytes(rows, 3, force_workspace=True) == 2 * 3 * (48 * 64 // 32) * 4
    big = rows.clone()
    big[1, 1], big[1, 2] = pc.OVER_LDS
    assert pc.OVER_LDS[0] * pc.OVER_LDS[1] > ops.POLY_LDS_BITS
    assert ops.train_prep_polygons_workspace_bytes(big, 3) == 2 * 3 * ((pc.OVER_LDS[0] * pc.OVER_LDS[1] + 31) // 32) * 4
    with pytest.raises(CggError, match='cgg_train_prep_polygons_workspace_bytes'):
        ops.train_prep_polygons_workspace_bytes(rows, 2)                 # the images own 3 instances


def test_driver_flag_is_exclusive():
    """tools/train.py: --synthetic-polygons HxW parses, and is refused next to the other raw synthetic streams"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('cgg_tools_train_polygons', os.path.join(root, 'tools', 'train.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    assert drv.parse_args(['cfg.py', '--synthetic-polygons', '48x64']).synthetic_polygons == '48x64'
    for other in ('--synthetic-u8', '--synthetic-panoptic'):
        with pytest.raises(SystemExit):
            drv.parse_args(['cfg.py', '--synthetic-polygons', '48x64', other, '48x64'])
