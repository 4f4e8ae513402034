"""CPU tests of the drawing rules (paint.py): the fill against the fixture produced by the reference's own `draw_masks`
(tests/golden/g12_paint.npz, written by tests/golden/make_golden_paint.py), the component labelling against hand-written answers
and scipy, the colour choice, and the argument checks of the new C symbols through the raw ABI."""
import ctypes
import os

import numpy as np
import pytest

import cgg_amd  # noqa: F401
from cgg_amd import _lib, paint

import paint_cases as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g12_paint.npz')


@pytest.mark.parametrize('alpha, tag', [(0.8, 'a08'), (0.5, 'a05'), (1.0, 'a10')])
def test_fill_equals_the_reference_draw_masks(alpha, tag):
    g = np.load(GOLDEN)
    assert g['img'].shape == (24, 40, 3) and g['masks'].shape == (6, 24, 40)
    assert (g['masks'][:3].all(axis=0)).any(), 'three masks share a region'
    got = paint.paint_instances_host(g['img'], g['masks'], g['colors'], alpha=alpha, edges=False)
    assert got.dtype == np.uint8 and np.array_equal(got, g['painted_' + tag])
    packed = pc.pack(g['masks'], 5)
    assert np.array_equal(paint.paint_instances_host(g['img'], packed, g['colors'], alpha=alpha, edges=False), g['painted_' + tag])


def test_adaptive_scales_equal_the_reference():
    g = np.load(GOLDEN)
    assert np.array_equal(paint.adaptive_scales(g['areas']), g['scales'])


def test_edges_and_boxes_known_answers():
    img = np.full((6, 7, 3), 100, np.uint8)
    m = np.zeros((1, 6, 7), bool)
    m[0, 1:5, 1:5] = True
    m[0, 0, 6] = True                                       # a corner pixel: the frame makes it an edge
    got = paint.paint_instances_host(img, m, [[200, 0, 50]], alpha=0.5)
    fill = np.array([150, 50, 75], np.uint8)                # 100 * 0.5 + c * 0.5, exact
    edge = (fill * (1 - 0.8) + np.array([255, 255, 255], np.uint8) * 0.8).astype(np.uint8)
    want = img.copy()
    want[1:5, 1:5] = edge
    want[2:4, 2:4] = fill                                   # the 2 x 2 interior has all four neighbours inside
    want[0, 6] = edge
    assert np.array_equal(got, want)
    # a box: 1-pixel frame of x 1..5, y 2..4; the part outside the image is not drawn; thickness above the box fills it
    none = np.zeros((1, 6, 7), bool)
    box = paint.paint_instances_host(img, none, [[0, 0, 0]], boxes=[[1.9, 2.2, 5.7, 4.9, 0.3]], box_colors=[[0, 255, 10]], thickness=1)
    bc = (np.array([100, 100, 100], np.uint8) * (1 - 0.8) + np.array([0, 255, 10], np.uint8) * 0.8).astype(np.uint8)
    want = img.copy()
    want[2:5, 1:6] = bc
    want[3, 2:5] = 100
    assert np.array_equal(box, want)
    thick = paint.paint_instances_host(img, none, [[0, 0, 0]], boxes=[[-2, 2, 5, 9]], box_colors=[[0, 255, 10]], thickness=5)
    want = img.copy()
    want[2:6, 0:6] = bc
    assert np.array_equal(thick, want)
    kept = paint.paint_instances_host(img, m, [[200, 0, 50]], keep=[0], boxes=[[0, 0, 3, 3]], box_colors=[[1, 2, 3]])
    assert np.array_equal(kept, img)


def test_components_known_answers():
    v = 9
    pan = np.array([[1, v, 1, 1],
                    [v, 1, v, v],
                    [2, v, v, 1],
                    [2, 2, v, 1]], np.int32)
    rec = paint.components_host(pan, v)
    # id 1: (0,0) - (1,1) - (0,2),(0,3) join by diagonals: root 0, area 4, sum_x 0+1+2+3, sum_y 0+1+0+0; the column at x = 3, rows 2..3,
    # is separate (its neighbours (1,2), (1,3), (2,2), (3,2) are void). id 2: root 8, area 3.
    assert rec.dtype == np.int64 and rec.tolist() == [[0, 1, 4, 6, 1], [8, 2, 3, 1, 8], [11, 1, 2, 6, 5]]
    big = paint.largest_components(rec)
    assert big.tolist() == [[0, 1, 4, 6, 1], [8, 2, 3, 1, 8]]
    # equal areas: the smallest root wins, whatever the order of the records
    tie = np.array([[40, 7, 5, 0, 0], [3, 7, 5, 1, 1], [90, 7, 5, 2, 2], [1, 8, 1, 0, 0]], np.int64)
    assert paint.largest_components(tie).tolist() == [[3, 7, 5, 1, 1], [1, 8, 1, 0, 0]]
    # two ids interleaved as a checkerboard: two components, the diagonals of different ids cross
    yy, xx = np.mgrid[0:5, 0:6]
    rec = paint.components_host(np.where((yy + xx) % 2 == 0, 3, 4).astype(np.int32), v)
    assert rec[:, :3].tolist() == [[0, 3, 15], [1, 4, 15]]
    assert paint.components_host(np.full((3, 3), v, np.int32), v).shape == (0, 5)
    # sums beyond 32 bits
    rec = paint.components_host(np.zeros((2048, 4096), np.int32), v)
    assert rec.tolist() == [[0, 0, 2048 * 4096, 2048 * (4095 * 4096 // 2), 4096 * (2047 * 2048 // 2)]] and rec[0, 3] > 2**32


@pytest.mark.parametrize('kind', pc.COMPONENT_KINDS)
@pytest.mark.parametrize('size', pc.COMPONENT_SIZES)
def test_components_equal_scipy(size, kind):
    ndimage = pytest.importorskip('scipy.ndimage')
    c = pc.component_case(size, kind)
    pan = c['pan']
    H, W = pan.shape
    yy, xx = np.mgrid[0:H, 0:W]
    want = []
    for v in np.unique(pan).tolist():
        if v == pc.VOID:
            continue
        lab, k = ndimage.label(pan == v, structure=np.ones((3, 3)))
        for j in range(1, k + 1):
            m = lab == j
            want.append([int((yy[m] * W + xx[m]).min()), v, int(m.sum()), int(xx[m].sum()), int(yy[m].sum())])
    want = np.array(sorted(want), np.int64).reshape(-1, 5)
    assert np.array_equal(c['records'], want)
    # the largest component per id as np.argmax over raster-ordered labels picks it: first maximum in scipy's (raster) label order
    big = paint.largest_components(c['records'])
    for row in big.tolist():
        lab, k = ndimage.label(pan == row[1], structure=np.ones((3, 3)))
        areas = np.bincount(lab.ravel())[1:]
        m = lab == int(np.argmax(areas)) + 1
        assert row[2] == int(m.sum()) and row[0] == int((yy[m] * W + xx[m]).min())


def test_instance_colors():
    labels = np.array([3, 3, 0, 3, 5, 0, 0, 5, 3, 3, 3, 3])
    palette = paint.get_palette(None, 6)
    assert np.array_equal(palette, np.random.RandomState(42).randint(0, 256, (6, 3)).astype(np.uint8))
    a = paint.instance_colors_host(labels, palette, seed=0)
    assert a.dtype == np.uint8 and a.shape == (12, 3)
    assert len({tuple(c) for c in a.tolist()}) == 12, 'two instances share a colour'
    for cls in (3, 0, 5):
        first = int(np.flatnonzero(labels == cls)[0])
        assert np.array_equal(a[first], palette[cls])
        later = a[labels == cls][1:].astype(np.int64)
        assert (np.abs(later - palette[cls].astype(np.int64)) <= 30 * 12).all()
    assert np.array_equal(a, paint.instance_colors_host(labels, palette, seed=0))
    assert not np.array_equal(a, paint.instance_colors_host(labels, palette, seed=1))
    # a single colour and a list of colours, as mask_color / bbox_color are given
    one = paint.instance_colors_host(labels, paint.get_palette((0, 255, 7), 6), seed=0)
    assert np.array_equal(one[0], [0, 255, 7]) and len({tuple(c) for c in one.tolist()}) == 12
    assert one.min() >= 0 and one.max() <= 255
    lst = paint.get_palette([(i, i, i) for i in range(6)], 6)
    assert np.array_equal(paint.instance_colors_host([4, 2], lst), [[4, 4, 4], [2, 2, 2]])
    assert paint.instance_colors_host([], palette).shape == (0, 3)


def test_panoptic_host_rule_known_answer():
    img = np.full((3, 4, 3), 50, np.uint8)
    pan = np.array([[7, 7, 7, 7], [7, 7, 7, 7], [7, 7, 7, 7]], np.int32)
    pan5 = np.pad(pan, 1, constant_values=9)                # a 5 x 6 map: the 7s are away from the frame
    img5 = np.full((5, 6, 3), 50, np.uint8)
    got = paint.paint_panoptic_host(img5, pan5, [7], [[250, 0, 50]], void=9, alpha=0.5)
    fill = np.array([150, 25, 50], np.uint8)
    edge = (fill * (1 - 0.8) + np.array([255, 255, 255], np.uint8) * 0.8).astype(np.uint8)
    want = img5.copy()
    want[1:4, 1:5] = edge
    want[2, 2:4] = fill
    assert np.array_equal(got, want)
    # on the frame every painted pixel of a 3-row map touches the outside or is interior: here only (1, 1) and (1, 2) are interior
    got = paint.paint_panoptic_host(img, pan, [7], [[250, 0, 50]], void=9, alpha=0.5)
    want = np.broadcast_to(edge, img.shape).copy()
    want[1, 1:3] = fill
    assert np.array_equal(got, want)
    assert np.array_equal(paint.paint_panoptic_host(img, pan, [9], [[1, 2, 3]], void=9), img)


def test_new_symbols_check_their_arguments_without_a_device():
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    einval, eunsup = -1, -2
    a, oma = 0.8, 1 - 0.8
    P = lib.cgg_paint_instances_u8
    assert P(null, p, 8, 8, p, 1, 8, 1, p, p, null, null, a, oma, 2, 1, null) == einval          # img
    assert b'null' in lib.cgg_last_error_string()
    assert P(p, null, 8, 8, p, 1, 8, 1, p, p, null, null, a, oma, 2, 1, null) == einval          # out
    assert P(p, p, 8, 8, null, 1, 8, 1, p, p, null, null, a, oma, 2, 1, null) == einval          # bits with n > 0
    assert P(p, p, 8, 8, p, 1, 8, 1, null, p, null, null, a, oma, 2, 1, null) == einval          # keep
    assert P(p, p, 8, 8, p, 1, 8, 1, p, null, null, null, a, oma, 2, 1, null) == einval          # colors
    assert P(p, p, 8, 8, p, 1, 8, 1, p, p, p, null, a, oma, 2, 1, null) == einval                # boxes without box_colors
    assert P(p, p, 0, 8, p, 1, 8, 1, p, p, null, null, a, oma, 2, 1, null) == einval             # H < 1
    assert P(p, p, 8, 0, p, 1, 8, 1, p, p, null, null, a, oma, 2, 1, null) == einval             # W < 1
    assert P(p, p, 8, 8, p, -1, 8, 1, p, p, null, null, a, oma, 2, 1, null) == einval            # n < 0
    assert P(p, p, 8, 9, p, 1, 8, 1, p, p, null, null, a, oma, 2, 1, null) == einval             # row_bytes * 8 < W
    assert P(p, p, 8, 8, p, 1, 7, 1, p, p, null, null, a, oma, 2, 1, null) == einval             # mask stride < H * row_bytes
    assert P(p, p, 8, 8, p, 1, 8, 1, p, p, null, null, a, oma, -1, 1, null) == einval            # thickness < 0
    assert P(p, p, 8, 8, p, 1, 8, 1, p, p, null, null, 1.5, oma, 2, 1, null) == einval           # alpha > 1
    assert P(p, p, 8, 8, p, 1, 8, 1, p, p, null, null, a, -0.1, 2, 1, null) == einval            # 1 - alpha < 0
    assert P(p, p, 8, 8, p, 1025, 8, 1, p, p, null, null, a, oma, 2, 1, null) == eunsup          # n > 1024
    assert b'1024' in lib.cgg_last_error_string()
    assert P(p, p, 1 << 15, (1 << 15) + 8, p, 1, 1 << 28, 1 << 13, p, p, null, null, a, oma, 2, 1, null) == eunsup      # > 2^31 bytes
    B = lib.cgg_pack_bool_rows_u8
    assert B(null, 4, 8, 1, p, null) == einval and B(p, 4, 8, 1, null, null) == einval
    assert B(p, -1, 8, 1, p, null) == einval and B(p, 4, 0, 1, p, null) == einval and B(p, 4, 9, 1, p, null) == einval
    assert B(null, 0, 8, 1, null, null) == 0                                                     # nothing to do
    L = lib.cgg_label_components_i32
    assert lib.cgg_label_components_workspace_bytes(65, 129) == 65 * 129 * 24
    assert lib.cgg_label_components_workspace_bytes(0, 5) == 0 and lib.cgg_label_components_workspace_bytes(1 << 16, 1 << 15) == 0
    assert L(null, 8, 8, 80, p, p, 4, p, null) == einval                                         # pan
    assert L(p, 8, 8, 80, null, p, 4, p, null) == einval                                         # ws
    assert L(p, 8, 8, 80, p, null, 4, p, null) == einval                                         # records with capacity > 0
    assert L(p, 8, 8, 80, p, p, 4, null, null) == einval                                         # status
    assert L(p, 0, 8, 80, p, p, 4, p, null) == einval and L(p, 8, 0, 80, p, p, 4, p, null) == einval
    assert L(p, 8, 8, 80, p, p, -1, p, null) == einval                                           # capacity < 0
    assert L(p, 8, 8, 80, odd, p, 4, p, null) == einval and L(p, 8, 8, 80, p, odd, 4, p, null) == einval      # misaligned
    assert L(p, 1 << 16, 1 << 15, 80, p, p, 4, p, null) == eunsup                                # H * W = 2^31
    assert b'31 bits' in lib.cgg_last_error_string()
    Q = lib.cgg_paint_panoptic_u8
    assert Q(null, p, p, 8, 8, p, p, 1, a, oma, 1, null) == einval and Q(p, null, p, 8, 8, p, p, 1, a, oma, 1, null) == einval
    assert Q(p, p, null, 8, 8, p, p, 1, a, oma, 1, null) == einval
    assert Q(p, p, p, 8, 8, null, p, 1, a, oma, 1, null) == einval and Q(p, p, p, 8, 8, p, null, 1, a, oma, 1, null) == einval
    assert Q(p, p, p, 0, 8, p, p, 1, a, oma, 1, null) == einval and Q(p, p, p, 8, 0, p, p, 1, a, oma, 1, null) == einval
    assert Q(p, p, p, 8, 8, p, p, -1, a, oma, 1, null) == einval
    assert Q(p, p, p, 8, 8, p, p, 1, 2.0, oma, 1, null) == einval
    assert Q(p, p, p, 8, 8, p, p, 1025, a, oma, 1, null) == eunsup
    assert Q(p, p, p, 1 << 15, (1 << 15) + 8, p, p, 1, a, oma, 1, null) == eunsup


def test_wrappers_refuse_what_the_kernels_cannot_read():
    import torch
    from cgg_amd import ops
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    bits = torch.zeros(1, 8, 1, dtype=torch.uint8)
    assert not ops.paint_instances_ok(img, bits)                                                 # not on a device
    with pytest.raises(_lib.CggError, match='gate'):
        ops.paint_instances(img, bits, torch.ones(1, dtype=torch.uint8), torch.zeros(1, 3, dtype=torch.uint8))
    assert not ops.label_components_ok(torch.zeros(8, 8, dtype=torch.int32))
    with pytest.raises(_lib.CggError):
        ops.label_components(torch.zeros(8, 8, dtype=torch.int32), 80)
    with pytest.raises(_lib.CggError, match='gate'):
        ops.paint_panoptic(img, torch.zeros(8, 8, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 3, dtype=torch.uint8))
    with pytest.raises(_lib.CggError):
        ops.pack_bool_masks(torch.zeros(1, 8, 8, dtype=torch.uint8))


def test_show_result_on_the_host(tmp_path):
    """A detector that was never moved to a device paints by the host rules: host-form results, both heads."""
    from types import SimpleNamespace
    from PIL import Image
    c = pc.instance_case((19, 37), 3, (0.8, 2))
    model = SimpleNamespace(parameters=lambda: iter(()), num_classes=pc.VOID)
    labels = [2, 0, 2]
    bbox_result = [c['boxes'][[1]], np.zeros((0, 5), np.float32), c['boxes'][[0, 2]]]
    mask_result = [[c['masks'][1]], [], [c['masks'][0], c['masks'][2]]]
    result = dict(all_results=(bbox_result, mask_result))
    got = paint.show_instances(model, c['img'], result, score_thr=0, show_labels=False)
    order = [1, 0, 2]                                       # by class, within a class in result order
    colors = paint.instance_colors_host([0, 2, 2], paint.get_palette(None, 3))
    box_colors = np.tile(np.array([[72, 101, 241]], np.uint8), (3, 1))
    want = paint.paint_instances_host(c['img'], c['masks'][order], colors, None, c['boxes'][order], box_colors)
    assert np.array_equal(got, want)
    none = paint.show_instances(model, c['img'], result, score_thr=0.9, show_labels=False)      # every score is 0.5
    assert np.array_equal(none, c['img'])
    out = tmp_path / 'sub' / 'painted.png'
    assert paint.show_instances(model, c['img'], result, score_thr=0, out_file=str(out)) is None
    with Image.open(out) as im:
        back = np.asarray(im.convert('RGB'))[:, :, ::-1]
    assert back.shape == c['img'].shape and back.dtype == np.uint8
    p = pc.panoptic_case((65, 129), 'all_but_void')
    got = paint.show_panoptic(model, p['img'], dict(panoptic_all_results=p['pan'].astype(np.int64)), show_labels=False)
    ids = p['ids']
    want = paint.paint_panoptic_host(p['img'], p['pan'], ids, paint.instance_colors_host(ids % 1000, paint.get_palette(None, 80)), pc.VOID)
    assert np.array_equal(got, want)
    labelled = paint.show_panoptic(model, p['img'], dict(panoptic_all_results=p['pan']))
    assert labelled.shape == p['img'].shape and labelled.dtype == np.uint8


def test_show_true_uses_matplotlib_or_raises_by_name(monkeypatch):
    """`show=True`: a window through matplotlib.pyplot where it is importable, CggError naming matplotlib where it is not; `out_file`
    switches the window off."""
    import sys
    import types
    from types import SimpleNamespace
    c = pc.instance_case((19, 37), 3, (0.8, 2))
    model = SimpleNamespace(parameters=lambda: iter(()), num_classes=pc.VOID)
    result = dict(all_results=([c['boxes']], [list(c['masks'])]))
    monkeypatch.setitem(sys.modules, 'matplotlib', None)              # `import matplotlib.pyplot` now raises ImportError
    monkeypatch.setitem(sys.modules, 'matplotlib.pyplot', None)
    with pytest.raises(_lib.CggError, match='matplotlib'):
        paint.show_instances(model, c['img'], result, score_thr=0, show_labels=False, show=True)
    with pytest.raises(_lib.CggError, match='matplotlib'):
        paint.show_panoptic(model, c['img'], dict(panoptic_all_results=np.zeros((19, 37), np.int32)), show_labels=False, show=True)
    calls = []
    plt = types.ModuleType('matplotlib.pyplot')
    for name in ('figure', 'imshow', 'axis', 'show', 'pause', 'close'):
        setattr(plt, name, lambda *a, _n=name, **k: calls.append((_n, a, k)))
    mpl = types.ModuleType('matplotlib')
    mpl.pyplot = plt
    monkeypatch.setitem(sys.modules, 'matplotlib', mpl)
    monkeypatch.setitem(sys.modules, 'matplotlib.pyplot', plt)
    want = paint.show_instances(model, c['img'], result, score_thr=0, show_labels=False)
    assert paint.show_instances(model, c['img'], result, score_thr=0, show_labels=False, show=True, win_name='w') is None
    assert [n for n, _, _ in calls] == ['figure', 'imshow', 'axis', 'show', 'close']
    assert calls[0][1] == ('w',) and np.array_equal(calls[1][1][0], want) and calls[3][2] == {}       # wait_time 0: a blocking show
    del calls[:]
    assert paint.show_instances(model, c['img'], result, score_thr=0, show_labels=False, show=True, wait_time=0.5) is None
    assert [n for n, _, _ in calls] == ['figure', 'imshow', 'axis', 'show', 'pause', 'close']
    assert calls[3][2] == dict(block=False) and calls[4][1] == (0.5,)


def test_ids_outside_int32_are_seen_before_the_conversion():
    import torch
    ok = np.array([[0, 2**31 - 1], [-2**31, 5]], np.int64)
    assert paint._fits_int32(ok) and paint._fits_int32(torch.from_numpy(ok)) and paint._fits_int32(ok.astype(np.int32))
    for bad in (2**31, 2**40 + 7, -2**31 - 1):
        m = ok.copy()
        m[1, 1] = bad
        assert not paint._fits_int32(m) and not paint._fits_int32(torch.from_numpy(m))
    assert not paint._fits_int32(ok.astype(np.float32))
