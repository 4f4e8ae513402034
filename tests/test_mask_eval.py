"""CPU tests of the COCO mask evaluation: the numpy rules of `cgg_amd.mask_eval` reproduce, exactly, what the reference's own
cocoeval.py recorded in tests/golden/g13_segm_eval.npz (per-image match records, precision, recall and scores -- float64 arrays
bit for bit, both sides do the same float64 operations -- in the normal and the class-agnostic run); the intersections agree with
unpacked bool arithmetic whatever the pad bits hold; the two C entry points return their documented error codes without a
device; `SegmEvaluator(device=None)` end to end gives the recorded base / novel / all AP50."""
import ctypes

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import _lib, mask_eval, ops

import mask_eval_cases as C


@pytest.fixture(scope='module')
def host_runs():
    """per mode: the host rule's per-image records of the fixture (computed once)"""
    z = C.fixture()
    return {tag: [C.host_records(im, int(z['W']), agn, z['cat_ids'], z['area_rngs'], z['iou_thrs'], int(z['max_dets'][-1]))[0]
                  for im in C.fixture_images()] for tag, agn in C.MODES}


@pytest.mark.parametrize('tag', [m[0] for m in C.MODES])
def test_evaluate_img_host_equals_the_reference_records(host_runs, tag):
    want = C.fixture_records(tag)
    n = 0
    for i, rec in enumerate(host_runs[tag]):
        C.assert_records_equal(rec, want[i], (tag, i))
        for k, per_area in enumerate(rec):
            for a, r in enumerate(per_area):
                if r is None:
                    continue
                n += 1
                assert r['dt_scores'].tobytes() == want[i][k][a]['dt_scores'].astype(np.float64).tobytes()
                assert np.array_equal(r['dt_index'] + 1, want[i][k][a]['dt_ids'])       # the generator numbers a detection index + 1
                # the generator numbers a ground truth index + 1: the reference's stored ids ARE the rule's index + 1
                assert set(np.unique(r['dt_match'])) <= set(want[i][k][a]['gt_ids'].tolist()) | {0}
    assert n == int(C.fixture()[tag + 'present'].sum()) and n > 40


def test_fixture_holds_the_cases_it_was_built_for():
    z = C.fixture()
    imgs = C.fixture_images()
    W = int(z['W'])
    assert (int(z['H']), W) == (37, 45) and z['det_bits'].shape[2] == 6
    assert len(imgs[2]['gt_cats']) == 0 and len(imgs[2]['det_cats']) > 0 and len(imgs[3]['det_cats']) == 0 and len(imgs[3]['gt_cats']) > 0
    assert 5 not in z['gt_cats'] and 5 in z['det_cats'] and 8 in z['gt_cats'] and 8 not in z['det_cats']
    assert (imgs[0]['det_cats'] == 1).sum() > int(z['max_dets'][-1])
    inter, area_d, area_g = mask_eval.mask_intersections_host(imgs[1]['det_bits'], imgs[1]['gt_bits'], W)
    iou = mask_eval.mask_iou_host(inter, area_d, area_g, imgs[1]['gt_crowd'])
    assert iou[0, 0] == iou[0, 1] == 0.8                                     # two ground truths, equal IoU to one detection
    assert (inter[2, 2], area_d[2], area_g[2], iou[2, 2]) == (1, 2, 1, 0.5)    # sits on the threshold
    inter0 = mask_eval.mask_intersections_host(imgs[0]['det_bits'], imgs[0]['gt_bits'], W)[0]
    assert imgs[0]['gt_crowd'][1] and (inter0[:, 1] > 0).sum() >= 2            # a crowd overlapped by two detections
    assert (z['gt_area'] > 1024).any() and (z['gt_area'] < 1024).any() and (z['gt_area'] == 1024).any()
    s = imgs[0]['det_scores'][imgs[0]['det_cats'] == 1]
    assert len(np.unique(s)) < len(s)                                          # equal scores within a category
    # the threshold-sitting pair matches at 0.5 and not above; the later of the two equal ground truths wins
    rec = C.fixture_records('std_')[1][2][0]
    assert rec['dt_match'][0].tolist() == [2, 3, 1] and rec['dt_match'][1].tolist() == [2, 0, 1]


@pytest.mark.parametrize('tag', [m[0] for m in C.MODES])
def test_accumulate_host_equals_the_reference_bit_for_bit(host_runs, tag):
    z = C.fixture()
    K, A, T = len(z['cat_ids']), len(z['area_rngs']), len(z['iou_thrs'])
    precision, recall, scores = mask_eval.accumulate_host(host_runs[tag], K, A, z['max_dets'], T, z['rec_thrs'])
    for name, got in (('precision', precision), ('recall', recall), ('scores', scores)):
        want = z[tag + name]
        assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
        assert got.tobytes() == want.tobytes(), name
    assert (precision > -1).any() and (precision == -1).any()
    # accumulate from the RECORDED per-image results too: the two halves of the rule are each pinned to the reference
    p2, r2, s2 = mask_eval.accumulate_host(C.fixture_records(tag), K, A, z['max_dets'], T, z['rec_thrs'])
    assert p2.tobytes() == z[tag + 'precision'].tobytes() and r2.tobytes() == z[tag + 'recall'].tobytes()
    assert s2.tobytes() == z[tag + 'scores'].tobytes()


def test_default_thresholds_are_the_reference_s():
    z = C.fixture()
    assert mask_eval.default_iou_thrs().tobytes() == z['iou_thrs'].tobytes()
    assert mask_eval.default_rec_thrs().tobytes() == z['rec_thrs'].tobytes()
    assert np.asarray(mask_eval.AREA_RNGS, np.float64).tobytes() == z['area_rngs'].tobytes()


@pytest.mark.parametrize('D,G,H,W,rb', [(5, 7, 37, 45, 6), (3, 4, 9, 64, 8), (4, 2, 5, 33, 7), (0, 3, 8, 8, 1), (3, 0, 8, 8, 1),
                                        (1, 1, 1, 1, 1)])
def test_mask_intersections_host_against_bool_arithmetic_with_garbage_pad_bits(D, G, H, W, rb):
    rs = np.random.RandomState(D * 100 + G * 10 + W)
    d, g = rs.rand(D, H, W) < 0.4, rs.rand(G, H, W) < 0.6
    bits = []
    for m in (d, g):
        b = rs.randint(0, 256, size=(m.shape[0], H, rb)).astype(np.uint8)              # garbage everywhere ...
        packed = np.packbits(m, axis=2, bitorder='little')
        nb = packed.shape[2]
        keep = np.zeros(rb, np.uint8)
        keep[:nb] = 255
        if W & 7:
            keep[nb - 1] = (1 << (W & 7)) - 1
        b &= ~keep                                                                     # ... except where pixels are
        b[:, :, :nb] |= packed
        bits.append(b)
    inter, area_d, area_g = mask_eval.mask_intersections_host(bits[0], bits[1], W)
    assert inter.dtype == np.int64 and inter.shape == (D, G)
    want = (d[:, None] & g[None]).reshape(D, G, H * W).sum(-1)
    assert np.array_equal(inter, want)
    assert np.array_equal(area_d, d.reshape(D, H * W).sum(-1)) and np.array_equal(area_g, g.reshape(G, H * W).sum(-1))
    if W & 7 or rb * 8 > W:
        assert bits[0].size == 0 or not np.array_equal(bits[0], np.packbits(d, axis=2, bitorder='little'))


def test_mask_iou_host_is_the_rleiou_rule():
    inter = np.array([[1, 0, 3], [0, 0, 2]])
    iou = mask_eval.mask_iou_host(inter, [2, 0], [1, 0, 4], [False, False, True])
    assert iou.dtype == np.float64
    assert iou.tolist() == [[0.5, 0.0, 1.5], [0.0, 0.0, 0.0]]          # crowd: inter / area_d; empty denominators: 0
    assert mask_eval.mask_iou_host(np.array([[1]]), [3], [1], [False])[0, 0] == np.float64(1) / np.float64(3)


def test_evaluate_img_host_returns_none_where_the_reference_does():
    rec = mask_eval.evaluate_img_host(np.zeros((0, 0)), [], [], [], [], [], [], [1, 2], mask_eval.AREA_RNGS, [0.5], 10, False)
    assert rec == [[None] * 4, [None] * 4]
    # class-agnostic: a detection of another category still makes every category's record
    rec = mask_eval.evaluate_img_host(np.zeros((1, 0)), [0.5], [2], [], [], [], [10], [1, 2], mask_eval.AREA_RNGS, [0.5], 10, True)
    assert all(r is not None and r['dt_match'].shape == (1, 1) for per_area in rec for r in per_area)


def test_c_abi_error_codes_without_a_device():
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 1)
    I = lib.cgg_mask_intersections_bits

    def inter(det=p, D=2, ds=16, gt=p, G=2, gs=16, H=8, W=12, rb=2, ws=p, out=p, ad=p, ag=p):
        return I(det, D, ds, gt, G, gs, H, W, rb, ws, out, ad, ag, null)

    assert inter(det=null) == -1 and b'null' in lib.cgg_last_error_string()
    assert inter(gt=null) == -1 and inter(ws=null) == -1 and inter(out=null) == -1 and inter(ad=null) == -1 and inter(ag=null) == -1
    assert inter(rb=1) == -1                       # row_bytes * 8 < W
    assert inter(ds=15) == -1 and inter(gs=15) == -1   # a stride below H * row_bytes
    assert inter(ws=odd) == -1 and b'aligned' in lib.cgg_last_error_string()
    assert inter(D=-1) == -1 and inter(H=0) == -1 and inter(W=0) == -1
    assert inter(D=1025) == -2 and inter(G=1025) == -2
    assert inter(H=1 << 16, W=1 << 15, rb=1 << 12, ds=1 << 28, gs=1 << 28) == -2          # H * W = 2^31
    assert inter(D=0, G=0, det=null, gt=null, ws=null, out=null, ad=null, ag=null) == 0   # legal, launches nothing
    wsb = lib.cgg_mask_intersections_workspace_bytes
    assert wsb(100, 30, 1024, 1024) == 512 * (100 * 30 + 130) * 4 and wsb(1024, 1024, 8, 8) == 4 * (1024 * 1024 + 2048) * 4
    assert wsb(0, 0, 8, 8) == 0 and wsb(1025, 1, 8, 8) == 0 and wsb(0, 3, 8, 8) == 1024 * 3 * 4

    M = lib.cgg_coco_match

    def match(inter=p, ad=p, ag=p, order=p, dc=p, gc=p, crowd=p, area=p, cats=p, K=2, rngs=p, A=4, thrs=p, T=10, D=2, G=2, max_det=10,
              dtm=p, dti=p, gti=p, counts=p):
        return M(inter, ad, ag, order, dc, gc, crowd, area, cats, K, rngs, A, thrs, T, D, G, max_det, 0, dtm, dti, gti, counts, null)

    for name in ('inter', 'ad', 'ag', 'order', 'dc', 'gc', 'crowd', 'area', 'cats', 'rngs', 'thrs', 'dtm', 'dti', 'gti', 'counts'):
        assert match(**{name: null}) == -1, name
    assert match(K=0) == -1 and match(A=0) == -1 and match(T=0) == -1 and match(D=-1) == -1 and match(max_det=-1) == -1
    assert match(area=odd) == -1
    assert match(T=65) == -2 and match(A=9) == -2 and match(K=1025) == -2 and match(D=1025) == -2 and match(G=1025) == -2


def test_ops_gate_and_cpu_tensors():
    assert ops.mask_eval_ok(0, 0, 1, 1) and ops.mask_eval_ok(1024, 1024, 1024, 1024) and ops.mask_eval_ok(1, 1, 1 << 15, (1 << 16) - 1)
    assert not ops.mask_eval_ok(1025, 1, 8, 8) and not ops.mask_eval_ok(1, 1025, 8, 8) and not ops.mask_eval_ok(1, 1, 1 << 15, 1 << 16)
    with pytest.raises(_lib.CggError, match='ROCm device'):
        ops.mask_intersections(torch.zeros(1, 8, 1, dtype=torch.uint8), torch.zeros(1, 8, 1, dtype=torch.uint8), 8)
    with pytest.raises(_lib.CggError, match='uint8'):
        ops.mask_intersections(torch.zeros(1, 8, 8, dtype=torch.bool), torch.zeros(1, 8, 1, dtype=torch.uint8), 8)


def _fixture_evaluator(class_agnostic, device=None):
    z = C.fixture()
    ev = mask_eval.SegmEvaluator(z['cat_ids'], unknown_cat_ids=z['unknown_cat_ids'], all_cat_ids=z['all_cat_ids'], max_dets=z['max_dets'],
                                 class_agnostic=class_agnostic, device=device)
    W = int(z['W'])
    label_of = {int(c): i for i, c in enumerate(z['cat_ids'])}
    for im in C.fixture_images():
        D = len(im['det_cats'])
        boxes = np.zeros((D, 5), np.float32)
        boxes[:, 4] = im['det_scores']
        gt = np.unpackbits(im['gt_bits'], axis=2, bitorder='little')[:, :, :W].astype(bool)
        ev.add(torch.tensor([label_of[int(c)] for c in im['det_cats']], dtype=torch.int64), torch.from_numpy(boxes),
               torch.from_numpy(im['det_bits']), gt, im['gt_cats'], im['gt_crowd'], im['gt_area'])
    return ev


@pytest.mark.parametrize('tag,agn', C.MODES)
def test_segm_evaluator_on_the_host_end_to_end(tag, agn):
    z = C.fixture()
    res = _fixture_evaluator(agn).summarize()
    for name in ('precision', 'recall', 'scores'):
        assert res[name].tobytes() == z[tag + name].tobytes(), name
    assert res['images'] == 6 and len(res['stats']) == 12
    assert (res['base_ap50'], res['novel_ap50'], res['all_ap50']) == tuple(z[tag + 'open_set_ap50'])
    # coco_open.py:583-637 by hand on the recorded precision: categories 1, 2 are base, 3, 8 novel, 5 is absent from the dataset
    per_cat = []
    for idx in range(5):
        r = z[tag + 'precision'][0, :, idx, 0, -1]
        per_cat.append(r[r > -1].mean() if (r > -1).any() else None)
    base = [per_cat[i] for i in (0, 1) if per_cat[i] is not None]
    novel = [per_cat[i] for i in (2, 4) if per_cat[i] is not None]
    assert res['base_ap50'] == np.array(base).mean() * 100 and res['novel_ap50'] == np.array(novel).mean() * 100
    assert res['all_ap50'] == np.array(base + novel).mean() * 100
    assert res['stats']['AP50'] == np.mean(z[tag + 'precision'][0][..., 0, -1][z[tag + 'precision'][0][..., 0, -1] > -1])


def test_segm_evaluator_defaults_and_skip_rule():
    z = C.fixture()
    ev = mask_eval.SegmEvaluator([1, 2])
    assert ev.max_dets == [100, 300, 1000] and ev.iou_thrs.tobytes() == z['iou_thrs'].tobytes() and ev.all_cat_ids == [1, 2]
    ev = mask_eval.SegmEvaluator([1, 2], skip_images_without_gt=True)
    bits = torch.zeros(1, 4, 1, dtype=torch.uint8)
    ev.add(torch.zeros(1, dtype=torch.int64), torch.ones(1, 5), bits, np.ones((1, 4, 8), bool), np.array([7]))    # no ground truth of 1, 2
    assert ev.records == []
    ev.add(torch.zeros(1, dtype=torch.int64), torch.ones(1, 5), bits, np.ones((1, 4, 8), bool), np.array([2]))
    assert len(ev.records) == 1
    with pytest.raises(ValueError, match='do not cover'):
        ev.add(torch.zeros(1, dtype=torch.int64), torch.ones(1, 5), bits, np.ones((1, 4, 9), bool), np.array([2]))


def test_segm_evaluator_takes_bool_bitmaps_for_the_detections():
    """a result whose geometry the head's bit-packing gate declines carries (D, H, W) bool masks: they are packed, not reinterpreted"""
    rs = np.random.RandomState(2)
    det, gt = rs.rand(3, 9, 21) < 0.5, rs.rand(2, 9, 21) < 0.5
    boxes = torch.rand(3, 5)
    a, b = mask_eval.SegmEvaluator([1, 2]), mask_eval.SegmEvaluator([1, 2])
    a.add(torch.tensor([0, 1, 0]), boxes, torch.from_numpy(det), gt, np.array([1, 2]))
    b.add(torch.tensor([0, 1, 0]), boxes, torch.from_numpy(mask_eval.pack_bool_rows_host(det)), gt, np.array([1, 2]))
    C.assert_records_equal(a.records[0], b.records[0])
    assert a.records[0][0][0]['dt_match'].shape == (10, 2)
