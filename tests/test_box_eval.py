"""CPU tests of the COCO box evaluation (`--eval bbox`): the numpy rules of `cgg_amd.mask_eval` reproduce, field for field, what the
reference's own cocoeval.py recorded with iouType 'bbox' in tests/golden/g15_bbox_eval.npz (per-image match records, precision,
recall, scores, open-set AP50; both runs); `box_iou_host` equals an exact-rational evaluation rounded once per operation, on a
case set that holds enough contraction-sensitive pairs for the device equality to see a contracted kernel; the two C entry points
return their documented error codes without a device; `BboxEvaluator(device=None)` image by image equals the one-shot run."""
import ctypes

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import _lib, mask_eval, ops

import box_eval_cases as C


@pytest.fixture(scope='module')
def host_runs():
    """per mode: the host rule's per-image records of the fixture (computed once)"""
    z = C.fixture()
    return {tag: [C.host_records(im, agn, z['cat_ids'], z['area_rngs'], z['iou_thrs'], int(z['max_dets'][-1]))[0]
                  for im in C.fixture_images()] for tag, agn in C.MODES}


@pytest.mark.parametrize('tag', [m[0] for m in C.MODES])
def test_evaluate_img_host_on_box_ious_equals_the_reference_records(host_runs, tag):
    z = C.fixture()
    want = C.fixture_records(tag)
    present = np.zeros(z[tag + 'present'].shape, bool)
    for i, rec in enumerate(host_runs[tag]):
        C.assert_records_equal(rec, want[i], (tag, i))
        for k, per_area in enumerate(rec):
            for a, r in enumerate(per_area):
                present[k, a, i] = r is not None
                if r is None:
                    continue
                assert r['dt_scores'].tobytes() == want[i][k][a]['dt_scores'].astype(np.float64).tobytes()
                assert np.array_equal(r['dt_index'] + 1, want[i][k][a]['dt_ids'])       # the generator numbers a detection index + 1
                assert set(np.unique(r['dt_match'])) <= set(want[i][k][a]['gt_ids'].tolist()) | {0}
    assert np.array_equal(present, z[tag + 'present']) and present.sum() > 40


def test_fixture_holds_the_cases_it_was_built_for():
    z = C.fixture()
    imgs = C.fixture_images()
    assert len(imgs) == 6 and z['max_dets'].tolist() == [1, 3, 10]
    assert len(imgs[2]['gt_cats']) == 0 and len(imgs[2]['det_cats']) > 0 and len(imgs[3]['det_cats']) == 0 and len(imgs[3]['gt_cats']) > 0
    assert 5 not in z['gt_cats'] and 5 in z['det_cats'] and 8 in z['gt_cats'] and 8 not in z['det_cats']
    assert (imgs[0]['det_cats'] == 1).sum() > int(z['max_dets'][-1])           # more detections of a category than every max_dets
    assert z['det_boxes5'].dtype == np.float32 and np.array_equal(z['det_boxes5'][:, :4], np.round(z['det_boxes5'][:, :4]))
    assert z['gt_boxes'].dtype == np.float64 and np.array_equal(z['gt_boxes'], np.round(z['gt_boxes'], 2))
    assert (z['gt_boxes'] != np.round(z['gt_boxes'])).any()
    _, iou, det, _ = C.host_records(imgs[1], False, z['cat_ids'], z['area_rngs'], z['iou_thrs'], 10)
    g = imgs[1]['gt_boxes']
    assert det[0, 0] + det[0, 2] == g[0, 0] and iou[0, 0] == 0.0               # the pair only touches: w == 0 exactly
    assert iou[1, 1] == 0.5                                                    # sits on the threshold
    assert iou[2, 2] == iou[2, 3] == np.float64(360) / np.float64(440)         # two ground truths, equal IoU to one detection
    iou0 = C.host_records(imgs[0], False, z['cat_ids'], z['area_rngs'], z['iou_thrs'], 10)[1]
    assert imgs[0]['gt_crowd'][1] and (iou0[:, 1] > 0).sum() >= 2              # a crowd overlapped by two detections
    assert (imgs[0]['det_boxes5'][3, :4] == 0).all() and not iou0[3].any()     # the empty-mask box
    for bound in (32.0 ** 2, 96.0 ** 2):
        assert {bound - 0.5, bound, bound + 0.5} <= set(z['gt_area'].tolist())
    s = imgs[0]['det_scores'][imgs[0]['det_cats'] == 1]
    assert len(np.unique(s)) < len(s)                                          # equal scores within a category
    # the touching pair never matches, the threshold-sitting pair matches at 0.5 only, the later of the two equal ground truths wins
    rec = C.fixture_records('std_')[1][2][0]
    assert rec['dt_match'][0].tolist() == [0, 4, 2] and rec['dt_match'][1].tolist() == [0, 4, 0]


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
    got = mask_eval.open_set_ap_host(precision, z['cat_ids'].tolist(), z['unknown_cat_ids'].tolist(), z['all_cat_ids'].tolist())
    assert np.array(got).tobytes() == z[tag + 'open_set_ap50'].tobytes()


def test_det_boxes_xywh_host_is_xyxy2xywh_on_widened_coordinates():
    b = np.array([[0.1, 0.2, 10.3, 7.7, 0.9], [3, 4, 3, 4, 0.5]], np.float32)
    got = mask_eval.det_boxes_xywh_host(b)
    assert got.dtype == np.float64 and got.shape == (2, 4)
    for row, src in zip(got, b):
        x0, y0, x1, y1 = (float(v) for v in src[:4])           # `tolist()`: float32 -> Python float
        assert row.tolist() == [x0, y0, x1 - x0, y1 - y0]
    assert got[0, 2] != np.float64(np.float32(10.3) - np.float32(0.1))        # the subtraction is float64's, not float32's
    assert mask_eval.det_boxes_xywh_host(np.zeros((0, 5), np.float32)).shape == (0, 4)


def test_box_iou_host_equals_the_rule_on_exact_rationals():
    det5, gt, crowd = C.case_boxes()
    rule, _ = C.case_iou_exact()
    got = mask_eval.box_iou_host(mask_eval.det_boxes_xywh_host(det5), gt, crowd)
    assert got.dtype == np.float64 and got.shape == (30, 14)
    assert got.tobytes() == rule.tobytes()
    assert got[0, 0] == 0.0 and got[1, 1] == 0.5 and not got[2].any()          # touching, on the threshold, the empty box
    assert (got[:, crowd] > 0).sum() >= 4 and (got > 0).sum() > 100
    assert mask_eval.box_iou_host(np.zeros((0, 4)), gt, crowd).shape == (0, 14)
    assert mask_eval.box_iou_host(mask_eval.det_boxes_xywh_host(det5), np.zeros((0, 4)), []).shape == (30, 0)


def test_case_set_holds_contraction_sensitive_pairs():
    """A condition on the inputs, not a measurement: for at least 8 overlapping pairs, a union formed as ONE fused
    (da + ga) - w * h gives another double quotient than the rule's. Without them the exact device comparison could not tell a
    contracted kernel from the rule. Counted on rationals (this Python has no math.fma)."""
    rule, fused = C.case_iou_exact()
    sensitive = (rule != fused) & (rule > 0)
    print('contraction-sensitive pairs:', int(sensitive.sum()), 'of', int((rule > 0).sum()), 'overlapping')
    assert sensitive.sum() >= 8


def test_c_abi_error_codes_without_a_device():
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 8 == 0
    odd = ctypes.c_void_p(p.value + 1)
    four = ctypes.c_void_p(p.value + 4)

    def iou(det=p, D=2, gt=p, crowd=p, G=2, out=p, ad=p):
        return lib.cgg_box_iou_f64(det, D, gt, crowd, G, out, ad, null)

    for name in ('det', 'gt', 'crowd', 'out', 'ad'):
        assert iou(**{name: null}) == -1, name
    assert b'null' in lib.cgg_last_error_string()
    assert iou(D=-1) == -1 and iou(G=-1) == -1
    assert iou(det=odd) == -1 and iou(gt=four) == -1 and iou(out=four) == -1 and iou(ad=four) == -1
    assert b'aligned' in lib.cgg_last_error_string()
    assert iou(D=1025) == -2 and iou(G=1025) == -2
    assert iou(D=0, det=null, out=null, ad=null) == 0 and iou(D=0, G=0, det=null, gt=null, crowd=null, out=null, ad=null) == 0

    def match(det=p, gt=p, order=p, dc=p, gc=p, crowd=p, area=p, cats=p, K=2, rngs=p, A=4, thrs=p, T=10, D=2, G=2, max_det=10,
              dtm=p, dti=p, gti=p, counts=p):
        return lib.cgg_coco_match_boxes(det, gt, order, dc, gc, crowd, area, cats, K, rngs, A, thrs, T, D, G, max_det, 0, dtm, dti, gti,
                                        counts, null)

    for name in ('det', 'gt', 'order', 'dc', 'gc', 'crowd', 'area', 'cats', 'rngs', 'thrs', 'dtm', 'dti', 'gti', 'counts'):
        assert match(**{name: null}) == -1, name
    assert match(K=0) == -1 and match(A=0) == -1 and match(T=0) == -1 and match(D=-1) == -1 and match(max_det=-1) == -1
    assert match(area=four) == -1 and match(gt=four) == -1 and match(det=odd) == -1
    assert match(T=65) == -2 and match(A=9) == -2 and match(K=1025) == -2 and match(D=1025) == -2 and match(G=1025) == -2


def test_ops_gate_and_cpu_tensors():
    assert ops.box_eval_ok(0, 0) and ops.box_eval_ok(1024, 1024)
    assert not ops.box_eval_ok(1025, 1) and not ops.box_eval_ok(1, 1025)
    det, gt, crowd = torch.zeros(2, 5), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, dtype=torch.uint8)
    with pytest.raises(_lib.CggError, match='ROCm device'):
        ops.box_iou(det, gt, crowd)
    with pytest.raises(_lib.CggError, match='float32'):
        ops.box_iou(det.double(), gt, crowd)
    with pytest.raises(_lib.CggError, match=r'\(D, 5\)'):
        ops.box_iou(torch.zeros(2, 4), gt, crowd)
    with pytest.raises(_lib.CggError, match='kernel gate'):
        ops.box_iou(torch.zeros(1025, 5), gt, crowd)
    with pytest.raises(_lib.CggError, match=r'\(G, 4\)'):
        ops.coco_match_boxes(det, torch.zeros(3, 5, dtype=torch.float64), None, None, None, crowd, None, None, None, None, 10, False)


def _evaluator(class_agnostic, **kw):
    z = C.fixture()
    return mask_eval.BboxEvaluator(z['cat_ids'], unknown_cat_ids=z['unknown_cat_ids'], all_cat_ids=z['all_cat_ids'],
                                   max_dets=z['max_dets'], class_agnostic=class_agnostic, **kw)


def _add(ev, im):
    z = C.fixture()
    label_of = {int(c): i for i, c in enumerate(z['cat_ids'])}
    ev.add(torch.tensor([label_of[int(c)] for c in im['det_cats']], dtype=torch.int64), torch.from_numpy(im['det_boxes5']),
           im['gt_boxes'], im['gt_cats'], im['gt_crowd'], im['gt_area'])


@pytest.mark.parametrize('tag,agn', C.MODES)
def test_bbox_evaluator_on_the_host_image_by_image_equals_the_one_shot_run(tag, agn):
    z = C.fixture()
    ev = _evaluator(agn)
    for im in C.fixture_images():
        _add(ev, im)
    res = ev.summarize()
    for name in ('precision', 'recall', 'scores'):
        assert res[name].tobytes() == z[tag + name].tobytes(), name
    assert res['images'] == 6 and len(res['stats']) == 12
    assert (res['base_ap50'], res['novel_ap50'], res['all_ap50']) == tuple(z[tag + 'open_set_ap50'])
    for rec, want in zip(ev.records, C.fixture_records(tag)):
        C.assert_records_equal(rec, want)
    text = mask_eval.format_summary('all_results', res, 'bbox')
    assert text.startswith('bbox all_results: 6 images') and 'AP50: base' in text
    assert mask_eval.format_summary('all_results', res).startswith('segm all_results: 6 images')     # the default keeps today's line


def test_bbox_evaluator_defaults_skip_rule_and_extra_records():
    z = C.fixture()
    ev = mask_eval.BboxEvaluator([1, 2])
    assert ev.max_dets == [100, 300, 1000] and ev.iou_thrs.tobytes() == z['iou_thrs'].tobytes() and ev.all_cat_ids == [1, 2]
    labels, boxes = torch.zeros(1, dtype=torch.int64), torch.tensor([[0., 0., 10., 10., 0.5]])
    # gt_area = None: the ground-truth box's w * h (32 x 32 = the bound itself counts as small)
    ev.add(labels, boxes, np.array([[0., 0., 32., 32.]]), np.array([1]))
    assert ev.records[0][0][1]['gt_ignore'].tolist() == [False] and ev.records[0][0][3]['gt_ignore'].tolist() == [True]
    ev = mask_eval.BboxEvaluator([1, 2], skip_images_without_gt=True)
    ev.add(labels, boxes, np.array([[0., 0., 5., 5.]]), np.array([7]))        # no ground truth of 1, 2
    assert ev.records == []
    ev.add(labels, boxes, np.array([[0., 0., 5., 5.]]), np.array([2]))
    assert len(ev.records) == 1
    with pytest.raises(ValueError, match=r'\(D, 5\)'):
        ev.add(labels, torch.zeros(1, 4), np.array([[0., 0., 5., 5.]]), np.array([2]))
    # two evaluators, each with half the images (two ranks): one's records as the other's extra_records give the whole run
    imgs = C.fixture_images()
    a, b, whole = _evaluator(False), _evaluator(False), _evaluator(False)
    for n, im in enumerate(imgs):
        _add(a if n < 3 else b, im)
        _add(whole, im)
    got, want = a.summarize(extra_records=b.image_records()), whole.summarize()
    assert got['precision'].tobytes() == want['precision'].tobytes() == z['std_precision'].tobytes()
    assert got['images'] == 6 and got['stats'] == want['stats']


def test_segm_evaluator_and_bbox_evaluator_share_everything_after_the_iou():
    for name in ('summarize', 'image_records', '_drain', '_parse', '_queue_match', '__init__'):
        assert getattr(mask_eval.BboxEvaluator, name) is getattr(mask_eval.SegmEvaluator, name), name
