"""Host side of the panoptic-quality evaluation (`cgg_amd.pq_eval`): the numpy rules reproduce fixture G14 -- recorded by executing
the reference's pq_evaluation.py, see tests/golden/make_golden_pq.py -- bit for bit; the restated `_pan2json`; both KeyErrors; the
accumulation of gathered records; the device gate's edges and the C entries' prototypes. No GPU."""
import numpy as np
import pytest

import cgg_amd  # noqa: F401
from cgg_amd import _lib, ops, pq_eval

import pq_cases as C


@pytest.fixture(scope='module')
def summary():
    ev = C.fixture_evaluator()
    for im in C.fixture_images():
        ev.add(im['pred_map'], im['pred'], im['gt_map'], im['gt'])
    return ev, ev.summarize()


def test_the_fixture_holds_the_cases_it_was_made_for():
    z = C.fixture()
    assert int(z['n_imgs']) == 6 and z['gt_maps'].shape == (6, 37, 45) and int(z['gt_id'].max()) == 2 ** 24 - 1
    ims = C.fixture_images()
    assert not ims[3]['pred_map'].any() and ims[3]['pred'] == [] and ims[4]['gt'] == [] and not ims[4]['gt_map'].any()
    assert 999 in ims[1]['gt_map'] and 999 not in [g['id'] for g in ims[1]['gt']]           # an id without a record
    assert [g['iscrowd'] for g in ims[1]['gt']] == [1, 0, 1]
    assert 11 in z['all_cat_ids'] and 11 not in z['stat_cats']                              # tp + fp + fn = 0
    assert set(z['pred_category_id'][z['pred_img'] < 5]) - set(z['gt_category_id'][z['gt_img'] < 5]) == {5}


def test_counts_and_iou_sums_equal_the_reference_bit_for_bit(summary):
    z = C.fixture()
    stats = summary[1]['stats']
    assert sorted(stats) == z['stat_cats'].tolist()
    for c, tp, fp, fn, iou in zip(z['stat_cats'], z['stat_tp'], z['stat_fp'], z['stat_fn'], z['stat_iou']):
        s = stats[int(c)]
        assert (s['tp'], s['fp'], s['fn']) == (int(tp), int(fp), int(fn)), c
        assert np.float64(s['iou']).view(np.int64) == iou.view(np.int64), c


def test_the_four_splits_and_the_copypaste_string_equal_the_reference(summary):
    z = C.fixture()
    res = summary[1]
    for name, tag in C.SPLITS:
        got = np.array([res['pq_results'][name][k] for k in C.SPLIT_KEYS], np.float64)
        assert got.view(np.int64).tolist() == z['split_' + tag].view(np.int64).tolist(), name
    classwise = np.array([[res['pq_results']['classwise'][int(c)][k] for k in ('pq', 'sq', 'rq', 'precision', 'recall')]
                          for c in z['all_cat_ids']], np.float64)
    assert classwise.view(np.int64).tolist() == z['classwise'].view(np.int64).tolist()
    r = res['results']
    twelve = [100 * z['split_' + tag][i] for tag in ('all', 'kth', 'ukth', 'st') for i in range(3)]
    assert [r[m + t] for t in ('', '_kth', '_ukth', '_st') for m in ('PQ', 'SQ', 'RQ')] == twelve
    assert r['PQ_copypaste'] == ' '.join(f'{v:.3f}' for v in twelve)
    assert int(res['pq_results']['All']['n']) == 6 and res['images'] == 6                   # category 11 is left out of n
    text = pq_eval.format_pq_summary(res['pq_results'])
    assert 'Panoptic Evaluation Results:' in text and all(f'{v:0.3f}' in text for v in twelve)
    assert [ln.split('|')[1].strip() for ln in text.splitlines() if ln.startswith('| ')] == ['', 'All', 'Known Things', 'Unknown Things', 'Stuff']


def test_the_image_records_hold_the_edge_cases(summary):
    recs = summary[0].image_records()
    r0, r1 = recs[0], recs[1]
    by_gt = {int(i): k for k, i in enumerate(r0['gt_id'])}
    assert r0['gt_match'][by_gt[7]] == -1                        # IoU exactly 0.5: inter 1, union 2
    g = by_gt[300]                                               # matched only through the VOID subtraction: 100 / (220 + 100 - 100 - 120)
    assert r0['gt_match'][g] >= 0 and r0['gt_iou'][g] == 1.0
    assert r0['gt_iou'][by_gt[2 ** 24 - 1]] == np.float64(110) / np.float64(120)          # 120 + 120 - 110 - 10 on VOID
    by_pred = {int(i): k for k, i in enumerate(r1['pred_id'])}
    ignored = {i: bool(r1['pred_ignored'][k]) for i, k in by_pred.items()}
    assert ignored == {60: False, 61: True, 62: False, 63: True, 64: False}         # the LAST crowd counts; 20 / 40 stays, 19 / 37 goes
    assert not r1['pred_matched'].any() and len(repr(r1)) < 2000


def test_both_map_forms_give_the_same_records(summary):
    ev = C.fixture_evaluator()
    for im in C.fixture_images():
        ev.add(im['pred_map'], im['pred'], C.to_rgb(im['gt_map']), im['gt'])
    for a, b in zip(ev.image_records(), summary[0].image_records()):
        C.assert_records_equal(a, b)
    with pytest.raises(Exception, match='pan_seg'):
        ev.add(np.zeros((4, 4), np.int32), [], np.zeros((4, 4), np.int64), [])


def test_pan_result_segments_host_on_a_hand_written_map():
    pan = np.array([[3, 3, 1001, 1001], [3, 2001, 2001, 4], [2, 2, 2, 4]], np.int64)            # 3 classes: 3 is void, 4 is not
    ids, segs = pq_eval.pan_result_segments_host(pan, 3, [10, 20, 30, 40, 50], [1, 1, 0, 0, 0])
    assert ids.tolist() == [[0, 0, 1001, 1001], [0, 2001, 2001, 4], [2, 2, 2, 4]] and pan[0, 0] == 3      # a copy
    assert segs == [dict(id=2, category_id=30, isthing=0, area=3), dict(id=4, category_id=50, isthing=0, area=2),
                    dict(id=1001, category_id=20, isthing=1, area=2), dict(id=2001, category_id=20, isthing=1, area=2)]
    # a value 0 (label 0 without an instance number) keeps its record and shares the id 0 with the void afterwards, as there
    ids, segs = pq_eval.pan_result_segments_host(np.array([[0, 3]]), 3, [10, 20, 30], [0, 1, 1])
    assert ids.tolist() == [[0, 0]] and segs == [dict(id=0, category_id=10, isthing=0, area=1)]


def test_both_key_errors_raise_by_name():
    gt = np.zeros((2, 3), np.int32)
    pred = np.array([[5, 5, 0], [6, 0, 0]], np.int32)
    with pytest.raises(KeyError, match='segment with ID 6 is presented in PNG and not presented in JSON'):
        pq_eval.pq_image_host(gt, [], pred, [dict(id=5, category_id=1)], image_id=3)
    with pytest.raises(KeyError, match=r'In the image with ID 3 the following segment IDs \[7\] are presented in JSON and not presented in PNG'):
        pq_eval.pq_image_host(gt, [], pred, [dict(id=5, category_id=1), dict(id=6, category_id=1), dict(id=7, category_id=2)], image_id=3)
    rec = pq_eval.pq_image_host(gt, [], pred, [dict(id=5, category_id=1), dict(id=6, category_id=1)])
    assert rec['pred_area'].tolist() == [2, 1] and rec['pred_ignored'].tolist() == [True, True]       # all of it on VOID


def test_a_ground_truth_with_an_understated_area_keeps_every_match():
    gt = np.full((2, 4), 9, np.int32)
    pred = np.array([[1, 1, 2, 2], [1, 1, 2, 2]], np.int32)
    rec = pq_eval.pq_image_host(gt, [dict(id=9, category_id=1, iscrowd=0, area=1)], pred, [dict(id=2, category_id=1), dict(id=1, category_id=1)])
    assert rec['gt_match'].tolist() == [1] and rec['extra'] == [(0, 0, 4.0)]                   # ascending pred id: 1, then 2
    s = pq_eval.pq_accumulate_host([rec])[1]
    assert (s['tp'], s['fp'], s['fn'], s['iou']) == (2, 0, 0, 8.0)


def test_records_of_two_ranks_accumulate_to_the_single_run(summary):
    ev, res = summary
    ims = C.fixture_images()
    ranks = [C.fixture_evaluator(), C.fixture_evaluator()]
    for i, im in enumerate(ims):
        ranks[i % 2].add(im['pred_map'], im['pred'], im['gt_map'], im['gt'])
    parts = [r.image_records() for r in ranks]
    in_order = [parts[i % 2][i // 2] for i in range(len(ims))]
    both = C.fixture_evaluator().summarize(extra_records=in_order)
    assert repr(both) == repr(res)
    for c, s in res['stats'].items():
        assert np.float64(both['stats'][c]['iou']).view(np.int64) == np.float64(s['iou']).view(np.int64)


def test_pq_eval_ok_at_its_edges():
    limit = int(_lib.load().cgg_dynamic_lds_limit())
    assert ops.pq_eval_ok(0, 0, 1, 1, True) and ops.pq_eval_ok(30, 40, 800, 1344, True)
    assert not ops.pq_eval_ok(30, 40, 800, 1344, False)                      # class 0 is stuff: the host rule
    assert ops.pq_eval_ok(1, 1, 1, 2 ** 31 - 1, True) and not ops.pq_eval_ok(1, 1, 2, 2 ** 30, True)
    assert not ops.pq_eval_ok(1, 1, 0, 5, True) and not ops.pq_eval_ok(-1, 1, 5, 5, True)
    assert not ops.pq_eval_ok(4097, 0, 5, 5, True) and ops.pq_eval_lds_bytes(4097, 0) == -1
    for G, P in ((0, 0), (1, 1), (8, 9), (30, 100), (300, 100)):
        assert ops.pq_eval_lds_bytes(G, P) == 4 * (G + 2) * (P + 1) + 8 * ops.pq_hash_size(G) + 8 * ops.pq_hash_size(P)
    assert [ops.pq_hash_size(n) for n in (0, 8, 9, 16, 17, 100)] == [16, 16, 32, 32, 64, 256]
    P = 100
    G = max(g for g in range(1, 4097) if ops.pq_eval_lds_bytes(g, P) <= limit)
    assert ops.pq_eval_lds_bytes(G, P) <= limit < ops.pq_eval_lds_bytes(G + 1, P)
    assert ops.pq_eval_ok(G, P, 37, 45, True) and not ops.pq_eval_ok(G + 1, P, 37, 45, True)


def test_the_c_entries_are_in_the_header():
    for name, n_args in (('cgg_pq_confusion_i32', 13), ('cgg_pq_match', 16), ('cgg_pq_eval_lds_bytes', 2),
                         ('cgg_pq_confusion_workspace_bytes', 2)):
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(_lib.load(), name)
    assert int(_lib.load().cgg_pq_confusion_workspace_bytes(3, 4)) == 4 * (5 * 5 + 2)
