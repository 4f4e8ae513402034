"""GPU tests of the device side of the panoptic-quality evaluation (csrc/pq_eval.hip): `PQEvaluator(device=...)` -- `ops.pq_confusion`
and `ops.pq_match` -- equals the numpy rule of `cgg_amd.pq_eval` field for field, the ious by their bit patterns (integer counts and
one IEEE double quotient per pair, so there is no tolerance), on the reference-made fixture G14, at the geometry edges of the
kernels and end to end through tools/test.py --eval PQ."""
import warnings

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import _lib, ops, pq_eval, registry, synthetic
from cgg_amd._lib import CggError, dev_ptr, stream_ptr

import pq_cases as C

pytestmark = pytest.mark.gpu


def _evaluators(dev):
    return (pq_eval.PQEvaluator(C.CAT_IDS, C.ISTHING, C.UNKNOWN, device=dev), pq_eval.PQEvaluator(C.CAT_IDS, C.ISTHING, C.UNKNOWN))


def _check(dev, pan_pred, pred, pan_gt, gt, pred_dev=None, expect_device=True):
    """one image through the device evaluator TWICE and through the host evaluator once: three equal records"""
    on_dev, on_host = _evaluators(dev)
    on_host.add(pan_pred, pred, pan_gt, gt)
    for _ in range(2):
        on_dev.add(pan_pred if pred_dev is None else pred_dev[0], pred if pred_dev is None else pred_dev[1], pan_gt, gt)
    assert on_dev.device_images == (2 if expect_device else 0)
    recs = on_dev.image_records()
    C.assert_records_equal(recs[0], on_host.records[0], 'device vs host')
    C.assert_records_equal(recs[1], recs[0], 'second run')
    return recs[0]


@pytest.mark.parametrize('rgb', [False, True])
def test_the_device_route_equals_the_host_rule_and_the_reference_on_the_fixture(dev, rgb):
    z = C.fixture()
    on_dev = C.fixture_evaluator(dev)
    on_host = C.fixture_evaluator()
    for i, im in enumerate(C.fixture_images()):
        gt_map = C.to_rgb(im['gt_map']) if rgb else im['gt_map']
        # the pred map alternately from the host and as a device tensor
        on_dev.add(torch.from_numpy(im['pred_map']).to(dev) if i % 2 else im['pred_map'], im['pred'], gt_map, im['gt'])
        on_host.add(im['pred_map'], im['pred'], gt_map, im['gt'])
    assert on_dev.device_images == 6
    for a, b in zip(on_dev.image_records(), on_host.image_records()):
        C.assert_records_equal(a, b)
    a, b = on_dev.summarize(), on_host.summarize()
    assert repr(a) == repr(b)
    for c, iou in zip(z['stat_cats'], z['stat_iou']):
        assert np.float64(a['stats'][int(c)]['iou']).view(np.int64) == iou.view(np.int64)
    for name, tag in C.SPLITS:
        got = np.array([a['pq_results'][name][k] for k in C.SPLIT_KEYS], np.float64)
        assert got.view(np.int64).tolist() == z['split_' + tag].view(np.int64).tolist(), name


# (H, W, ground truths, preds): one pixel; one row whose width is no multiple of the four-pixel load (a tail of one); the fixture's
# geometry (a tail of one, rows that straddle the groups of four); a width of 4 k + 3 over several rows; more than one workgroup
# (96 x 130 = 12480 pixels = 3120 groups of four, 13 workgroups); no ground truth; no pred
SHAPES = [(1, 1, 1, 1), (1, 257, 3, 4), (37, 45, 8, 10), (5, 131, 6, 6), (96, 130, 30, 40), (37, 45, 0, 9), (37, 45, 7, 0)]


@pytest.mark.parametrize('H,W,G,P', SHAPES)
@pytest.mark.parametrize('rgb', [False, True])
def test_seeded_images_with_an_explicit_list(dev, H, W, G, P, rgb):
    c = C.random_case(H * 3 + W + G, H, W, G, P)
    assert len(c['gt']) == G and (P > 0 or (c['pan_pred'] == C.NUM_CLASSES).all())              # P = 0: the pred is all void
    rec = _check(dev, c['pan_pred'], c['pred'], C.to_rgb(c['pan_gt']) if rgb else c['pan_gt'], c['gt'])
    if (H, W) == (96, 130):
        assert (rec['gt_match'] >= 0).sum() >= 3 and rec['pred_ignored'].any() and (~rec['pred_matched']).any()


def test_ids_that_collide_in_both_id_tables(dev):
    """8 ground truths -> a table of 16 entries, ids = 16 k + 3 (one chain of probes), among them 2^24 - 13 and, in its own slot,
    2^24 - 1; the pred's values 16000 k + 5 collide modulo 16 and 32 (and their label, 5, is not void)"""
    gt_ids = [16 * k + 3 for k in (1, 2, 3, 50, 1000, 2 ** 20 - 1)] + [2 ** 24 - 1, 19]
    assert ops.pq_hash_size(len(gt_ids)) == 16 and sum(i % 16 == 3 for i in gt_ids) == 7
    c = C.random_case(77, 37, 45, len(gt_ids), 9, gt_ids=gt_ids + [67])
    values = np.unique(c['pan_pred'])
    values = values[values % 1000 != C.NUM_CLASSES]
    pan = c['pan_pred'].copy()
    pred = []
    for k, v in enumerate(values.tolist()):
        new = 16000 * (k + 1) + 5
        pan[c['pan_pred'] == v] = new
        pred.append(dict(id=new, category_id=C.CAT_IDS[v % 1000]))
    assert len(pred) >= 6 and ops.pq_hash_size(len(pred)) in (16, 32)
    rec = _check(dev, pan, pred, c['pan_gt'], c['gt'])
    assert int(rec['gt_id'].max()) >= 2 ** 24 - 13 and sum(int(i) % 16 == 3 for i in rec['gt_id']) >= 6
    _check(dev, pan, pred, C.to_rgb(c['pan_gt']), c['gt'])


@pytest.mark.parametrize('rgb', [False, True])
def test_pred_from_a_device_segment_table_with_rows_that_merge_and_rows_of_area_zero(dev, rgb):
    c = C.random_case(5, 64, 72, 12, 14)
    table, n_kept = C.table_of(c['pan_pred'], 40, seed=2)
    values = table[:n_kept, 0]
    assert (values == -1).sum() == 2 and (table[:n_kept, 2] == 0).sum() == 2 and len(values) - len(np.unique(values)) >= 2
    # as the batched fusion leaves them: the image's block of a (B, Q, 4) table, n_kept one element of a (B,) tensor, the map a
    # view into a flat tensor at an offset that is no multiple of 16 bytes
    tables = torch.zeros(3, 40, 4, dtype=torch.int32, device=dev)
    kept = torch.tensor([40, n_kept, 0], dtype=torch.int32, device=dev)
    tables[1] = torch.from_numpy(table).to(dev)
    flat = torch.full((64 * 72 + 8,), 12345, dtype=torch.int32, device=dev)
    pan = flat[3:3 + 64 * 72].view(64, 72)
    pan.copy_(torch.from_numpy(c['pan_pred']).to(dev))
    rec = _check(dev, c['pan_pred'], None, C.to_rgb(c['pan_gt']) if rgb else c['pan_gt'], c['gt'],
                 pred_dev=(pan, dict(n_kept=kept[1], table=tables[1], scores=None)))
    assert rec['pred_id'].tolist() == [s['id'] for s in c['pred']] and rec['pred_area'].tolist() == [s['area'] for s in c['pred']]
    # the same table from the host (numpy), the map from the host
    _check(dev, c['pan_pred'], None, c['pan_gt'], c['gt'], pred_dev=(c['pan_pred'], dict(n_kept=n_kept, table=table)))


def _gate_edge(P):
    limit = int(_lib.load().cgg_dynamic_lds_limit())
    return max(g for g in range(1, 4097) if ops.pq_eval_lds_bytes(g, P) <= limit)


def test_shapes_just_inside_and_just_outside_the_lds_gate(dev):
    P = 20
    G = _gate_edge(P)
    c = C.random_case(9, 37, 45, 12, P)
    used = {g['id'] for g in c['gt']} | set(np.unique(c['pan_gt']).tolist())
    spare = [i for i in range(1, 3 * G) if i not in used]
    for n_gt, inside in ((G, True), (G + 1, False)):
        # ground truths without a pixel fill the list up: false negatives, in both routes
        gt = c['gt'] + [dict(id=spare[k], category_id=C.CAT_IDS[k % 7], iscrowd=0, area=k + 1) for k in range(n_gt - len(c['gt']))]
        pred = c['pred']
        assert len(pred) <= P
        # the pred as a table of exactly P rows, the first len(pred) valid
        tab = np.zeros((P, 4), np.int32)
        for k, s in enumerate(pred):
            tab[k] = [s['id'], C.CAT_IDS.index(s['category_id']), s['area'], k]
        assert ops.pq_eval_ok(n_gt, P, 37, 45, True) == inside
        rec = _check(dev, c['pan_pred'], None, c['pan_gt'], gt, pred_dev=(c['pan_pred'], dict(n_kept=len(pred), table=tab)),
                     expect_device=inside)
        assert len(rec['gt_id']) == n_gt
    # the C entries refuse the outside shape by name
    n_gt = G + 1
    pan = torch.zeros(37, 45, dtype=torch.int32, device=dev)
    ids = torch.arange(1, n_gt + 1, dtype=torch.int32, device=dev)
    tab = torch.zeros(P, 4, dtype=torch.int32, device=dev)
    kept = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.zeros((n_gt + 2) * (P + 1) + 2, dtype=torch.int32, device=dev)
    with pytest.raises(CggError, match=r'cgg_pq_confusion_i32 failed \(rc=-2\).*bytes of LDS'):
        ops._call('cgg_pq_confusion_i32', dev_ptr(pan), dev_ptr(pan), 0, 37, 45, dev_ptr(ids), n_gt, dev_ptr(tab), dev_ptr(kept), P, 7,
                  dev_ptr(ws), stream_ptr(dev))
    with pytest.raises(CggError, match='outside the kernel gate'):
        ops.pq_confusion(pan, tab, kept, pan, ids, 7)
    buf = torch.zeros(64 + 16 * n_gt + 16 * P, dtype=torch.uint8, device=dev)
    with pytest.raises(CggError, match=r'cgg_pq_match failed \(rc=-2\)'):
        ops._call('cgg_pq_match', dev_ptr(ws), dev_ptr(ids), dev_ptr(buf), dev_ptr(ids), n_gt, dev_ptr(tab), dev_ptr(kept), P, dev_ptr(buf),
                  dev_ptr(buf), dev_ptr(buf), dev_ptr(buf), dev_ptr(buf), dev_ptr(buf), dev_ptr(buf), stream_ptr(dev))
    torch.cuda.synchronize()


def test_class_zero_as_stuff_takes_the_host_rule(dev):
    c = C.random_case(4, 37, 45, 5, 6)
    isthing = [0] + C.ISTHING[1:]
    on_dev, on_host = (pq_eval.PQEvaluator(C.CAT_IDS, isthing, C.UNKNOWN, device=d) for d in (dev, None))
    for ev in (on_dev, on_host):
        ev.add(c['pan_pred'], c['pred'], c['pan_gt'], c['gt'])
    assert on_dev.device_images == 0
    C.assert_records_equal(on_dev.image_records()[0], on_host.records[0])


def test_on_a_stream_that_is_not_the_default(dev):
    c = C.random_case(21, 37, 45, 8, 10)
    on_dev, on_host = _evaluators(dev)
    on_host.add(c['pan_pred'], c['pred'], c['pan_gt'], c['gt'])
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        on_dev.add(torch.from_numpy(c['pan_pred']).to(dev), c['pred'], c['pan_gt'], c['gt'])
    assert on_dev.device_images == 1
    C.assert_records_equal(on_dev.image_records()[0], on_host.records[0])
    torch.cuda.current_stream(dev).wait_stream(side)


def test_the_status_word_becomes_the_named_errors(dev):
    gt = np.zeros((2, 3), np.int32)
    pred = np.array([[5, 5, 0], [6, 9, C.NUM_CLASSES + 3000]], np.int32)
    ev = _evaluators(dev)[0]
    ev.add(pred, [dict(id=5, category_id=1)], gt, [])
    with pytest.raises(KeyError, match='In the image with ID 0 segment with ID 6 is presented in PNG and not presented in JSON'):
        ev.image_records()
    ev = _evaluators(dev)[0]
    ev.add(pred, [dict(id=5, category_id=1), dict(id=6, category_id=1), dict(id=9, category_id=1), dict(id=70, category_id=2)], gt, [])
    with pytest.raises(KeyError, match=r'the following segment IDs \[70\] are presented in JSON and not presented in PNG'):
        ev.image_records()
    # a ground truth whose recorded area understates its pixels matches two preds: the device record cannot hold that
    ev = _evaluators(dev)[0]
    ev.add(np.array([[1001, 1001, 2001, 2001]], np.int32), [dict(id=1001, category_id=2), dict(id=2001, category_id=2)],
           np.full((1, 4), 9, np.int32), [dict(id=9, category_id=2, iscrowd=0, area=1)])
    with pytest.raises(ValueError, match='matches more than one prediction'):
        ev.image_records()
    assert ev.device_images == 1


def _tiny_panoptic_model(tmp_path, seed):
    from cgg_amd.checkpoint import save_checkpoint
    from util import randomize
    cfg = synthetic.model_config(num_things=8, num_stuff=2, num_unknown=3, num_queries=20, depth=50, enc_layers=2, dec_layers=3,
                                 vocab=500, num_points=256, panoptic=True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = registry.build_detector(cfg)
    randomize(model, seed=seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_var.fill_(1.0)
            m.running_mean.zero_()
    ck = save_checkpoint(model, str(tmp_path / 'w.pth'))
    cfg_file = tmp_path / 'tiny.py'
    cfg_file.write_text('model = ' + repr(cfg) + '\npq_eval = dict(unknown_cat_ids=[6, 7, 8])\n')
    return model, str(cfg_file), ck


def test_tools_test_eval_pq(dev, tmp_path, capsys):
    """tools/test.py --eval PQ on a --data stream with ground truth: the pipelined run and the sequential run write the same
    pq_eval.json, and it is the summary of a host evaluator fed with the maps the driver returns; a stream without ground truth
    gets a message"""
    import importlib.util
    import json
    import os
    model, cfg_file, ck = _tiny_panoptic_model(tmp_path, seed=21)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('cgg_tools_test_pq', os.path.join(root, 'tools', 'test.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    common = [cfg_file, ck, '--data', 'pq_cases:eval_stream', '--eval', 'PQ', '--precision', 'bf16']
    a = drv.main(common + ['--work-dir', str(tmp_path / 'a')])
    b = drv.main(common[:5] + ['pq'] + common[6:] + ['--work-dir', str(tmp_path / 'b'), '--no-pipeline'])
    out = capsys.readouterr().out
    assert out.count('Panoptic Evaluation Results:') == 2 and 'Unknown Things' in out and 'PQ_copypaste: ' in out
    text_a, text_b = (tmp_path / 'a' / 'pq_eval.json').read_text(), (tmp_path / 'b' / 'pq_eval.json').read_text()
    assert text_a == text_b
    got = json.loads(text_a)
    assert len(a) == len(b) == 6 and got['images'] == 5 and len(got['results']['PQ_copypaste'].split()) == 12
    fh = model.panoptic_fusion_head
    ev = pq_eval.PQEvaluator(list(range(1, 11)), [1] * 8 + [0] * 2, [6, 7, 8], num_classes=fh.num_classes)
    metas = [m for _, m in C.eval_stream(None, 0, 1)]
    for res, m in zip(b, metas[:5]):
        assert res['panoptic_all_results'].shape == (64, 64) and set(res['panoptic_segments']) >= {'n_kept', 'table'}
        ev.add(res['panoptic_all_results'], None, m['gt_pan_seg'], m['gt_segments'])
    want = ev.summarize()
    assert json.dumps(got['results']) == json.dumps(want['results'])
    assert got['stats'] == {str(k): dict(tp=v['tp'], fp=v['fp'], fn=v['fn'], iou=float(v['iou'])) for k, v in sorted(want['stats'].items())}
    assert sum(v['tp'] + v['fp'] + v['fn'] for v in got['stats'].values()) > 0
    # no ground truth in the stream (the synthetic images): a message; another metric keeps today's message
    drv.main([cfg_file, ck, '--num-images', '2', '--synthetic', '64', '--eval', 'PQ', 'bbox', '--precision', 'bf16', '--no-pipeline'])
    out = capsys.readouterr().out
    assert '--eval PQ: the stream carries no ground truth' in out and 'outside this build' in out
