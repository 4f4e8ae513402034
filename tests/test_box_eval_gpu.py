"""GPU tests of the device side of the COCO box evaluation (csrc/mask_eval.hip): `ops.box_iou` and `ops.coco_match_boxes` equal the
numpy rules of `cgg_amd.mask_eval` exactly -- IEEE double operations in a fixed order, contraction off, so there is no tolerance
and doubles are compared by their bit patterns -- on the contraction-sensitive case set, at the geometry edges of the kernels, on
the reference-made fixture and on seeded images; `BboxEvaluator` on the device equals the host evaluator in every array; one `add`
replays from a captured graph; `tools/test.py --eval bbox segm` end to end."""
import warnings

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import mask_eval, ops, registry, synthetic

import box_eval_cases as C

pytestmark = pytest.mark.gpu


def _t(dev, x, dt):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device=dev, dtype=dt)


def _check_box_iou(dev, det5, gt, crowd):
    det = mask_eval.det_boxes_xywh_host(det5)
    want = mask_eval.box_iou_host(det, gt, crowd)
    want_area = det[:, 2] * det[:, 3]
    iou, area_d = ops.box_iou(_t(dev, det5, torch.float32), _t(dev, gt, torch.float64), _t(dev, crowd, torch.uint8))
    torch.cuda.synchronize()
    assert iou.dtype == torch.float64 and tuple(iou.shape) == want.shape and tuple(area_d.shape) == want_area.shape
    got, got_area = iou.cpu().numpy(), area_d.cpu().numpy()
    differ = got.view(np.int64) != want.view(np.int64)
    assert not differ.any(), (int(differ.sum()), np.argwhere(differ)[:4].tolist())
    assert got_area.tobytes() == want_area.tobytes()
    return want


# (D, G): empty sides; one pair; less than a wave; more than one block of 256 pairs, nothing a multiple of 64
@pytest.mark.parametrize('D,G', [(0, 3), (3, 0), (1, 1), (5, 7), (65, 33), (130, 70)])
def test_box_iou_equals_the_host_rule(dev, D, G):
    im = C.random_image(D * 7 + G, D=D, G=G, K=3)
    want = _check_box_iou(dev, im['det_boxes5'], im['gt_boxes'].reshape(G, 4), im['gt_crowd'])
    if D * G > 30:
        assert (want > 0).sum() > D and (want == 0).any()


def test_box_iou_on_the_contraction_sensitive_case_set(dev):
    """the case set holds pairs for which a fused union gives another quotient (test_box_eval.py counts them): bit equality with
    the rule here means the kernel's products were not contracted into its adds"""
    det5, gt, crowd = C.case_boxes()
    rule, fused = C.case_iou_exact()
    assert ((rule != fused) & (rule > 0)).sum() >= 8
    want = _check_box_iou(dev, det5, gt, crowd)
    assert want.tobytes() == rule.tobytes()


def _device_match(dev, im, cat_ids, area_rngs, iou_thrs, max_det, agn):
    scores = _t(dev, im['det_boxes5'][:, 4], torch.float32)
    order = torch.sort(scores, descending=True, stable=True).indices.to(torch.int32)
    out = ops.coco_match_boxes(_t(dev, im['det_boxes5'], torch.float32), _t(dev, im['gt_boxes'].reshape(-1, 4), torch.float64), order,
                               _t(dev, im['det_cats'], torch.int32), _t(dev, im['gt_cats'], torch.int32),
                               _t(dev, im['gt_crowd'], torch.uint8), _t(dev, im['gt_area'], torch.float64), _t(dev, cat_ids, torch.int32),
                               _t(dev, area_rngs, torch.float64), _t(dev, iou_thrs, torch.float64), max_det, agn)
    torch.cuda.synchronize()
    dtm, dti, gti, counts = (o.cpu().numpy() for o in out)
    return mask_eval.records_from_match(dtm, dti, gti, counts, order.cpu().numpy(), im['det_cats'], im['det_boxes5'][:, 4], cat_ids, agn), \
        (dtm, dti, gti, counts)


def _check_match(dev, im, cat_ids, max_det, agn, area_rngs=None, iou_thrs=None, where=''):
    """device records == host records in every array; what lies past D_k / G_k is written, as zeros"""
    area_rngs = np.asarray(mask_eval.AREA_RNGS, np.float64) if area_rngs is None else area_rngs          # A = 4
    iou_thrs = mask_eval.default_iou_thrs() if iou_thrs is None else iou_thrs                             # T = 10
    want = C.host_records(im, agn, cat_ids, area_rngs, iou_thrs, max_det)[0]
    got, (dtm, dti, gti, counts) = _device_match(dev, im, cat_ids, area_rngs, iou_thrs, max_det, agn)
    C.assert_records_equal(got, want, where)
    for k in range(len(got)):
        for a in range(len(area_rngs)):
            if got[k][a] is not None:
                assert np.array_equal(got[k][a]['dt_index'], want[k][a]['dt_index'])
        assert not dtm[k, :, :, counts[k, 0]:].any() and not dti[k, :, :, counts[k, 0]:].any() and not gti[k, :, counts[k, 1]:].any()
    return want, counts


@pytest.mark.parametrize('tag,agn', C.MODES)
def test_coco_match_boxes_equals_the_host_rule_on_the_fixture(dev, tag, agn):
    z = C.fixture()
    want_all = C.fixture_records(tag)
    for i, im in enumerate(C.fixture_images()):
        want, _ = _check_match(dev, im, z['cat_ids'], int(z['max_dets'][-1]), agn, z['area_rngs'], z['iou_thrs'], (tag, i))
        C.assert_records_equal(want, want_all[i], (tag, i, 'reference'))


def test_coco_match_boxes_quotients_sit_on_the_thresholds(dev):
    """The double quotient the kernel forms is the rule's, bit for bit: thresholds are set to the float64 IoU itself, to the next
    double below and to the next above. A detection matches at t iff iou >= min(t, 1 - 1e-10), so one unit in the last place in
    the kernel's arithmetic would flip a match against the host rule."""
    det5, gt, crowd = C.case_boxes()
    iou = mask_eval.box_iou_host(mask_eval.det_boxes_xywh_host(det5), gt, crowd)
    rule, fused = C.case_iou_exact()
    # one detection per ground truth (its best, among contraction-sensitive pairs where there is one), each pair a category of its own
    pairs = []
    for g in range(2, 14):
        if crowd[g]:
            continue
        sens = np.nonzero((rule[:, g] != fused[:, g]) & (rule[:, g] > 0.3))[0]
        pairs.append((int(sens[0]) if len(sens) else int(np.argmax(iou[:, g])), g))
    n = len(pairs)
    assert n >= 9 and sum(rule[d, g] != fused[d, g] for d, g in pairs) >= 4
    im = dict(det_boxes5=det5[[d for d, _ in pairs]].copy(), det_cats=np.arange(n), gt_boxes=gt[[g for _, g in pairs]],
              gt_cats=np.arange(n), gt_crowd=np.zeros(n, bool), gt_area=np.full(n, 100.0))
    im['det_boxes5'][:, 4] = np.linspace(0.9, 0.1, n)
    area_rngs = np.array([[0, 1e10]])
    for lo in range(0, n, 3):
        q = np.array([iou[pairs[i]] for i in range(lo, min(lo + 3, n))])
        thrs = np.sort(np.concatenate([q, np.nextafter(q, 0), np.nextafter(q, 1)]))
        want, _ = _check_match(dev, im, np.arange(n), 100, False, area_rngs, thrs, lo)
        for i in range(lo, min(lo + 3, n)):
            m = want[i][0]['dt_match'][:, 0]
            assert m[thrs <= iou[pairs[i]]].all() and not m[thrs > iou[pairs[i]]].any()      # the flip happens exactly at the quotient


@pytest.mark.parametrize('D,G,chunks', [(64, 32, 1), (65, 32, 2), (20, 300, 4)])
def test_coco_match_boxes_on_one_category_at_the_lds_threshold(dev, D, G, chunks):
    """D_k * G_k = 64 x 32 = 2048 entries: the category's IoU block fits the LDS block; 65 x 32 = 2080: two chunks of detections (64
    and 1); 20 x 300: chunks of 6 detections and a last one of 2"""
    im = C.random_image(640 + D, D=D, G=G, K=1)
    want, counts = _check_match(dev, im, np.array([1]), 100, False)
    per_chunk = D if D * G <= 2048 else 2048 // G
    assert counts.tolist() == [[D, G]] and -(-D // per_chunk) == chunks
    matches = want[0][0]['dt_match']
    assert (matches > 0).sum() > 40 and (matches == 0).sum() > 40


@pytest.mark.parametrize('agn', [False, True])
def test_coco_match_boxes_cuts_130_detections_to_max_det(dev, agn):
    """D = 130: two full ballots and a partial one; class-agnostic, every category takes the 100 best of all 130"""
    im = C.random_image(130, D=130, G=24, K=2)
    want, counts = _check_match(dev, im, np.array([1, 2]), 100, agn)
    assert (counts[:, 0] == 100).all() if agn else (counts[:, 0].sum() == 130 and counts[:, 0].max() < 100)
    im1 = C.random_image(131, D=130, G=24, K=1)                      # one category holds all 130: the cut without class_agnostic
    _, counts = _check_match(dev, im1, np.array([1]), 100, False)
    assert counts.tolist() == [[100, 24]]


@pytest.mark.parametrize('agn', [False, True])
def test_coco_match_boxes_with_empty_categories(dev, agn):
    """K = 5 of which two have neither a detection nor a ground truth (None records), A = 4 and T = 10, the defaults"""
    im = C.random_image(55, D=100, G=40, K=3)
    want, counts = _check_match(dev, im, np.array([1, 7, 2, 9, 3]), 30 if agn else 7, agn)
    assert counts[1].tolist() == ([30, 0] if agn else [0, 0]) and (want[3][0] is None) == (not agn)
    matches = np.concatenate([r['dt_match'].ravel() for per_area in want for r in per_area if r is not None])
    assert (matches > 0).sum() > 50 and (matches == 0).sum() > 50
    assert any(r['dt_ignore'].any() for per_area in want for r in per_area if r is not None)


def _assert_summaries_equal(a, b):
    assert set(a) == set(b)
    for name in ('precision', 'recall', 'scores'):
        assert a[name].tobytes() == b[name].tobytes(), name
    assert a['stats'] == b['stats'] and a['images'] == b['images']
    assert np.array_equal(np.array([a['base_ap50'], a['novel_ap50'], a['all_ap50']]),
                          np.array([b['base_ap50'], b['novel_ap50'], b['all_ap50']]), equal_nan=True)


@pytest.mark.parametrize('D', [1024, 1025])
def test_gate_1024_takes_the_kernel_and_1025_the_numpy_rule(dev, D, monkeypatch):
    calls = []
    real = ops.coco_match_boxes
    monkeypatch.setattr(ops, 'coco_match_boxes', lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    im = C.random_image(D, D=D, G=6, K=2)
    kw = dict(max_dets=(1, 10, 40), iou_thrs=np.array([0.5, 0.75]))
    on_dev, on_host = mask_eval.BboxEvaluator([1, 2], device=dev, **kw), mask_eval.BboxEvaluator([1, 2], device=None, **kw)
    labels = torch.from_numpy(im['det_cats'] - 1)
    on_dev.add(labels.to(dev), torch.from_numpy(im['det_boxes5']).to(dev), im['gt_boxes'], im['gt_cats'], im['gt_crowd'], im['gt_area'])
    on_host.add(labels, torch.from_numpy(im['det_boxes5']), im['gt_boxes'], im['gt_cats'], im['gt_crowd'], im['gt_area'])
    assert len(calls) == (1 if D == 1024 else 0)
    _assert_summaries_equal(on_dev.summarize(), on_host.summarize())
    C.assert_records_equal(on_dev.records[0], on_host.records[0])


@pytest.mark.parametrize('tag,agn', C.MODES)
def test_bbox_evaluator_on_the_device_equals_the_host_evaluator(dev, tag, agn):
    z = C.fixture()
    kw = dict(unknown_cat_ids=z['unknown_cat_ids'], all_cat_ids=z['all_cat_ids'], max_dets=z['max_dets'], class_agnostic=agn)
    on_dev, on_host = mask_eval.BboxEvaluator(z['cat_ids'], device=dev, **kw), mask_eval.BboxEvaluator(z['cat_ids'], device=None, **kw)
    label_of = {int(c): i for i, c in enumerate(z['cat_ids'])}
    for n, im in enumerate(C.fixture_images()):
        labels = torch.tensor([label_of[int(c)] for c in im['det_cats']], dtype=torch.int64)
        boxes = torch.from_numpy(im['det_boxes5'])
        on_host.add(labels, boxes, im['gt_boxes'], im['gt_cats'], im['gt_crowd'], im['gt_area'])
        # the device evaluator takes device results
        on_dev.add(labels.to(dev), boxes.to(dev), im['gt_boxes'], im['gt_cats'], im['gt_crowd'], im['gt_area'])
    a, b = on_dev.summarize(), on_host.summarize()
    _assert_summaries_equal(a, b)
    for ra, rb in zip(on_dev.records, on_host.records):
        C.assert_records_equal(ra, rb)
    assert a['precision'].tobytes() == z[tag + 'precision'].tobytes()
    assert (a['base_ap50'], a['novel_ap50'], a['all_ap50']) == tuple(z[tag + 'open_set_ap50'])
    # gt_crowd = None and gt_area = None: no crowd, the ground-truth box's w * h -- the same on both sides
    on_dev, on_host = mask_eval.BboxEvaluator(z['cat_ids'], device=dev, **kw), mask_eval.BboxEvaluator(z['cat_ids'], device=None, **kw)
    im = C.fixture_images()[0]
    labels = torch.tensor([label_of[int(c)] for c in im['det_cats']], dtype=torch.int64)
    on_dev.add(labels.to(dev), torch.from_numpy(im['det_boxes5']).to(dev), im['gt_boxes'], im['gt_cats'])
    on_host.add(labels, torch.from_numpy(im['det_boxes5']), im['gt_boxes'], im['gt_cats'])
    _assert_summaries_equal(on_dev.summarize(), on_host.summarize())


def test_one_add_replays_from_a_captured_graph(dev):
    """the launch of one `add` under torch.cuda.graph, single-stream: two replays on new inputs give the records of the host rule
    both times"""
    ims = [C.random_image(s, D=20, G=9, K=5) for s in (41, 42)]
    cat_ids, rngs, thrs = np.arange(1, 6), np.asarray(mask_eval.AREA_RNGS, np.float64), mask_eval.default_iou_thrs()
    st = dict(det=_t(dev, ims[0]['det_boxes5'], torch.float32), gt=_t(dev, ims[0]['gt_boxes'], torch.float64),
              order=torch.zeros(20, dtype=torch.int32, device=dev), det_cats=_t(dev, ims[0]['det_cats'], torch.int32),
              gt_cats=_t(dev, ims[0]['gt_cats'], torch.int32), crowd=_t(dev, ims[0]['gt_crowd'], torch.uint8),
              area=_t(dev, ims[0]['gt_area'], torch.float64))
    consts = (_t(dev, cat_ids, torch.int32), _t(dev, rngs, torch.float64), _t(dev, thrs, torch.float64))

    def launches():
        return ops.coco_match_boxes(st['det'], st['gt'], st['order'], st['det_cats'], st['gt_cats'], st['crowd'], st['area'], *consts, 10, False)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launches()                                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = launches()
    for im in (ims[1], ims[0]):
        order = torch.sort(_t(dev, im['det_boxes5'][:, 4], torch.float32), descending=True, stable=True).indices.to(torch.int32)
        for key, src, dt in (('det', im['det_boxes5'], torch.float32), ('gt', im['gt_boxes'], torch.float64),
                             ('det_cats', im['det_cats'], torch.int32), ('gt_cats', im['gt_cats'], torch.int32),
                             ('crowd', im['gt_crowd'], torch.uint8), ('area', im['gt_area'], torch.float64)):
            st[key].copy_(_t(dev, src, dt))
        st['order'].copy_(order)
        graph.replay()
        torch.cuda.synchronize()
        dtm, dti, gti, counts = (o.cpu().numpy() for o in out)
        got = mask_eval.records_from_match(dtm, dti, gti, counts, order.cpu().numpy(), im['det_cats'], im['det_boxes5'][:, 4], cat_ids, False)
        want = C.host_records(im, False, cat_ids, rngs, thrs, 10)[0]
        C.assert_records_equal(got, want)


def test_tools_test_eval_bbox_next_to_segm(dev, tmp_path, capsys):
    """tools/test.py --eval bbox segm on a --data stream with box and mask ground truth prints both summaries and writes
    bbox_eval.json, whose numbers are those of a host BboxEvaluator fed with the results the driver returns; proposal_fast is
    refused by name"""
    import importlib.util
    import json
    import os
    from cgg_amd.checkpoint import save_checkpoint
    from util import randomize
    cfg = synthetic.model_config(num_things=10, num_stuff=0, num_unknown=3, num_queries=20, depth=50, enc_layers=2, dec_layers=3,
                                 vocab=500, num_points=256)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = registry.build_detector(cfg)
    randomize(model, seed=21)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_var.fill_(1.0)
            m.running_mean.zero_()
    ck = save_checkpoint(model, str(tmp_path / 'w.pth'))
    cfg_file = tmp_path / 'tiny.py'
    cfg_file.write_text('model = ' + repr(cfg) + '\nsegm_eval = dict(unknown_cat_ids=[3, 4], max_dets=(1, 5, 20))\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('cgg_tools_test_bbox', os.path.join(root, 'tools', 'test.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    common = [str(cfg_file), ck, '--data', 'box_eval_cases:eval_stream', '--precision', 'bf16', '--no-pipeline']
    with pytest.raises(SystemExit, match='proposal_fast'):
        drv.main(common + ['--eval', 'bbox', 'proposal_fast'])
    results = drv.main(common + ['--eval', 'bbox', 'segm', '--work-dir', str(tmp_path / 'a')])
    out = capsys.readouterr().out
    assert 'bbox all_results: 5 images' in out and 'segm all_results: 5 images' in out and out.count('AP50: base') >= 2
    assert (tmp_path / 'a' / 'segm_eval.json').exists()
    summary = json.loads((tmp_path / 'a' / 'bbox_eval.json').read_text())
    assert len(results) == 6 and set(summary) == {k for k in results[0] if k.endswith('_results')}
    metas = [m for _, m in C.eval_stream(None, 0, 1)]
    fh = model.panoptic_fusion_head
    for key, got in summary.items():
        n_cls = getattr(fh, key.replace('_results', '_classes'))
        ev = mask_eval.BboxEvaluator(list(range(1, n_cls + 1)), unknown_cat_ids=[3, 4], max_dets=(1, 5, 20), skip_images_without_gt=True)
        for res, m in zip(results, metas[:5]):
            labels, boxes, _ = res[key]
            ev.add(labels, boxes, m['gt_boxes_xywh'], m['gt_labels'], m['gt_crowd'], m['gt_area'])
        want = ev.summarize()
        assert got['images'] == want['images'] == 5
        assert json.dumps(got['stats']) == json.dumps(want['stats'])
        assert json.dumps([got['base_ap50'], got['novel_ap50'], got['all_ap50']]) == \
            json.dumps([want['base_ap50'], want['novel_ap50'], want['all_ap50']])
    # bbox alone keeps the masks as they are (no --mask-bits), proposal is the same run under its name, and a stream without
    # ground truth keeps the driver's message
    drv.main([str(cfg_file), ck, '--num-images', '2', '--synthetic', '64', '--eval', 'proposal', '--precision', 'bf16', '--no-pipeline'])
    out = capsys.readouterr().out
    assert '--eval proposal: the stream carries no ground truth' in out and '"results": "bool arrays"' in out
