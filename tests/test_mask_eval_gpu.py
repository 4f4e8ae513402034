"""GPU tests of the device side of the COCO mask evaluation (csrc/mask_eval.hip): `ops.mask_intersections` and `ops.coco_match` equal
the numpy rules of `cgg_amd.mask_eval` exactly -- integers, and IEEE double operations in a fixed order, so there is no tolerance --
at the geometry edges of the kernels, on the reference-made fixture and on a seeded random image; `SegmEvaluator` on the device
equals the host evaluator in every array; the two launches of one `add` replay from a captured graph."""
import warnings

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import mask_eval, ops, registry, runtime, synthetic

import mask_eval_cases as C

pytestmark = pytest.mark.gpu


def _planes(rs, n, H, W, rb, density, pad):
    """(n, H, rb) uint8 bit planes of random pixels; pad bits random ('rand'), all ones ('ones') or zero"""
    m = rs.rand(n, H, W) < density
    packed = np.packbits(m, axis=2, bitorder='little')
    nb = packed.shape[2]
    b = np.zeros((n, H, rb), np.uint8) if pad == 'zero' else (np.full((n, H, rb), 255, np.uint8) if pad == 'ones' else
                                                                rs.randint(0, 256, size=(n, H, rb)).astype(np.uint8))
    keep = np.zeros(rb, np.uint8)
    keep[:nb] = 255
    if W & 7:
        keep[nb - 1] = (1 << (W & 7)) - 1
    b &= ~keep
    b[:, :, :nb] |= packed
    return b


def _check_intersections(dev, det, gt, W, det_t=None, gt_t=None):
    want = mask_eval.mask_intersections_host(det, gt, W)
    det_t = torch.from_numpy(det).to(dev) if det_t is None else det_t
    gt_t = torch.from_numpy(gt).to(dev) if gt_t is None else gt_t
    got = ops.mask_intersections(det_t, gt_t, W)
    torch.cuda.synchronize()
    for g, w, name in zip(got, want, ('inter', 'area_d', 'area_g')):
        assert g.dtype == torch.int32 and tuple(g.shape) == w.shape, name
        assert np.array_equal(g.cpu().numpy().astype(np.int64), w), name
    return want


# (D, G, H, W, row_bytes): empty sides; one pixel; the fixture's geometry (6-byte rows: byte loads); the 16-plane register
# sub-tiles crossed in both directions with odd W (17-byte rows); rows of 36 bytes (4-byte loads, seven rows and a bit per slab);
# 48-byte rows padded past W (16-byte loads, a whole quad of pad) with two blocks of ground truths; several slabs and two blocks
# of detections (33-byte rows -> (100, 40, 256, 264)); rows of half a slab (128 bytes, the last slab with one row); rows longer
# than a slab, by byte loads (520 bytes: three chunks, the last of two words) and by 16-byte loads (272 bytes: 64 + 4 words)
SHAPES = [(0, 3, 8, 8, 1), (3, 0, 8, 8, 1), (1, 1, 1, 1, 1), (5, 7, 37, 45, 6), (33, 17, 70, 129, 17), (9, 5, 50, 281, 36),
          (20, 70, 19, 300, 48), (100, 40, 256, 264, 33), (3, 2, 5, 1024, 128), (3, 2, 5, 4150, 520), (2, 3, 3, 2170, 272)]


@pytest.mark.parametrize('D,G,H,W,rb', SHAPES)
def test_mask_intersections_equals_the_host_rule(dev, D, G, H, W, rb):
    rs = np.random.RandomState(D * 7 + G * 3 + W)
    det, gt = _planes(rs, D, H, W, rb, 0.45, 'rand'), _planes(rs, G, H, W, rb, 0.3, 'rand')
    inter, area_d, area_g = _check_intersections(dev, det, gt, W)
    if D and G and H * W > 64:
        assert inter.min() > 0 and (area_d > 0).all()       # every pair is exercised


def test_mask_intersections_with_16_byte_rows_and_several_slabs(dev):
    """(100, 40, 256, 264) with rows padded to 48 bytes: the wide-load path over 52 slabs, two blocks of detections"""
    rs = np.random.RandomState(5)
    det, gt = _planes(rs, 100, 256, 264, 48, 0.5, 'rand'), _planes(rs, 40, 256, 264, 48, 0.2, 'rand')
    _check_intersections(dev, det, gt, 264)


def test_mask_intersections_pad_bits_of_ones_and_large_strides(dev):
    rs = np.random.RandomState(6)
    D, G, H, W, rb = 6, 4, 21, 43, 16
    det, gt = _planes(rs, D, H, W, rb, 0.5, 'ones'), _planes(rs, G, H, W, rb, 0.5, 'ones')
    assert det[:, :, 6:].min() == 255 and (det[:, :, 5] >> 3).min() == 31
    _check_intersections(dev, det, gt, W)
    # planes further apart than H * row_bytes (a slice of a larger buffer, garbage between the planes), on both sides
    big_d = torch.randint(0, 256, (D, H + 3, rb), dtype=torch.uint8, device=dev)
    big_g = torch.randint(0, 256, (G, 2 * H, rb), dtype=torch.uint8, device=dev)
    big_d[:, :H] = torch.from_numpy(det).to(dev)
    big_g[:, :H] = torch.from_numpy(gt).to(dev)
    det_t, gt_t = big_d[:, :H], big_g[:, :H]
    assert det_t.stride(0) == (H + 3) * rb and not det_t.is_contiguous()
    _check_intersections(dev, det, gt, W, det_t, gt_t)


def _device_match(dev, im, inter, area_d, area_g, cat_ids, area_rngs, iou_thrs, max_det, agn):
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x)).to(device=dev, dtype=dt)        # noqa: E731
    scores = t(im['det_scores'], torch.float32)
    order = torch.sort(scores, descending=True, stable=True).indices.to(torch.int32)
    out = ops.coco_match(t(inter, torch.int32), t(area_d, torch.int32), t(area_g, torch.int32), order, t(im['det_cats'], torch.int32),
                         t(im['gt_cats'], torch.int32), t(im['gt_crowd'], torch.uint8), t(im['gt_area'], torch.float64),
                         t(cat_ids, torch.int32), t(area_rngs, torch.float64), t(iou_thrs, torch.float64), max_det, agn)
    torch.cuda.synchronize()
    dtm, dti, gti, counts = (o.cpu().numpy() for o in out)
    return mask_eval.records_from_match(dtm, dti, gti, counts, order.cpu().numpy(), im['det_cats'], im['det_scores'], cat_ids, agn), \
        (dtm, dti, gti, counts)


@pytest.mark.parametrize('tag,agn', C.MODES)
def test_coco_match_equals_the_host_rule_on_the_fixture(dev, tag, agn):
    z = C.fixture()
    want_all = C.fixture_records(tag)
    for i, im in enumerate(C.fixture_images()):
        want, iou, inter, area_d, area_g = C.host_records(im, int(z['W']), agn, z['cat_ids'], z['area_rngs'], z['iou_thrs'],
                                                          int(z['max_dets'][-1]))
        got, raw = _device_match(dev, im, inter, area_d, area_g, z['cat_ids'], z['area_rngs'], z['iou_thrs'], int(z['max_dets'][-1]), agn)
        C.assert_records_equal(got, want, (tag, i, 'host rule'))
        C.assert_records_equal(got, want_all[i], (tag, i, 'reference'))
        for k in range(len(got)):
            for a in range(4):
                if got[k][a] is not None:
                    assert np.array_equal(got[k][a]['dt_index'], want[k][a]['dt_index'])
        # what lies past D_k / G_k is written, as zeros
        dtm, dti, gti, counts = raw
        for k in range(len(got)):
            assert not dtm[k, :, :, counts[k, 0]:].any() and not dti[k, :, :, counts[k, 0]:].any() and not gti[k, :, counts[k, 1]:].any()


def test_coco_match_quotients_sit_on_the_thresholds(dev):
    """The double quotient the kernel forms is numpy's, bit for bit: for pairs with small integer areas, thresholds are set to the
    float64 quotient itself, to the next double below and to the next above. A detection matches at t iff iou >= min(t, 1 - 1e-10),
    so one unit in the last place in the kernel's division would flip a match against the host rule."""
    pairs = [(1, 2), (1, 3), (2, 3), (3, 7), (5, 9), (7, 11), (10, 13), (49, 97), (1000, 1999), (123457, 222223)]
    n = len(pairs)
    inter = np.zeros((n, n), np.int64)
    area_d, area_g = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i, (a, b) in enumerate(pairs):                     # union = b: area_d = a, area_g = b, d inside g
        inter[i, i], area_d[i], area_g[i] = a, a, b
    iou = mask_eval.mask_iou_host(inter, area_d, area_g, np.zeros(n, bool))
    assert all(iou[i, i] == np.float64(a) / np.float64(b) for i, (a, b) in enumerate(pairs))
    im = dict(det_scores=np.linspace(0.9, 0.1, n).astype(np.float32), det_cats=np.arange(n), gt_cats=np.arange(n),
              gt_crowd=np.zeros(n, bool), gt_area=area_g.astype(np.float64))
    area_rngs = np.array([[0, 1e10]])
    for lo in range(0, n, 3):
        q = np.array([iou[i, i] for i in range(lo, min(lo + 3, n))])
        thrs = np.sort(np.concatenate([q, np.nextafter(q, 0), np.nextafter(q, 1)]))
        want = mask_eval.evaluate_img_host(iou, im['det_scores'], im['det_cats'], im['gt_cats'], im['gt_crowd'], im['gt_area'], area_d,
                                           np.arange(n), area_rngs, thrs, 100, False)
        got, _ = _device_match(dev, im, inter, area_d, area_g, np.arange(n), area_rngs, thrs, 100, False)
        C.assert_records_equal(got, want, lo)
        for i in range(lo, min(lo + 3, n)):
            m = want[i][0]['dt_match'][:, 0]
            assert m[thrs <= iou[i, i]].all() and not m[thrs > iou[i, i]].any()      # the flip happens exactly at the quotient


@pytest.mark.parametrize('agn', [False, True])
def test_coco_match_on_a_random_image(dev, agn):
    im = C.random_image(31)                                # D = 100, G = 40, K = 12
    cat_ids = np.arange(1, 13)
    thrs, rngs = mask_eval.default_iou_thrs(), np.asarray(mask_eval.AREA_RNGS)
    want, iou, inter, area_d, area_g = C.host_records(im, im['W'], agn, cat_ids, rngs, thrs, 30 if agn else 7)
    got, _ = _device_match(dev, im, inter, area_d, area_g, cat_ids, rngs, thrs, 30 if agn else 7, agn)
    C.assert_records_equal(got, want, agn)
    matches = np.concatenate([r['dt_match'].ravel() for per_area in want for r in per_area if r is not None])
    assert (matches > 0).sum() > 50 and (matches == 0).sum() > 50
    assert any(r['dt_ignore'].any() for per_area in want for r in per_area if r is not None)


def _evaluators(dev, agn):
    z = C.fixture()
    kw = dict(unknown_cat_ids=z['unknown_cat_ids'], all_cat_ids=z['all_cat_ids'], max_dets=z['max_dets'], class_agnostic=agn)
    return mask_eval.SegmEvaluator(z['cat_ids'], device=dev, **kw), mask_eval.SegmEvaluator(z['cat_ids'], device=None, **kw)


def _assert_summaries_equal(a, b):
    assert set(a) == set(b)
    for name in ('precision', 'recall', 'scores'):
        assert a[name].tobytes() == b[name].tobytes(), name
    assert a['stats'] == b['stats'] and a['images'] == b['images']
    assert np.array_equal(np.array([a['base_ap50'], a['novel_ap50'], a['all_ap50']]),
                          np.array([b['base_ap50'], b['novel_ap50'], b['all_ap50']]), equal_nan=True)


@pytest.mark.parametrize('tag,agn', C.MODES)
def test_segm_evaluator_on_the_device_equals_the_host_evaluator(dev, tag, agn):
    z = C.fixture()
    W = int(z['W'])
    on_dev, on_host = _evaluators(dev, agn)
    label_of = {int(c): i for i, c in enumerate(z['cat_ids'])}
    for n, im in enumerate(C.fixture_images()):
        D = len(im['det_cats'])
        boxes = np.zeros((D, 5), np.float32)
        boxes[:, 4] = im['det_scores']
        labels = torch.tensor([label_of[int(c)] for c in im['det_cats']], dtype=torch.int64)
        gt = np.unpackbits(im['gt_bits'], axis=2, bitorder='little')[:, :, :W]        # uint8 bitmaps on the host
        on_host.add(labels, torch.from_numpy(boxes), torch.from_numpy(im['det_bits']), gt, im['gt_cats'], im['gt_crowd'], im['gt_area'])
        # the device evaluator takes device results; ground truth alternately as host uint8 and as device bool bitmaps
        gt_in = gt if n % 2 == 0 else torch.from_numpy(gt.astype(bool)).to(dev)
        on_dev.add(labels.to(dev), torch.from_numpy(boxes).to(dev), torch.from_numpy(im['det_bits']).to(dev), gt_in, im['gt_cats'],
                   im['gt_crowd'], im['gt_area'])
    a, b = on_dev.summarize(), on_host.summarize()
    _assert_summaries_equal(a, b)
    for ra, rb in zip(on_dev.records, on_host.records):
        C.assert_records_equal(ra, rb)
    assert a['precision'].tobytes() == z[tag + 'precision'].tobytes()
    assert (a['base_ap50'], a['novel_ap50'], a['all_ap50']) == tuple(z[tag + 'open_set_ap50'])


def test_one_add_replays_from_a_captured_graph(dev):
    """the two launches of one `add` (intersections, then matching) under torch.cuda.graph, single-branch: two replays on new
    inputs give the records of the host rule both times"""
    z = C.fixture()
    ims = [C.random_image(s, D=20, G=9, K=5, H=37, W=45) for s in (41, 42)]
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x)).to(device=dev, dtype=dt)        # noqa: E731
    cat_ids, rngs, thrs = np.arange(1, 6), z['area_rngs'], z['iou_thrs']
    st = dict(det=t(ims[0]['det_bits'], torch.uint8), gt=t(ims[0]['gt_bits'], torch.uint8), order=torch.zeros(20, dtype=torch.int32, device=dev),
              det_cats=t(ims[0]['det_cats'], torch.int32), gt_cats=t(ims[0]['gt_cats'], torch.int32),
              crowd=t(ims[0]['gt_crowd'], torch.uint8), area=t(ims[0]['gt_area'], torch.float64))
    consts = (t(cat_ids, torch.int32), t(rngs, torch.float64), t(thrs, torch.float64))

    def launches():
        inter, area_d, area_g = ops.mask_intersections(st['det'], st['gt'], 45)
        return ops.coco_match(inter, area_d, area_g, st['order'], st['det_cats'], st['gt_cats'], st['crowd'], st['area'], *consts, 10, False)

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
        order = torch.sort(t(im['det_scores'], torch.float32), descending=True, stable=True).indices.to(torch.int32)
        for key, src, dt in (('det', im['det_bits'], torch.uint8), ('gt', im['gt_bits'], torch.uint8), ('det_cats', im['det_cats'], torch.int32),
                             ('gt_cats', im['gt_cats'], torch.int32), ('crowd', im['gt_crowd'], torch.uint8), ('area', im['gt_area'], torch.float64)):
            st[key].copy_(t(src, dt))
        st['order'].copy_(order)
        graph.replay()
        torch.cuda.synchronize()
        dtm, dti, gti, counts = (o.cpu().numpy() for o in out)
        got = mask_eval.records_from_match(dtm, dti, gti, counts, order.cpu().numpy(), im['det_cats'], im['det_scores'], cat_ids, False)
        want = C.host_records(im, 45, False, cat_ids, rngs, thrs, 10)[0]
        C.assert_records_equal(got, want)


def test_tiny_model_end_to_end_device_evaluator_equals_host_evaluator(dev):
    """simple_test(device_results=True, mask_bits=True) of a tiny random-weight model at 64 x 64 against synthetic ground truth"""
    from util import randomize
    cfg = synthetic.model_config(num_things=10, num_stuff=0, num_unknown=3, num_queries=20, depth=50, enc_layers=2, dec_layers=3,
                                 vocab=500, num_points=256)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = registry.build_detector(cfg)
    randomize(model, seed=23)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_var.fill_(1.0)
            m.running_mean.zero_()
    model = model.to(dev).eval()
    model.panoptic_fusion_head.test_cfg['max_per_image'] = 20
    B, H, W = 2, 64, 64
    metas = synthetic.img_metas(B, H, W)
    img = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad(), runtime.precision_scope('bf16'):
        results = model.simple_test(img, metas, rescale=True, device_results=True, mask_bits=True)
    fh = model.panoptic_fusion_head
    key = next(k for k in ('all_results', 'base_results', 'novel_results') if k in results[0])
    n_classes = dict(all_results=fh.all_classes, base_results=fh.base_classes, novel_results=fh.novel_classes)[key]
    cat_ids = list(range(1, n_classes + 1))
    kw = dict(unknown_cat_ids=cat_ids[-3:], max_dets=(1, 5, 20))
    on_dev, on_host = mask_eval.SegmEvaluator(cat_ids, device=dev, **kw), mask_eval.SegmEvaluator(cat_ids, device=None, **kw)
    rs = np.random.RandomState(9)
    n_det = 0
    for res in results:
        labels, boxes, bits = res[key]
        assert bits.dtype == torch.uint8 and tuple(bits.shape[1:]) == (H, W // 8)
        n_det += bits.shape[0]
        # ground truth: the first detections' own masks with noise (so that something matches), with their categories, and a crowd
        un = np.unpackbits(bits[:4].cpu().numpy(), axis=-1, bitorder='little').astype(bool)
        gt = np.concatenate([un & (rs.rand(*un.shape) < 0.9), rs.rand(2, H, W) < 0.3])
        gt_cats = np.concatenate([np.asarray(cat_ids)[labels[:len(un)].cpu().numpy()], [1, 2]])
        crowd = np.zeros(len(gt), bool)
        crowd[-1] = True
        on_dev.add(labels, boxes, bits, gt, gt_cats, crowd)
        on_host.add(labels, boxes, bits, gt, gt_cats, crowd)
    assert n_det > 0
    a, b = on_dev.summarize(), on_host.summarize()
    _assert_summaries_equal(a, b)
    for ra, rb in zip(on_dev.records, on_host.records):
        C.assert_records_equal(ra, rb)
    assert (a['precision'] > 0).any()


def test_tools_test_eval_segm(dev, tmp_path, capsys):
    """tools/test.py --eval segm on a --data stream with ground truth: the pipelined run and the sequential run write the same
    summary, and it is the summary of a host evaluator fed with the results the driver returns; a stream without ground truth keeps
    the driver's message"""
    import importlib.util
    import json
    import os
    import sys
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
    spec = importlib.util.spec_from_file_location('cgg_tools_test_eval', os.path.join(root, 'tools', 'test.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    common = [str(cfg_file), ck, '--data', 'mask_eval_cases:eval_stream', '--eval', 'segm', '--precision', 'bf16']
    a = drv.main(common + ['--work-dir', str(tmp_path / 'a')])
    b = drv.main(common + ['--work-dir', str(tmp_path / 'b'), '--no-pipeline'])
    out = capsys.readouterr().out
    assert 'segm all_results: 5 images' in out and 'AP50: base' in out
    text_a, text_b = (tmp_path / 'a' / 'segm_eval.json').read_text(), (tmp_path / 'b' / 'segm_eval.json').read_text()
    assert text_a == text_b
    summary = json.loads(text_a)
    assert len(a) == len(b) == 6 and set(summary) == {k for k in a[0] if k.endswith('_results')}
    metas = [m for _, m in C.eval_stream(None, 0, 1)]
    fh = model.panoptic_fusion_head
    for key, got in summary.items():
        n_cls = getattr(fh, key.replace('_results', '_classes'))
        ev = mask_eval.SegmEvaluator(list(range(1, n_cls + 1)), unknown_cat_ids=[3, 4], max_dets=(1, 5, 20), skip_images_without_gt=True)
        for res, m in zip(b, metas[:5]):
            labels, boxes, bits = res[key]
            # --eval segm sets --mask-bits: bit planes where the head's gate allows them, bool bitmaps elsewhere; both are taken
            assert (bits.dtype, bits.shape[1:]) in ((np.uint8, (64, 8)), (np.bool_, (64, 64)))
            ev.add(labels, boxes, torch.from_numpy(bits), m['gt_masks'], m['gt_labels'], m['gt_crowd'], m['gt_area'])
        want = ev.summarize()
        assert got['images'] == want['images'] == 5
        assert json.dumps(got['stats']) == json.dumps(want['stats'])
        assert json.dumps([got['base_ap50'], got['novel_ap50'], got['all_ap50']]) == \
            json.dumps([want['base_ap50'], want['novel_ap50'], want['all_ap50']])
    # no ground truth in the stream (the synthetic images): the option is reported as unavailable, as before
    drv.main([str(cfg_file), ck, '--num-images', '2', '--synthetic', '64', '--eval', 'segm', '--precision', 'bf16', '--no-pipeline'])
    assert 'carries no ground truth' in capsys.readouterr().out
