"""GPU tests of the batched device-side panoptic fusion (`cgg_panoptic_fuse_batched`, `panoptic_postprocess_batched`): against
the oracle, against the per-image device path, its segment table, both sides of the argmax kernel's footprint gate, capture and
replay on new data, and the captured detector pipeline. The fixture and the oracle helpers live in tests/test_panoptic_fuse.py."""
import functools
import warnings

import numpy as np
import pytest
import torch

import cgg_amd  # noqa: F401
from cgg_amd import maskformer_fusion_head as mfh
from cgg_amd import registry, synthetic
from cgg_amd.mask2former_head import LowResMasks
from oracle import head as OH

import test_panoptic_fuse as T

pytestmark = pytest.mark.gpu

NCLS, NTH = T.NCLS, T.NTH


def assert_panoptic_equal(got, want, dbg, eps, what):
    """tests/test_fullsize_gpu.py's rule, restated: int32 maps EXACTLY equal except on pixels whose decision sits within `eps` of
    a tie in the oracle (argmax margin, or the winner's distance to the 0.5 threshold); at most 1e-3 of the pixels may differ."""
    assert got.shape == want.shape and got.dtype == torch.int32, (got.shape, want.shape, got.dtype)
    diff = got != want
    n = int(diff.sum())
    if n:
        explained = (dbg['pixel_margin'] <= eps) | (dbg['half_margin'] <= eps)
        bad = diff & ~explained
        assert not bool(bad.any()), (what, int(bad.sum()), n)
    assert n <= 1e-3 * diff.numel(), (what, n)
    return n


def fusion_head(dev, table, flt, limit=T.LIMIT):
    fh = registry.build_head(dict(type='MaskFormerFusionHeadOpen', num_things_classes=NTH, num_stuff_classes=NCLS - NTH,
                                  panoptic_mode=True,
                                  test_cfg=dict(eval_types=['all_results'], object_mask_thr=T.THR, iou_thr=T.IOU,
                                                filter_low_score=flt, stuff_area_limit=limit))).to(dev)
    fh.all_class_embs = table.to(dev)
    return fh


@functools.lru_cache(maxsize=None)
def oracle_maps(order, metas_key, rescale, flt, limit=T.LIMIT):
    """[(want `_emb`, want plain, debug)] per image of the batch `order`, from the concatenated-table inputs the device gets"""
    metas = METAS_BY_KEY[metas_key]
    emb, logits, table = T.batch_inputs(order)
    out = []
    for b in range(len(order)):
        mp = T.resized(logits[b], metas[b], rescale)
        dbg = {}
        want = OH.panoptic_postprocess_emb(emb[b], mp, table, NCLS, NTH, T.THR, T.IOU, flt, limit, debug=dbg)
        plain = OH.panoptic_postprocess(emb[b] @ table.t(), mp, NCLS, NTH, T.THR, T.IOU, flt)
        out.append((want, plain, dbg))
    return out


GATE_METAS = [T.meta((152, 212), (20, 28))]
METAS_BY_KEY = {'batch': T.METAS, 'gate': GATE_METAS}


@functools.lru_cache(maxsize=None)
def device_inputs(order, dev):
    emb, logits, table = T.batch_inputs(order)
    return emb.to(dev), logits.to(dev), (emb @ table.t()).to(dev), table


@pytest.mark.parametrize('rescale', [False, True])
@pytest.mark.parametrize('flt', [True, False])
def test_batched_maps_equal_the_oracle(dev, rescale, flt):
    order = (0, 1, 2)
    emb, logits, mask_cls, table = device_inputs(order, dev)
    fh = fusion_head(dev, table, flt)
    wants = oracle_maps(order, 'batch', rescale, flt)
    for variant, x in (('emb', emb), ('plain', mask_cls)):
        maps, info = fh.panoptic_postprocess_batched(x, LowResMasks(logits, T.UP), T.METAS, rescale, emb=variant == 'emb',
                                                     with_segments=True, debug=True)
        assert info['n_kept'].cpu().tolist() == [70, 0, 70]
        blocks = info['blocks'].cpu().tolist()
        assert blocks[0][0] > 0 and blocks[2][0] > 0 and blocks[0][1] == 0 and blocks[2][1] == 0, blocks    # inside the gate
        assert blocks[1] == [0, 0]                                                                         # nothing kept: no work
        for b in (0, 2):
            want, plain, dbg = wants[b]
            T.assert_decision_margins(dbg)
            assert assert_panoptic_equal(want, want, dbg, 1e-5, 'oracle against itself') == 0
            n = assert_panoptic_equal(maps[b].cpu(), want if variant == 'emb' else plain, dbg, 1e-5, (variant, b, rescale, flt))
            print(f'batched vs oracle ({variant}, image {b}, rescale={rescale}, filter={flt}): {n} of {want.numel()} pixels differ')
        assert maps[1].shape == wants[1][0].shape and bool((maps[1] == NCLS).all()) and bool((wants[1][0] == NCLS).all())


@pytest.mark.parametrize('rescale', [False, True])
def test_batched_equals_the_per_image_device_path(dev, rescale):
    order = (0, 1, 2)
    emb, logits, mask_cls, table = device_inputs(order, dev)
    fh = fusion_head(dev, table, True)
    wants = oracle_maps(order, 'batch', rescale, True)
    maps = fh.panoptic_postprocess_batched(emb, LowResMasks(logits, T.UP), T.METAS, rescale, emb=True)
    plain = fh.panoptic_postprocess_batched(mask_cls, LowResMasks(logits, T.UP), T.METAS, rescale, emb=False)
    for b in range(3):
        one = fh.panoptic_postprocess_emb(emb[b], LowResMasks(logits[b], T.UP), fh.all_class_embs, T.METAS[b], rescale)
        one_plain = fh.panoptic_postprocess(mask_cls[b], LowResMasks(logits[b], T.UP), T.METAS[b], rescale)
        if b == 1:
            assert torch.equal(maps[b], one) and torch.equal(plain[b], one_plain)
            continue
        dbg = wants[b][2]
        n = assert_panoptic_equal(maps[b].cpu(), one.cpu(), dbg, 1e-5, ('emb', b, rescale))
        m = assert_panoptic_equal(plain[b].cpu(), one_plain.cpu(), dbg, 1e-5, ('plain', b, rescale))
        print(f'batched vs per-image device path (image {b}, rescale={rescale}): {n} (emb) / {m} (plain) pixels differ')


def test_segment_table_from_the_device(dev):
    order = (0, 1, 2)
    emb, logits, mask_cls, table = device_inputs(order, dev)
    fh = fusion_head(dev, table, True)
    for variant, x in (('emb', emb), ('plain', mask_cls)):
        maps, info = fh.panoptic_postprocess_batched(x, LowResMasks(logits, T.UP), T.METAS, True, emb=variant == 'emb',
                                                     with_segments=True)
        n_kept, tab, scores = info['n_kept'].cpu().numpy(), info['table'].cpu().numpy(), info['scores'].cpu().numpy()
        for b in range(3):
            seg = maps[b].cpu().numpy()
            rows = mfh.segments_info(tab[b], n_kept[b], NTH, scores[b])
            vals, cnts = np.unique(seg[seg != NCLS], return_counts=True)
            assert {d['id']: d['area'] for d in rows} == dict(zip(vals.tolist(), cnts.tolist())), (variant, b)
            # thing ids: category + i * 1000, i counting up in query order over the ACCEPTED things (painted or not)
            t = tab[b][:n_kept[b]]
            things = t[t[:, 0] >= 1000]
            assert things[:, 0].tolist() == [int(c) + 1000 * (i + 1) for i, c in enumerate(things[:, 1])]
            assert bool((np.diff(t[:, 3]) > 0).all()) and bool((things[:, 1] < NTH).all())
            assert bool((tab[b][n_kept[b]:] == np.array([-1, -1, 0, -1])).all())
            assert bool((scores[b][:n_kept[b]] > T.THR).all()) and bool((scores[b][n_kept[b]:] == 0).all())
            if b != 1:
                assert len(things) >= 40 and any(not d['isthing'] for d in rows)


def test_footprint_gate_global_memory_side(dev):
    """ori_shape (20, 28) with rescale: the first tile row's 16 output rows reach across ~32 x 54 low-resolution samples per
    query -- more than the LDS window takes for 8 queries -- so those blocks read global memory with the same expressions (the
    standard batch, asserted above, stays inside the gate). Stuff areas sit within a pixel of the limit here: maps only."""
    emb, logits, _, table = device_inputs((0,), dev)
    fh = fusion_head(dev, table, True, limit=4)
    want, _, dbg = oracle_maps((0,), 'gate', True, True, 4)[0]
    maps, info = fh.panoptic_postprocess_batched(emb, LowResMasks(logits, T.UP), GATE_METAS, True, emb=True, debug=True)
    blocks = info['blocks'].cpu().tolist()
    print(f'footprint gate: blocks [LDS, global] = {blocks}')
    assert blocks[0][1] > 0, blocks
    got = maps[0].cpu()
    print(f'footprint gate: {int((got != want).sum())} of {want.numel()} pixels differ from the oracle')
    assert_panoptic_equal(got, want, dbg, 1e-5, 'global-memory side of the gate')


def test_capture_and_replay_on_new_data(dev):
    """ONE graph holds the whole batched call; replayed on other inputs written into the same buffers (other kept counts per
    slot) it returns what the eager call returns on them, exactly."""
    orders = [(0, 1, 2), (2, 1, 0), (1, 2, 0)]
    table = T.batch_inputs(orders[0])[2]
    fh = fusion_head(dev, table, True)
    eager = []
    for order in orders:
        emb, logits, _, _ = device_inputs(order, dev)
        maps, info = fh.panoptic_postprocess_batched(emb, LowResMasks(logits, T.UP), T.METAS, True, emb=True, with_segments=True)
        eager.append(([m.clone() for m in maps], {k: v.clone() for k, v in info.items()}))
    assert [e[1]['n_kept'].cpu().tolist() for e in eager] == [[70, 0, 70], [70, 0, 70], [0, 70, 70]]
    emb_s, logits_s = (t.clone() for t in device_inputs(orders[0], dev)[:2])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        maps, info = fh.panoptic_postprocess_batched(emb_s, LowResMasks(logits_s, T.UP), T.METAS, True, emb=True, with_segments=True)
    for order, (want_maps, want_info) in zip(orders[1:] + orders[:1], eager[1:] + eager[:1]):
        emb, logits, _, _ = device_inputs(order, dev)
        emb_s.copy_(emb)
        logits_s.copy_(logits)
        graph.replay()
        torch.cuda.synchronize()
        print(f'replay {order}: n_kept {info["n_kept"].cpu().tolist()}, pixels differing from the eager call',
              [int((got != want).sum()) for got, want in zip(maps, want_maps)], ', table entries differing',
              int((info['table'] != want_info['table']).sum()), ', scores differing', int((info['scores'] != want_info['scores']).sum()))
        for k in want_info:
            assert torch.equal(info[k], want_info[k]), (order, k)
        for got, want in zip(maps, want_maps):
            assert torch.equal(got, want), order


def test_detector_pipeline_captures_panoptic_postprocessing(dev):
    """`detector_pipeline` of a panoptic model has no eager tail any more and returns, submission after submission, the maps
    `simple_test` returns eagerly; the per-image switch brings the tail back."""
    from cgg_amd.pipeline import detector_pipeline
    from util import randomize
    cfg = synthetic.model_config(num_things=10, num_stuff=4, num_unknown=3, num_queries=20, depth=50, panoptic=True, enc_layers=2,
                                 dec_layers=3, vocab=500, num_points=256)
    # random weights: low thresholds, so that the maps hold segments
    cfg['test_cfg'].update(object_mask_thr=0.05, iou_thr=0.05, stuff_area_limit=16)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = registry.build_detector(cfg)
    randomize(model, seed=9)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_var.fill_(1.0)
            m.running_mean.zero_()
    model = model.to(dev).eval()
    B, H, W = 2, 128, 160
    metas = synthetic.img_metas(B, H, W, ori=(100, 130))
    imgs = [synthetic.structured_images(B, H, W, seed=s).to(dev) for s in (3, 4)]
    with torch.no_grad():
        want = [[r['panoptic_all_results'].clone() for r in model.simple_test(im, metas, rescale=True, device_results=True)]
                for im in imgs]
        torch.cuda.synchronize()
        pipe = detector_pipeline(model, imgs[0], metas, stages=3, rescale=True, device_results=True)
        assert pipe.tail is None
        got = []
        for im in imgs:
            res = pipe.wait(pipe.submit(im))
            got.append([r['panoptic_all_results'].clone() for r in res])
        pipe.flush()
        torch.cuda.synchronize()
        # host results with `with_segments`: numpy maps and COCO-panoptic dicts that describe them
        for r in model.simple_test(imgs[0], metas, rescale=True, with_segments=True):
            seg, rows = r['panoptic_all_results'], r['panoptic_segments']
            vals, cnts = np.unique(seg[seg != model.num_classes], return_counts=True)
            assert isinstance(seg, np.ndarray) and {d['id']: d['area'] for d in rows} == dict(zip(vals.tolist(), cnts.tolist()))
            assert all(set(d) == {'id', 'category_id', 'isthing', 'area', 'score', 'query'} for d in rows)
        try:
            mfh.PER_IMAGE_PANOPTIC = True
            per_image = [r['panoptic_all_results'] for r in model.simple_test(imgs[0], metas, rescale=True, device_results=True)]
            torch.cuda.synchronize()
        finally:
            mfh.PER_IMAGE_PANOPTIC = False
    for w_b, g_b in zip(want, got):
        for w, g in zip(w_b, g_b):
            assert w.shape == (100, 130) and torch.equal(w, g)
    print('pipeline maps: distinct values per image', [[int(torch.unique(w).numel()) for w in w_b] for w_b in want],
          '; pixels differing from the per-image path', [int((a != b).sum()) for a, b in zip(want[0], per_image)])
    assert all(torch.unique(w).numel() > 1 for w_b in want for w in w_b), 'the fixture paints nothing: the comparison is empty'
