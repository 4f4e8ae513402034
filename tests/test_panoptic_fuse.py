"""CPU tests of the batched panoptic fusion: the written rule (`panoptic_decide_host`) against the oracle, hand-made counters
at the rule's edges, the segment-table helper and the C ABI's argument checks. Also holds the fixture that
tests/test_panoptic_fuse_gpu.py runs on the device."""
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

import cgg_amd  # noqa: F401
from cgg_amd import _lib
from cgg_amd.maskformer_fusion_head import panoptic_decide_host, segments_info
from oracle import head as OH

NCLS, NTH, D = 12, 8, 64
UP = (160, 224)
THR, IOU, LIMIT = 0.8, 0.8, 256           # stuff_area_limit: 4096 scaled by the 1/16 area ratio of this fixture to configs[4]


def small_case(Q=96, h=40, w=56, seed=0, ncls=12, nth=8, D=64, grid=(7, 10)):
    g = torch.Generator().manual_seed(seed)
    cls_embs = torch.randn(ncls + 1, D, generator=g); cls_embs[-1] = 0
    emb = torch.zeros(Q, D)
    ys = torch.arange(h).view(h, 1).float(); xs = torch.arange(w).view(1, w).float()
    logits = -6 + 0.3 * torch.randn(Q, h, w, generator=g)
    k = 0
    for gy in range(grid[0]):
        for gx in range(grid[1]):
            cy = (gy + 0.5) * h / grid[0] + float(torch.randn(1, generator=g)) * 0.8
            cx = (gx + 0.5) * w / grid[1] + float(torch.randn(1, generator=g)) * 0.8
            r = 2.0 + float(torch.rand(1, generator=g)) * (1.5 if k % 7 else 5.0)
            c = int(torch.randint(0, ncls, (1,), generator=g))
            emb[k] = cls_embs[c] * 0.5
            logits[k] = 6 - ((ys - cy)**2 + (xs - cx)**2) / r**2 * 6 + 0.3 * torch.randn(h, w, generator=g)
            k += 1
    nrej = (Q - k) * 2 // 3
    for q in range(k, k + nrej):
        emb[q] = torch.randn(D, generator=g) * 1e-3
        logits[q] = 3 * torch.randn(1, generator=g) + torch.randn(h, w, generator=g)
    for q in range(k + nrej, Q):
        emb[q] = -cls_embs[:-1].mean(0) * 2
        logits[q] = 4 + torch.randn(h, w, generator=g)
    return emb, logits, cls_embs


def meta(img_shape, ori_shape):
    return dict(img_shape=img_shape + (3,), ori_shape=ori_shape + (3,), pad_shape=UP + (3,), batch_input_shape=UP, scale_factor=1.0,
                flip=False)


# the batch: image 1 keeps nothing (emb = 0 scores every class 1/13, all logits -6)
METAS = [meta((152, 212), (96, 134)), meta((160, 201), (230, 289)), meta((160, 201), (230, 289))]
SEEDS = [5, None, 0]


@functools.lru_cache(maxsize=None)
def image_inputs(i):
    """(emb (Q, D), logits (Q, h, w), cls_embs (13, D)) of batch image i with its OWN class table"""
    if SEEDS[i] is None:
        _, logits, cls_embs = small_case(seed=0)
        return torch.zeros(96, D), torch.full_like(logits, -6.0), cls_embs
    return small_case(seed=SEEDS[i])


@functools.lru_cache(maxsize=None)
def batch_inputs(order=(0, 1, 2)):
    """The images `order` as ONE batch against ONE class table: images 0 and 2 were made with different tables, so the table is
    [table of image 0 | table of image 2] along D and each embedding is zero in the other half -- every dot product keeps its
    terms. -> (emb (B, Q, 2D), logits (B, Q, h, w), cls_embs (13, 2D))"""
    t0, t2 = image_inputs(0)[2], image_inputs(2)[2]
    table = torch.cat([t0, t2], 1)
    embs, logits = [], []
    for i in order:
        e, lg, _ = image_inputs(i)
        z = torch.zeros_like(e)
        embs.append(torch.cat([e, z], 1) if i == 0 else torch.cat([z, e], 1))
        logits.append(lg)
    return torch.stack(embs), torch.stack(logits), table


def resized(logits, m, rescale):
    """the oracle's mask_pred of one image: upsample to batch_input_shape, crop img_shape, (rescale to ori_shape)"""
    up = F.interpolate(logits[None], UP, mode='bilinear', align_corners=False)[0]
    return OH.crop_rescale(up, m, rescale)


def assert_decision_margins(dbg):
    """no segment-level decision of the fixture sits near its threshold, so a pixel-level tie cannot move a segment"""
    assert dbg['kept'] == 70, dbg['kept']
    assert float(dbg['score_margin'].min()) > 0.1
    assert min(dbg['ratio_margin']) > 0.01
    assert min(dbg['stuff_margin']) >= 5


@functools.lru_cache(maxsize=None)
def oracle_case(i, rescale):
    """everything the host-rule tests need of image i, computed once with torch on the CPU from the oracle-resized masks"""
    emb, logits, cls_embs = image_inputs(i)
    mp = resized(logits, METAS[i], rescale)
    scores, labels = OH.cls_emb_scores(emb, cls_embs).max(-1)
    keep = labels.ne(NCLS) & (scores > THR)
    cs, cc, cm = scores[keep], labels[keep], mp.sigmoid()[keep]
    ids = (cs.view(-1, 1, 1) * cm).argmax(0)
    half = cm >= 0.5
    n = int(keep.sum())
    counts = [[int((ids == k).sum()), int(half[k].sum()), int(((ids == k) & half[k]).sum())] for k in range(n)]
    return dict(emb=emb, cls_embs=cls_embs, mp=mp, classes=cc.tolist(), counts=counts, ids=ids.numpy(),
                win_half=half.gather(0, ids[None])[0].numpy(), query=torch.nonzero(keep).flatten().tolist(), scores=cs.tolist())


def paint(c, lut_val, lut_half):
    lv, lh = np.asarray(lut_val), np.asarray(lut_half).astype(bool)
    v = lv[c['ids']]
    ok = (v >= 0) & (~lh[c['ids']] | c['win_half'])
    return np.where(ok, v, NCLS).astype(np.int32)


def test_host_rule_matches_the_oracle():
    """`panoptic_decide_host` on torch-made counters + a numpy LUT paint == the oracle's maps, both variants, rescale and
    filter_low_score on and off. Same arithmetic on the same machine: exact."""
    for i in (0, 2):
        for rescale in (False, True):
            c = oracle_case(i, rescale)
            assert len(c['classes']) == 70
            for flt in (True, False):
                dbg = {}
                want = OH.panoptic_postprocess_emb(c['emb'], c['mp'], c['cls_embs'], NCLS, NTH, THR, IOU, flt, LIMIT, debug=dbg)
                assert_decision_margins(dbg)
                ids = torch.unique(want)
                assert 40 <= int((ids >= 1000).sum()) <= 50 and int(((ids >= NTH) & (ids < NCLS)).sum()) == 4 and bool((want == NCLS).any())
                lut_val, lut_half, area = panoptic_decide_host(c['classes'], c['counts'], NTH, IOU, flt, LIMIT, True)
                got = paint(c, lut_val, lut_half)
                assert np.array_equal(got, want.numpy()), (i, rescale, flt, int((got != want.numpy()).sum()))
                for k, v in enumerate(lut_val):                      # `area` is what the paint step wrote (things: one slot per value)
                    if v >= 1000:
                        assert area[k] == int((got == v).sum()), (k, v)
                    if v < 0:
                        assert area[k] == 0
                # plain variant: same scores from the classification logits emb @ E^T
                want = OH.panoptic_postprocess(c['emb'] @ c['cls_embs'].t(), c['mp'], NCLS, NTH, THR, IOU, flt)
                lut_val, lut_half, _ = panoptic_decide_host(c['classes'], c['counts'], NTH, IOU, flt, LIMIT, False)
                got = paint(c, lut_val, lut_half)
                assert np.array_equal(got, want.numpy()), ('plain', i, rescale, flt, int((got != want.numpy()).sum()))


def test_host_rule_on_hand_made_counters():
    # a thing whose filtered area is 0 still consumes an instance id
    lv, lh, area = panoptic_decide_host([3, 2], [[10, 10, 0], [9, 9, 9]], NTH, 0.8, True, 256, True)
    assert lv == [3 + 1000, 2 + 2000] and lh == [1, 1] and area == [0, 9]
    # a ratio of exactly iou_thr is kept (4 / 5 in float64 is the float64 0.8), just below is not
    lv, _, area = panoptic_decide_host([1, 1], [[4, 5, 4], [399, 500, 399]], NTH, 0.8, False, 256, True)
    assert lv == [1 + 1000, -1] and area == [4, 0]
    # areas of 0 fail before the division
    assert panoptic_decide_host([1, 1], [[0, 5, 0], [5, 0, 0]], NTH, 0.8, False, 256, True)[0] == [-1, -1]
    # `_emb` stuff: an unfiltered area of exactly the limit is kept, one pixel less is not; painted without the filter, after the
    # things, and it takes no instance id
    lv, lh, area = panoptic_decide_host([9, 10, 0], [[256, 256, 200], [255, 255, 255], [7, 7, 7]], NTH, 0.8, True, 256, True)
    assert lv == [9, -1, 1000] and lh == [0, 0, 1] and area == [256, 0, 7]
    # plain variant: stuff in query order, filtered like a thing, no area limit
    lv, lh, area = panoptic_decide_host([9, 10], [[256, 256, 200], [3, 3, 2]], NTH, 0.8, True, 256, False)
    assert lv == [9, 10] and lh == [1, 1] and area == [200, 2]


def test_segments_info_equals_unique_of_the_map():
    merged_somewhere = False
    for i, rescale, defer in ((0, False, True), (2, True, True), (0, True, False), (2, False, False)):
        c = oracle_case(i, rescale)
        lut_val, lut_half, area = panoptic_decide_host(c['classes'], c['counts'], NTH, IOU, True, LIMIT, defer)
        seg = paint(c, lut_val, lut_half)
        n = len(lut_val)
        table = np.full((96, 4), -1, dtype=np.int32)
        table[:n] = np.stack([lut_val, c['classes'], area, c['query']], 1)
        info = segments_info(table, n, NTH, scores=np.asarray(c['scores'] + [0.0] * (96 - n), dtype=np.float32))
        vals, cnts = np.unique(seg[seg != NCLS], return_counts=True)
        assert {d['id']: d['area'] for d in info} == dict(zip(vals.tolist(), cnts.tolist()))
        assert len({d['id'] for d in info}) == len(info)
        for d in info:
            assert d['isthing'] == (d['id'] >= 1000) and d['category_id'] == d['id'] % 1000 and d['score'] > THR
            assert c['classes'][c['query'].index(d['query'])] == d['category_id']
        painted = sum(1 for v, a in zip(lut_val, area) if v >= 0 and a > 0)
        merged_somewhere |= painted > len(info)
        things = [d['id'] // 1000 for d in info if d['isthing']]
        assert things == sorted(things)
    assert merged_somewhere, 'no two stuff queries of one class were merged into one row'


def test_c_abi_argument_checks_without_a_device():
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(logits=p, Q=100, ws_bytes=1 << 30):
        return lib.cgg_panoptic_fuse_batched(logits, p, p, p, p, p, p, p, p, ws_bytes, 2, Q, 40, 56, 160, 224, 160, 224, 2 * 160 * 224,
                                             12, 8, 0.8, 0.8, 1, 256, 1, null)
    assert call(logits=null) == -1                                        # CGG_EINVAL
    assert b'null' in lib.cgg_last_error_string()
    assert call(Q=0) == -1
    assert call(ws_bytes=16) == -1                                        # workspace too small
    assert call(Q=1025) == -2                                             # CGG_EUNSUPPORTED
    assert lib.cgg_panoptic_fuse_batched_workspace_bytes(2, 100, 2 * 800 * 1333) > 0
    assert lib.cgg_panoptic_fuse_batched_workspace_bytes(2, 100, 2 * 800 * 1333) >= 4 * 2 * 800 * 1333
    assert lib.cgg_panoptic_fuse_batched_workspace_bytes(0, 100, 10) == 0
