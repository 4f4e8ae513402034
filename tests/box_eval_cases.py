"""Shared by test_box_eval.py and test_box_eval_gpu.py: the fixture g15_bbox_eval.npz (made by tests/golden/make_golden_bbox.py from the
reference's own cocoeval.py with iouType 'bbox') split into images and recorded per-image results; the seeded case set of box
pairs with its exact-rational evaluation; seeded images for the matcher; a `tools/test.py --data` stream with box ground truth."""
import functools
import os
from fractions import Fraction

import numpy as np

from cgg_amd import mask_eval

from mask_eval_cases import MODES, assert_records_equal        # noqa: F401  (the same modes and the same comparison)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g15_bbox_eval.npz')


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def fixture_images():
    """list of dict(det_boxes5, det_scores, det_cats, gt_boxes, gt_cats, gt_crowd, gt_area), one per image"""
    z = fixture()
    out = []
    for i in range(int(z['n_imgs'])):
        d, g = z['det_img'] == i, z['gt_img'] == i
        out.append(dict(det_boxes5=z['det_boxes5'][d], det_scores=z['det_boxes5'][d][:, 4], det_cats=z['det_cats'][d],
                        gt_boxes=z['gt_boxes'][g], gt_cats=z['gt_cats'][g], gt_crowd=z['gt_crowd'][g], gt_area=z['gt_area'][g]))
    return out


def fixture_records(tag):
    """the recorded evalImgs of one run as records[i][k][a] = None | dict(dt_match (T, D_k), dt_ignore, gt_ignore, dt_scores, dt_ids,
    gt_ids), the layout `evaluate_img_host` returns"""
    z = fixture()
    present, nd, ng = z[tag + 'present'], z[tag + 'nd'], z[tag + 'ng']
    K, A, I = present.shape
    T = len(z['iou_thrs'])
    recs = [[[None] * A for _ in range(K)] for _ in range(I)]
    pd = pg = 0
    for k in range(K):
        for a in range(A):
            for i in range(I):
                if not present[k, a, i]:
                    continue
                d, g = int(nd[k, a, i]), int(ng[k, a, i])
                recs[i][k][a] = dict(dt_match=z[tag + 'dt_match'][pd * T:(pd + d) * T].reshape(T, d),
                                     dt_ignore=z[tag + 'dt_ignore'][pd * T:(pd + d) * T].reshape(T, d),
                                     gt_ignore=z[tag + 'gt_ignore'][pg:pg + g], dt_scores=z[tag + 'dt_scores'][pd:pd + d],
                                     dt_ids=z[tag + 'dt_ids'][pd:pd + d], gt_ids=z[tag + 'gt_ids'][pg:pg + g])
                pd, pg = pd + d, pg + g
    assert pd == len(z[tag + 'dt_scores']) and pg == len(z[tag + 'gt_ignore'])
    return recs


def host_records(im, class_agnostic, cat_ids, area_rngs, iou_thrs, max_det):
    """the host rule on one image dict -> (records [K][A], iou (D, G), det_xywh (D, 4), area_d (D,))"""
    det = mask_eval.det_boxes_xywh_host(im['det_boxes5'])
    iou = mask_eval.box_iou_host(det, im['gt_boxes'], im['gt_crowd'])
    area_d = det[:, 2] * det[:, 3]
    rec = mask_eval.evaluate_img_host(iou, im['det_boxes5'][:, 4], im['det_cats'], im['gt_cats'], im['gt_crowd'], im['gt_area'], area_d,
                                      cat_ids, area_rngs, iou_thrs, max_det, class_agnostic)
    return rec, iou, det, area_d


# ---- the case set of the IoU arithmetic --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_boxes():
    """(det_boxes5 (30, 5) float32, gt_xywh (14, 4) float64, gt_crowd (14,) bool): seeded boxes of the kind the evaluation meets --
    ground truths with two-decimal coordinates, detections that are jittered ground truths rounded to integers (so that most pairs
    of a detection and its ground truth overlap, and many others do) -- with the fixture's special pairs in front: one that only
    touches, one with IoU exactly 0.5, the empty box, and two crowds."""
    rs = np.random.RandomState(105)
    gts = [(30.0, 20.0, 10.0, 10.0), (0.0, 0.0, 10.0, 20.0)]
    dets = [(20, 20, 30, 30), (0, 0, 10, 10), (0, 0, 0, 0)]
    while len(gts) < 14:
        gts.append(tuple(round(float(v), 2) for v in (rs.uniform(0, 60), rs.uniform(0, 60), rs.uniform(20, 140), rs.uniform(20, 140))))
    while len(dets) < 30:
        x, y, w, h = gts[2 + len(dets) % 12]
        dx, dy, dw, dh = (int(v) for v in rs.randint(-6, 7, size=4))
        x0, y0 = max(0, int(round(x)) + dx), max(0, int(round(y)) + dy)
        dets.append((x0, y0, x0 + max(1, int(round(w)) + dw), y0 + max(1, int(round(h)) + dh)))
    det5 = np.zeros((30, 5), np.float32)
    det5[:, :4] = np.array(dets, np.float32)
    det5[:, 4] = np.round(rs.rand(30), 2)
    crowd = np.zeros(14, bool)
    crowd[[5, 11]] = True
    return det5, np.array(gts, np.float64), crowd


def _rn(x):
    """a Fraction rounded once to the nearest double (Python's integer true division is correctly rounded)"""
    return x.numerator / x.denominator


def box_iou_exact(d, g, crowd, fused=False):
    """`bbIou` of one pair of xywh boxes (doubles) on exact rationals, rounded once per operation of the rule. fused=True: the
    variant a contracting compiler makes of it, u = fma(-w, h, da + ga) -- the product w * h unrounded inside the subtraction."""
    F = Fraction
    dx, dy, dw, dh = (F(float(v)) for v in d)
    gx, gy, gw, gh = (F(float(v)) for v in g)
    da, ga = _rn(dw * dh), _rn(gw * gh)
    w = _rn(F(min(_rn(dw + dx), _rn(gw + gx))) - max(dx, gx))
    if w <= 0:
        return 0.0
    h = _rn(F(min(_rn(dh + dy), _rn(gh + gy))) - max(dy, gy))
    if h <= 0:
        return 0.0
    i = _rn(F(w) * F(h))
    if crowd:
        u = da
    elif fused:
        u = _rn(F(_rn(F(da) + F(ga))) - F(w) * F(h))
    else:
        u = _rn(F(_rn(F(da) + F(ga))) - F(i))
    return _rn(F(i) / F(u))


@functools.lru_cache(maxsize=None)
def case_iou_exact():
    """-> (iou (30, 14) by the rule on rationals, the same with the fused union) of `case_boxes`"""
    det5, gt, crowd = case_boxes()
    det = mask_eval.det_boxes_xywh_host(det5)
    rule = np.array([[box_iou_exact(d, g, c) for g, c in zip(gt, crowd)] for d in det])
    fused = np.array([[box_iou_exact(d, g, c, fused=True) for g, c in zip(gt, crowd)] for d in det])
    return rule, fused


# ---- images for the matcher ----------------------------------------------------------------------------------------------------------
def random_image(seed, D=100, G=40, K=12, size=300):
    """a seeded image whose detections are jittered copies of its ground truths (so that matches happen at every threshold), with
    ties in the scores, crowds, and annotation areas on both sides of the bounds; categories 1..K"""
    rs = np.random.RandomState(seed)
    gt = np.stack([np.round(rs.uniform(0, size * 0.6, G), 2), np.round(rs.uniform(0, size * 0.6, G), 2),
                   np.round(rs.uniform(4, size * 0.4, G), 2), np.round(rs.uniform(4, size * 0.4, G), 2)], axis=1)
    gt_cats = rs.randint(1, K + 1, size=G)
    det5 = np.zeros((D, 5), np.float32)
    det_cats = np.zeros(D, np.int64)
    for d in range(D):
        if G == 0:                                         # no ground truth: any box, category 1
            det5[d, :4], det_cats[d] = (d, d, d + 10, d + 20), 1
            continue
        g = rs.randint(0, G)
        x, y, w, h = gt[g]
        x0, y0 = max(0, int(round(x)) + rs.randint(-3, 4)), max(0, int(round(y)) + rs.randint(-3, 4))
        det5[d, :4] = (x0, y0, x0 + max(1, int(round(w)) + rs.randint(-3, 4)), y0 + max(1, int(round(h)) + rs.randint(-3, 4)))
        det_cats[d] = gt_cats[g] if rs.rand() < 0.85 else rs.randint(1, K + 1)
    det5[:, 4] = np.round(rs.rand(D), 1)
    area = gt[:, 2] * gt[:, 3]
    area[::5] = rs.choice([1023.0, 1024.0, 1025.0, 9216.0, 9217.0, 200.0], size=len(area[::5]))
    return dict(det_boxes5=det5, det_scores=det5[:, 4], det_cats=det_cats, gt_boxes=gt, gt_cats=gt_cats.astype(np.int64),
                gt_crowd=rs.rand(G) < 0.15, gt_area=area)


def eval_stream(cfg, rank, world):
    """a `tools/test.py --data` stream: 5 prepared 64 x 64 images whose metas carry mask AND box ground truth (rectangles of
    categories 1..4, one crowd, one with its own area; the boxes are the rectangles' with two-decimal offsets), and a sixth image
    without any"""
    import torch
    from cgg_amd import synthetic
    g = torch.Generator().manual_seed(5)
    rs = np.random.RandomState(3)
    meta = synthetic.img_metas(1, 64, 64)[0]
    for i in range(6):
        img = torch.randn(3, 64, 64, generator=g)
        gt = np.zeros((4, 64, 64), bool)
        boxes = np.zeros((4, 4), np.float64)
        for m, b in zip(gt, boxes):
            r0, c0 = rs.randint(0, 40), rs.randint(0, 40)
            h, w = rs.randint(8, 40), rs.randint(8, 40)
            m[r0:r0 + h, c0:c0 + w] = True
            b[:] = (c0 + 0.25, r0 + 0.5, min(w, 64 - c0) - 0.25, min(h, 64 - r0) - 0.75)
        extra = dict(gt_masks=gt, gt_boxes_xywh=boxes, gt_labels=np.array([1, 2, 3, 4]), gt_crowd=np.array([False, False, True, False]),
                     gt_area=np.array([gt[0].sum(), 1500.0, gt[2].sum(), gt[3].sum()], np.float64)) if i < 5 else {}
        if i % world == rank:
            yield img, dict(meta, filename=f'eval_{i}.jpg', **extra)
