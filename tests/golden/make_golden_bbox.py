#!/usr/bin/env python
"""Generate tests/golden/g15_bbox_eval.npz by EXECUTING THE REFERENCE'S OWN open_set/utils/eval/cocoeval.py with iouType='bbox'.

Runs only where the reference tree is at hand; the fixture (inputs + recorded outputs, no reference source) is committed and is
what travels. Usage:  python tests/golden/make_golden_bbox.py REFERENCE_ROOT

The pattern is G13's (make_golden_eval.py, whose loader and minimal COCO-like object are imported): `pycocotools.mask` is a stub
module whose `iou(dt, gt, iscrowd)` is this package's numpy rule -- here `mask_eval.box_iou_host` on the lists of xywh boxes that
`computeIoU` hands over for iouType 'bbox', [] when either list is empty. EVERYTHING AFTER THE IoU MATRIX -- `_prepare`, `evaluate`,
`evaluateImg`, `accumulate` -- IS THE REFERENCE'S CODE. A detection annotation carries `bbox` = `mask_eval.det_boxes_xywh_host` of its
float32 (x0, y0, x1, y1, score) row (the reference's `xyxy2xywh`) and `area` = w * h, as `loadRes` sets them for box results.

The dataset: 6 images, categories 1, 2, 3, 5, 8 with 5 absent from the ground truth and 8 without detections, max_dets = (1, 3, 10).
Detection boxes are integer-valued, as the post-processing emits them; ground-truth boxes have two-decimal coordinates.
  image 0   13 detections of category 1 (more than every max_dets entry), several with equal scores; a crowd ground truth
            overlapped by two detections; the empty-mask box (0, 0, 0, 0); annotation areas of exactly 32^2 and 96^2 and half a
            pixel to either side of both; detections of category 5
  image 1   a pair that only touches (w == 0 exactly); a pair with IoU exactly 0.5 (i = 100, u = 200); two ground truths with
            equal IoU (360 / 440) to one detection
  image 2   detections, no ground truth          image 3   ground truth, no detection
  image 4, 5  seeded random boxes: detections are jittered ground truths rounded to integers plus noise, scores rounded to one
            decimal (ties); annotation areas below the box's w * h (a mask's), one crowd
Two runs are recorded: the normal one, and `class_agnostic` (every detection given category 1, as the reference's caller does).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for path in (ROOT, HERE):
    if path not in sys.path:
        sys.path.insert(0, path)

from make_golden_eval import CAT_IDS, MAX_DETS, _Coco, load_reference_cocoeval        # noqa: E402


def dataset():
    """-> list over images of dict(det_boxes5 (D, 5) float32, det_cats, gt_boxes (G, 4) float64 xywh, gt_cats, gt_crowd, gt_area)"""
    rs = np.random.RandomState(15)
    imgs = []

    def image(dets, gts):
        """dets: (x0, y0, x1, y1, score, category); gts: (x, y, w, h, category, crowd, area or None = w * h)"""
        gt_boxes = np.array([g[:4] for g in gts], np.float64).reshape(-1, 4)
        return dict(det_boxes5=np.array([d[:5] for d in dets], np.float32).reshape(-1, 5),
                    det_cats=np.array([d[5] for d in dets], np.int64),
                    gt_boxes=gt_boxes, gt_cats=np.array([g[4] for g in gts], np.int64), gt_crowd=np.array([g[5] for g in gts], bool),
                    gt_area=np.array([gt_boxes[i, 2] * gt_boxes[i, 3] if g[6] is None else g[6] for i, g in enumerate(gts)], np.float64))

    # image 0
    gts = [(10.25, 12.5, 40.75, 30.31, 1, False, None), (60.0, 60.0, 100.0, 80.0, 1, True, None),
           (5.5, 100.25, 32.0, 32.0, 2, False, 1024.0), (50.1, 150.2, 33.3, 31.7, 2, False, 1023.5),
           (100.0, 5.0, 40.0, 30.0, 1, False, 1024.5), (150.5, 20.25, 96.0, 96.0, 3, False, 9216.0),
           (10.0, 150.0, 97.5, 95.25, 1, False, 9215.5), (120.0, 150.0, 99.99, 93.01, 3, False, 9216.5)]
    dets = [(10, 13, 51, 43, 0.9, 1), (62, 64, 110, 100, 0.8, 1), (100, 90, 158, 138, 0.8, 1), (0, 0, 0, 0, 0.85, 1),
            (5, 100, 38, 132, 0.7, 2), (50, 150, 84, 182, 0.7, 2), (101, 6, 139, 34, 0.6, 1), (150, 20, 246, 117, 0.9, 3),
            (12, 151, 108, 244, 0.75, 1), (121, 149, 219, 242, 0.5, 3), (1, 1, 9, 9, 0.6, 5), (20, 20, 40, 40, 0.4, 5)]
    for i in range(7):
        x0, y0 = int(rs.randint(0, 180)), int(rs.randint(0, 180))
        dets.append((x0, y0, x0 + int(rs.randint(5, 60)), y0 + int(rs.randint(5, 60)), [0.8, 0.5, 0.5, 0.3, 0.95, 0.5, 0.2][i], 1))
    imgs.append(image(dets, gts))
    # image 1
    gts = [(30.0, 20.0, 10.0, 10.0, 3, False, None), (0.0, 0.0, 10.0, 20.0, 3, False, None), (48.0, 50.0, 20.0, 20.0, 3, False, None),
           (52.0, 50.0, 20.0, 20.0, 3, False, None)]
    dets = [(20, 20, 30, 30, 0.9, 3), (0, 0, 10, 10, 0.6, 3), (50, 50, 70, 70, 0.7, 3), (100, 100, 120, 130, 0.7, 1)]
    imgs.append(image(dets, gts))
    # image 2: no ground truth;  image 3: no detection
    imgs.append(image([(5, 5, 20, 20, 0.8, 1), (8, 12, 30, 40, 0.6, 2), (0, 0, 45, 4, 0.6, 2)], []))
    imgs.append(image([], [(3.25, 3.75, 27.5, 27.0, 8, False, None), (25.5, 20.1, 19.33, 16.67, 1, False, 1024.0),
                           (30.0, 0.0, 15.0, 6.0, 3, True, None)]))
    # images 4, 5
    for n_img in range(2):
        gts, dets = [], []
        for i in range(7):
            x, y = round(float(rs.uniform(0, 150)), 2), round(float(rs.uniform(0, 150)), 2)
            w, h = round(float(rs.uniform(8, 120)), 2), round(float(rs.uniform(8, 120)), 2)
            cat = [1, 2, 3, 8, 1, 2, 1][i]
            gts.append((x, y, w, h, cat, n_img == 1 and i == 4, round(w * h * float(rs.uniform(0.5, 0.9)), 1) if i % 2 else None))
            for j in range(2 if cat != 8 else 0):
                dx, dy, dw, dh = (int(v) for v in rs.randint(-4, 5, size=4))
                x0, y0 = max(0, int(round(x)) + dx), max(0, int(round(y)) + dy)
                dets.append((x0, y0, x0 + max(1, int(round(w)) + dw), y0 + max(1, int(round(h)) + dh), round(float(rs.rand()), 1),
                             cat if rs.rand() < 0.8 else int(rs.choice([1, 2, 3, 5]))))
        for i in range(4):
            x0, y0 = int(rs.randint(0, 150)), int(rs.randint(0, 150))
            dets.append((x0, y0, x0 + int(rs.randint(1, 90)), y0 + int(rs.randint(1, 90)), round(float(rs.rand()), 1),
                         int(rs.choice([1, 2, 3, 5]))))
        imgs.append(image(dets, gts))
    return imgs


def _iou_stub(dt, gt, iscrowd):
    from cgg_amd import mask_eval
    if len(dt) == 0 or len(gt) == 0:
        return []
    return mask_eval.box_iou_host(np.array(dt, np.float64), np.array(gt, np.float64), np.array(iscrowd, bool))


def run(ref, imgs, class_agnostic):
    from cgg_amd import mask_eval
    gt_anns, dt_anns = [], []
    for i, im in enumerate(imgs):
        for j in range(len(im['gt_cats'])):
            gt_anns.append(dict(id=j + 1, image_id=i + 1, category_id=int(im['gt_cats'][j]), bbox=im['gt_boxes'][j].tolist(),
                                area=float(im['gt_area'][j]), iscrowd=int(im['gt_crowd'][j])))
        xywh = mask_eval.det_boxes_xywh_host(im['det_boxes5'])
        for j in range(len(im['det_cats'])):
            bbox = xywh[j].tolist()
            dt_anns.append(dict(id=j + 1, image_id=i + 1, category_id=1 if class_agnostic else int(im['det_cats'][j]), bbox=bbox,
                                area=bbox[2] * bbox[3], score=float(im['det_boxes5'][j, 4])))
    ev = ref.COCOeval(_Coco(gt_anns, len(imgs)), _Coco(dt_anns, len(imgs)), 'bbox')
    ev.params.maxDets = list(MAX_DETS)
    ev.params.class_agnostic = class_agnostic
    ev.evaluate()
    ev.accumulate()
    K, A, I, T = len(CAT_IDS), len(ev.params.areaRng), len(imgs), len(ev.params.iouThrs)
    assert ev.params.iouType == 'bbox' and list(ev.params.catIds) == CAT_IDS and len(ev.evalImgs) == K * A * I
    present = np.zeros((K, A, I), bool)
    nd, ng = np.zeros((K, A, I), np.int64), np.zeros((K, A, I), np.int64)
    flat = dict(dt_match=[], dt_ignore=[], gt_ignore=[], dt_scores=[], dt_ids=[], gt_ids=[])
    for k in range(K):
        for a in range(A):
            for i in range(I):
                e = ev.evalImgs[(k * A + a) * I + i]
                if e is None:
                    continue
                present[k, a, i] = True
                nd[k, a, i], ng[k, a, i] = len(e['dtIds']), len(e['gtIds'])
                assert e['dtMatches'].shape == (T, nd[k, a, i]) and e['maxDet'] == MAX_DETS[-1]
                flat['dt_match'].append(np.asarray(e['dtMatches']).astype(np.int32).ravel())
                flat['dt_ignore'].append(np.asarray(e['dtIgnore']).astype(bool).reshape(T, -1).ravel())
                flat['gt_ignore'].append(np.asarray(e['gtIgnore']).astype(bool).ravel())
                flat['dt_scores'].append(np.asarray(e['dtScores'], np.float64).ravel())
                flat['dt_ids'].append(np.asarray(e['dtIds'], np.int64).ravel())
                flat['gt_ids'].append(np.asarray(e['gtIds'], np.int64).ravel())
    tag = 'agn_' if class_agnostic else 'std_'
    out = {tag + 'present': present, tag + 'nd': nd, tag + 'ng': ng}
    dtypes = dict(dt_match=np.int32, dt_ignore=bool, gt_ignore=bool, dt_scores=np.float64, dt_ids=np.int64, gt_ids=np.int64)
    for name, parts in flat.items():
        out[tag + name] = np.concatenate(parts) if parts else np.zeros(0, dtypes[name])
    for name in ('precision', 'recall', 'scores'):
        out[tag + name] = np.asarray(ev.eval[name], np.float64)
    return out, ev.params


def main(ref_root):
    from cgg_amd import mask_eval
    ref = load_reference_cocoeval(ref_root)
    sys.modules['pycocotools.mask'].iou = _iou_stub        # (the loader installed G13's mask stub)
    imgs = dataset()
    out = dict(cat_ids=np.array(CAT_IDS, np.int64), max_dets=np.array(MAX_DETS, np.int64), unknown_cat_ids=np.array([3, 8], np.int64),
               all_cat_ids=np.array([1, 2, 3, 8], np.int64), n_imgs=np.int64(len(imgs)))
    for key in ('det_boxes5', 'det_cats', 'gt_boxes', 'gt_cats', 'gt_crowd', 'gt_area'):
        out[key] = np.concatenate([im[key] for im in imgs])
    out['det_img'] = np.concatenate([np.full(len(im['det_cats']), i, np.int64) for i, im in enumerate(imgs)])
    out['gt_img'] = np.concatenate([np.full(len(im['gt_cats']), i, np.int64) for i, im in enumerate(imgs)])
    for agn in (False, True):
        res, params = run(ref, imgs, agn)
        out.update(res)
    out['iou_thrs'] = np.asarray(params.iouThrs, np.float64)
    out['rec_thrs'] = np.asarray(params.recThrs, np.float64)
    out['area_rngs'] = np.asarray(params.areaRng, np.float64)
    # base / novel / all AP50 by the rule of coco_open.py:583-637 on the recorded precision, as in G13
    for tag in ('std_', 'agn_'):
        out[tag + 'open_set_ap50'] = np.array(mask_eval.open_set_ap_host(out[tag + 'precision'], CAT_IDS, [3, 8], [1, 2, 3, 8]))
    path = os.path.join(HERE, 'g15_bbox_eval.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
