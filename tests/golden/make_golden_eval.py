#!/usr/bin/env python
"""Generate tests/golden/g13_segm_eval.npz by EXECUTING THE REFERENCE'S OWN open_set/utils/eval/cocoeval.py.

Runs only where the reference tree is at hand; the fixture (inputs + recorded outputs, no reference source) is committed and is
what travels. Usage:  python tests/golden/make_golden_eval.py REFERENCE_ROOT

cocoeval.py imports `pycocotools.mask` for one function, `iou(dt, gt, iscrowd)`, and pycocotools is not installed. THE IoU RULE
IS THEREFORE RESTATED HERE: `pycocotools.mask` is a stub module whose `iou` is this package's numpy rule
(`mask_eval.mask_intersections_host` + `mask_eval.mask_iou_host`: inter / union, inter / area_d for a crowd, 0 for an empty
denominator, [] when either list is empty, as pycocotools answers). EVERYTHING AFTER THE IoU MATRIX -- `_prepare`, `evaluate`,
`evaluateImg`, `accumulate` -- IS THE REFERENCE'S CODE, run on a minimal COCO-like object (getImgIds, getCatIds, getAnnIds,
loadAnns, annToRLE returning the bitmap). The file uses the removed alias `np.float`; this process sets `np.float = float`.

The dataset: 6 images of 37 x 45 (6 bytes per row, the last one partial; nothing a multiple of 32), categories 1, 2, 3, 5, 8 with
5 absent from the ground truth and 8 without detections, max_dets = (1, 3, 10):
  image 0   12 detections of category 1 (more than every max_dets entry), several with equal scores; a crowd ground truth
            overlapped by two detections; a ground truth of 1280 pixels (above 32^2) and small ones; detections of category 5
  image 1   two ground truths with equal IoU (0.8) to one detection; a pair with IoU exactly 0.5 (inter 1, union 2)
  image 2   detections, no ground truth          image 3   ground truth, no detection
  image 4, 5  seeded random boxes: detections are jittered ground truths plus noise, scores rounded to one decimal (ties);
            annotation areas that differ from the pixel count, one exactly 32^2, one crowd
Two runs are recorded: the normal one, and `class_agnostic` (every detection given category 1, as the reference's caller does).
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W = 37, 45
CAT_IDS = [1, 2, 3, 5, 8]
MAX_DETS = (1, 3, 10)


def _rect(r0, r1, c0, c1):
    m = np.zeros((H, W), bool)
    m[r0:r1, c0:c1] = True
    return m


def dataset():
    """-> list over images of dict(det_masks (D, H, W) bool, det_scores, det_cats, gt_masks, gt_cats, gt_crowd, gt_area)"""
    rs = np.random.RandomState(13)
    imgs = []

    def image(dets, gts):
        D, G = len(dets), len(gts)
        return dict(det_masks=np.array([d[0] for d in dets], bool).reshape(D, H, W),
                    det_scores=np.array([d[1] for d in dets], np.float32), det_cats=np.array([d[2] for d in dets], np.int64),
                    gt_masks=np.array([g[0] for g in gts], bool).reshape(G, H, W), gt_cats=np.array([g[1] for g in gts], np.int64),
                    gt_crowd=np.array([g[2] for g in gts], bool),
                    gt_area=np.array([float(g[0].sum()) if g[3] is None else g[3] for g in gts], np.float64))

    # image 0
    gts = [(_rect(2, 12, 3, 15), 1, False, None), (_rect(15, 35, 0, 30), 1, True, None), (_rect(0, 32, 5, 45), 2, False, None),
           (_rect(33, 37, 38, 45), 2, False, None), (_rect(13, 15, 0, 9), 1, False, None)]
    dets = [(_rect(2, 12, 4, 16), 0.9, 1), (_rect(16, 24, 2, 14), 0.8, 1), (_rect(22, 34, 10, 28), 0.8, 1),
            (_rect(0, 31, 6, 45), 0.7, 2), (_rect(33, 37, 37, 44), 0.7, 2), (_rect(1, 9, 1, 9), 0.6, 5), (_rect(20, 30, 20, 40), 0.4, 5)]
    for i in range(9):
        r0, c0 = rs.randint(0, H - 6), rs.randint(0, W - 6)
        dets.append((_rect(r0, r0 + rs.randint(2, 12), c0, c0 + rs.randint(2, 14)), [0.8, 0.5, 0.5, 0.3, 0.95, 0.5, 0.2, 0.1, 0.9][i], 1))
    dets.append((_rect(13, 15, 0, 8), 0.5, 1))
    imgs.append(image(dets, gts))
    # image 1
    one = np.zeros((H, W), bool)
    one[30, 40] = True
    two = one.copy()
    two[30, 41] = True
    gts = [(_rect(10, 14, 8, 18), 3, False, None), (_rect(10, 14, 10, 20), 3, False, None), (one, 3, False, None)]
    dets = [(_rect(10, 14, 10, 18), 0.9, 3), (_rect(10, 14, 8, 17), 0.6, 3), (two, 0.7, 3), (_rect(0, 5, 0, 5), 0.7, 1)]
    imgs.append(image(dets, gts))
    # image 2: no ground truth;  image 3: no detection
    imgs.append(image([(_rect(5, 20, 5, 20), 0.8, 1), (_rect(8, 30, 12, 40), 0.6, 2), (_rect(0, 4, 0, 45), 0.6, 2)], []))
    imgs.append(image([], [(_rect(3, 30, 3, 30), 8, False, None), (_rect(20, 36, 25, 44), 1, False, 1024.0),
                           (_rect(0, 6, 30, 45), 3, True, None)]))
    # images 4, 5
    for n_img in range(2):
        gts, dets = [], []
        for i in range(7):
            r0, c0 = rs.randint(0, H - 8), rs.randint(0, W - 8)
            h, w = rs.randint(3, H - r0 + 1), rs.randint(3, W - c0 + 1)
            m = _rect(r0, r0 + h, c0, c0 + w) & (rs.rand(H, W) < 0.95)
            cat = [1, 2, 3, 8, 1, 2, 1][i]
            area = [None, 1024.0, None, None, 1023.5, 1024.5, None][i] if n_img == 0 else None
            gts.append((m, cat, n_img == 1 and i == 4, area))
            for j in range(2 if cat != 8 else 0):
                dr, dc = rs.randint(-2, 3), rs.randint(-2, 3)
                d = np.roll(np.roll(m, dr, 0), dc, 1) & (rs.rand(H, W) < 0.9)
                dets.append((d, round(float(rs.rand()), 1), cat if rs.rand() < 0.8 else int(rs.choice([1, 2, 3, 5]))))
        for i in range(4):
            dets.append((rs.rand(H, W) < 0.1, round(float(rs.rand()), 1), int(rs.choice([1, 2, 3, 5]))))
        imgs.append(image(dets, gts))
    return imgs


class _Coco:
    """the few methods of pycocotools.coco.COCO that cocoeval.py calls, over a list of annotation dicts"""

    def __init__(self, anns, n_imgs):
        self.anns = anns
        self.n_imgs = n_imgs

    def getImgIds(self):
        return list(range(1, self.n_imgs + 1))

    def getCatIds(self):
        return list(CAT_IDS)

    def getAnnIds(self, imgIds=(), catIds=()):
        imgIds, catIds = set(imgIds), set(catIds)
        return [i for i, a in enumerate(self.anns)
                if (not imgIds or a['image_id'] in imgIds) and (not catIds or a['category_id'] in catIds)]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]

    def annToRLE(self, ann):
        return ann['segmentation']


def _iou_stub(dt, gt, iscrowd):
    from cgg_amd import mask_eval
    if len(dt) == 0 or len(gt) == 0:
        return []
    d = mask_eval.pack_bool_rows_host(np.array(dt, bool))
    g = mask_eval.pack_bool_rows_host(np.array(gt, bool))
    inter, area_d, area_g = mask_eval.mask_intersections_host(d, g, W)
    return mask_eval.mask_iou_host(inter, area_d, area_g, np.array(iscrowd, bool))


def load_reference_cocoeval(ref_root):
    pkg = types.ModuleType('pycocotools')
    mask = types.ModuleType('pycocotools.mask')
    mask.iou = _iou_stub
    pkg.mask = mask
    sys.modules['pycocotools'], sys.modules['pycocotools.mask'] = pkg, mask
    np.float = float            # the alias numpy removed; cocoeval.py:390 uses it
    path = os.path.join(ref_root, 'open_set', 'utils', 'eval', 'cocoeval.py')
    spec = importlib.util.spec_from_file_location('ref_cocoeval', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, imgs, class_agnostic):
    gt_anns, dt_anns = [], []
    for i, im in enumerate(imgs):
        for j in range(len(im['gt_cats'])):
            gt_anns.append(dict(id=j + 1, image_id=i + 1, category_id=int(im['gt_cats'][j]), segmentation=im['gt_masks'][j],
                                area=float(im['gt_area'][j]), iscrowd=int(im['gt_crowd'][j])))
        for j in range(len(im['det_cats'])):
            dt_anns.append(dict(id=j + 1, image_id=i + 1, category_id=1 if class_agnostic else int(im['det_cats'][j]),
                                segmentation=im['det_masks'][j], area=float(im['det_masks'][j].sum()),
                                score=float(im['det_scores'][j])))
    ev = ref.COCOeval(_Coco(gt_anns, len(imgs)), _Coco(dt_anns, len(imgs)), 'segm')
    ev.params.maxDets = list(MAX_DETS)
    ev.params.class_agnostic = class_agnostic
    ev.evaluate()
    ev.accumulate()
    K, A, I, T = len(CAT_IDS), len(ev.params.areaRng), len(imgs), len(ev.params.iouThrs)
    assert list(ev.params.catIds) == CAT_IDS and len(ev.evalImgs) == K * A * I
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
    imgs = dataset()
    out = dict(H=np.int64(H), W=np.int64(W), cat_ids=np.array(CAT_IDS, np.int64), max_dets=np.array(MAX_DETS, np.int64),
               unknown_cat_ids=np.array([3, 8], np.int64), all_cat_ids=np.array([1, 2, 3, 8], np.int64))
    for key in ('det_scores', 'det_cats', 'gt_cats', 'gt_crowd', 'gt_area'):
        out[key] = np.concatenate([im[key] for im in imgs])
    out['det_bits'] = np.concatenate([mask_eval.pack_bool_rows_host(im['det_masks']) for im in imgs])
    out['gt_bits'] = np.concatenate([mask_eval.pack_bool_rows_host(im['gt_masks']) for im in imgs])
    out['det_img'] = np.concatenate([np.full(len(im['det_cats']), i, np.int64) for i, im in enumerate(imgs)])
    out['gt_img'] = np.concatenate([np.full(len(im['gt_cats']), i, np.int64) for i, im in enumerate(imgs)])
    out['n_imgs'] = np.int64(len(imgs))
    for agn in (False, True):
        res, params = run(ref, imgs, agn)
        out.update(res)
    out['iou_thrs'] = np.asarray(params.iouThrs, np.float64)
    out['rec_thrs'] = np.asarray(params.recThrs, np.float64)
    out['area_rngs'] = np.asarray(params.areaRng, np.float64)
    # base / novel / all AP50 by the rule of coco_open.py:583-637 on the recorded precision (that file needs mmdet and a dataset to
    # run; its twelve lines of arithmetic are restated in mask_eval.open_set_ap_host)
    for tag in ('std_', 'agn_'):
        out[tag + 'open_set_ap50'] = np.array(mask_eval.open_set_ap_host(out[tag + 'precision'], CAT_IDS, [3, 8], [1, 2, 3, 8]))
    path = os.path.join(HERE, 'g13_segm_eval.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
