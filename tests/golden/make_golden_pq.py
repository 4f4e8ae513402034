#!/usr/bin/env python
"""Generate tests/golden/g14_pq_eval.npz by EXECUTING THE REFERENCE'S OWN open_set/utils/eval/pq_evaluation.py.

Runs only where the reference tree is at hand; the fixture (inputs + recorded outputs, no reference source) is committed and is
what travels. Usage:  python tests/golden/make_golden_pq.py REFERENCE_ROOT

pq_evaluation.py imports `panopticapi.utils` for `get_traceback` and `rgb2id`, and panopticapi is not installed. BOTH ARE STUBBED
HERE: `get_traceback` is the identity decorator, and `rgb2id` IS RESTATED as R + 256 G + 65536 B on an integer array. EVERYTHING ELSE
IS THE REFERENCE'S CODE: `pq_compute_single_core` is called directly on the whole list of images (ONE core: the reference's
`pq_compute_multi_core` splits the list over `multiprocessing.cpu_count()` processes, which changes the order of its float sums),
then `PQStat.pq_average` for the four splits of `evaluate_pan_json`. The id maps reach it as RGB PNGs written with PIL into a
temporary directory. The pred records are given as `_pan2json` would write them (id, category_id, isthing, area); that method
needs the dataset class and is not executed.

The dataset: 6 images of 37 x 45, labels -> category ids 1, 2, 3, 5, 8, 9, 11 (9 and 11 stuff, 3 and 5 unknown), ids up to 2^24 - 1:
  image 0   a match between ground truth 2^24 - 1 and a pred; a pair with IoU exactly 0.5 (inter 1, union 2, the pred's other pixel on a stuff segment: not a match); a match
            that exists only because the pred's pixels on VOID are subtracted from the union; a stuff match
  image 1   two crowds of category 1, of which the last in record order counts: a pred inside the first is a false positive, a
            pred inside the second is ignored; an unmatched pred whose void + crowd share is exactly 0.5 (false positive) and one
            with 19 of 37 pixels (ignored); a ground-truth id in the map without a record, under a pred
  image 2   a pred of category 5, which no ground truth has; a ground truth of category 8, which no pred has; a match of the
            unknown category 3; a stuff match
  image 3   the pred is all void          image 4   no ground-truth segment
  image 5   seeded blocks: ground truth of random ids, preds that are shifted copies, some with another category, one crowd
Category 11 appears nowhere: tp + fp + fn = 0, it is left out of every n.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

H, W = 37, 45
ALL_CAT_IDS = [1, 2, 3, 5, 8, 9, 11]
ISTHING = [1, 1, 1, 1, 1, 0, 0]
UNKNOWN_CAT_IDS = [3, 5]
TOP = 2 ** 24 - 1


def _paint(segs):
    """[(id, category, crowd, area or None, [(r0, r1, c0, c1) | (r, c)])] painted in order -> the (H, W) int32 id map"""
    m = np.zeros((H, W), np.int32)
    for sid, _, _, _, shapes in segs:
        for s in shapes:
            if len(s) == 4:
                m[s[0]:s[1], s[2]:s[3]] = sid
            else:
                m[s[0], s[1]] = sid
    return m


def dataset():
    """-> list over images of dict(gt_map, gt (id, category_id, iscrowd, area), pred_map, pred (id, category_id))"""
    rs = np.random.RandomState(14)
    imgs = []

    def image(gt_segs, pred_segs, gt_extra=()):
        gt_map, pred_map = _paint(list(gt_segs) + list(gt_extra)), _paint(pred_segs)
        gt = [dict(id=s[0], category_id=s[1], iscrowd=int(bool(s[2])), area=int((gt_map == s[0]).sum()) if s[3] is None else s[3])
              for s in gt_segs]
        pred = [dict(id=s[0], category_id=s[1]) for s in pred_segs]
        return dict(gt_map=gt_map, gt=gt, pred_map=pred_map, pred=pred)

    # image 0
    imgs.append(image(
        [(40, 9, 0, None, [(26, 37, 0, 30)]), (TOP, 1, 0, None, [(2, 12, 3, 15)]), (7, 2, 0, None, [(30, 20)]),
         (300, 3, 0, None, [(15, 25, 0, 10)])],
        [(5001, 1, 0, None, [(2, 12, 4, 16)]), (41, 9, 0, None, [(27, 37, 0, 30)]), (9, 2, 0, None, [(30, 20), (30, 21)]),
         (301, 3, 0, None, [(15, 25, 0, 22)])]))
    # image 1
    imgs.append(image(
        [(50, 1, 1, None, [(0, 10, 0, 20)]), (52, 2, 0, None, [(10, 20, 25, 45)]), (51, 1, 1, None, [(20, 30, 0, 20)])],
        [(60, 1, 0, None, [(0, 10, 0, 10)]), (61, 1, 0, None, [(20, 30, 0, 10)]), (62, 1, 0, None, [(18, 22, 25, 35)]),
         (63, 1, 0, None, [(18, 22, 36, 45), (22, 36)]), (64, 2, 0, None, [(31, 36, 30, 40)])],
        gt_extra=[(999, 0, 0, None, [(31, 36, 30, 40)])]))
    # image 2
    imgs.append(image(
        [(70, 8, 0, None, [(0, 8, 0, 8)]), (71, 9, 0, None, [(20, 37, 0, 45)]), (72, 3, 0, None, [(10, 18, 20, 32)])],
        [(80, 5, 0, None, [(0, 6, 30, 40)]), (81, 9, 0, None, [(22, 37, 0, 45)]), (82, 3, 0, None, [(10, 18, 21, 33)])]))
    # image 3: the pred is all void;  image 4: no ground-truth segment
    imgs.append(image([(10, 1, 0, None, [(3, 20, 3, 20)]), (11, 9, 0, None, [(25, 37, 0, 45)])], []))
    imgs.append(image([], [(90, 1, 0, None, [(5, 15, 5, 15)]), (91, 9, 0, None, [(20, 37, 0, 45)])]))
    # image 5: blocks of 9 x 9 (the last row and column of blocks are cut by the border)
    gt_segs, pred_segs = [], []
    for i, (br, bc) in enumerate([(r, c) for r in range(0, H, 9) for c in range(0, W, 9)]):
        if rs.rand() < 0.15:
            continue
        label = int(rs.randint(0, 6))
        gid = int(rs.randint(1, TOP)) if i else TOP
        gt_segs.append((gid, ALL_CAT_IDS[label], i == 7, None, [(br, br + 9, bc, bc + 9)]))
        if rs.rand() < 0.85:
            dr, dc = int(rs.randint(0, 4)), int(rs.randint(0, 4))
            cat = ALL_CAT_IDS[label] if rs.rand() < 0.8 else ALL_CAT_IDS[int(rs.randint(0, 6))]
            pred_segs.append((int(rs.randint(1, TOP)), cat, 0, None, [(min(br + dr, H - 1), br + 9, min(bc + dc, W - 1), bc + 9)]))
    imgs.append(image(gt_segs, pred_segs))
    return imgs


def load_reference_pq(ref_root):
    pkg = types.ModuleType('panopticapi')
    utils = types.ModuleType('panopticapi.utils')
    utils.get_traceback = lambda f: f

    def rgb2id(color):
        color = np.asarray(color)
        c = color.astype(np.int64) if color.dtype == np.uint8 else color
        return c[..., 0] + 256 * c[..., 1] + 256 * 256 * c[..., 2]

    utils.rgb2id = rgb2id
    pkg.utils = utils
    sys.modules['panopticapi'], sys.modules['panopticapi.utils'] = pkg, utils
    path = os.path.join(ref_root, 'open_set', 'utils', 'eval', 'pq_evaluation.py')
    spec = importlib.util.spec_from_file_location('ref_pq_evaluation', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_png(path, ids):
    from PIL import Image
    rgb = np.stack([ids % 256, (ids // 256) % 256, (ids // 65536) % 256], axis=2).astype(np.uint8)
    Image.fromarray(rgb).save(path)


def main(ref_root):
    ref = load_reference_pq(ref_root)
    imgs = dataset()
    annotation_set = []
    with tempfile.TemporaryDirectory() as tmp:
        gt_folder, pred_folder = os.path.join(tmp, 'gt'), os.path.join(tmp, 'pred')
        os.makedirs(gt_folder)
        os.makedirs(pred_folder)
        for i, im in enumerate(imgs):
            name = f'{i:06d}.png'
            _write_png(os.path.join(gt_folder, name), im['gt_map'])
            _write_png(os.path.join(pred_folder, name), im['pred_map'])
            label_of = {c: k for k, c in enumerate(ALL_CAT_IDS)}
            pred = [dict(id=p['id'], category_id=p['category_id'], isthing=ISTHING[label_of[p['category_id']]],
                         area=int((im['pred_map'] == p['id']).sum())) for p in im['pred']]
            annotation_set.append((dict(image_id=i, segments_info=[dict(g) for g in im['gt']], file_name=name),
                                   dict(image_id=i, segments_info=pred, file_name=name)))
        pq_stat = ref.pq_compute_single_core(0, annotation_set, gt_folder, pred_folder)
    categories = {c: dict(id=c, isthing=t) for c, t in zip(ALL_CAT_IDS, ISTHING)}
    cats = sorted(pq_stat.pq_per_cat)
    out = dict(H=np.int64(H), W=np.int64(W), n_imgs=np.int64(len(imgs)), all_cat_ids=np.array(ALL_CAT_IDS, np.int64),
               isthing=np.array(ISTHING, np.int64), unknown_cat_ids=np.array(UNKNOWN_CAT_IDS, np.int64),
               gt_maps=np.stack([im['gt_map'] for im in imgs]).astype(np.int32),
               pred_maps=np.stack([im['pred_map'] for im in imgs]).astype(np.int32),
               stat_cats=np.array(cats, np.int64), stat_tp=np.array([pq_stat[c].tp for c in cats], np.int64),
               stat_fp=np.array([pq_stat[c].fp for c in cats], np.int64), stat_fn=np.array([pq_stat[c].fn for c in cats], np.int64),
               stat_iou=np.array([pq_stat[c].iou for c in cats], np.float64))
    for side, keys in (('gt', ('id', 'category_id', 'iscrowd', 'area')), ('pred', ('id', 'category_id'))):
        out[side + '_img'] = np.array([i for i, im in enumerate(imgs) for _ in im[side]], np.int64)
        for k in keys:
            out[f'{side}_{k}'] = np.array([s[k] for im in imgs for s in im[side]], np.int64)
    keys = ('pq', 'sq', 'rq', 'n', 'precision', 'recall')
    for tag, isthing, isunknown in (('all', None, None), ('kth', True, False), ('ukth', True, True), ('st', False, None)):
        res, classwise = pq_stat.pq_average(categories, isthing=isthing, isunknown=isunknown, unknown_cat_ids=UNKNOWN_CAT_IDS)
        out['split_' + tag] = np.array([res[k] for k in keys], np.float64)
        if tag == 'all':
            out['classwise'] = np.array([[classwise[c][k] for k in ('pq', 'sq', 'rq', 'precision', 'recall')] for c in ALL_CAT_IDS],
                                        np.float64)
    path = os.path.join(HERE, 'g14_pq_eval.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')
    for c in cats:
        print(c, pq_stat[c])


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
