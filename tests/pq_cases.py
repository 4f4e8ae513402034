"""Shared inputs of the panoptic-quality tests: fixture G14 (made by tests/golden/make_golden_pq.py, which executes the reference's
pq_evaluation.py) and seeded generators of id maps, record lists and segment tables."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g14_pq_eval.npz')
SPLITS = (('All', 'all'), ('Known Things', 'kth'), ('Unknown Things', 'ukth'), ('Stuff', 'st'))
SPLIT_KEYS = ('pq', 'sq', 'rq', 'n', 'precision', 'recall')


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fixture_images():
    """per image dict(gt_map, gt [records], pred_map (void = 0), pred [records])"""
    z = fixture()
    out = []
    for i in range(int(z['n_imgs'])):
        g, p = z['gt_img'] == i, z['pred_img'] == i
        gt = [dict(id=int(a), category_id=int(b), iscrowd=int(c), area=int(d))
              for a, b, c, d in zip(z['gt_id'][g], z['gt_category_id'][g], z['gt_iscrowd'][g], z['gt_area'][g])]
        pred = [dict(id=int(a), category_id=int(b)) for a, b in zip(z['pred_id'][p], z['pred_category_id'][p])]
        out.append(dict(gt_map=z['gt_maps'][i].copy(), gt=gt, pred_map=z['pred_maps'][i].copy(), pred=pred))
    return out


def fixture_evaluator(device=None):
    from cgg_amd.pq_eval import PQEvaluator
    z = fixture()
    return PQEvaluator(z['all_cat_ids'], z['isthing'], z['unknown_cat_ids'], device=device)


def to_rgb(ids):
    ids = np.asarray(ids).astype(np.int64)
    return np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], axis=2).astype(np.uint8)


def assert_records_equal(a, b, where=''):
    """two image records of `pq_eval.pq_image_host`, field for field; the ious by their bit patterns"""
    assert set(a) == set(b), where
    for k in ('gt_id', 'gt_cat', 'gt_crowd', 'gt_match', 'pred_id', 'pred_cat', 'pred_area', 'pred_matched', 'pred_ignored'):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (where, k, a[k], b[k])
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype, (where, k)
    assert np.asarray(a['gt_iou'], np.float64).view(np.int64).tolist() == np.asarray(b['gt_iou'], np.float64).view(np.int64).tolist(), where
    assert list(a['extra']) == list(b['extra']), where


NUM_CLASSES = 7
CAT_IDS = [1, 2, 3, 5, 8, 9, 11]
ISTHING = [1, 1, 1, 1, 1, 0, 0]
UNKNOWN = [3, 5]


def random_case(seed, H, W, n_gt, n_pred, gt_ids=None, crowd_every=5):
    """Seeded image: a ground-truth map of n_gt segments (random rectangles painted over VOID, ids random below 2^24 or `gt_ids`, one
    id painted WITHOUT a record when n_gt > 2, every crowd_every-th record a crowd, one record without a pixel when n_gt > 3) and
    a RAW result map (label + instance * 1000, void = NUM_CLASSES) of n_pred segments that are shifted ground-truth rectangles and
    noise, things and stuff -> dict(pan_pred int32, pred [records as pan_result_segments_host finds them], pan_gt int32, gt)"""
    rs = np.random.RandomState(seed)
    gt_map = np.zeros((H, W), np.int32)
    ids = list(gt_ids) if gt_ids is not None else sorted({int(v) for v in rs.randint(1, 2 ** 24, size=4 * n_gt + 4)})
    ids = [int(i) for i in rs.permutation(ids)[:n_gt + 1]]
    rects = []
    for k in range(n_gt):
        r0, c0 = int(rs.randint(0, H)), int(rs.randint(0, W))
        r1, c1 = min(H, r0 + int(rs.randint(1, max(2, H // 2)))), min(W, c0 + int(rs.randint(1, max(2, W // 2))))
        rects.append((r0, r1, c0, c1))
        if not (n_gt > 3 and k == 1):                   # (record 1 owns no pixel)
            gt_map[r0:r1, c0:c1] = ids[k]
    if n_gt > 2 and len(ids) > n_gt:
        gt_map[H // 2:H // 2 + 2, W // 3:W // 3 + 3] = ids[n_gt]        # an id without a record
    labels = [int(rs.randint(0, NUM_CLASSES)) for _ in range(n_gt)]
    gt = [dict(id=ids[k], category_id=CAT_IDS[labels[k]], iscrowd=int(labels[k] < 5 and k % crowd_every == crowd_every - 1),
               area=int((gt_map == ids[k]).sum())) for k in range(n_gt)]
    pan = np.full((H, W), NUM_CLASSES, np.int32)
    inst = 0
    for k in range(n_pred):
        if k < n_gt and rs.rand() < 0.8:
            r0, r1, c0, c1 = rects[k]
            label = labels[k] if rs.rand() < 0.8 else int(rs.randint(0, NUM_CLASSES))
            r0, c0 = min(r0 + int(rs.randint(0, 2)), H - 1), min(c0 + int(rs.randint(0, 2)), W - 1)
        else:
            r0, c0 = int(rs.randint(0, H)), int(rs.randint(0, W))
            r1, c1 = min(H, r0 + int(rs.randint(1, max(2, H // 3)))), min(W, c0 + int(rs.randint(1, max(2, W // 3))))
            label = int(rs.randint(0, NUM_CLASSES))
        inst += 1
        pan[r0:max(r1, r0 + 1), c0:max(c1, c0 + 1)] = label + (inst * 1000 if ISTHING[label] else 0)
    from cgg_amd.pq_eval import pan_result_segments_host
    _, pred = pan_result_segments_host(pan, NUM_CLASSES, CAT_IDS, ISTHING)
    return dict(pan_pred=pan, pred=pred, pan_gt=gt_map, gt=gt)


def table_of(pan, Q, seed):
    """A segment table as the batched fusion leaves it, for the RAW map `pan`: (Q, 4) int32 rows [value, label, area, query] in a
    seeded order, n_kept of them valid. Stuff values are split over TWO rows whose areas add (they merge); among the valid rows are
    rows that painted nothing (area 0, and value -1); the rows past n_kept hold values of the map with positive areas, which must
    not count."""
    rs = np.random.RandomState(seed)
    rows = []
    for value in np.unique(pan):
        label = int(value) % 1000
        if label == NUM_CLASSES:
            continue
        area = int((pan == value).sum())
        if not ISTHING[label] and area > 1:
            rows += [[int(value), label, area - area // 2], [int(value), label, area // 2]]
        else:
            rows.append([int(value), label, area])
    rows += [[-1, 2, 0], [5 + 77000, 5 % NUM_CLASSES, 0], [-1, 0, 7]]
    rows = [rows[i] for i in rs.permutation(len(rows))]
    n_kept = len(rows)
    assert n_kept < Q, (n_kept, Q)
    table = np.zeros((Q, 4), np.int32)
    for k, r in enumerate(rows):
        table[k] = r + [k]
    for k in range(n_kept, Q):                          # garbage past n_kept
        v = rows[k % n_kept]
        table[k] = [max(v[0], 0) + 1000 * (k % 2), v[1], 9, k]
    return table, n_kept


def eval_stream(cfg, rank, world):
    """a `tools/test.py --data` stream: 5 prepared 64 x 64 images whose metas carry panoptic ground truth (the id map in its two
    forms in turn, and the records), and a sixth image without any"""
    import torch
    from cgg_amd import synthetic
    g = torch.Generator().manual_seed(5)
    meta = synthetic.img_metas(1, 64, 64)[0]
    for i in range(6):
        img = torch.randn(3, 64, 64, generator=g)
        extra = {}
        if i < 5:
            pan, segments = synthetic.pq_ground_truth((64, 64), 8, 2, seed=40 + i)
            extra = dict(gt_pan_seg=pan, gt_segments=segments)
        if i % world == rank:
            yield img, dict(meta, filename=f'pq_{i}.jpg', **extra)
