"""Shared by test_mask_eval.py and test_mask_eval_gpu.py: the fixture g13_segm_eval.npz (made by tests/golden/make_golden_eval.py from
the reference's own cocoeval.py) split into images and recorded per-image results, a seeded random image, and the comparison of
two record lists."""
import functools
import os

import numpy as np

from cgg_amd import mask_eval

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g13_segm_eval.npz')
MODES = (('std_', False), ('agn_', True))


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def fixture_images():
    """list of dict(det_bits, det_scores, det_cats, gt_bits, gt_cats, gt_crowd, gt_area), one per image"""
    z = fixture()
    out = []
    for i in range(int(z['n_imgs'])):
        d, g = z['det_img'] == i, z['gt_img'] == i
        out.append(dict(det_bits=z['det_bits'][d], det_scores=z['det_scores'][d], det_cats=z['det_cats'][d], gt_bits=z['gt_bits'][g],
                        gt_cats=z['gt_cats'][g], gt_crowd=z['gt_crowd'][g], gt_area=z['gt_area'][g]))
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


def host_records(im, width, class_agnostic, cat_ids, area_rngs, iou_thrs, max_det):
    """the host rule on one image dict -> (records [K][A], iou, inter, area_d, area_g)"""
    inter, area_d, area_g = mask_eval.mask_intersections_host(im['det_bits'], im['gt_bits'], width)
    iou = mask_eval.mask_iou_host(inter, area_d, area_g, im['gt_crowd'])
    rec = mask_eval.evaluate_img_host(iou, im['det_scores'], im['det_cats'], im['gt_cats'], im['gt_crowd'], im['gt_area'], area_d,
                                      cat_ids, area_rngs, iou_thrs, max_det, class_agnostic)
    return rec, iou, inter, area_d, area_g


def assert_records_equal(got, want, where=''):
    """two [K][A] record lists: None in the same places, every array equal in dtype-independent value and in shape"""
    assert len(got) == len(want), where
    for k, (gk, wk) in enumerate(zip(got, want)):
        assert len(gk) == len(wk), (where, k)
        for a, (g, w) in enumerate(zip(gk, wk)):
            assert (g is None) == (w is None), (where, k, a)
            if g is None:
                continue
            for name in ('dt_match', 'dt_ignore', 'gt_ignore', 'dt_scores'):
                x, y = np.asarray(g[name]), np.asarray(w[name])
                assert x.shape == y.shape, (where, k, a, name, x.shape, y.shape)
                assert np.array_equal(x, y), (where, k, a, name)


def random_image(seed, D=100, G=40, K=12, H=48, W=77):
    """a seeded image whose detections are noisy copies of its ground truths (so that matches happen at every threshold), with ties
    in the scores, crowds, and areas on both sides of the bounds; categories 1..K"""
    rs = np.random.RandomState(seed)
    gt = np.zeros((G, H, W), bool)
    for g in range(G):
        r0, c0 = rs.randint(0, H - 4), rs.randint(0, W - 4)
        gt[g, r0:r0 + rs.randint(2, H - r0 + 1), c0:c0 + rs.randint(2, W - c0 + 1)] = True
    gt_cats = rs.randint(1, K + 1, size=G)
    det = np.zeros((D, H, W), bool)
    det_cats = np.zeros(D, np.int64)
    for d in range(D):
        g = rs.randint(0, G)
        keep = rs.rand(H, W) < rs.choice([1.0, 0.97, 0.9, 0.7, 0.5])
        det[d] = np.roll(gt[g], rs.randint(-1, 2), axis=rs.randint(0, 2)) & keep
        det_cats[d] = gt_cats[g] if rs.rand() < 0.85 else rs.randint(1, K + 1)
    det[:3] = gt[:3]                                   # IoU exactly 1
    area = gt.reshape(G, -1).sum(1).astype(np.float64)
    area[::5] = rs.choice([1023.0, 1024.0, 1025.0, 9216.0, 9217.0, 200.0], size=len(area[::5]))
    return dict(det_bits=mask_eval.pack_bool_rows_host(det), det_scores=np.round(rs.rand(D), 1).astype(np.float32), det_cats=det_cats,
                gt_bits=mask_eval.pack_bool_rows_host(gt), gt_cats=gt_cats.astype(np.int64), gt_crowd=rs.rand(G) < 0.15, gt_area=area,
                H=H, W=W, det_masks=det, gt_masks=gt)


def eval_stream(cfg, rank, world):
    """a `tools/test.py --data` stream: 5 prepared 64 x 64 images whose metas carry ground truth (rectangles of categories 1..4, one
    crowd, one with its own area), and a sixth image without any"""
    import torch
    from cgg_amd import synthetic
    g = torch.Generator().manual_seed(5)
    rs = np.random.RandomState(3)
    meta = synthetic.img_metas(1, 64, 64)[0]
    for i in range(6):
        img = torch.randn(3, 64, 64, generator=g)
        gt = np.zeros((4, 64, 64), bool)
        for m in gt:
            r0, c0 = rs.randint(0, 40), rs.randint(0, 40)
            m[r0:r0 + rs.randint(8, 40), c0:c0 + rs.randint(8, 40)] = True
        extra = dict(gt_masks=gt, gt_labels=np.array([1, 2, 3, 4]), gt_crowd=np.array([False, False, True, False]),
                     gt_area=np.array([gt[0].sum(), 1500.0, gt[2].sum(), gt[3].sum()], np.float64)) if i < 5 else {}
        if i % world == rank:
            yield img, dict(meta, filename=f'eval_{i}.jpg', **extra)
